"""
Episode histories on the device: the board frames of selected episodes.

The reference's ``SafeLifeLogWrapper`` appends ``game.board`` and ``game.goals`` to ``history['board']`` and
``history['goals']`` after every step (safelife_logger.py:560-592), and ``SafeLifeLogger.log_episode`` keeps the trajectory
when ``(num_episodes - 1) % video_interval == 0`` (:338-347): ``np.savez_compressed(vname, **history)``, then the video.
``EpisodeHistory`` is that trajectory for a ``SafeLifeVectorEnv`` whose boards never leave the device, by LIVE CAPTURE: behind
every ``step()`` two small launches (``slhip_history_capture``, csrc/sl_history.hip) copy the boards of a small, fixed set of
WATCHED envs into frame slots, and the reference's interval rule decides at the episode's end which slots are kept.  No step
kernel changes; the model is in include/safelife_hip.h and restated in tests/episode_history_ref.py.

* ``watch``: the envs that are recorded.  ``slots``: how many histories fit -- one per watched env that is recording plus
  the kept ones that have not been released.  A slot is ``(time_limit + 1) * H * W * 2`` bytes.
* An episode is numbered as the episode log numbers its rows (``num_episodes - 1`` of the reference, over ALL envs); a
  watched env's episode with number ``i`` is kept iff ``i % interval == 0``.  Its last frame -- the board as the agent left
  it, which an in-kernel reload has overwritten by the time the step returns -- comes from the env's finished-episode queue,
  which is why the env needs ``side_effects=``.
* A slot keeps one goals plane: histories are for pools whose goals are static (all shipped levels).

``MultiAgentEpisodeHistory`` is the same recorder for a ``SafeLifeMultiAgentVectorEnv`` (``slhip_history_capture_multi``: the
same bookkeeping kernel reading A records per env): an episode ends where ALL agents are done, as the reference logs on
``np.all(done)``; its length is the env's step count; ``success`` is a bit per agent.

Video export stays with the caller: ``frames(i)`` hands over the RGB frames, ``save(i, path)`` the reference's ``.npz``.
"""
import ctypes as C

import numpy as np

from . import _hip
from .levels import LevelPool

#: numpy's view of ``struct sl_history_entry``
ENTRY_DTYPE = np.dtype([("row", "<i8"), ("env", "<i4"), ("level", "<i4"), ("episode_idx", "<i4"), ("length", "<i4"),
                        ("slot", "<i4"), ("success", "u1"), ("times_up", "u1"), ("flags", "u1"), ("reserved", "u1")])
assert ENTRY_DTYPE.itemsize == 32
_SPAWNING = 1 << 7      # CellTypes.spawning


def static_goals(pool_goals, torch, device):
    """bool [L]: the reference's ``_static_goals`` (safelife_game.py:753-760) of every goal array uint16 [L,H,W] -- one CA
    step neither changes it nor leaves a spawning cell.  One ``advance_board`` launch on the device."""
    from . import speedups
    g = np.ascontiguousarray(pool_goals, np.uint16)
    L = g.shape[0]
    d = torch.from_numpy(g.view(np.int16)).to(device)
    stepped = speedups.advance_board_batch(d, torch.zeros(L, dtype=torch.float32, device=device),
                                           torch.ones((L, 4), dtype=torch.int64, device=device))
    new = stepped.cpu().numpy().view(np.uint16)
    return ~((new & _SPAWNING) != 0).any(axis=(1, 2)) & (new == g).all(axis=(1, 2))


class _EpisodeHistoryBase(object):
    """What the two recorders share: the arguments, the device state, the rewind and the host side.  A subclass says which
    pools it takes (``_check_agents``), what else it asks of its env (``_check_env``), where the env keeps what the capture
    reads (``_env_state``) and which entry point captures (``_capture``)."""

    def __init__(self, pool, num_envs, watch, slots, interval=1, max_bytes=1 << 30):
        if not isinstance(pool, LevelPool):
            raise TypeError("pool must be a LevelPool")
        self._check_agents(int(getattr(pool, "n_agents", 1)))
        if getattr(pool, "refreshable", False):
            raise ValueError("episode histories refuse a refreshable pool: a slot keeps one goals plane and the level it "
                             "names, and a refresh replaces both under a recording episode")
        self.pool = pool
        self.num_envs, self.slots, self.interval, self.max_bytes = int(num_envs), int(slots), int(interval), int(max_bytes)
        w = np.unique(np.asarray(watch, np.int64).reshape(-1))
        if len(w) != np.asarray(watch).size:
            raise ValueError("watch must hold distinct env indices")
        if self.num_envs < 1 or len(w) < 1 or w[0] < 0 or w[-1] >= self.num_envs:
            raise ValueError("watch must hold at least one env index in 0..num_envs-1")
        if len(w) > _hip.HIST_MAX_WATCH:
            raise ValueError("at most %d watched envs, got %d" % (_hip.HIST_MAX_WATCH, len(w)))
        if not 1 <= self.slots <= _hip.HIST_MAX_SLOTS:
            raise ValueError("slots must lie in 1..%d" % _hip.HIST_MAX_SLOTS)
        if self.interval < 1:
            raise ValueError("interval must be at least 1")
        self.watch = w.astype(np.int32)
        self.env = None
        self.t = None

    def slot_bytes(self, time_limit):
        """``K * (T + 1) * H * W * 2``: the goals plane and T board frames of every slot."""
        H, W = self.pool.shape
        return self.slots * (int(time_limit) + 1) * H * W * 2

    # ---- the env's side

    def _check_env(self, pool, num_envs, time_limit, side_effects, torch, device):
        """Refuses an env this recorder cannot serve (called by the env before anything is allocated)."""
        if self.env is not None:
            raise ValueError("this %s already serves an env" % type(self).__name__)
        if pool is not self.pool:
            raise ValueError("the episode history was built for another pool")
        if int(num_envs) != self.num_envs:
            raise ValueError("the episode history was built for %d envs, the env has %d" % (self.num_envs, num_envs))
        if not side_effects:
            raise ValueError("an episode history needs the env's finished-episode queue (side_effects=dict(capacity=...)): "
                             "an episode's last frame is the board as the agent left it, and after an in-kernel reload "
                             "only the queue still holds it")
        if int(time_limit) < 1:
            raise ValueError("an episode history needs a time limit: a slot holds time_limit frames")
        need = self.slot_bytes(time_limit)
        if need > self.max_bytes:
            H, W = pool.shape
            raise ValueError("the episode history's slots need %d bytes (slots %d * (time_limit %d + 1) * %d * %d * 2), "
                             "max_bytes allows %d" % (need, self.slots, time_limit, H, W, self.max_bytes))
        if device is None:      # (the first thing here that needs one)
            device = _hip.device()
        moving = np.flatnonzero(~static_goals(pool.arrays()["pool_goals"], torch, device))
        if len(moving):
            raise ValueError("episode histories need static goals: a slot keeps ONE goals plane, because the "
                             "finished-episode queue keeps no goals and the last frame's goals exist nowhere after the "
                             "reload; the goals of pool slot(s) %s change under a CA step (safelife_game.py:753-760)"
                             % moving[:8].tolist())

    STEPPERS = ("the step and the recorder's capture are ordered on one stream: on the slice streams and the queues, and "
                "inside a many-step launch, nothing would copy the frames")

    def _attach(self, env):
        torch, dev = env.torch, env.device
        B, n, K, T = self.num_envs, len(self.watch), self.slots, env.time_limit
        H, W = self.pool.shape
        t = self.t = {}
        t["watch"] = torch.from_numpy(self.watch).to(dev)
        t["owner"] = torch.full((n,), -1, dtype=torch.int32, device=dev)
        t["cur_level"] = torch.zeros(n, dtype=torch.int32, device=dev)
        t["cur_episode"] = torch.zeros(n, dtype=torch.int32, device=dev)
        t["slot_state"] = torch.zeros(K, dtype=torch.int32, device=dev)
        t["entries"] = torch.zeros((K, ENTRY_DTYPE.itemsize // 8), dtype=torch.int64, device=dev)
        t["counters"] = torch.zeros(len(_hip.HIST_COUNTERS), dtype=torch.int64, device=dev)
        t["goals"] = torch.zeros((K, H, W), dtype=torch.int16, device=dev)
        t["frames"] = torch.zeros((K, T, H, W), dtype=torch.int16, device=dev)
        t["orders"] = torch.zeros((n, _hip.HIST_ORDER_WORDS), dtype=torch.int32, device=dev)
        s = self.struct = _hip.EpisodeHistory()
        s.B, s.n_watch, s.n_slots, s.T, s.H, s.W, s.interval = B, n, K, T, H, W, self.interval
        for name, ctype in _hip.EpisodeHistory._fields_:
            if ctype is C.c_void_p:
                setattr(s, name, t[name].data_ptr())
        self._sref = C.byref(s)
        self._lib = _hip.lib()
        self.torch, self.env, self.time_limit = torch, env, T
        # (the env's state tensors live as long as it does, and a flush writes the fresh queue INTO struct.finished)
        self._env_t, self._out, self._queue = self._env_state(env)
        self._rewind()

    def _rewind(self, mask=None):
        """After the envs (those with mask != 0) have been reset from outside the step: their episodes start over at frame
        0 on their new level; an env without a slot takes a free one."""
        et = self._env_t
        _hip.check(self._lib.slhip_history_rewind(self._sref, _hip.ptr(et["goals"]), _hip.ptr(et["scalars"]), _hip.ptr(mask),
                                                  _hip.current_stream_ptr()))

    def _after_step(self):
        """Two launches behind the step, in front of the episode run's and the log's harvests."""
        run = getattr(self.env, "episode_run", None)
        active = run.t["active"] if (run is not None and run._live) else None
        et = self._env_t
        rc = self._capture(_hip.ptr(et["board"]), _hip.ptr(et["goals"]), _hip.ptr(et["scalars"]), _hip.ptr(self._out),
                           self._queue, _hip.ptr(active), _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)

    def _checkpoint_state(self):
        """``checkpoint.py``: the slots with their frames, the listing, and where every watched env's episode stands."""
        self._need_state()
        config = dict(num_envs=self.num_envs, slots=self.slots, interval=self.interval, watch=self.watch.tolist(),
                      time_limit=self.time_limit, board_shape=self.pool.shape)
        names = ("owner", "cur_level", "cur_episode", "slot_state", "entries", "counters", "goals", "frames", "orders")
        return config, {}, {k: self.t[k] for k in names}

    def _queue_replaced(self):
        """``side_effects_flush()`` has installed a fresh queue: the cursor starts over."""
        self.t["counters"][4].zero_()

    # ---- host side

    def _need_state(self):
        if self.t is None:
            raise ValueError("the episode history has no device state yet: hand it to %s(episode_history=...)" % self.ENV)

    def counters(self):
        """``kept`` (histories filed), ``missed`` (episodes the rule kept whose env owned no slot), ``incomplete`` (kept
        histories without their last frame: the queue had overflowed), and ``episodes`` (numbered so far)."""
        self._need_state()
        raw = self.t["counters"].cpu().numpy().tolist()
        return {k: raw[j] for j, k in enumerate(_hip.HIST_COUNTERS) if k in ("episodes", "kept", "missed", "incomplete")}

    def entries(self):
        """The kept histories that have not been released, in episode order: a structured array of ``ENTRY_DTYPE`` (``row``:
        the episode's number, the episode log's row index; ``level``: the pool slot that was played; ``flags`` & 2: the last
        frame is missing)."""
        self._need_state()
        all_ = self.t["entries"].cpu().numpy().view(ENTRY_DTYPE).reshape(-1)
        live = all_[(all_["flags"] & _hip.HIST_LIVE) != 0]
        return live[np.argsort(live["row"], kind="stable")]

    def _entry(self, i):
        listing = self.entries()
        if not -len(listing) <= int(i) < len(listing):
            raise IndexError("history %d of %d" % (i, len(listing)))
        en = listing[int(i)]
        return en, int(en["length"]) - (1 if en["flags"] & _hip.HIST_NO_FINAL else 0)

    def history(self, i, device=False):
        """``{'board': uint16 [length,H,W], 'goals': uint16 [length,H,W]}`` of the i-th listed history, the goals broadcast
        from the slot's plane: what the reference hands ``np.savez_compressed``.  ``device=True``: int16 device tensors (the
        same bytes), the board a view of the slot."""
        en, n = self._entry(i)
        s = int(en["slot"])
        board, goals = self.t["frames"][s, :n], self.t["goals"][s]
        if device:
            return {"board": board, "goals": goals.expand(n, -1, -1)}
        g = goals.cpu().numpy().view(np.uint16)
        return {"board": board.cpu().numpy().view(np.uint16), "goals": np.broadcast_to(g, (n,) + g.shape).copy()}

    def save(self, i, path):
        """Writes the i-th listed history as the reference's ``.npz`` (keys ``board`` and ``goals``)."""
        np.savez_compressed(path, **self.history(i))

    def frames(self, i, out=None):
        """RGB frames uint8 ``[length, H*14, W*14, 3]`` of the i-th listed history through ``render.render_board`` on the
        device: a device tensor, no host copy of the boards."""
        from . import render
        en, n = self._entry(i)
        s = int(en["slot"])
        if n == 0:          # (an episode of one step whose last frame was lost)
            H, W = self.pool.shape
            return self.torch.empty((0, H * render.SPRITE_SIZE, W * render.SPRITE_SIZE, 3), dtype=self.torch.uint8,
                                    device=self.t["frames"].device)
        return render.render_board(self.t["frames"][s, :n], self.t["goals"][s], out=out)

    def release(self, indices=None):
        """Hands the slots of the listed histories `indices` (default: all) back.  A watched env that owns no slot takes a
        free one where its next episode starts.  Returns the number of slots released."""
        listing = self.entries()
        pick = listing if indices is None else listing[np.atleast_1d(np.asarray(indices, np.int64))]
        if len(pick) == 0:
            return 0
        slots = self.torch.from_numpy(np.unique(pick["slot"]).astype(np.int64)).to(self.t["slot_state"].device)
        self.t["slot_state"][slots] = _hip.HIST_SLOT_FREE
        self.t["entries"][slots] = 0
        return int(slots.numel())


class EpisodeHistory(_EpisodeHistoryBase):
    """
    pool : LevelPool            single-agent, not refreshable, static goals
    num_envs : int              of the env it will serve
    watch : ints                the watched envs: distinct indices in 0..num_envs-1 (sorted here), at most 1024
    slots : int                 frame slots, 1..1024
    interval : int              the reference's ``video_interval``, >= 1
    max_bytes : int             the slot memory the recorder may allocate (default 1 GiB)

    Attach with ``SafeLifeVectorEnv(pool, ..., side_effects=dict(...), episode_history=h)``; a recorder serves one env.  Only
    ``step()`` and ``reset()`` drive it.  ``entries()`` lists the kept histories in episode order; ``history(i)``, ``save(i,
    path)`` and ``frames(i)`` read the i-th of that listing; ``release()`` hands slots back, and a watched env that found no
    free slot picks one up where its next episode starts.
    """
    ENV = "SafeLifeVectorEnv"

    def _check_agents(self, A):
        if A > 1:
            raise ValueError("episode histories serve a single-agent SafeLifeVectorEnv: this pool has %d agents per level "
                             "(multi-agent histories are out of scope here: MultiAgentEpisodeHistory records them)" % A)

    def _env_state(self, env):
        return env.t, env.t["out"], C.byref(env.struct.finished)

    def _capture(self, board, goals, scalars, out, queue, active, stream):
        return self._lib.slhip_history_capture(self._sref, board, goals, scalars, out, queue, active, stream)


class MultiAgentEpisodeHistory(_EpisodeHistoryBase):
    """
    The recorder of a ``SafeLifeMultiAgentVectorEnv``: the arguments, the listing and the readers of ``EpisodeHistory``, for
    a ``LevelPool(levels, n_agents=A)`` with A >= 1.  The reference records these envs as it records the others -- a frame
    after every step until ``np.all(done)`` -- so an episode ends on the step where the last agent finishes (the step on
    which the env reloads and the ``MultiAgentEpisodeLog`` files its row: ``row`` is that row's index), ``length`` is the
    number of steps the env took (the largest ``episode_length`` of its agents), ``times_up`` holds for all agents or none,
    and ``success`` is a bit per agent: ``success(entry)`` unpacks it.  ``reserved`` carries A.

    Attach with ``SafeLifeMultiAgentVectorEnv(pool, ..., side_effects=dict(...), episode_history=h)``; the env must reload
    itself (``auto_reset=True``).
    """
    ENV = "SafeLifeMultiAgentVectorEnv"

    def _check_agents(self, A):
        if not 1 <= A <= _hip.SL_MAX_AGENTS:
            raise ValueError("1..%d agents per level, this pool has %d" % (_hip.SL_MAX_AGENTS, A))
        self.n_agents = A

    def _check_env(self, pool, num_envs, time_limit, side_effects, torch, device, n_agents=None, auto_reset=True):
        if n_agents is not None and int(n_agents) != self.n_agents:
            raise ValueError("the episode history was built for %d agents per env, the env has %d" % (self.n_agents, n_agents))
        if not auto_reset:
            raise ValueError("an episode history needs auto_reset=True: an env that stays all-done would end an episode on "
                             "every step where the reference saves the episode once")
        _EpisodeHistoryBase._check_env(self, pool, num_envs, time_limit, side_effects, torch, device)

    def _env_state(self, env):
        return env.base.t, env.t["out"], C.byref(env.base.struct.finished)

    def _capture(self, board, goals, scalars, out, queue, active, stream):
        return self._lib.slhip_history_capture_multi(self._sref, board, goals, scalars, out, self.n_agents, queue, active,
                                                     stream)

    def success(self, entry):
        """bool [A]: every agent's ``info['episode']['success']`` of a listed entry."""
        return ((int(entry["success"]) >> np.arange(self.n_agents)) & 1).astype(bool)
