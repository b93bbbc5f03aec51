"""
Evaluation runs on the device: exactly N episodes, then the envs retire.

The reference's trainers call ``run_episodes(testing_envs)`` every ``test_interval`` and ``run_episodes(envs['benchmark'],
num_episodes=1000)`` at the end (training/base_algo.py:278-318, ppo.py:216, dqn.py:210, start-training.py:278-281).
``EpisodeRun`` is that bounded run for a ``SafeLifeVectorEnv`` or a ``SafeLifeMultiAgentVectorEnv``; the step kernels do not
change -- three small kernels on the caller's stream sit around the fused step (csrc/sl_episode_run.hip).

The model.  A run is ``N = num_episodes`` TICKETS ``0 .. N-1`` over the pool's ``L`` slots and ``G`` envs (``G =
global_envs``: the env count over all shards; env ``e`` of a shard has the global index ``g = env_offset + e``)::

    ticket t  ->  (slot, env, k) = (t % L, t % G, t // G)

Ticket ``t`` is played on slot ``t % L`` by the env with global index ``t % G``, as that env's ``k``-th episode of the run;
the other way round env ``g`` plays the tickets ``g, g + G, g + 2 G, ...`` below ``N``.  The deal is static, so it needs no
per-env successor: it is what the stride rule does with ``first_level = g % L`` and ``level_stride = G % L`` under
``auto_reset`` (``env_arguments()``).  An env whose first ticket is ``>= N`` never becomes active.  An env that has played its
last ticket RETIRES: it keeps stepping (under action 0) and the step kernel keeps reloading it, but from the next step on its
output records are zeroed behind the step, so nothing downstream -- the episode log's harvest, a rollout, a replay buffer,
the caller -- sees these PHANTOM episodes.  The finished-episode queue of ``side_effects=`` still receives them, because the
step kernel files them: ``tickets(batch)`` tells them apart.  A phantom episode under action 0 ends at the time limit, so a
queue of ``capacity = N + B`` holds a whole run that is flushed at its end.

Where this differs from ``base_algo.run_episodes``, on purpose: the reference's envs share one level iterator, so WHICH env
plays a level depends on finishing order, while the set of episodes is the same (the iterator's first N levels); with more
envs than episodes the reference steps all of them and abandons the stragglers, here envs ``>= N`` never start; and the
reference resets a dropped env once more, consuming a level nobody plays -- the phantom episode here.  DESIGN.md section 6c.

Before the first ``start()`` an attached run does nothing; after a run has ended every record stays zero until the next
``start()``.  Do not ``reset()`` the env while a run is live: an episode's ticket is counted from the env's episode counter
at ``start()``.
"""
import ctypes as C

import numpy as np

from . import _hip
from .levels import LevelPool

#: numpy's view of ``struct sl_episode_run_row``
ROW_DTYPE = np.dtype([("slot", "<i4"), ("env", "<i4"), ("episode_idx", "<i4"), ("step", "<i4"), ("length", "<i4"),
                      ("reward", "<f4"), ("success", "u1"), ("times_up", "u1"), ("flags", "u1"), ("reserved", "u1"),
                      ("reserved2", "<i4")])
#: numpy's view of ``struct sl_episode_run_agent``
AGENT_DTYPE = np.dtype([("length", "<i4"), ("reward", "<f4"), ("success", "u1"), ("times_up", "u1"), ("reserved", "u1", (2,)),
                        ("reserved2", "<i4")])
assert ROW_DTYPE.itemsize == 32 and AGENT_DTYPE.itemsize == 16


def ticket_of(env, k, global_envs):
    """The ticket of global env ``env``'s ``k``-th episode of a run (may be ``>= N``: not a ticket of that run)."""
    return int(env) + int(global_envs) * int(k)


def deal(ticket, n_slots, global_envs):
    """``ticket -> (slot, env, k)``."""
    t = int(ticket)
    return t % int(n_slots), t % int(global_envs), t // int(global_envs)


class EpisodeRun(object):
    """
    pool : LevelPool            not refreshable: the run owns the successor rule
    num_envs : int              envs of the env it will serve (this shard's)
    num_episodes : int          N, at least 1
    n_agents : int              agents per env (the pool's)
    env_offset, global_envs     this shard's first global env index, and the env count over all shards (default: num_envs)

    Build the env with ``SafeLifeVectorEnv(pool, num_envs, episode_run=run, **run.env_arguments())`` (or the multi-agent
    class).  A run refuses a ``level_schedule`` and a refreshable pool (both own the successor rule), ``wrappers`` (the
    reference's evaluation envs carry none, env_factory.py:277-284) and the sliced and queue steppers (nothing would harvest
    their episode ends).  It works with ``side_effects=`` and ``episode_log=``.
    """

    def __init__(self, pool, num_envs, num_episodes, *, n_agents=1, env_offset=0, global_envs=None):
        if not isinstance(pool, LevelPool):
            raise TypeError("pool must be a LevelPool")
        if getattr(pool, "refreshable", False):
            raise ValueError("an episode run and a refreshable pool both own the successor rule: the run deals ticket t to "
                             "slot t % L by the stride rule, a refreshable pool replaces it with its table (pool_next)")
        self.pool = pool
        self.num_envs, self.num_episodes = int(num_envs), int(num_episodes)
        self.n_agents, self.env_offset = int(n_agents), int(env_offset)
        self.global_envs = self.num_envs if global_envs is None else int(global_envs)
        if self.num_envs < 1 or self.num_episodes < 1:
            raise ValueError("num_envs and num_episodes must be at least 1")
        if self.n_agents != int(getattr(pool, "n_agents", 1)):
            raise ValueError("the run was asked for %d agents per env, the pool has %d" % (self.n_agents, pool.n_agents))
        if not 1 <= self.n_agents <= _hip.SL_MAX_AGENTS:
            raise ValueError("n_agents must lie in 1..%d" % _hip.SL_MAX_AGENTS)
        if self.env_offset < 0 or self.env_offset + self.num_envs > self.global_envs:
            raise ValueError("the shard's envs %d..%d must lie inside the %d global envs"
                             % (self.env_offset, self.env_offset + self.num_envs - 1, self.global_envs))
        self.n_slots = int(pool.n_slots)
        g = self.env_offset + np.arange(self.num_envs)
        #: tickets this shard plays
        self.num_tickets = int(sum(len(range(int(x), self.num_episodes, self.global_envs)) for x in g))
        self.env = None
        self.t = None
        self.steps = 0              # step() calls since the last start()
        self._live = False

    # ---- the deal

    def env_arguments(self):
        """``first_level``, ``level_stride`` and ``auto_reset`` for the env's constructor (``env_offset`` is the
        caller's)."""
        g = self.env_offset + np.arange(self.num_envs)
        return dict(first_level=(g % self.n_slots).astype(np.int32), level_stride=self.global_envs % self.n_slots,
                    auto_reset=True)

    def _check_env(self, pool, num_envs, n_agents, auto_reset, first_level, level_stride, env_offset, level_schedule,
                   wrappers):
        """Refuses an env this run cannot serve (called by the env classes before anything is allocated)."""
        if self.env is not None:
            raise ValueError("this EpisodeRun already serves an env")
        if pool is not self.pool:
            raise ValueError("the episode run was built for another pool")
        if int(num_envs) != self.num_envs or int(n_agents) != self.n_agents:
            raise ValueError("the episode run was built for %d envs of %d agent(s), the env has %d of %d"
                             % (self.num_envs, self.n_agents, num_envs, n_agents))
        if level_schedule is not None:
            raise ValueError("an episode run and a level schedule both own the successor rule: the run deals ticket t to slot "
                             "t % L by the stride rule, a schedule redraws the successor table before every step")
        if wrappers:
            raise ValueError("an episode run takes no wrappers: the reference's evaluation envs carry none "
                             "(env_factory.py:277-284), and a retired env's wrapped reward would not be masked")
        want = self.env_arguments()
        first = None if first_level is None else np.broadcast_to(np.asarray(first_level, np.int64), (self.num_envs,))
        if (not auto_reset or int(env_offset) != self.env_offset or first is None
                or not np.array_equal(first, want["first_level"]) or int(level_stride) != want["level_stride"]):
            raise ValueError("an episode run needs the env built with run.env_arguments() -- auto_reset=True, first_level = "
                             "(env_offset + e) %% L, level_stride = global_envs %% L -- and the run's env_offset (%d): that "
                             "is the static deal ticket t -> slot t %% L" % self.env_offset)

    STEPPERS = ("the step and the run's harvest are ordered on one stream: on the slice streams and the queues nothing would "
                "file the episode ends or mask the retired envs")

    # ---- device side

    def _attach(self, env):
        """``env``: the ``SafeLifeVectorEnv`` or ``SafeLifeMultiAgentVectorEnv`` (checked by ``_check_env`` before)."""
        torch = env.torch
        base = getattr(env, "base", env)
        B, N, A, dev = self.num_envs, self.num_episodes, self.n_agents, env.device
        t = self.t = {}
        t["active"] = torch.zeros(B, dtype=torch.uint8, device=dev)
        t["played"] = torch.zeros(B, dtype=torch.int32, device=dev)
        t["base_episode"] = torch.zeros(B, dtype=torch.int32, device=dev)
        t["counters"] = torch.zeros(len(_hip.RUN_COUNTERS), dtype=torch.int32, device=dev)
        t["results"] = torch.zeros((N, ROW_DTYPE.itemsize // 4), dtype=torch.int32, device=dev)
        t["agent_results"] = torch.zeros((N, A, AGENT_DTYPE.itemsize // 4), dtype=torch.int32, device=dev)
        t["side_effects"] = torch.zeros((N, 2), dtype=torch.float64, device=dev)
        t["first_level"] = torch.from_numpy(self.env_arguments()["first_level"]).to(dev)
        s = self.struct = _hip.EpisodeRun()
        s.B, s.G, s.env_offset, s.N, s.L, s.n_agents = B, self.global_envs, self.env_offset, N, self.n_slots, A
        for name in ("active", "played", "base_episode", "counters", "results", "agent_results", "side_effects"):
            setattr(s, name, t[name].data_ptr())
        self._sref = C.byref(s)
        self._lib = _hip.lib()
        self.torch, self.env, self._base = torch, env, base
        self._multi = base is not env
        self._tickets = None

    @property
    def active(self):
        """uint8 [B] on the device: 1 while the env has a ticket to play."""
        return self.t["active"]

    def start(self):
        """Puts every env on slot ``g % L`` whatever it played before -- the ``level_idx`` and ``loaded`` columns as the
        constructor leaves them, then ``env.reset()`` -- and starts the run behind that reset: episode counters noted,
        ``active = (g < N)``, counters and the result table zeroed.  A second ``start()`` replays the same slots; the random
        streams differ through the envs' episode counters, as the reference's do from run to run.  Returns the first
        observation."""
        env, base, cols = self.env, self._base, _hip.SCALAR_COLS
        if env is None:
            raise ValueError("the episode run is not attached to an env")
        base._settle()
        sc = base.t["scalars"]
        sc[:, cols["level_idx"]] = self.t["first_level"]
        sc[:, cols["loaded"]] = 0
        base.goal_cache_invalidate()            # (level_idx was written from outside the library)
        obs = env.reset()
        _hip.check(self._lib.slhip_episode_run_start(self._sref, _hip.ptr(sc), _hip.current_stream_ptr()))
        self.steps, self._live = 0, True
        return obs

    def _after_step(self):
        """One launch behind the step, in front of the log's harvest."""
        if not self._live:
            return
        self.steps += 1
        entry = self._lib.slhip_episode_run_harvest_multi if self._multi else self._lib.slhip_episode_run_harvest
        rc = entry(self._sref, _hip.ptr(self.env.t["out"]), self.steps, _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)

    def _checkpoint_state(self):
        """``checkpoint.py``: the result table and the counters of the last run.  A live run is refused."""
        from . import checkpoint
        checkpoint.refuse_run(self)
        self._need_state()
        config = dict(num_envs=self.num_envs, num_episodes=self.num_episodes, n_agents=self.n_agents,
                      env_offset=self.env_offset, global_envs=self.global_envs, n_slots=self.n_slots)
        names = ("active", "played", "base_episode", "counters", "results", "agent_results", "side_effects")
        return config, dict(steps=self.steps, _live=self._live), {k: self.t[k] for k in names}

    def tickets(self, batch, weights=None, _scores=False):
        """The tickets of a ``SideEffectBatch``'s entries, int32 [capacity] on the device: -1 for a retired env's phantom
        episode, for an episode from before the run and for the slots past the batch's count."""
        torch = self.torch
        q = _hip.EpisodeQueue()
        q.capacity, q.env_base = int(batch.rec_tensor.shape[0]), 0
        q.count, q.records = batch.count.data_ptr(), batch.rec_tensor.data_ptr()
        out = torch.empty(q.capacity, dtype=torch.int32, device=batch.rec_tensor.device)
        args = (None, None, None, None)
        if _scores:
            emd = batch.scores_all()
            batch.wait()
            args = (_hip.ptr(emd["scores"]), _hip.ptr(batch.keys), _hip.ptr(emd["n_cells"]), C.byref(weights))
        _hip.check(self._lib.slhip_episode_run_tickets(self._sref, C.byref(q), _hip.ptr(out), *args,
                                                       _hip.current_stream_ptr()))
        return out

    def side_effects(self, batch, side_effect_weights=None):
        """Scatters the weighted side-effect totals ``(agent, inaction)`` of a flushed batch's entries into the ``[N, 2]``
        column of the result table, by ticket, and returns that column (float64, on the device).  The weights are the env's
        episode log's when it has one (the totals then equal the log's joined rows bit for bit), else
        ``side_effect_weights`` (``{cell name: weight}``, safelife_env.py:185-192)."""
        log = getattr(self.env, "episode_log", None)
        if side_effect_weights is None and log is not None:
            w = log._weights
        else:
            from .side_effects import name_to_cell
            weights = dict(side_effect_weights or {})
            if len(weights) > _hip.SL_SE_MAX_KEYS:
                raise ValueError("at most %d side-effect weights, got %d" % (_hip.SL_SE_MAX_KEYS, len(weights)))
            w = _hip.LogWeights()
            w.n = len(weights)
            for j, (name, weight) in enumerate(weights.items()):
                w.cell[j], w.weight[j] = name_to_cell(name), float(weight)
        self._tickets = self.tickets(batch, w, _scores=True)
        return self.t["side_effects"]

    # ---- host side

    def _need_state(self):
        if self.t is None:
            raise ValueError("the episode run has no device state yet: hand it to the env (episode_run=...)")

    def finished(self):
        """True when no env of this shard has a ticket left (one 4-byte read).  True before the first ``start()``."""
        self._need_state()
        return int(self.t["counters"][1].item()) == 0

    def counters(self):
        """``completed`` (tickets filed), ``in_progress`` (active envs), ``env_steps`` (steps taken by active envs)."""
        self._need_state()
        raw = self.t["counters"].cpu().numpy().tolist()
        return {k: v for k, v in zip(_hip.RUN_COUNTERS, raw) if k != "reserved"}

    def results_device(self):
        """The result table as it lies on the device: ``results`` int32 [N, 8] (``struct sl_episode_run_row``),
        ``agent_results`` int32 [N, A, 4] (``struct sl_episode_run_agent``), ``side_effects`` float64 [N, 2]."""
        self._need_state()
        return {k: self.t[k] for k in ("results", "agent_results", "side_effects")}

    def results(self):
        """The result table, rows by ticket: a structured numpy array with the fields of ``ROW_DTYPE`` (``flags`` & 1: the
        ticket has been played; & 2: ``side_effects`` has been filled), ``side_effects`` float64 (2,) and ``agents``
        (``AGENT_DTYPE`` (A,): every agent's length, reward, success, times_up; the row's own are agent 0's)."""
        self._need_state()
        rows = self.t["results"].cpu().numpy().view(ROW_DTYPE).reshape(-1)
        agents = self.t["agent_results"].cpu().numpy().view(AGENT_DTYPE).reshape(-1, self.n_agents)
        dt = np.dtype(ROW_DTYPE.descr + [("side_effects", "<f8", (2,)), ("agents", AGENT_DTYPE, (self.n_agents,))])
        out = np.zeros(len(rows), dt)
        for name in ROW_DTYPE.names:
            out[name] = rows[name]
        out["side_effects"] = self.t["side_effects"].cpu().numpy()
        out["agents"] = agents
        return out
