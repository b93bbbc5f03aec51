"""
The episode log on the device: what the reference's ``SafeLifeLogger`` computes (safelife_logger.py), without a host visit
per step.

* ``SafeLifeLogWrapper`` counts ``<type>_steps`` and calls ``log_episode()`` when an episode ends (:560-581);
* ``log_episode()`` turns the episode into ``reward / reward_possible``, ``reward_needed``, ``length``, ``success``, the
  side-effect fraction and ``combined_score`` (:262-354, :671-716);
* ``log_scalars()`` folds them into running summaries, Polyak 0.99 for training and a plain mean otherwise (:372-381);
* ``summarize_run_file()`` prints the run's headline (:719-762).

``EpisodeLog`` keeps a ring of ROWS on the device, one per finished episode.  After every ``step()`` one kernel writes the
rows of the episodes that ended, in ascending env order (``slhip_episode_log_harvest``); ``flush()`` joins the side-effect
totals of the env's finished-episode queue into their rows (``slhip_episode_log_join``) and folds the new rows into the five
running summaries (``slhip_episode_log_summaries``); ``run_summary()`` is ``summarize_run_file`` over the ring
(``slhip_episode_log_run_summary``).  The exact arithmetic is in include/safelife_hip.h and restated in
tests/episode_log_ref.py.  Files, tensorboard, wandb, video and ``reward_frac_needed`` stay with the caller: ``records()``
hands over what the JSON log holds.

``EpisodeLog`` serves a single-agent ``SafeLifeVectorEnv``.  ``MultiAgentEpisodeLog`` serves a
``SafeLifeMultiAgentVectorEnv`` with the same surface: one row per env episode, filed on the step where all its agents are
done (``slhip_episode_log_harvest_multi``), per-agent ``length`` / ``reward`` / ``success`` / ``score`` beside the row's one
side-effect fraction, and running summaries under the reference's ``<agent name>-`` prefixed keys
(``slhip_episode_log_join_multi`` / ``_summaries_multi`` / ``_run_summary_multi``; restated in
tests/episode_log_multi_ref.py).
"""
import ctypes as C

import numpy as np

from . import _hip
from .levels import LevelPool, available_points, initial_colors

#: numpy's view of ``struct sl_episode_log_row``
ROW_DTYPE = np.dtype([("index", "<i8"), ("training_steps", "<i8"), ("prev", "<i8"), ("env", "<i4"), ("level", "<i4"),
                      ("episode_idx", "<i4"), ("length", "<i4"), ("reward", "<f4"), ("reward_possible", "<i4"),
                      ("reward_needed", "<i4"), ("success", "u1"), ("times_up", "u1"), ("flags", "u1"), ("reserved", "u1"),
                      ("reward_frac", "<f8"), ("side_effects", "<f8", (2,)), ("side_effects_frac", "<f8"), ("score", "<f8")])
assert ROW_DTYPE.itemsize == 96
_DEFAULT_POLYAK = {"training": 0.99}
RUN_SUMMARY_FIELDS = ("rows", "success", "avg_length", "side_effects", "reward", "score", "side_effects_std", "reward_std",
                      "score_std", "successful_length", "successful_length_std", "successes")


class _EpisodeLogBase(object):
    """What ``EpisodeLog`` and ``MultiAgentEpisodeLog`` share: the arguments' checks, the device state, the calls of the
    entry points and the host's views.  A subclass says what differs: ``_struct`` (its ctypes struct), ``_suffix`` (of its
    ``slhip_episode_log_*`` entry points), ``_env_class`` (for the messages), ``n_keys`` (summary chains), ``row_dtype``,
    ``available`` (int32 [L] or [L, A]; ``cur_required`` is [B] or [B, A] with it), ``_check_agents()``,
    ``_extra_state()``, ``_now()``, ``harvest()`` (the call of every step: no layer under it) with ``_after_step()``,
    ``summary()`` and ``records()``."""

    def __init__(self, pool, num_envs, capacity, episode_type, summary_polyak, side_effect_weights):
        if not isinstance(pool, LevelPool):
            raise TypeError("pool must be a LevelPool")
        self._check_agents(int(pool.n_agents))
        self.pool = pool
        num_envs, capacity, episode_type = int(num_envs), int(capacity), str(episode_type)
        if num_envs < 1:
            raise ValueError("num_envs must be at least 1")
        if capacity < num_envs:
            raise ValueError("capacity (%d) must be at least num_envs (%d): one step can end every env's episode"
                             % (capacity, num_envs))
        p = _DEFAULT_POLYAK.get(episode_type, 1.0) if summary_polyak is None else float(summary_polyak)
        if not (np.isfinite(p) and p >= 0.0):
            raise ValueError("summary_polyak must be finite and not negative, got %r" % (summary_polyak,))
        from .side_effects import name_to_cell
        weights = dict(side_effect_weights or {})
        if len(weights) > _hip.SL_SE_MAX_KEYS:
            raise ValueError("at most %d side-effect weights, got %d" % (_hip.SL_SE_MAX_KEYS, len(weights)))
        w = self._weights = _hip.LogWeights()
        w.n = len(weights)
        for j, (name, weight) in enumerate(weights.items()):
            w.cell[j], w.weight[j] = name_to_cell(name), float(weight)
        self.num_envs, self.capacity, self.episode_type, self.summary_polyak = num_envs, capacity, episode_type, p
        self.side_effect_weights = weights
        self.env = None
        self.t = None

    def _extra_state(self):
        """-> {struct field: int} and {struct field: numpy array, which becomes a device tensor of that name} beyond
        ``sl_episode_log``'s."""
        return {}, {}

    def reward_possible(self, points_on_level_exit=1):
        """What the logger records as ``reward_possible`` (:286-287), int32 of ``available``'s shape."""
        return (self.available.astype(np.int64) + int(points_on_level_exit)).astype(np.int32)

    # ---- device side

    def allocate(self, torch, device, points_on_level_exit=1):
        """The device state (the env calls this through ``_attach``; a caller with step records of its own calls it and
        ``harvest()`` itself)."""
        B, cap, dev, n = self.num_envs, self.capacity, device, self.n_keys
        fields, arrays = self._extra_state()
        self.torch = torch
        t = self.t = {}
        t["rows"] = torch.zeros((cap, self.row_dtype.itemsize // 8), dtype=torch.int64, device=dev)
        t["rows"][:, 0] = -1                        # (no row's index)
        # counters | counts | values | weights in one buffer: summary() is one host visit
        t["state"] = torch.zeros(5 + 3 * n, dtype=torch.int64, device=dev)
        t["counters"], t["count"] = t["state"][0:5], t["state"][5:5 + n]
        t["value"] = t["state"][5 + n:5 + 2 * n].view(torch.float64)
        t["weight"] = t["state"][5 + 2 * n:].view(torch.float64)
        t["cur_slot"] = torch.zeros(B, dtype=torch.int32, device=dev)
        t["cur_required"] = torch.zeros((B,) + self.available.shape[1:], dtype=torch.int32, device=dev)
        t["cur_episode"] = torch.zeros(B, dtype=torch.int32, device=dev)
        t["last_row"] = torch.full((B,), -1, dtype=torch.int64, device=dev)
        t["reward_possible"] = torch.from_numpy(self.reward_possible(points_on_level_exit)).to(dev)
        for name, array in arrays.items():
            t[name] = torch.from_numpy(array).to(dev)
        t["run_summary"] = torch.zeros(_hip.LOG_RUN_SUMMARY, dtype=torch.float64, device=dev)
        s = self.struct = self._struct()
        s.capacity, s.B, s.L, s.polyak = cap, B, self.pool.n_slots, self.summary_polyak
        for name, value in fields.items():
            setattr(s, name, value)
        for name in ("rows", "counters", "cur_slot", "cur_required", "cur_episode", "last_row", "reward_possible", "value",
                     "count", "weight") + tuple(arrays):
            setattr(s, name, t[name].data_ptr())
        self._sref = C.byref(s)
        self._lib = _hip.lib()
        self._harvest_entry, self._join_entry, self._summaries_entry, self._run_summary_entry = (
            getattr(self._lib, "slhip_episode_log_" + name + self._suffix)
            for name in ("harvest", "join", "summaries", "run_summary"))
        return t

    def _attach(self, env):
        if self.env is not None:
            raise ValueError("this %s already serves an env" % type(self).__name__)
        if env.pool is not self.pool:
            raise ValueError("the episode log was built for another pool")
        if env.num_envs != self.num_envs:
            raise ValueError("the episode log was built for %d envs, the env has %d" % (self.num_envs, env.num_envs))
        self.allocate(env.torch, env.device, getattr(env, "base", env).struct.exit_points)
        self.env = env
        self._rewind()

    def _rewind(self, mask=None):
        """After the envs (those with mask != 0) have been reset from outside the step: their episodes start over."""
        t, torch = self.t, self.torch
        for name, value in self._now().items():
            sel = None if mask is None else (mask != 0 if value.dim() == 1 else (mask != 0)[:, None])
            t[name].copy_(value if sel is None else torch.where(sel, value, t[name]))
        if mask is None:
            t["last_row"].fill_(-1)
        else:
            t["last_row"].masked_fill_(mask != 0, -1)

    def _checkpoint_state(self):
        """``checkpoint.py``: the row ring, the counters with the summaries' counts, values and Polyak weights (one buffer),
        and what the log knows of every env's running episode."""
        self._device_state()
        config = dict(num_envs=self.num_envs, capacity=self.capacity, episode_type=self.episode_type,
                      summary_polyak=self.summary_polyak, n_keys=self.n_keys, row_bytes=self.row_dtype.itemsize,
                      side_effect_weights=self.side_effect_weights)
        return config, {}, {k: self.t[k] for k in ("rows", "state", "cur_slot", "cur_required", "cur_episode", "last_row")}

    def join(self, count, records, scores, keys, n_cells):
        """The join of one flushed queue (device tensors: count int32 [1], records int32 [C,8], scores float64 [C,K,2], keys
        [C,K] 16-bit, n_cells int32 [C,K]; one entry per env episode) on the current stream."""
        q = _hip.EpisodeQueue()
        q.capacity, q.env_base = int(records.shape[0]), 0
        q.count, q.records = count.data_ptr(), records.data_ptr()
        _hip.check(self._join_entry(self._sref, C.byref(q), _hip.ptr(scores), _hip.ptr(keys), _hip.ptr(n_cells),
                                       C.byref(self._weights), _hip.current_stream_ptr()))

    def summarise(self):
        """Folds the rows not yet consumed into the running summaries, on the current stream."""
        _hip.check(self._summaries_entry(self._sref, _hip.current_stream_ptr()))

    def flush(self):
        """On the caller's stream: with a side-effect queue on the env, ``side_effects_flush()``, ``scores_all()`` and the
        join; then the summaries.  Returns the ``SideEffectBatch`` or None.  Without a queue ``side_effects`` and ``score``
        simply never count."""
        env, batch = self.env, None
        if env is None:
            raise ValueError("the episode log is not attached to an env")
        if getattr(env, "base", env)._se is not None:
            batch = env.side_effects_flush()
            emd = batch.scores_all()
            self.join(batch.count, batch.rec_tensor, emd["scores"], batch.keys, emd["n_cells"])
        self.summarise()
        return batch

    def reset_summary(self):
        """``SafeLifeLogger.reset_summary()`` (safelife_logger.py:406-414): the running summaries start over --
        ``summary_stats``, ``summary_counts`` and the weights the next values meet go to zero, on the caller's stream.  Rows
        and counters stay; rows not yet summarised are still folded in by the next ``flush()``."""
        self._device_state()[5:].zero_()

    # ---- host side: each of these is one visit

    def _device_state(self):
        if self.t is None:
            raise ValueError("the episode log has no device state yet: hand it to %s(episode_log=...)" % self._env_class)
        return self.t["state"]

    def _state(self):
        raw, n = self._device_state().cpu().numpy(), self.n_keys
        return (dict(zip(_hip.LOG_COUNTERS, raw[0:5].tolist())), raw[5:5 + n].copy(),
                raw[5 + n:5 + 2 * n].copy().view(np.float64), raw[5 + 2 * n:].copy().view(np.float64))

    def counters(self):
        """``n_rows``, ``steps``, ``episodes``, ``summarised``, ``unmatched``."""
        return self._state()[0]

    def rows(self, first=None):
        """The rows [max(first, n_rows - capacity), n_rows) in row order: a numpy record array of ``self.row_dtype``
        (``ROW_DTYPE``, or ``multi_row_dtype(A)``: the header's fields and ``agents`` [A])."""
        n_rows = self.counters()["n_rows"]
        lo = max(0 if first is None else int(first), n_rows - self.capacity, 0)
        ring = self.t["rows"].cpu().numpy().view(self.row_dtype).reshape(-1)
        return ring[np.arange(lo, max(n_rows, lo)) % self.capacity]

    def _level_names(self, level_names):
        if level_names is None:
            level_names = [getattr(lv, "name", None) or "level-%d" % k for k, lv in enumerate(self.pool.levels)]
        return level_names

    def run_summary(self, first_row=0):
        """``summarize_run_file`` over the rows [max(first_row, n_rows - capacity), n_rows): its five means (``success``,
        ``avg_length``, ``side_effects``, ``reward``, ``score``), the printed standard deviations, the successful length
        and the row count.  With several agents ``success``, ``avg_length``, ``reward``, ``score`` and the successful
        length are over all rows x agents entries and ``side_effects`` over the rows; ``rows`` is the number of rows,
        ``successes`` of successful entries."""
        out = self.t["run_summary"]
        _hip.check(self._run_summary_entry(self._sref, int(first_row), _hip.ptr(out), _hip.current_stream_ptr()))
        vals = out.cpu().numpy()
        res = dict(zip(RUN_SUMMARY_FIELDS, vals.tolist()))
        res["rows"], res["successes"] = int(vals[0]), int(vals[11])
        return res


class EpisodeLog(_EpisodeLogBase):
    """
    pool : LevelPool            single-agent
    num_envs : int              of the env it will serve
    capacity : int              rows of the ring, >= num_envs; older rows are overwritten
    episode_type : str          "training" | "validation" | "benchmark" | ... : the prefix of the summary's keys
    summary_polyak : float      None: 0.99 for training, else 1.0 (``SafeLifeLogger._defaults``)
    side_effect_weights : {cell name: weight} or None
                                safelife_env.py:185-192; at most 24 entries.  None: every total is 0, as an env without
                                weights has no ``total`` (combined_score :704)

    Attach with ``SafeLifeVectorEnv(pool, ..., episode_log=log)``; a log serves one env.  Only ``step()`` and ``reset()``
    drive it.  ``reset(mask)`` forgets the reset envs' row chains: flush before it, or the queue entries of those envs count
    as ``unmatched``.
    """
    _struct, _suffix, _env_class = _hip.EpisodeLog, "", "SafeLifeVectorEnv"
    n_keys = len(_hip.LOG_KEYS)
    row_dtype = ROW_DTYPE

    def __init__(self, pool, num_envs, capacity, episode_type="training", summary_polyak=None, side_effect_weights=None):
        super(EpisodeLog, self).__init__(pool, num_envs, capacity, episode_type, summary_polyak, side_effect_weights)
        # per slot: agent 0's available points (safelife_game.py:696-709), as LevelSchedule computes them
        self.available = np.zeros(pool.n_slots, np.int32)
        for k, lv in enumerate(pool.levels):
            table = pool.points_table[pool.pool_table_idx[k]].astype(np.int64)
            self.available[k] = available_points(table, pool.initial_counts[k], initial_colors(lv.board))

    def _check_agents(self, A):
        if A > 1:
            raise ValueError("the episode log serves a single-agent SafeLifeVectorEnv: this pool has %d agents per level "
                             "(MultiAgentEpisodeLog serves a SafeLifeMultiAgentVectorEnv)" % A)

    def _now(self):
        sc, cols = self.env.t["scalars"], _hip.SCALAR_COLS
        return {"cur_slot": sc[:, cols["level_idx"]], "cur_required": sc[:, cols["required_points"]],
                "cur_episode": sc[:, cols["episode_idx"]]}

    def harvest(self, out, scalars):
        """One launch on the current stream: rows for the envs whose record in `out` (int32 [B,4], ``struct sl_step_out``)
        says done; `scalars` int32 [B,16] as the step left them."""
        rc = self._harvest_entry(self._sref, _hip.ptr(out), _hip.ptr(scalars), self.num_envs, _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)

    def _after_step(self):
        self.harvest(self.env.t["out"], self.env.t["scalars"])

    def summary(self):
        """``{"training/length": ..., ...}`` for the keys that have met a finite value, plus ``training/steps`` and
        ``training/episodes`` (``summary_stats`` and ``cumulative_stats`` as log_scalars keys them)."""
        counters, count, value, _ = self._state()
        tag = self.episode_type
        out = {"%s/%s" % (tag, key): float(value[k]) for k, key in enumerate(_hip.LOG_KEYS) if count[k] > 0}
        out[tag + "/steps"], out[tag + "/episodes"] = counters["steps"], counters["episodes"]
        return out

    def records(self, level_names=None, first=None):
        """The rows as the reference's ``log_data`` dicts (:282-302) without ``time``, for whoever writes the JSON log.
        ``level_names``: one title per pool slot (default: the pool's levels' names, where they have one)."""
        return rows_to_records(self.rows(first), self._level_names(level_names))


def multi_row_dtype(n_agents):
    """numpy's view of ``struct sl_episode_log_row_multi`` followed by its ``n_agents`` ``sl_episode_log_agent`` records
    (``SL_LOG_ROW_MULTI_BYTES``)."""
    agent = np.dtype([("length", "<i4"), ("reward", "<f4"), ("reward_possible", "<i4"), ("reward_needed", "<i4"),
                      ("success", "u1"), ("times_up", "u1"), ("name", "u1"), ("reserved", "u1", (5,)),
                      ("reward_frac", "<f8"), ("score", "<f8")])
    row = np.dtype([("index", "<i8"), ("training_steps", "<i8"), ("prev", "<i8"), ("env", "<i4"), ("level", "<i4"),
                    ("episode_idx", "<i4"), ("flags", "u1"), ("n_agents", "u1"), ("reserved", "u1", (2,)),
                    ("side_effects", "<f8", (2,)), ("side_effects_frac", "<f8"), ("agents", agent, (int(n_agents),))])
    assert row.itemsize == _hip.log_row_multi_bytes(n_agents)
    return row


class MultiAgentEpisodeLog(_EpisodeLogBase):
    """
    The episode log for a ``SafeLifeMultiAgentVectorEnv``: what ``SafeLifeLogger`` does when ``info['episode']`` holds
    arrays over the agents (safelife_logger.py:289-291, :319-328).  A row per env EPISODE, filed on the step where all its
    agents are done; ``length``, ``reward``, ``success``, ``reward_possible``, ``reward_needed``, ``reward_frac`` and ``score``
    per agent, the side-effect totals and their fraction per row; running summaries ``<name>-length | -reward | -success |
    -score`` per distinct agent name, where of two agents of one level with the same name the last one counts (``tb_data``
    is a dict) and a key is only moved by episodes whose level has an agent of that name.  There is no ``side_effects``
    summary: the reference hands ``log_scalars`` a shape-(1,) array there, which it skips.

    pool : LevelPool(levels, n_agents=A)        a pool with one agent per level logs arrays and ``agent0-`` keys too
    num_envs, capacity, episode_type, summary_polyak, side_effect_weights : as ``EpisodeLog``
    agent_names : one list of A names per pool slot, or None: ``agent0 .. agent{A-1}`` for every slot (what
                  ``safelife_amd.game`` names them); at most 16 distinct names

    Attach with ``SafeLifeMultiAgentVectorEnv(pool, ..., episode_log=log)`` (``auto_reset=True``); the surface is
    ``EpisodeLog``'s.
    """
    _struct, _suffix, _env_class = _hip.EpisodeLogMulti, "_multi", "SafeLifeMultiAgentVectorEnv"
    n_keys = _hip.LOG_MAX_NAMES * len(_hip.LOG_MULTI_KEYS)

    def __init__(self, pool, num_envs, capacity, episode_type="training", summary_polyak=None, side_effect_weights=None,
                 agent_names=None):
        super(MultiAgentEpisodeLog, self).__init__(pool, num_envs, capacity, episode_type, summary_polyak,
                                                   side_effect_weights)
        A, L = self.n_agents, pool.n_slots
        if agent_names is None:
            agent_names = [["agent%d" % a for a in range(A)]] * L
        agent_names = [[str(n) for n in names] for names in agent_names]
        if len(agent_names) != L or any(len(names) != A for names in agent_names):
            raise ValueError("agent_names must hold one list of %d names for each of the pool's %d slots" % (A, L))
        self.agent_names = agent_names
        self.names = []                     # the distinct names, in order of appearance
        self.name_id = np.zeros((L, A), np.uint8)
        for k, names in enumerate(agent_names):
            for a, name in enumerate(names):
                if name not in self.names:
                    self.names.append(name)
                self.name_id[k, a] = min(self.names.index(name), _hip.LOG_NO_NAME)
        if len(self.names) > _hip.LOG_MAX_NAMES:
            raise ValueError("at most %d distinct agent names, got %d" % (_hip.LOG_MAX_NAMES, len(self.names)))
        # per slot and agent: the agent's own table against the level's counts (safelife_game.py:696-709), as LevelSchedule
        self.available = np.zeros((L, A), np.int32)
        for k, lv in enumerate(pool.levels):
            colors = initial_colors(lv.board)
            for a in range(A):
                idx = pool.pool_agent_table_idx[k, a] if A > 1 else pool.pool_table_idx[k]
                self.available[k, a] = available_points(pool.points_table[idx].astype(np.int64), pool.initial_counts[k], colors)
        self.row_dtype = multi_row_dtype(A)

    def _check_agents(self, A):
        self.n_agents = A
        if not 1 <= A <= _hip.SL_MAX_AGENTS:
            raise ValueError("the pool must have 1 to %d agents per level, not %d" % (_hip.SL_MAX_AGENTS, A))

    def _extra_state(self):
        return {"n_agents": self.n_agents, "n_names": len(self.names)}, {"name_id": self.name_id}

    def _now(self):
        sc, cols = self.env.base.t["scalars"], _hip.SCALAR_COLS
        return {"cur_slot": sc[:, cols["level_idx"]], "cur_episode": sc[:, cols["episode_idx"]],
                "cur_required": self.env.t["agents"][:, :, _hip.AGENT_COLS["required_points"]]}

    def harvest(self, out, agents, scalars):
        """One launch on the current stream: rows for the envs ALL of whose records in `out` (int32 [B,A,4], ``struct
        sl_step_out``) say done; `agents` int32 [B,A,12] and `scalars` int32 [B,16] as the step left them."""
        rc = self._harvest_entry(self._sref, _hip.ptr(out), _hip.ptr(agents), _hip.ptr(scalars), self.num_envs,
                                 _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)

    def _after_step(self):
        self.harvest(self.env.t["out"], self.env.t["agents"], self.env.base.t["scalars"])

    def summary(self):
        """``{"training/agent0-length": ..., ...}`` for the keys that have met a finite value, name by name in the order
        the pool first shows them, plus ``training/steps`` and ``training/episodes``."""
        counters, count, value, _ = self._state()
        tag, Q = self.episode_type, len(_hip.LOG_MULTI_KEYS)
        out = {}
        for n, name in enumerate(self.names):
            for q, key in enumerate(_hip.LOG_MULTI_KEYS):
                if count[n * Q + q] > 0:
                    out["%s/%s-%s" % (tag, name, key)] = float(value[n * Q + q])
        out[tag + "/steps"], out[tag + "/episodes"] = counters["steps"], counters["episodes"]
        return out

    def records(self, level_names=None, first=None):
        """The rows as the reference's ``log_data`` dicts (:282-302) without ``time``: lists over the agents, and the
        ``agents`` key with their names."""
        return multi_rows_to_records(self.rows(first), self._level_names(level_names), self.names)


def multi_rows_to_records(rows, level_names, names):
    """``log_data`` of log_episode() for every row of a ``multi_row_dtype`` array, in the reference's key order; `names`:
    the log's distinct agent names, which the rows' name ids index."""
    out = []
    for r in rows:
        ag = r["agents"]
        d = {"length": [int(v) for v in ag["length"]], "reward": [float(v) for v in ag["reward"]],
             "success": [bool(v) for v in ag["success"]]}
        if r["flags"] & _hip.LOG_JOINED:
            d["side_effects"] = {"total": [float(r["side_effects"][0]), float(r["side_effects"][1])]}
        d["agents"] = [names[int(v)] if int(v) < len(names) else None for v in ag["name"]]
        d["level_name"] = level_names[int(r["level"])]
        d["reward_possible"] = [int(v) for v in ag["reward_possible"]]
        d["reward_needed"] = [int(v) for v in ag["reward_needed"]]
        out.append(d)
    return out


def rows_to_records(rows, level_names):
    """``log_data`` of log_episode() for every row of a ``ROW_DTYPE`` array: ``side_effects`` (``{"total": [agent,
    inaction]}``) only where the row has been joined."""
    out = []
    for r in rows:
        d = {"length": int(r["length"]), "reward": float(r["reward"]), "success": bool(r["success"])}
        if r["flags"] & _hip.LOG_JOINED:
            d["side_effects"] = {"total": [float(r["side_effects"][0]), float(r["side_effects"][1])]}
        d["level_name"] = level_names[int(r["level"])]
        d["reward_possible"] = int(r["reward_possible"])
        d["reward_needed"] = int(r["reward_needed"])
        out.append(d)
    return out
