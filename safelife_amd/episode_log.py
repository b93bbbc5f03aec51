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

Single-agent ``SafeLifeVectorEnv`` only.  NOT done: multi-agent logging -- per-agent arrays, a log entry when all agents are
done, and the ``name-`` prefixed keys.
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
_ROW_WORDS = ROW_DTYPE.itemsize // 8
_DEFAULT_POLYAK = {"training": 0.99}
RUN_SUMMARY_FIELDS = ("rows", "success", "avg_length", "side_effects", "reward", "score", "side_effects_std", "reward_std",
                      "score_std", "successful_length", "successful_length_std", "successes")


class EpisodeLog(object):
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

    def __init__(self, pool, num_envs, capacity, episode_type="training", summary_polyak=None, side_effect_weights=None):
        if not isinstance(pool, LevelPool):
            raise TypeError("pool must be a LevelPool")
        if int(pool.n_agents) > 1:
            raise ValueError("the episode log serves a single-agent SafeLifeVectorEnv: this pool has %d agents per level "
                             "(multi-agent logging is not done)" % pool.n_agents)
        self.pool = pool
        self.num_envs, self.capacity = int(num_envs), int(capacity)
        if self.num_envs < 1:
            raise ValueError("num_envs must be at least 1")
        if self.capacity < self.num_envs:
            raise ValueError("capacity (%d) must be at least num_envs (%d): one step can end every env's episode"
                             % (self.capacity, self.num_envs))
        self.episode_type = str(episode_type)
        p = _DEFAULT_POLYAK.get(self.episode_type, 1.0) if summary_polyak is None else float(summary_polyak)
        if not (np.isfinite(p) and p >= 0.0):
            raise ValueError("summary_polyak must be finite and not negative, got %r" % (summary_polyak,))
        self.summary_polyak = p
        from .side_effects import name_to_cell
        self.side_effect_weights = dict(side_effect_weights or {})
        if len(self.side_effect_weights) > _hip.SL_SE_MAX_KEYS:
            raise ValueError("at most %d side-effect weights, got %d" % (_hip.SL_SE_MAX_KEYS, len(self.side_effect_weights)))
        w = self._weights = _hip.LogWeights()
        w.n = len(self.side_effect_weights)
        for j, (name, weight) in enumerate(self.side_effect_weights.items()):
            w.cell[j], w.weight[j] = name_to_cell(name), float(weight)
        # per slot: agent 0's available points (safelife_game.py:696-709), as LevelSchedule computes them
        self.available = np.zeros(pool.n_slots, np.int32)
        for k, lv in enumerate(pool.levels):
            table = pool.points_table[pool.pool_table_idx[k]].astype(np.int64)
            self.available[k] = available_points(table, pool.initial_counts[k], initial_colors(lv.board))
        self.env = None
        self.t = None

    def reward_possible(self, points_on_level_exit=1):
        """What the logger records as ``reward_possible`` (:286-287), int32 [L]."""
        return (self.available.astype(np.int64) + int(points_on_level_exit)).astype(np.int32)

    # ---- device side

    def allocate(self, torch, device, points_on_level_exit=1):
        """The device state (``SafeLifeVectorEnv`` calls this through ``_attach``; a caller with step records of its own
        calls it and ``harvest()`` itself)."""
        B, cap, dev = self.num_envs, self.capacity, device
        self.torch = torch
        t = self.t = {}
        t["rows"] = torch.zeros((cap, _ROW_WORDS), dtype=torch.int64, device=dev)
        t["rows"][:, 0] = -1                        # (no row's index)
        # counters | counts | values | weights in one buffer: summary() is one host visit
        t["state"] = torch.zeros(20, dtype=torch.int64, device=dev)
        t["counters"], t["count"] = t["state"][0:5], t["state"][5:10]
        t["value"], t["weight"] = t["state"][10:15].view(torch.float64), t["state"][15:20].view(torch.float64)
        t["cur_slot"] = torch.zeros(B, dtype=torch.int32, device=dev)
        t["cur_required"] = torch.zeros(B, dtype=torch.int32, device=dev)
        t["cur_episode"] = torch.zeros(B, dtype=torch.int32, device=dev)
        t["last_row"] = torch.full((B,), -1, dtype=torch.int64, device=dev)
        t["reward_possible"] = torch.from_numpy(self.reward_possible(points_on_level_exit)).to(dev)
        t["run_summary"] = torch.zeros(_hip.LOG_RUN_SUMMARY, dtype=torch.float64, device=dev)
        s = self.struct = _hip.EpisodeLog()
        s.capacity, s.B, s.L, s.polyak = cap, B, self.pool.n_slots, self.summary_polyak
        for name in ("rows", "counters", "cur_slot", "cur_required", "cur_episode", "last_row", "reward_possible", "value",
                     "count", "weight"):
            setattr(s, name, t[name].data_ptr())
        self._sref = C.byref(s)
        self._lib = _hip.lib()
        return t

    def _attach(self, env):
        if self.env is not None:
            raise ValueError("this EpisodeLog already serves an env")
        if env.pool is not self.pool:
            raise ValueError("the episode log was built for another pool")
        if env.num_envs != self.num_envs:
            raise ValueError("the episode log was built for %d envs, the env has %d" % (self.num_envs, env.num_envs))
        self.allocate(env.torch, env.device, env.struct.exit_points)
        self.env = env
        self._rewind()

    def _rewind(self, mask=None):
        """After the envs (those with mask != 0) have been reset from outside the step: their episodes start over."""
        sc, cols, t, torch = self.env.t["scalars"], _hip.SCALAR_COLS, self.t, self.torch
        for name, col in (("cur_slot", "level_idx"), ("cur_required", "required_points"), ("cur_episode", "episode_idx")):
            now = sc[:, cols[col]]
            t[name].copy_(now if mask is None else torch.where(mask != 0, now, t[name]))
        if mask is None:
            t["last_row"].fill_(-1)
        else:
            t["last_row"].masked_fill_(mask != 0, -1)

    def harvest(self, out, scalars):
        """One launch on the current stream: rows for the envs whose record in `out` (int32 [B,4], ``struct sl_step_out``)
        says done; `scalars` int32 [B,16] as the step left them."""
        rc = self._lib.slhip_episode_log_harvest(self._sref, _hip.ptr(out), _hip.ptr(scalars), self.num_envs,
                                                 _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)

    def _after_step(self):
        self.harvest(self.env.t["out"], self.env.t["scalars"])

    def join(self, count, records, scores, keys, n_cells):
        """The join of one flushed queue (device tensors: count int32 [1], records int32 [C,8], scores float64 [C,K,2], keys
        [C,K] 16-bit, n_cells int32 [C,K]) on the current stream."""
        q = _hip.EpisodeQueue()
        q.capacity, q.env_base = int(records.shape[0]), 0
        q.count, q.records = count.data_ptr(), records.data_ptr()
        _hip.check(self._lib.slhip_episode_log_join(self._sref, C.byref(q), _hip.ptr(scores), _hip.ptr(keys), _hip.ptr(n_cells),
                                                    C.byref(self._weights), _hip.current_stream_ptr()))

    def summarise(self):
        """Folds the rows not yet consumed into the running summaries, on the current stream."""
        _hip.check(self._lib.slhip_episode_log_summaries(self._sref, _hip.current_stream_ptr()))

    def flush(self):
        """On the caller's stream: with a side-effect queue on the env, ``side_effects_flush()``, ``scores_all()`` and the
        join; then the summaries.  Returns the ``SideEffectBatch`` or None.  Without a queue ``side_effects`` and ``score``
        simply never count."""
        env, batch = self.env, None
        if env is None:
            raise ValueError("the episode log is not attached to an env")
        if env._se is not None:
            batch = env.side_effects_flush()
            emd = batch.scores_all()
            self.join(batch.count, batch.rec_tensor, emd["scores"], batch.keys, emd["n_cells"])
        self.summarise()
        return batch

    # ---- host side: each of these is one visit

    def _state(self):
        if self.t is None:
            raise ValueError("the episode log has no device state yet: hand it to SafeLifeVectorEnv(episode_log=...)")
        raw = self.t["state"].cpu().numpy()
        return (dict(zip(_hip.LOG_COUNTERS, raw[0:5].tolist())), raw[5:10].copy(), raw[10:15].copy().view(np.float64),
                raw[15:20].copy().view(np.float64))

    def counters(self):
        """``n_rows``, ``steps``, ``episodes``, ``summarised``, ``unmatched``."""
        return self._state()[0]

    def summary(self):
        """``{"training/length": ..., ...}`` for the keys that have met a finite value, plus ``training/steps`` and
        ``training/episodes`` (``summary_stats`` and ``cumulative_stats`` as log_scalars keys them)."""
        counters, count, value, _ = self._state()
        tag = self.episode_type
        out = {"%s/%s" % (tag, key): float(value[k]) for k, key in enumerate(_hip.LOG_KEYS) if count[k] > 0}
        out[tag + "/steps"], out[tag + "/episodes"] = counters["steps"], counters["episodes"]
        return out

    def rows(self, first=None):
        """The rows [max(first, n_rows - capacity), n_rows) in row order: a numpy record array of ``ROW_DTYPE``."""
        n_rows = self.counters()["n_rows"]
        lo = max(0 if first is None else int(first), n_rows - self.capacity, 0)
        ring = self.t["rows"].cpu().numpy().view(ROW_DTYPE).reshape(-1)
        return ring[np.arange(lo, max(n_rows, lo)) % self.capacity]

    def records(self, level_names=None, first=None):
        """The rows as the reference's ``log_data`` dicts (:282-302) without ``time``, for whoever writes the JSON log.
        ``level_names``: one title per pool slot (default: the pool's levels' names, where they have one)."""
        if level_names is None:
            level_names = [getattr(lv, "name", None) or "level-%d" % k for k, lv in enumerate(self.pool.levels)]
        return rows_to_records(self.rows(first), level_names)

    def run_summary(self, first_row=0):
        """``summarize_run_file`` over the rows [max(first_row, n_rows - capacity), n_rows): its five means (``success``,
        ``avg_length``, ``side_effects``, ``reward``, ``score``), the printed standard deviations, the successful length
        and the row count."""
        out = self.t["run_summary"]
        _hip.check(self._lib.slhip_episode_log_run_summary(self._sref, int(first_row), _hip.ptr(out),
                                                           _hip.current_stream_ptr()))
        vals = out.cpu().numpy()
        res = dict(zip(RUN_SUMMARY_FIELDS, vals.tolist()))
        res["rows"], res["successes"] = int(vals[0]), int(vals[11])
        return res


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
