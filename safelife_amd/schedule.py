"""
Level schedules on the device: which level family an env plays next, and how much of a level its exit asks for.

The reference's trainers do not cycle a fixed list of levels (training/env_factory.py):

* every task scales each level's ``min_performance`` by a ``LinearSchedule`` of the training step
  (``MinPerformanceScheduler``, :363-373: 0.001 -> 1.0 between 5e5 and 2e6 steps);
* ``append-spawn`` / ``prune-spawn`` flip a coin between two level families, the probability itself on a schedule
  (``SwitchingLevelIterator``, :155-174);
* ``curriculum-append-spawn`` and the ``asym1`` tasks pick the family by a softmax over the recent slope of performance
  (``CurricularLevelIterator``, :51-146).

``LevelSchedule`` does the same for a ``SafeLifeVectorEnv`` or a ``SafeLifeMultiAgentVectorEnv`` without a host visit per
reset.  The pool is a large
pre-generated library that stays resident, cut into *groups* (families: contiguous slot ranges).  Before every step one
kernel redraws the successor table the step kernels read (``sl_env_batch.pool_next``), after every step one kernel files the
finished episodes' performances into their group's ring, and when the exit-difficulty schedule moves one kernel rewrites
``pool_scalars[l].required_step``.  The step kernels themselves are untouched.

With several agents per env (the reference's ``asym1`` / ``curriculum-asym1`` tasks) every agent has its own required points
-- ``pool_agents[l][a].required_step``, from the agent's own points table -- and an episode files ONE record, on the step
where the env's last agent finishes: the average over the agents of reward / reward_possible (env_factory.py:91-101).

One difference to the reference, by construction: the draw is per SLOT and step, not per env.  Two envs whose episodes
end on the same slot in the same step load the same successor (their random streams still differ through the env's
``stream_salt``).  The reference's envs share one iterator queue, so neither side promises independent draws per env.

The draw's exact model (``draw_words`` / ``draw_model`` below, restated in tests/schedule_ref.py) is spelled out in
include/safelife_hip.h next to ``slhip_schedule_draw``.
"""
import ctypes as C

import numpy as np

from . import _hip
from .levels import LevelPool, available_points, initial_colors

_G64 = 0x9E3779B97F4A7C15           # splitmix64's increment
_K = 0x100000001B3                  # the counter's stride (slhip_sample_actions)
_MASK = (1 << 64) - 1
#: the counter of ``first_levels`` -- the steps' draws count up from 0 and never get here
FIRST_LEVELS_COUNTER = _MASK


class LinearSchedule(object):
    """Piecewise linear in the training step with constant ends: ``env_factory.LinearSchedule`` without its logger
    (``UnivariateSpline(t, y, k=1, s=0, ext='const')``).  Evaluated on the host, as in the reference, and in the
    arithmetic of the spline's evaluation (FITPACK, a degree-1 B-spline): in the knot interval [t0, t1) of x, with
    f = 1 / (t1 - t0), the value is y0 * (f * (t1 - x)) + y1 * (f * (x - t0)) -- ``np.interp`` differs in the last bits."""

    def __init__(self, t, y):
        self.t = [float(v) for v in np.asarray(t, np.float64).ravel()]
        self.y = [float(v) for v in np.asarray(y, np.float64).ravel()]
        if len(self.t) < 2 or len(self.t) != len(self.y) or not all(a < b for a, b in zip(self.t, self.t[1:])):
            raise ValueError("LinearSchedule needs at least two knots with increasing t and one y each")

    def __call__(self, training_steps):
        t, y = self.t, self.y
        x = min(max(float(training_steps), t[0]), t[-1])
        k = len(t) - 2                          # (x = t[-1] belongs to the last interval)
        for i in range(len(t) - 1):
            if t[i] <= x < t[i + 1]:
                k = i
                break
        f = 1.0 / (t[k + 1] - t[k])
        return y[k] * (f * (t[k + 1] - x)) + y[k + 1] * (f * (x - t[k]))


def _hash(seed, counter, i):
    """splitmix64's finalizer of seed + G64 * (counter * K + i + 1) mod 2^64; i: np.uint64 array."""
    with np.errstate(over="ignore"):
        base = np.uint64((int(counter) * _K + 1) & _MASK)
        z = np.uint64(int(seed) & _MASK) + np.uint64(_G64) * (base + i)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def draw_words(seed, counter, index):
    """The two 64-bit words of draw `index` (a slot, or a global env index) under (seed, counter)."""
    i = np.atleast_1d(np.asarray(index)).astype(np.uint64)
    with np.errstate(over="ignore"):
        return _hash(seed, counter, np.uint64(2) * i), _hash(seed, counter, np.uint64(2) * i + np.uint64(1))


def _mulhi(z, n):
    """The high 64 bits of z * n (z uint64 array, 0 < n < 2^32)."""
    n = np.uint64(n)
    lo, hi = z & np.uint64(0xFFFFFFFF), z >> np.uint64(32)
    with np.errstate(over="ignore"):
        return (hi * n + ((lo * n) >> np.uint64(32))) >> np.uint64(32)


def draw_model(groups, probs, seed, counter, index):
    """What ``slhip_schedule_draw`` writes for the slots `index` (int32 array): group g = the first with cum[g] > u * cum[-1]
    (u the top 53 bits of word 1, cum the sequential float64 running sum; none: the last group with p > 0), member =
    start[g] + (word 2 * len[g] >> 64)."""
    p = np.asarray(probs, np.float64)
    z1, z2 = draw_words(seed, counter, index)
    u = (z1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    cum = np.zeros(len(p))
    acc = 0.0
    for g in range(len(p)):
        acc = acc + float(p[g])
        cum[g] = acc
    t = u * cum[-1]
    g = (cum[None, :] > t[:, None]).argmax(axis=1)
    none = ~(cum[None, :] > t[:, None]).any(axis=1)
    g[none] = np.flatnonzero(p > 0).max()
    out = np.zeros(len(z1), np.int32)
    for k, (start, n) in enumerate(groups):
        sel = g == k
        out[sel] = start + _mulhi(z2[sel], n).astype(np.int64)
    return out


def _check_probs(p, G):
    p = np.asarray(p, np.float64).ravel()
    if len(p) != G:
        raise ValueError("one probability per group (%d), got %d" % (G, len(p)))
    if not np.isfinite(p).all() or (p < 0).any() or not p.sum() > 0:
        raise ValueError("group probabilities must be finite, non-negative and not all zero: %r" % (p.tolist(),))
    return p


class LevelSchedule(object):
    """
    pool : LevelPool            not refreshable: slots are never rewritten; ``LevelPool(levels, n_agents=A)`` for the
                                multi-agent env
    groups : [(start, len), ...] or [range, ...]
                                1..8 disjoint slot ranges of at least one slot; slots outside every group are never drawn
    mode : "uniform"            equal group probabilities (the reference's curriculum "uniform" as well)
           "switching"          two groups, probabilities ``[1 - p, p]``; ``p_switch``: a float or a callable of the training
                                step (``LinearSchedule``) -- ``SwitchingLevelIterator``
           "curriculum"         a softmax over the slope of each group's last ``lookback`` performances, computed on the
                                device -- ``CurricularLevelIterator`` (``curriculum="uniform"``: its other distribution)
    seed : int                  of the successor draws and of ``first_levels``
    min_performance_fraction : None, a float, or a callable of the training step -- ``MinPerformanceScheduler``'s factor;
                                the kernel that rewrites the pool's required points runs only when the value changed.
                                None leaves what the pool was built with.
    lookback : int              records per group the curriculum looks at (the reference: 100)

    ``training_steps`` is the argument of the callables; the driver sets it (the runners do, from their ``num_steps``).
    Attach with ``SafeLifeVectorEnv(pool, ..., level_schedule=schedule)`` or, for a pool with ``n_agents`` agents,
    ``SafeLifeMultiAgentVectorEnv(pool, ..., level_schedule=schedule)``; a schedule serves one env.

    ``available``: the points each level offers, int32 ``[L]`` -- ``[L, A]`` for a pool with A > 1 agents, every agent's own
    table against the level's counts.
    """

    MODES = ("uniform", "switching", "curriculum")

    def __init__(self, pool, groups, *, mode, seed, p_switch=None, curriculum=None, min_performance_fraction=None,
                 lookback=100):
        if not isinstance(pool, LevelPool):
            raise TypeError("pool must be a LevelPool")
        if pool.refreshable:
            raise ValueError("a level schedule and a refreshable pool both own the successor table (pool_next): "
                             "build the pool without refreshable=True")
        self.n_agents = int(pool.n_agents)
        self.pool = pool
        L = pool.n_slots
        gs = []
        for g in groups:
            if isinstance(g, range):
                if g.step != 1:
                    raise ValueError("a group is a contiguous slot range")
                g = (g.start, len(g))
            start, n = int(g[0]), int(g[1])
            if n < 1 or start < 0 or start + n > L:
                raise ValueError("group (%d, %d) is empty or reaches outside the pool's %d slots" % (start, n, L))
            gs.append((start, n))
        if not 1 <= len(gs) <= _hip.SCHEDULE_MAX_GROUPS:
            raise ValueError("1 to %d groups, got %d" % (_hip.SCHEDULE_MAX_GROUPS, len(gs)))
        order = sorted(gs)
        for (a, n), (b, _) in zip(order, order[1:]):
            if a + n > b:
                raise ValueError("groups overlap")
        self.groups = tuple(gs)
        if mode not in self.MODES:
            raise ValueError("mode must be one of %r" % (self.MODES,))
        self.mode = mode
        if mode == "switching":
            if len(gs) != 2:
                raise ValueError("switching takes exactly two groups")
            if p_switch is None:
                raise ValueError("switching needs p_switch (a probability or a callable of the training step)")
        elif p_switch is not None:
            raise ValueError("p_switch belongs to mode='switching'")
        if curriculum not in (None, "progress_estimate", "uniform") or (curriculum is not None and mode != "curriculum"):
            raise ValueError("curriculum is 'progress_estimate' or 'uniform', with mode='curriculum'")
        self.curriculum = curriculum or "progress_estimate"
        self.p_switch = p_switch
        self.min_performance_fraction = min_performance_fraction
        self.lookback = int(lookback)
        if not 2 <= self.lookback <= _hip.SCHEDULE_MAX_LOOKBACK:
            raise ValueError("lookback must lie in 2..%d" % _hip.SCHEDULE_MAX_LOOKBACK)
        self.seed = int(seed) & _MASK
        self.training_steps = 0
        # per slot: the level's own min_performance and agent 0's available points (safelife_game.py:696-709)
        self.min_performance = np.array([lv.min_performance for lv in pool.levels], np.float64)
        self.available = np.zeros(L if self.n_agents == 1 else (L, self.n_agents), np.int32)
        for k, lv in enumerate(pool.levels):
            colors = initial_colors(lv.board)
            if self.n_agents == 1:
                table = pool.points_table[pool.pool_table_idx[k]].astype(np.int64)
                self.available[k] = available_points(table, pool.initial_counts[k], colors)
                continue
            for a in range(self.n_agents):      # the agent's own table against the level's counts, as LevelPool's
                table = pool.points_table[pool.pool_agent_table_idx[k, a]].astype(np.int64)
                self.available[k, a] = available_points(table, pool.initial_counts[k], colors)
        self.env = None
        self.draws = 0
        self._fraction_sent = None

    @classmethod
    def from_pools(cls, level_lists, *, pool_args=None, **kwargs):
        """One ``LevelPool`` of several level lists laid end to end, one group per list."""
        level_lists = [list(x) for x in level_lists]
        groups, at = [], 0
        for x in level_lists:
            groups.append((at, len(x)))
            at += len(x)
        pool = LevelPool([lv for x in level_lists for lv in x], **(pool_args or {}))
        return cls(pool, groups, **kwargs)

    # ---- host side of the model

    def group_probs(self):
        """The G probabilities handed to the draw by value at the current training step (None in curriculum mode with
        the progress estimate: those live on the device)."""
        G = len(self.groups)
        if self.mode == "switching":
            p = self.p_switch(self.training_steps) if callable(self.p_switch) else self.p_switch
            p = float(p)
            if not 0.0 <= p <= 1.0:
                raise ValueError("p_switch must lie in [0, 1], got %r" % p)
            return np.array([1.0 - p, p])
        if self.mode == "uniform" or self.curriculum == "uniform":
            return np.full(G, 1.0 / G)
        return None

    def fraction(self):
        f = self.min_performance_fraction
        if f is None:
            return None
        f = float(f(self.training_steps) if callable(f) else f)
        if not np.isfinite(f):
            raise ValueError("min_performance_fraction must be finite, got %r" % f)
        return f

    def first_levels(self, num_envs, env_offset=0):
        """The envs' first slots: the draw's model on the host for the global env indices ``env_offset + e`` under the
        reserved counter, with the probabilities of training step 0 (curriculum: equal), so a switching run does not
        start spread evenly over both families."""
        p = self.group_probs()
        if p is None:
            p = np.full(len(self.groups), 1.0 / len(self.groups))
        index = int(env_offset) + np.arange(int(num_envs), dtype=np.int64)
        return draw_model(self.groups, _check_probs(p, len(self.groups)), self.seed, FIRST_LEVELS_COUNTER, index)

    def reward_possible(self, points_on_level_exit=1):
        """What the logger records as ``reward_possible`` (safelife_logger.py:286-287): ``available`` plus the exit's
        points, int32 in the shape of ``available``."""
        return (self.available.astype(np.int64) + int(points_on_level_exit)).astype(np.int32)

    # ---- device side (SafeLifeVectorEnv and SafeLifeMultiAgentVectorEnv call these)

    def _check_env(self, pool, n_agents):
        """Raises unless this schedule can serve an env on `pool` with `n_agents` agents per board (None: a
        SafeLifeVectorEnv)."""
        if n_agents is None:
            if self.n_agents > 1:
                raise ValueError("this level schedule was built on a pool with %d agents per level: it serves a "
                                 "SafeLifeMultiAgentVectorEnv, not a single-agent SafeLifeVectorEnv" % self.n_agents)
        elif int(n_agents) != self.n_agents:
            raise ValueError("this level schedule was built on a pool with %d agent%s per level and cannot serve a "
                             "multi-agent env with %d" % (self.n_agents, "" if self.n_agents == 1 else "s", n_agents))
        if pool is not self.pool:
            raise ValueError("the schedule was built for another pool")

    def _attach(self, env):
        if self.env is not None:
            raise ValueError("this LevelSchedule already serves an env")
        # a SafeLifeMultiAgentVectorEnv keeps the boards, the scalars and the pool in its single-agent base env
        multi = getattr(env, "n_agents", None) is not None
        base = env.base if multi else env
        self._check_env(env.pool, env.n_agents if multi else None)
        torch, dev = env.torch, env.device
        self.env, self._base, self._multi = env, base, multi
        G, n, L, B = len(self.groups), self.lookback, self.pool.n_slots, env.num_envs
        t = self.t = {}
        t["min_performance"] = torch.from_numpy(self.min_performance).to(dev)
        t["available"] = torch.from_numpy(self.available).to(dev)
        t["reward_possible"] = torch.from_numpy(self.reward_possible(base.struct.exit_points)).to(dev)
        t["cur_slot"] = base.t["scalars"][:, _hip.SCALAR_COLS["level_idx"]].clone()
        t["ring"] = torch.zeros((G, n), dtype=torch.float64, device=dev)
        t["count"] = torch.ones(G, dtype=torch.int64, device=dev)
        t["episodes"] = torch.zeros(G, dtype=torch.int64, device=dev)
        t["pos"] = torch.ones(G, dtype=torch.int32, device=dev)
        t["best"] = torch.zeros(G, dtype=torch.float64, device=dev)
        t["mean"] = torch.zeros(G, dtype=torch.float64, device=dev)
        t["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
        t["probs"] = torch.full((G,), 1.0 / G, dtype=torch.float64, device=dev)
        t["pool_next"] = torch.arange(L, dtype=torch.int32, device=dev)
        if multi:       # the per-agent arrays [L, A] travel in the wrapping struct (the inner two pointers stay null)
            m = self._mstruct = _hip.LevelScheduleMulti()
            m.n_agents = self.n_agents
            m.available, m.reward_possible = t["available"].data_ptr(), t["reward_possible"].data_ptr()
            m.pool_agents, m.out = env.t["pool_agents"].data_ptr(), env.t["out"].data_ptr()
            s = self.struct = m.s
            self._mref = C.byref(m)
            per_slot = ("min_performance",)
        else:
            s = self.struct = _hip.LevelSchedule()
            per_slot = ("min_performance", "available", "reward_possible")
        s.G, s.lookback, s.L = G, n, L
        for g, (start, length) in enumerate(self.groups):
            s.start[g], s.len[g] = start, length
        for name in per_slot + ("cur_slot", "ring", "count", "episodes", "pos", "best", "mean", "status"):
            setattr(s, name, t[name].data_ptr())
        self._sref = C.byref(s)
        self._lib = _hip.lib()
        # shards of one run draw different tables: the seed carries the global index of env 0, as DQNRunner's does
        self._kernel_seed = (self.seed + _G64 * int(base.env_offset)) & _MASK
        self._on_device = self.mode == "curriculum" and self.curriculum == "progress_estimate"
        self.draws = 0
        self._fraction_sent = None
        return t["pool_next"]

    def _rewind(self, mask=None):
        """After the envs (those with mask != 0) have been reset from outside the step: their episodes start over."""
        now = self._base.t["scalars"][:, _hip.SCALAR_COLS["level_idx"]]
        if mask is None:
            self.t["cur_slot"].copy_(now)
        else:
            self.t["cur_slot"].copy_(self.env.torch.where(mask != 0, now, self.t["cur_slot"]))

    def _before_step(self):
        """The successor table for the step that follows and, when the schedule moved, the required points."""
        lib, st = self._lib, _hip.current_stream_ptr()
        L = self.pool.n_slots
        f = self.fraction()
        if f is not None and f != self._fraction_sent:
            if self._multi:
                _hip.check(lib.slhip_schedule_required_multi(self._mref, f, st))
            else:
                _hip.check(lib.slhip_schedule_required(self._sref, f, _hip.ptr(self.env.t["pool_scalars"]), L, st))
            self._fraction_sent = f
        if self._on_device:
            _hip.check(lib.slhip_schedule_curriculum(self._sref, _hip.ptr(self.t["probs"]), st))
            probs = None
        else:
            p = _check_probs(self.group_probs(), len(self.groups))
            probs = (C.c_double * len(p))(*p.tolist())
        rc = lib.slhip_schedule_draw(self._sref, probs, _hip.ptr(self.t["probs"]), self._kernel_seed, self.draws,
                                     _hip.ptr(self.t["pool_next"]), L, st)
        if rc:
            _hip.check(rc)
        self.draws += 1

    def _after_step(self):
        env = self.env
        if self._multi:
            rc = self._lib.slhip_schedule_harvest_multi(self._mref, _hip.ptr(self._base.t["scalars"]), env.num_envs,
                                                        _hip.current_stream_ptr())
        else:
            rc = self._lib.slhip_schedule_harvest(self._sref, _hip.ptr(env.t["out"]), _hip.ptr(env.t["scalars"]),
                                                  env.num_envs, _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)

    _CHECKPOINT_TENSORS = ("cur_slot", "ring", "count", "episodes", "pos", "best", "mean", "status", "probs", "pool_next")

    def _checkpoint_state(self):
        """``checkpoint.py``: the rings, the successor table of the last draw, and the host's counters (``_fraction_sent``:
        the required points in the env's ``pool_scalars`` / ``pool_agents`` are the env's state)."""
        if self.env is None:
            raise ValueError("checkpoint: the level schedule is not attached to an env")
        config = dict(groups=self.groups, mode=self.mode, curriculum=self.curriculum, lookback=self.lookback, seed=self.seed,
                      n_agents=self.n_agents, n_slots=self.pool.n_slots)
        scalars = dict(training_steps=self.training_steps, draws=self.draws, _fraction_sent=self._fraction_sent)
        return config, scalars, {k: self.t[k] for k in self._CHECKPOINT_TENSORS}

    def stats(self):
        """Per group, read back now: ``episodes``, ``records`` (the ring's count, the first 0.0 included), ``best``
        (best_perf_lvl*), ``recent`` (recent<lookback>_perf_lvl*), ``probabilities`` (the device's in curriculum mode, else
        the current host values), and ``status`` (``_hip.SCHEDULE_BAD_PROBS``: a draw fell back to equal probabilities)."""
        if self.env is None:
            raise ValueError("the schedule is not attached to an env")
        t = self.t
        p = t["probs"].cpu().numpy() if self._on_device else self.group_probs()
        return {"episodes": t["episodes"].cpu().numpy(), "records": t["count"].cpu().numpy(),
                "best": t["best"].cpu().numpy(), "recent": t["mean"].cpu().numpy(), "probabilities": np.asarray(p),
                "status": int(t["status"].item())}
