"""
The level-schedule kernels (csrc/sl_schedule.hip, include/safelife_hip.h "level schedules") restated on the host.  numpy
and Python floats only; nothing here loads the library or imports safelife_amd.schedule.

Everything is an EXACT model -- integer arithmetic mod 2^64 in Python ints, float64 arithmetic one IEEE operation at a
time in the kernels' order -- except the ``exp`` of the curriculum's softmax, which is libm's here and the device's there.

The draw of slot s under (seed, counter), with z(i) = splitmix64's finalizer of seed + G * (counter * K + i + 1) mod 2^64:
    z1 = z(2 s), z2 = z(2 s + 1)
    u = (z1 >> 11) * 2^-53;  cum[g] = p_0 + ... + p_g summed in index order;  t = u * cum[G-1]
    g = the first group with cum[g] > t; none: the last group with p_g > 0
    pool_next[s] = start[g] + (z2 * len[g] >> 64)           (bias of the member draw: at most len / 2^64)
"""
import math

import numpy as np

G64 = 0x9E3779B97F4A7C15
K = 0x100000001B3
MASK = (1 << 64) - 1
BAD_PROBS = 1


def linear_schedule(t, y, x):
    """env_factory.LinearSchedule: piecewise linear through (t, y), constant outside -- in the arithmetic of FITPACK's
    evaluation of a degree-1 B-spline (what UnivariateSpline(k=1, s=0, ext='const') calls): with [t0, t1) the knot
    interval of x (the last one for x = t[-1]) and f = 1 / (t1 - t0), y0 * (f * (t1 - x)) + y1 * (f * (x - t0)).
    np.interp's y0 + slope * (x - t0) differs from it in the last bits."""
    t, y = [float(v) for v in t], [float(v) for v in y]
    x = min(max(float(x), t[0]), t[-1])
    k = len(t) - 2
    for i in range(len(t) - 1):
        if t[i] <= x < t[i + 1]:
            k = i
            break
    f = 1.0 / (t[k + 1] - t[k])
    return y[k] * (f * (t[k + 1] - x)) + y[k + 1] * (f * (x - t[k]))


def required_points(min_performance, fraction, available):
    """max(0, int(ceil((mp * fraction) * available))): two float64 products, rounded one after the other."""
    v = (float(min_performance) * float(fraction)) * float(int(available))
    if v != v or v <= 0.0:
        return 0
    if v >= 2.0 ** 31:                  # (the host's levels.required_points has no int32 to overflow; the device saturates)
        return 2 ** 31 - 1
    return min(int(math.ceil(v)), 2 ** 31 - 1)


def z(seed, counter, i):
    x = (int(seed) + G64 * ((int(counter) * K + int(i) + 1) & MASK)) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def device_probs(p):
    """What the draw makes of a device array: itself, or equal probabilities and the status bit when an entry is negative
    or not finite or the sum is 0 or not finite.  -> (probs, status bits)"""
    p = [float(x) for x in p]
    s = 0.0
    for x in p:
        s = s + x
    if any(not (x >= 0.0) or math.isinf(x) for x in p) or not s > 0.0 or math.isinf(s):
        return [1.0] * len(p), BAD_PROBS
    return p, 0


def draw_one(groups, probs, seed, counter, index):
    """-> (group, slot) of draw `index`"""
    z1, z2 = z(seed, counter, 2 * index), z(seed, counter, 2 * index + 1)
    u = float(z1 >> 11) * 2.0 ** -53
    cum, acc = [], 0.0
    for p in probs:
        acc = acc + float(p)
        cum.append(acc)
    t = u * cum[-1]
    g = next((k for k in range(len(cum)) if cum[k] > t), None)
    if g is None:
        g = max(k for k in range(len(cum)) if probs[k] > 0)
    start, n = groups[g]
    return g, start + ((z2 * n) >> 64)


def draw(groups, probs, seed, counter, L):
    """pool_next int32 [L] of slhip_schedule_draw."""
    return np.array([draw_one(groups, probs, seed, counter, s)[1] for s in range(L)], np.int32)


def draw_many(groups, probs, seed, counter, index):
    """draw_one for arrays of counters and indices (broadcast), in wrapping np.uint64 arithmetic: -> (group, slot) int64
    arrays.  For the statistics, which need many draws; held to draw_one by the tests."""
    counter, index = np.broadcast_arrays(np.asarray(counter, np.uint64), np.asarray(index, np.uint64))
    with np.errstate(over="ignore"):
        def zz(i):
            x = np.uint64(int(seed) & MASK) + np.uint64(G64) * (counter * np.uint64(K) + i + np.uint64(1))
            x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return x ^ (x >> np.uint64(31))
        z1, z2 = zz(np.uint64(2) * index), zz(np.uint64(2) * index + np.uint64(1))
    u = (z1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    cum, acc = [], 0.0
    for p in probs:
        acc = acc + float(p)
        cum.append(acc)
    t = u * cum[-1]
    g = np.full(t.shape, -1, np.int64)
    for k in range(len(cum) - 1, -1, -1):
        g[cum[k] > t] = k
    g[g < 0] = max(k for k in range(len(cum)) if probs[k] > 0)
    slot = np.zeros(t.shape, np.int64)
    for k, (start, n) in enumerate(groups):
        sel = g == k
        hi, lo = z2[sel] >> np.uint64(32), z2[sel] & np.uint64(0xFFFFFFFF)
        with np.errstate(over="ignore"):
            slot[sel] = start + ((hi * np.uint64(n) + ((lo * np.uint64(n)) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)
    return g, slot


def slope(y):
    """Least-squares slope of y_0 .. y_{n-1} against 0 .. n-1 in closed form, summed in index order."""
    n = float(len(y))
    xbar, sxx = (n - 1.0) / 2.0, n * (n * n - 1.0) / 12.0
    sxy = 0.0
    for i, v in enumerate(y):
        sxy = sxy + (float(i) - xbar) * float(v)
    return sxy / sxx


def softmax_of_progress(tp):
    """env_factory.py:121-127 on the G progress estimates."""
    tp = [float(x) for x in tp]
    scale = abs(tp[0])
    for x in tp[1:]:
        a = abs(x)
        if a < scale or a != a:
            scale = a
    out = []
    with np.errstate(all="ignore"):
        for x in tp:
            v = 0.0 if x < 0.0 else x
            v = float(np.float64(v) / np.float64(scale))        # (numpy: x / 0 is inf or NaN, not an exception)
            if v != v or math.isinf(v):
                v = 0.0
            out.append(v)
    mx = max(out)
    e = [math.exp(v - mx) for v in out]
    s = 0.0
    for v in e:
        s = s + v
    return [v / s for v in e]


class ScheduleModel(object):
    """The rings and counters of struct sl_level_schedule and the two kernels that move them."""

    def __init__(self, groups, lookback, reward_possible, cur_slot):
        self.groups = [(int(a), int(n)) for a, n in groups]
        self.lookback = n = int(lookback)
        G = len(self.groups)
        self.reward_possible = np.asarray(reward_possible, np.int32)
        self.cur_slot = np.array(cur_slot, np.int32)
        self.ring = np.zeros((G, n), np.float64)
        self.count = np.ones(G, np.int64)
        self.episodes = np.zeros(G, np.int64)
        self.pos = np.ones(G, np.int32)
        self.best = np.zeros(G, np.float64)
        self.mean = np.zeros(G, np.float64)

    def group_of(self, slot):
        for g, (a, n) in enumerate(self.groups):
            if a <= slot < a + n:
                return g
        return -1

    def records(self, g):
        """The ring's records, oldest first."""
        n = self.lookback
        if self.count[g] < n:
            return self.ring[g, :self.count[g]].tolist()
        p = int(self.pos[g])
        return self.ring[g, p:].tolist() + self.ring[g, :p].tolist()

    def harvest(self, done, episode_reward, level_idx):
        """slhip_schedule_harvest: done uint8 [B], episode_reward float32 [B] (sl_step_out), level_idx int32 [B]
        (sl_env_scalars after the step)."""
        touched = set()
        for e in np.flatnonzero(np.asarray(done)):
            slot = int(self.cur_slot[e])
            g = self.group_of(slot)
            if g < 0:
                continue
            with np.errstate(all="ignore"):
                perf = float(np.float64(np.float32(episode_reward[e])) / np.float64(self.reward_possible[slot]))
            if perf != perf or math.isinf(perf):
                perf = 0.0
            self.ring[g, self.pos[g]] = perf
            self.pos[g] = (self.pos[g] + 1) % self.lookback
            self.count[g] += 1
            self.episodes[g] += 1
            if perf > self.best[g]:
                self.best[g] = perf
            touched.add(g)
        for g in touched:
            rec = self.records(g)
            s = 0.0
            for v in rec:
                s = s + v
            self.mean[g] = s / float(len(rec))
        self.cur_slot[:] = np.asarray(level_idx, np.int32)

    def progress(self):
        tp = []
        for g in range(len(self.groups)):
            if self.count[g] < self.lookback:
                tp.append(0.2 / float(self.lookback))
            else:
                tp.append(10.0 * slope(self.records(g)))
        return tp

    def curriculum(self):
        """slhip_schedule_curriculum -> probabilities [G]"""
        return np.array(softmax_of_progress(self.progress()), np.float64)
