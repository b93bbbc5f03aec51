"""
The episode log in plain numpy and Python floats, sharing nothing with the kernels: what include/safelife_hip.h says
slhip_episode_log_harvest / _join / _summaries / _run_summary compute, one IEEE operation at a time (a Python float is a
float64 and +, -, *, / round once each).  tests/test_episode_log_host.py holds it against what the reference's
SafeLifeLogger logged (tests/golden/episode_log_cases.npz); tests/test_episode_log_gpu.py holds the kernels against it, bit
for bit.
"""
import math

import numpy as np

ROW_DTYPE = np.dtype([("index", "<i8"), ("training_steps", "<i8"), ("prev", "<i8"), ("env", "<i4"), ("level", "<i4"),
                      ("episode_idx", "<i4"), ("length", "<i4"), ("reward", "<f4"), ("reward_possible", "<i4"),
                      ("reward_needed", "<i4"), ("success", "u1"), ("times_up", "u1"), ("flags", "u1"), ("reserved", "u1"),
                      ("reward_frac", "<f8"), ("side_effects", "<f8", (2,)), ("side_effects_frac", "<f8"), ("score", "<f8")])
KEYS = ("side_effects", "length", "reward", "success", "score")
JOINED, MAX_HOPS, MAX_KEYS, EMPTY_KEY = 1, 64, 24, 0xFFFF
NAN = float("nan")
DBL_MAX = 1.7976931348623157e308


def reward_frac(reward, reward_possible):
    return float(np.float32(reward)) / float(max(int(reward_possible), 1))


def at_least_one(x):
    """np.maximum(x, 1): a NaN stays."""
    return x if x != x else (x if x > 1.0 else 1.0)


def combined(agent, inaction, rfrac, length):
    """combined_score() :706-714 from the two totals -> (side_effects_frac, score)."""
    frac = agent / at_least_one(inaction)
    speed = 1.0 - float(int(length)) / 1000.0
    return frac, (75.0 * rfrac + 25.0 * speed) - 200.0 * frac


def nan_to_num(x):
    if x != x:
        return 0.0
    if math.isinf(x):
        return DBL_MAX if x > 0 else -DBL_MAX
    return x


def entry_totals(weights, keys, scores, n_cells):
    """One queue entry's totals: weights [(cell, weight), ...], keys [K], scores [K,2], n_cells [K]."""
    if n_cells[0] < 0:
        return [NAN, NAN]
    total = [0.0, 0.0]
    for k in range(len(keys)):
        key = int(keys[k]) & 0xFFFF
        if key == EMPTY_KEY:
            continue
        wk = 0.0
        for cell, weight in weights:
            if cell == key:
                wk = wk + float(weight)
        for j in range(2):
            s = float(scores[k][j])
            if s == s:
                total[j] = total[j] + wk * s
    return total


class LogModel(object):
    def __init__(self, B, capacity, polyak, reward_possible, weights=()):
        self.B, self.capacity, self.polyak = int(B), int(capacity), float(polyak)
        self.reward_possible = np.asarray(reward_possible, np.int32)
        self.weights = list(weights)
        self.rows = np.zeros(self.capacity, ROW_DTYPE)
        self.rows["index"] = -1
        self.n_rows = self.steps = self.episodes = self.summarised = self.unmatched = 0
        self.cur_slot, self.cur_required, self.cur_episode = (np.zeros(B, np.int32) for _ in range(3))
        self.last_row = np.full(B, -1, np.int64)
        self.value, self.count, self.weight = [0.0] * 5, [0] * 5, [0.0] * 5

    def counters(self):
        return dict(n_rows=self.n_rows, steps=self.steps, episodes=self.episodes, summarised=self.summarised,
                    unmatched=self.unmatched)

    def rewind(self, scalars, mask=None):
        """scalars: dict of int arrays [B] (level_idx, required_points, episode_idx)."""
        sel = np.ones(self.B, bool) if mask is None else np.asarray(mask) != 0
        self.cur_slot[sel] = scalars["level_idx"][sel]
        self.cur_required[sel] = scalars["required_points"][sel]
        self.cur_episode[sel] = scalars["episode_idx"][sel]
        self.last_row[sel] = -1

    def harvest(self, out, scalars):
        """out: dict of arrays [B] (done, success, times_up, episode_reward float32, episode_length) -- only the done byte
        of an env that is not done is looked at; scalars as in rewind(), after the step."""
        n = 0
        for e in range(self.B):
            if not out["done"][e]:
                continue
            idx = self.n_rows + n
            row = self.rows[idx % self.capacity]
            slot = int(self.cur_slot[e])
            rp = int(self.reward_possible[slot]) if 0 <= slot < len(self.reward_possible) else 0
            row["index"], row["training_steps"], row["prev"] = idx, self.steps + e + 1, self.last_row[e]
            row["env"], row["level"], row["episode_idx"] = e, slot, self.cur_episode[e]
            row["length"], row["reward"] = out["episode_length"][e], out["episode_reward"][e]
            row["reward_possible"], row["reward_needed"] = rp, self.cur_required[e]
            row["success"], row["times_up"] = out["success"][e], out["times_up"][e]
            row["flags"] = row["reserved"] = 0
            row["reward_frac"] = reward_frac(out["episode_reward"][e], rp)
            row["side_effects"] = NAN
            row["side_effects_frac"] = row["score"] = NAN
            self.last_row[e] = idx
            n += 1
        self.cur_slot[:] = scalars["level_idx"]
        self.cur_required[:] = scalars["required_points"]
        self.cur_episode[:] = scalars["episode_idx"]
        self.steps += self.B
        self.episodes += n
        self.n_rows += n

    def find(self, env, episode_idx):
        """The ring position of the row of (env, episode_idx) along the env's chain, or None."""
        r = int(self.last_row[env]) if 0 <= env < self.B else -1
        for _ in range(MAX_HOPS):
            if r < 0 or r >= self.n_rows or r < self.n_rows - self.capacity:
                return None
            row = self.rows[r % self.capacity]
            if row["index"] != r:
                return None
            if row["env"] == env and row["episode_idx"] == episode_idx:
                return r % self.capacity
            r = int(row["prev"])
        return None

    def apply(self, at, total):
        row = self.rows[at]
        frac, score = combined(float(total[0]), float(total[1]), float(row["reward_frac"]), row["length"])
        row["side_effects"] = total
        row["side_effects_frac"], row["score"] = frac, score
        row["flags"] |= JOINED

    def join(self, count, records, scores, keys, n_cells):
        """records: dict of int arrays [C] (env, episode_idx); scores [C,K,2], keys [C,K], n_cells [C,K]."""
        for i in range(min(max(int(count), 0), len(records["env"]))):
            at = self.find(int(records["env"][i]), int(records["episode_idx"][i]))
            if at is None:
                self.unmatched += 1
                continue
            self.apply(at, entry_totals(self.weights, keys[i], scores[i], n_cells[i]))

    def row_range(self, first):
        lo = min(max(int(first), self.n_rows - self.capacity, 0), self.n_rows)
        return self.rows[np.arange(lo, self.n_rows) % self.capacity]

    def summarise(self):
        p = self.polyak
        for row in self.row_range(self.summarised):
            vals = (float(row["side_effects_frac"]), float(int(row["length"])), float(row["reward_frac"]),
                    1.0 if row["success"] else 0.0, float(row["score"]))
            for k, v in enumerate(vals):
                if v != v or math.isinf(v):
                    continue
                w = self.weight[k]
                self.value[k] = (v + w * self.value[k]) / (1.0 + w)
                self.count[k] += 1
                self.weight[k] = p * (1.0 + w) if p < 1.0 else float(self.count[k])
        self.summarised = self.n_rows

    def summary(self, tag="training"):
        out = {"%s/%s" % (tag, key): self.value[k] for k, key in enumerate(KEYS) if self.count[k] > 0}
        out[tag + "/steps"], out[tag + "/episodes"] = self.steps, self.episodes
        return out

    def run_summary(self, first_row=0):
        """12 floats, as slhip_episode_log_run_summary lays them out."""
        cols = [[] for _ in range(6)]
        for row in self.row_range(first_row):
            frac, score = combined(nan_to_num(float(row["side_effects"][0])), nan_to_num(float(row["side_effects"][1])),
                                   float(row["reward_frac"]), row["length"])
            vals = (1.0 if row["success"] else 0.0, float(int(row["length"])), frac, float(row["reward_frac"]), score)
            for k, v in enumerate(vals):
                cols[k].append(v)
            if row["success"]:
                cols[5].append(float(int(row["length"])))
        mean, sd = [], []
        for col in cols:
            s = 0.0
            for v in col:
                s = s + v
            m = _div(s, len(col))
            q = 0.0
            for v in col:
                d = v - m
                q = q + d * d
            mean.append(m)
            sd.append(_sqrt(_div(q, len(col))))
        return np.array([float(len(cols[0])), mean[0], mean[1], mean[2], mean[3], mean[4], sd[2], sd[3], sd[4], mean[5],
                         sd[5], float(len(cols[5]))])


def _div(a, n):
    if n == 0:
        return NAN          # (0.0 / 0.0)
    return a / float(n)


def _sqrt(x):
    return NAN if x != x or x < 0 else (x if math.isinf(x) else math.sqrt(x))


def same_floats(a, b):
    """Bit for bit, except that every NaN equals every NaN (the payload and sign of a NaN an operation makes differ between
    machines)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool((nan == np.isnan(b)).all() and (a[~nan].view(np.int64) == b[~nan].view(np.int64)).all())


def assert_rows_equal(got, want):
    assert len(got) == len(want)
    for name in ROW_DTYPE.names:
        if ROW_DTYPE[name].base.kind == "f":
            assert same_floats(got[name], want[name]), name
        else:
            assert np.array_equal(got[name], want[name]), name
