"""
The multi-agent episode log in plain numpy and Python floats, sharing nothing with the kernels: what include/safelife_hip.h
says slhip_episode_log_harvest_multi / _join_multi / _summaries_multi / _run_summary_multi compute, one IEEE operation at a
time.  tests/test_episode_log_multi_host.py holds it against what the reference's SafeLifeLogger logged for multi-agent
episodes (tests/golden/episode_log_multi_cases.npz); tests/test_episode_log_multi_gpu.py holds the kernels against it, bit for
bit.  The scalar helpers are those of tests/episode_log_ref.py.
"""
import math

import numpy as np

from tests.episode_log_ref import JOINED, MAX_HOPS, NAN, _div, _sqrt, at_least_one, entry_totals, nan_to_num, same_floats

QUANTITIES = ("length", "reward", "success", "score")
MAX_NAMES, NO_NAME, MAX_AGENTS = 16, 0xFF, 8


def row_dtype(n_agents):
    agent = np.dtype([("length", "<i4"), ("reward", "<f4"), ("reward_possible", "<i4"), ("reward_needed", "<i4"),
                      ("success", "u1"), ("times_up", "u1"), ("name", "u1"), ("reserved", "u1", (5,)),
                      ("reward_frac", "<f8"), ("score", "<f8")])
    return np.dtype([("index", "<i8"), ("training_steps", "<i8"), ("prev", "<i8"), ("env", "<i4"), ("level", "<i4"),
                     ("episode_idx", "<i4"), ("flags", "u1"), ("n_agents", "u1"), ("reserved", "u1", (2,)),
                     ("side_effects", "<f8", (2,)), ("side_effects_frac", "<f8"), ("agents", agent, (int(n_agents),))])


def agent_score(rfrac, length, frac):
    """combined_score() :711-714 for one agent, given the row's side-effect fraction."""
    speed = 1.0 - float(int(length)) / 1000.0
    return (75.0 * rfrac + 25.0 * speed) - 200.0 * frac


class MultiLogModel(object):
    """reward_possible int [L, A]; name_id int [L, A] in 0 .. n_names-1."""

    def __init__(self, B, A, capacity, polyak, reward_possible, name_id, n_names, weights=()):
        self.B, self.A, self.capacity, self.polyak = int(B), int(A), int(capacity), float(polyak)
        self.reward_possible = np.asarray(reward_possible, np.int32).reshape(-1, self.A)
        self.name_id = np.asarray(name_id, np.uint8).reshape(-1, self.A)
        self.n_names = int(n_names)
        self.weights = list(weights)
        self.rows = np.zeros(self.capacity, row_dtype(self.A))
        self.rows["index"] = -1
        self.n_rows = self.steps = self.episodes = self.summarised = self.unmatched = 0
        self.cur_slot, self.cur_episode = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self.cur_required = np.zeros((B, self.A), np.int32)
        self.last_row = np.full(B, -1, np.int64)
        n = MAX_NAMES * len(QUANTITIES)
        self.value, self.count, self.weight = [0.0] * n, [0] * n, [0.0] * n

    def counters(self):
        return dict(n_rows=self.n_rows, steps=self.steps, episodes=self.episodes, summarised=self.summarised,
                    unmatched=self.unmatched)

    def rewind(self, scalars, mask=None):
        """scalars: level_idx, episode_idx int [B]; required_points int [B, A] (the agents' states)."""
        sel = np.ones(self.B, bool) if mask is None else np.asarray(mask) != 0
        self.cur_slot[sel] = scalars["level_idx"][sel]
        self.cur_required[sel] = scalars["required_points"][sel]
        self.cur_episode[sel] = scalars["episode_idx"][sel]
        self.last_row[sel] = -1

    def harvest(self, out, scalars):
        """out: arrays [B, A] (done, success, times_up, episode_reward float32, episode_length); of an env that has not
        finished only the done bytes are looked at.  scalars as in rewind(), after the step."""
        # the finished envs in ascending order, all at once (a batch has up to 16385 envs): row n_rows + rank
        fin = np.flatnonzero((np.asarray(out["done"]) != 0).all(axis=1))
        n = len(fin)
        idx = self.n_rows + np.arange(n, dtype=np.int64)
        pos = idx % self.capacity                       # (capacity >= B: distinct)
        slot = self.cur_slot[fin]
        known = (slot >= 0) & (slot < len(self.reward_possible))
        safe = np.where(known, slot, 0)
        rp = np.where(known[:, None], self.reward_possible[safe], 0).astype(np.int32)
        rows, ag = self.rows, self.rows["agents"]
        rows["index"][pos], rows["training_steps"][pos], rows["prev"][pos] = idx, self.steps + fin + 1, self.last_row[fin]
        rows["env"][pos], rows["level"][pos], rows["episode_idx"][pos] = fin, slot, self.cur_episode[fin]
        rows["flags"][pos], rows["n_agents"][pos], rows["reserved"][pos] = 0, self.A, 0
        rows["side_effects"][pos], rows["side_effects_frac"][pos] = NAN, NAN
        reward = np.asarray(out["episode_reward"], np.float32)[fin]
        ag["length"][pos], ag["reward"][pos] = np.asarray(out["episode_length"])[fin], reward
        ag["reward_possible"][pos], ag["reward_needed"][pos] = rp, self.cur_required[fin]
        ag["success"][pos], ag["times_up"][pos] = np.asarray(out["success"])[fin], np.asarray(out["times_up"])[fin]
        ag["name"][pos] = np.where(known[:, None], self.name_id[safe], NO_NAME)
        ag["reserved"][pos] = 0
        ag["reward_frac"][pos] = reward.astype(np.float64) / np.maximum(rp, 1).astype(np.float64)   # (one IEEE division each)
        ag["score"][pos] = NAN
        self.last_row[fin] = idx
        self.cur_slot[:] = scalars["level_idx"]
        self.cur_required[:] = scalars["required_points"]
        self.cur_episode[:] = scalars["episode_idx"]
        self.steps += self.B
        self.episodes += n
        self.n_rows += n

    def find(self, env, episode_idx):
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
        frac = float(total[0]) / at_least_one(float(total[1]))
        row["side_effects"] = total
        row["side_effects_frac"] = frac
        for a in range(self.A):
            g = row["agents"][a]
            g["score"] = agent_score(float(g["reward_frac"]), g["length"], frac)
        row["flags"] |= JOINED

    def join(self, count, records, scores, keys, n_cells):
        for i in range(min(max(int(count), 0), len(records["env"]))):
            at = self.find(int(records["env"][i]), int(records["episode_idx"][i]))
            if at is None:
                self.unmatched += 1
                continue
            self.apply(at, entry_totals(self.weights, keys[i], scores[i], n_cells[i]))

    def row_range(self, first):
        lo = min(max(int(first), self.n_rows - self.capacity, 0), self.n_rows)
        return self.rows[np.arange(lo, self.n_rows) % self.capacity]

    def fold(self, row):
        """log_scalars() for one row: per name the LAST agent that carries it, then the four quantities."""
        p, Q = self.polyak, len(QUANTITIES)
        last = {}
        for a in range(self.A):
            last[int(row["agents"][a]["name"])] = a
        for name in range(self.n_names):
            if name not in last:
                continue
            g = row["agents"][last[name]]
            vals = (float(int(g["length"])), float(g["reward_frac"]), 1.0 if g["success"] else 0.0, float(g["score"]))
            for q, v in enumerate(vals):
                if v != v or math.isinf(v):
                    continue
                k = name * Q + q
                w = self.weight[k]
                self.value[k] = (v + w * self.value[k]) / (1.0 + w)
                self.count[k] += 1
                self.weight[k] = p * (1.0 + w) if p < 1.0 else float(self.count[k])

    def summarise(self):
        for row in self.row_range(self.summarised):
            self.fold(row)
        self.summarised = self.n_rows

    def summary(self, names, tag="training"):
        Q = len(QUANTITIES)
        out = {}
        for n, name in enumerate(names):
            for q, key in enumerate(QUANTITIES):
                if self.count[n * Q + q] > 0:
                    out["%s/%s-%s" % (tag, name, key)] = self.value[n * Q + q]
        out[tag + "/steps"], out[tag + "/episodes"] = self.steps, self.episodes
        return out

    def run_summary(self, first_row=0):
        """12 floats, as slhip_episode_log_run_summary_multi lays them out."""
        cols = [[] for _ in range(6)]       # success, length, side_effects_frac (per row), reward_frac, score, successful length
        for row in self.row_range(first_row):
            frac = nan_to_num(float(row["side_effects"][0])) / at_least_one(nan_to_num(float(row["side_effects"][1])))
            cols[2].append(frac)
            for a in range(self.A):
                g = row["agents"][a]
                cols[0].append(1.0 if g["success"] else 0.0)
                cols[1].append(float(int(g["length"])))
                cols[3].append(float(g["reward_frac"]))
                cols[4].append(agent_score(float(g["reward_frac"]), g["length"], frac))
                if g["success"]:
                    cols[5].append(float(int(g["length"])))
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
        return np.array([float(len(cols[2])), mean[0], mean[1], mean[2], mean[3], mean[4], sd[2], sd[3], sd[4], mean[5],
                         sd[5], float(len(cols[5]))])


def assert_rows_equal(got, want):
    """Every field bit for bit (a NaN equals a NaN), the agents' fields included."""
    assert len(got) == len(want) and got.dtype == want.dtype

    def walk(a, b, where):
        for name in a.dtype.names:
            x, y = a[name], b[name]
            if x.dtype.names:
                walk(x, y, where + name + ".")
            elif x.dtype.kind == "f" and x.dtype.itemsize == 8:
                assert same_floats(x, y), where + name
            elif x.dtype.kind == "f":
                assert np.array_equal(x.view(np.int32), y.view(np.int32)), where + name
            else:
                assert np.array_equal(x, y), where + name

    walk(got, want, "")
