"""
DQN's replay restated in numpy, written env by env the way the reference's add_to_replay reads (training/dqn.py:110-134)
-- it shares nothing with the kernels, which keep one ring over t mod n for all envs and place pushes by a prefix sum --
plus the EXACT host models of the device sampler (slhip_replay_sample) and of the epsilon-greedy draw
(slhip_sample_actions_eps).  numpy only; nothing here loads the library.

    Replay(capacity, B, n, gamma).add(obs, actions, rewards, done, next_obs)

keeps ``ring`` (a list of capacity tuples (obs, action, float64 reward, next_obs, done) or None), ``idx`` and per env a
list of up to n window entries, newest first.  Observations are whatever the caller hands over (tags or byte rows).
"""
import os

import numpy as np

from tests import policy_ref

MASK = (1 << 64) - 1


class Replay(object):
    def __init__(self, capacity, B, n, gamma):
        self.capacity, self.B, self.n = int(capacity), int(B), int(n)
        self.G = gamma ** np.arange(1, n)               # the reference's expression: float64 [n-1]
        self.ring = [None] * self.capacity
        self.idx = 0
        self.windows = [[] for _ in range(B)]           # per env: [obs, action, float64 reward], newest first
        self.steps = 0

    def push(self, *row):
        self.ring[self.idx % self.capacity] = row
        self.idx += 1

    def add(self, obs, actions, rewards, done, next_obs):
        rewards = np.asarray(rewards)
        assert rewards.dtype in (np.dtype(np.float32), np.dtype(np.float64))
        for b in range(self.B):
            win = self.windows[b]
            r = np.float64(rewards[b])                  # float32 or float64 scalar, widened before the product
            d = bool(done[b])
            oldest = win.pop() if len(win) == self.n else None
            for k, entry in enumerate(win):             # entry k becomes slot k + 1
                entry[2] = np.float64(entry[2] + np.float64(r * self.G[k]))
            win.insert(0, [obs[b], int(actions[b]), r])
            if oldest is not None:
                self.push(oldest[0], oldest[1], oldest[2], obs[b], d)
            if d:
                for o, a, rew in win:
                    self.push(o, a, rew, next_obs[b], d)
                self.windows[b] = []
        self.steps += 1

    def __len__(self):
        return min(self.idx, self.capacity)

    def pending(self):
        return sum(len(w) for w in self.windows)

    def fill(self):
        return np.array([len(w) for w in self.windows], np.int32)

    def window_rewards(self):
        """float64 [n,B]: slot k = the step k steps back, 0 where empty."""
        out = np.zeros((self.n, self.B), np.float64)
        for b, w in enumerate(self.windows):
            for k, e in enumerate(w):
                out[k, b] = e[2]
        return out


def min_len(capacity, B, n, steps_added):
    """ReplayBuffer.min_len's bound."""
    return min(capacity, max(0, B * (steps_added - n)))


# ------------------------------------------------------------------------------------------------ the draws' models

def splitmix(seed, counter, i):
    """z of the kernels for Python ints: the splitmix64 finalizer of seed + G * (counter * K + i + 1) mod 2^64."""
    z = (seed + policy_ref.G * ((counter * policy_ref.K + i + 1) & MASK)) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sample_model(N, k, seed, counter):
    """What slhip_replay_sample writes for a ring that holds N rows: Floyd's algorithm, int64 [k].  k <= N."""
    assert 1 <= k <= N
    seed, counter = int(seed) & MASK, int(counter) & MASK
    out, seen = [], set()
    for i in range(k):
        j = N - k + i
        t = (splitmix(seed, counter, i) * (j + 1)) >> 64
        pick = j if t in seen else t
        out.append(pick)
        seen.add(pick)
    return np.array(out, np.int64)


def eps_model(qvals, epsilon, seed, counter, first_env=0):
    """What slhip_sample_actions_eps writes, row e drawing as env first_env + e: (actions int32 [B], random bool [B])."""
    q = np.asarray(qvals)
    assert q.dtype == np.float32 and q.ndim == 2
    B, A = q.shape
    seed, counter = int(seed) & MASK, int(counter) & MASK
    actions, was_random = np.zeros(B, np.int32), np.zeros(B, bool)
    greedy = np.argmax(q, axis=1)                       # first maximum; a NaN is the maximum, the first NaN wins
    for e in range(B):
        z = splitmix(seed, counter, int(first_env) + e)
        u = np.float32(z >> 40) * np.float32(2.0 ** -24)
        if float(u) < float(epsilon):
            actions[e], was_random[e] = ((z & 0xFFFFFFFF) * A) >> 32, True
        else:
            actions[e] = greedy[e]
    return actions, was_random


# ------------------------------------------------------------------------------------------------------ the fixture

_cases = None


def load_cases():
    """tests/golden/replay_cases.npz (make_golden_replay.py) as a list of dicts: n, B, T, capacity, gamma, R, D, A [T,B],
    dump_steps and ``dumps`` -- three dicts with idx, the ring's columns (obs_b, obs_t, action, reward, next_b, next_t,
    done) and the windows (fill [B]; w_reward, w_action, w_obs_t [n,B]).  Loaded once; nobody writes into it."""
    global _cases
    if _cases is None:
        out = []
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "replay_cases.npz")) as d:
            z = {k: d[k] for k in d.files}
        for i in range(len(z["n"])):
            n, B, T = int(z["n"][i]), int(z["B"][i]), int(z["T"][i])
            so, ro = int(z["step_offsets"][i]), int(z["r_offsets"][i])
            c = dict(index=i, n=n, B=B, T=T, capacity=int(z["capacity"][i]), gamma=float(z["gamma"][i]),
                     R=z["R64" if z["reward_f64"][i] else "R32"][ro:ro + T * B].reshape(T, B),
                     D=z["D"][so:so + T * B].reshape(T, B), A=z["A"][so:so + T * B].reshape(T, B),
                     dump_steps=[int(s) for s in z["dump_steps"][i]], dumps=[])
            for j in range(3):
                q = 3 * i + j
                e0, e1 = int(z["entry_offsets"][q]), int(z["entry_offsets"][q + 1])
                w0, wn0 = int(z["win_offsets"][q]), int(z["winn_offsets"][q])
                dump = dict(idx=int(z["idx"][q]), fill=z["w_fill"][w0:w0 + B].astype(np.int32))
                for name in ("obs_b", "obs_t", "action", "reward", "next_b", "next_t", "done"):
                    dump[name] = z["e_" + name][e0:e1]
                for name in ("w_reward", "w_action", "w_obs_t"):
                    dump[name] = z[name][wn0:wn0 + n * B].reshape(n, B)
                c["dumps"].append(dump)
            for a in [c["R"], c["D"], c["A"]] + [v for dmp in c["dumps"] for v in dmp.values() if isinstance(v, np.ndarray)]:
                a.setflags(write=False)
            c["id"] = "n%d-T%d-B%d-%s-g%g-cap%d" % (n, T, B, c["R"].dtype.name, c["gamma"], c["capacity"])
            out.append(c)
        _cases = out
    return _cases


def replay_case(case, make_obs=None):
    """Feed a golden case's step stream to ``Replay``; yields (steps done, Replay) after every step.  Observations are the
    tags (b, t) unless ``make_obs(b, t)`` builds something else."""
    n, B, T = case["n"], case["B"], case["T"]
    make_obs = make_obs or (lambda b, t: (b, t))
    rep = Replay(case["capacity"], B, n, case["gamma"])
    for t in range(T):
        obs = [make_obs(b, t) for b in range(B)]
        nxt = [make_obs(b, t + 1) for b in range(B)]
        rep.add(obs, case["A"][t], case["R"][t], case["D"][t], nxt)
        yield t + 1, rep


def ring_columns(rep, tag=lambda o: o):
    """The ring of a tag-fed ``Replay`` as the fixture's columns (slots [0, len))."""
    rows = rep.ring[:len(rep)]
    cols = dict(obs_b=np.array([tag(r[0])[0] for r in rows], np.int16), obs_t=np.array([tag(r[0])[1] for r in rows], np.int16),
                action=np.array([r[1] for r in rows], np.int32), reward=np.array([r[2] for r in rows], np.float64),
                next_b=np.array([tag(r[3])[0] for r in rows], np.int16),
                next_t=np.array([tag(r[3])[1] for r in rows], np.int16), done=np.array([r[4] for r in rows], np.uint8))
    return cols
