#!/usr/bin/env python3
"""
Writes tests/golden/gae_cases.npz by RUNNING THE REFERENCE's PPO.gen_training_batch (training/ppo.py:74-143) on the CPU:
what slhip_training_batch and tests/gae_ref.py are held to, bit for bit.

    python tests/golden/make_golden_gae.py

Runs where make_golden.py runs (it needs the reference's Python, loaded through make_golden.import_reference()).  The
reference's trainer is driven with scripted envs and a table model:

  - env b returns the recorded reward R[t,b] (a numpy scalar of the case's dtype) and done flag D[t,b] at its t-th step,
    whatever the action; its observation is the pair (b, t) with t the number of steps it has taken in all, so every row
    of the flattened batch says which (t, b) it is;
  - the model looks V[t,b] up from the observation (V has T + 1 rows: row T is V(next_obs) of the last step) and returns
    uniform policies.

Per case (flat arrays, case i at [offsets[i], offsets[i+1]) -- v_offsets for V):
    T, B, reward_f64, gamma, lmda     the case
    R32 / R64    rewards [T,B], in the array of the case's dtype only, T * B values from r_offsets[i]
    D            done uint8 [T,B]
    V            float32 [T+1,B]
    returns, advantages, values, action_prob    float32 [T,B]: the reference's outputs, mapped back to [T,B]

Cases: T in {1, 2, 3, 20} x B in {1, 63, 64, 65, 257} x both reward dtypes; (gamma, lmda) cycles through (0.97, 0.95),
(1, 1), (0, 0), (0.5, 0.999) so that every pair meets every T, both dtypes and every B; columns 0-4 of a case (B = 1: the
one column takes them in turn, case after case) are: never done, done at every step, done only at T-1, done only at T-2
(a length-1 open tail), done only at t = 0; the others draw done with probability 0.3.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

N_ACTIONS = 9
PAIRS = ((0.97, 0.95), (1.0, 1.0), (0.0, 0.0), (0.5, 0.999))
TS, BS = (1, 2, 3, 20), (1, 63, 64, 65, 257)


def special_column(kind, T):
    d = np.zeros(T, np.uint8)
    if kind == 1:
        d[:] = 1
    elif kind == 2:
        d[T - 1] = 1
    elif kind == 3 and T >= 2:
        d[T - 2] = 1
    elif kind == 4:
        d[0] = 1
    return d


def make_cases():
    rng = np.random.default_rng(20261018)
    singles = 0                                 # cases with one column so far
    for f64 in (False, True):
        for ti, T in enumerate(TS):
            for bi, B in enumerate(BS):
                gamma, lmda = PAIRS[(ti + bi + (2 if f64 else 0)) % 4]
                if T == 20 and B == 257:        # the reference's own defaults on the largest window, both dtypes
                    gamma, lmda = PAIRS[0]
                D = (rng.random((T, B)) < 0.3).astype(np.uint8)
                for k in range(min(5, B)):
                    D[:, k] = special_column(k if B > 1 else singles % 5, T)
                R = rng.normal(0.0, 1.0, (T, B))
                R[rng.random((T, B)) < 0.2] = 0.0                  # most steps of the game score nothing
                R = R.astype(np.float64 if f64 else np.float32)
                V = rng.normal(0.0, 2.0, (T + 1, B)).astype(np.float32)
                yield dict(T=T, B=B, f64=f64, gamma=gamma, lmda=lmda, R=R, D=D, V=V)
                singles += B == 1


def run_reference(PPO, torch, case):
    T, B, R, D, V = case["T"], case["B"], case["R"], case["D"], case["V"]

    class ScriptedEnv(object):
        def __init__(self, b):
            self.b, self.t = b, 0

        def obs(self):
            return np.array([self.b, self.t], np.float32)

        def reset(self):
            return self.obs()

        def step(self, action):
            r, d = R[self.t, self.b], bool(D[self.t, self.b])
            self.t += 1
            return self.obs(), r, d, {}

    class TableModel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.unused = torch.nn.Parameter(torch.zeros(1))       # (the trainer builds an optimiser)
            self.table = torch.from_numpy(V)

        def forward(self, obs):
            b, t = obs[:, 0].to(torch.int64), obs[:, 1].to(torch.int64)
            return self.table[t, b], torch.full((obs.shape[0], N_ACTIONS), 1.0 / N_ACTIONS, dtype=torch.float32)

    envs = [ScriptedEnv(b) for b in range(B)]
    algo = PPO(TableModel(), training_envs=envs, gamma=case["gamma"], lmda=case["lmda"])
    out = algo.gen_training_batch(T)
    obs = out.obs.numpy()
    b, t = obs[:, 0].astype(np.int64), obs[:, 1].astype(np.int64)
    assert len(b) == T * B and len(set(zip(t.tolist(), b.tolist()))) == T * B and t.max() == T - 1
    got = {}
    for name in ("returns", "advantages", "values", "action_prob"):
        x = getattr(out, name)
        assert x.dtype == torch.float32
        a = np.zeros((T, B), np.float32)
        a[t, b] = x.numpy()
        got[name] = a
    assert np.array_equal(got["values"], V[:T])
    assert algo.num_steps == T * B
    return got


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    import make_golden
    make_golden.import_reference()
    import torch
    from training.ppo import PPO
    PPO.compute_device = torch.device("cpu")
    torch.set_num_threads(1)

    meta = {k: [] for k in ("T", "B", "reward_f64", "gamma", "lmda")}
    flat = {k: [] for k in ("R32", "R64", "D", "V", "returns", "advantages", "values", "action_prob")}
    offsets, r_offsets, v_offsets = [0], [], [0]
    for case in make_cases():
        got = run_reference(PPO, torch, case)
        T, B = case["T"], case["B"]
        meta["T"].append(T), meta["B"].append(B), meta["reward_f64"].append(int(case["f64"]))
        meta["gamma"].append(case["gamma"]), meta["lmda"].append(case["lmda"])
        key = "R64" if case["f64"] else "R32"
        r_offsets.append(sum(len(x) for x in flat[key]))            # where the case starts in ITS rewards array
        flat[key].append(case["R"].ravel())
        flat["D"].append(case["D"].ravel()), flat["V"].append(case["V"].ravel())
        for name in ("returns", "advantages", "values", "action_prob"):
            flat[name].append(got[name].ravel())
        offsets.append(offsets[-1] + T * B), v_offsets.append(v_offsets[-1] + (T + 1) * B)
        print("T=%2d B=%3d %s gamma=%g lmda=%g  done %.2f" % (T, B, "f64" if case["f64"] else "f32", case["gamma"],
                                                              case["lmda"], case["D"].mean()), flush=True)
    arrays = dict(T=np.array(meta["T"], np.int32), B=np.array(meta["B"], np.int32),
                  reward_f64=np.array(meta["reward_f64"], np.uint8), gamma=np.array(meta["gamma"], np.float64),
                  lmda=np.array(meta["lmda"], np.float64), n_actions=np.array(N_ACTIONS, np.int32),
                  offsets=np.array(offsets, np.int64), v_offsets=np.array(v_offsets, np.int64),
                  r_offsets=np.array(r_offsets, np.int64))
    for name, parts in flat.items():
        arrays[name] = np.concatenate(parts)
    out = os.path.join(HERE, "gae_cases.npz")
    write_npz(out, arrays)
    print("gae_cases: %d cases, %d bytes" % (len(meta["T"]), os.path.getsize(out)))


if __name__ == "__main__":
    main()
