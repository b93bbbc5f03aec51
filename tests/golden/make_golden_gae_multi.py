#!/usr/bin/env python3
"""
Writes tests/golden/gae_multi_cases.npz by RUNNING THE REFERENCE's PPO.gen_training_batch (training/ppo.py:74-143 over
training/base_algo.py:152-244) on the CPU with multi-agent envs, TWICE in a row per case -- the second window starts with
whoever was gone at the end of the first: what slhip_training_batch_multi and tests/gae_multi_ref.py are held to, bit for
bit.

    python tests/golden/make_golden_gae_multi.py

Runs where make_golden_gae.py runs.  The reference's trainer is driven with scripted envs (single_agent = False) and a
table model:

  - env b has A agents.  At its t-th step (t counts all its steps, over both windows) agent a leaves if F[t,b,a] is set
    and it is still there; from then on its done flag stays 1.  reset() -- which the reference calls once all agents are
    done -- brings everybody back.  Rewards are R[t,b,:], an array of the case's dtype; the observation of agent a is
    (b, a, t), so every row of the flattened batch says which (t, b, a) it is;
  - the model looks V[t,b,a] up from the observation (V has 2T + 1 rows) and returns uniform policies.

Per case (flat arrays; case i at [offsets[i], offsets[i+1]), its rewards from r_offsets[i] in the array of ITS dtype, its
bootstrap values from b_offsets[i]):
    T, B, A, reward_f64, gamma, lmda     the case
    R32 / R64    rewards [2,T,B,A] as the envs returned them
    D            uint8 [2,T,B,A]: the done flags the envs returned (1 for an agent that is gone)
    V_boot       float32 [2,B,A]: V rows T and 2T, what the model says about the observation after each window
    valid        uint8 [2,T,B,A]: 1 where the reference's batch has a row
    returns, advantages, values, action_prob    float32 [2,T,B,A]: the reference's outputs, 0 where valid is 0

Cases: T in {1, 2, 3, 20} x A in {1, 2, 3, 8} x both reward dtypes with B such that B * A takes the values 1..3, 63, 64,
65 and 255..258 (SMALL and WIDE below: the widest windows are not crossed with everything, to stay below 1 MiB; A = 8 at B * A =
256 is left out first); the (gamma, lmda) cycle of make_golden_gae.py.  Scripted envs of a case with A >= 2 (B = 1: env 3's
script): env 0 -- agent 0 never leaves, agent 1 leaves at t = 0 and stays away for both windows; env 1 -- all agents leave
together at T // 2; env 2 -- agent 1 leaves at T-2, everybody else at T-1, so the env resets exactly at the end of window
1; env 3 -- agent 0 leaves at t = 0, the others at t = 1.  Everything else leaves with a probability per step that depends
on A.  With A = 1 the five scripted columns of make_golden_gae.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_gae import N_ACTIONS, PAIRS, special_column, write_npz  # noqa: E402

LEAVE_P = {1: 0.3, 2: 0.2, 3: 0.25, 8: 0.45}
SMALL = {1: (1, 2, 3, 65), 2: (1, 32), 3: (1, 21), 8: (1, 8)}          # every T, both dtypes
# (T, A, B, float64 rewards): B * A of 255 .. 258
WIDE = ((1, 1, 257, False), (2, 1, 257, True), (3, 1, 257, False), (1, 2, 128, True), (2, 2, 129, False),
        (3, 2, 128, False), (3, 2, 129, True), (1, 3, 85, False), (2, 3, 86, True), (3, 3, 85, True), (3, 3, 86, False),
        (20, 3, 86, False), (20, 2, 128, True))


def case_list():
    out = []
    for f64 in (False, True):
        for T in (1, 2, 3, 20):
            for A in (1, 2, 3, 8):
                for B in SMALL[A]:
                    out.append((T, A, B, f64))
    return out + list(WIDE)


def script(F, T, A, kind):
    """Window 1 of one env's leaving flags F [2T, A]."""
    if kind == 0:
        F[:, 0] = 0
        F[:, 1] = 0
        F[0, 1] = 1
    elif kind == 1:
        F[:T] = 0
        F[T // 2] = 1
    elif kind == 2:
        F[:T] = 0
        F[T - 1] = 1
        if T >= 2:
            F[T - 1, 1], F[T - 2, 1] = 0, 1
    elif kind == 3:
        F[0], F[0, 0] = 0, 1
        if T >= 2:
            F[1], F[1, 1:] = 0, 1


def make_cases():
    rng = np.random.default_rng(20261019)
    singles = 0
    for i, (T, A, B, f64) in enumerate(case_list()):
        gamma, lmda = PAIRS[i % 4]
        if T == 20 and B * A >= 255:
            gamma, lmda = PAIRS[0]
        F = (rng.random((2 * T, B, A)) < LEAVE_P[A]).astype(np.uint8)
        if A == 1:
            for k in range(min(5, B)):
                F[:T, k, 0] = special_column(k if B > 1 else singles % 5, T)
            singles += B == 1
        elif B == 1:
            script(F[:, 0], T, A, 3)
        else:
            for k in range(min(4, B)):
                script(F[:, k], T, A, k)
        R = rng.normal(0.0, 1.0, (2 * T, B, A))
        R[rng.random((2 * T, B, A)) < 0.2] = 0.0
        R = R.astype(np.float64 if f64 else np.float32)
        V = rng.normal(0.0, 2.0, (2 * T + 1, B, A)).astype(np.float32)
        yield dict(T=T, B=B, A=A, f64=f64, gamma=gamma, lmda=lmda, F=F, R=R, V=V)


def run_reference(PPO, torch, case):
    T, B, A, F, R, V = case["T"], case["B"], case["A"], case["F"], case["R"], case["V"]
    D = np.zeros((2 * T, B, A), np.uint8)
    resets_at = []

    class ScriptedEnv(object):
        single_agent = False

        def __init__(self, b):
            self.b, self.t, self.gone = b, 0, np.zeros(A, bool)

        def obs(self):
            return np.array([[self.b, a, self.t] for a in range(A)], np.float32)

        def reset(self):
            if self.t:
                resets_at.append((self.t - 1, self.b))
            self.gone[:] = False
            return self.obs()

        def step(self, actions):
            actions = np.asarray(actions)
            assert actions.shape == (A,) and not actions[self.gone].any()       # a gone agent is handed 0
            self.gone = self.gone | (F[self.t, self.b] != 0)
            D[self.t, self.b] = self.gone
            r = R[self.t, self.b].copy()
            self.t += 1
            return self.obs(), r, self.gone.copy(), {}

    class TableModel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.unused = torch.nn.Parameter(torch.zeros(1))
            self.table = torch.from_numpy(V)

        def forward(self, obs):
            b, a, t = (obs[:, k].to(torch.int64) for k in range(3))
            return self.table[t, b, a], torch.full((obs.shape[0], N_ACTIONS), 1.0 / N_ACTIONS, dtype=torch.float32)

    envs = [ScriptedEnv(b) for b in range(B)]
    algo = PPO(TableModel(), training_envs=envs, gamma=case["gamma"], lmda=case["lmda"])
    got = {name: np.zeros((2, T, B, A), np.float32) for name in ("returns", "advantages", "values", "action_prob")}
    valid = np.zeros((2, T, B, A), np.uint8)
    for w in range(2):
        out = algo.gen_training_batch(T)
        obs = out.obs.numpy().astype(np.int64)
        b, a, t = obs[:, 0], obs[:, 1], obs[:, 2] - w * T
        assert t.min() >= 0 and t.max() <= T - 1 and len(set(zip(t.tolist(), b.tolist(), a.tolist()))) == len(t)
        valid[w, t, b, a] = 1
        for name in got:
            x = getattr(out, name)
            assert x.dtype == torch.float32
            got[name][w, t, b, a] = x.numpy()
    assert np.array_equal(got["values"], np.where(valid != 0, V[:2 * T].reshape(2, T, B, A), np.float32(0)))
    got["valid"], got["D"] = valid, D.reshape(2, T, B, A)
    mid = [t for t, b in resets_at if t % T != T - 1]
    return got, len(mid)


def main():
    import make_golden
    make_golden.import_reference()
    import torch
    from training.ppo import PPO
    PPO.compute_device = torch.device("cpu")
    torch.set_num_threads(1)

    meta = {k: [] for k in ("T", "B", "A", "reward_f64", "gamma", "lmda")}
    flat = {k: [] for k in ("R32", "R64", "D", "V_boot", "valid", "returns", "advantages", "values", "action_prob")}
    offsets, r_offsets, b_offsets = [0], [], [0]
    for case in make_cases():
        got, mid_resets = run_reference(PPO, torch, case)
        T, B, A = case["T"], case["B"], case["A"]
        inactive = int((got["valid"] == 0).sum())
        # what a test could otherwise pass without: gaps, and envs that reload inside a window
        if A >= 2 and T >= 3:
            assert inactive > 0 and mid_resets > 0, (T, B, A)
        if A == 1:
            assert inactive == 0
        if A >= 2 and B >= 4:
            v = got["valid"]
            assert v[:, :, 0, 0].all() and v[:, :, 0, 1].sum() == 1 and v[0, 0, 0, 1]   # env 0: never leaves / gone at once
            assert got["D"][0, T - 1, 2].all() and v[1, 0, 2].all()                     # env 2 reloads at the end of window 1
        for k in ("T", "B", "A"):
            meta[k].append(case[k])
        meta["reward_f64"].append(int(case["f64"])), meta["gamma"].append(case["gamma"]), meta["lmda"].append(case["lmda"])
        key = "R64" if case["f64"] else "R32"
        r_offsets.append(sum(len(x) for x in flat[key]))
        # (rewards of rows the reference never saw are zeroed: they carry no information, and zeros pack well)
        flat[key].append(np.where(got["valid"] != 0, case["R"].reshape(2, T, B, A), 0).astype(case["R"].dtype).ravel())
        flat["V_boot"].append(case["V"][[T, 2 * T]].ravel())
        for name in ("D", "valid", "returns", "advantages", "values", "action_prob"):
            flat[name].append(got[name].ravel())
        offsets.append(offsets[-1] + 2 * T * B * A), b_offsets.append(b_offsets[-1] + 2 * B * A)
        print("T=%2d B=%3d A=%d %s gamma=%g lmda=%g  inactive %.2f  mid-window resets %d"
              % (T, B, A, "f64" if case["f64"] else "f32", case["gamma"], case["lmda"],
                 inactive / got["valid"].size, mid_resets), flush=True)
    valid = np.concatenate(flat["valid"])
    frac = 1.0 - valid.mean()
    assert 0.15 <= frac <= 0.60, frac
    arrays = dict(T=np.array(meta["T"], np.int32), B=np.array(meta["B"], np.int32), A=np.array(meta["A"], np.int32),
                  reward_f64=np.array(meta["reward_f64"], np.uint8), gamma=np.array(meta["gamma"], np.float64),
                  lmda=np.array(meta["lmda"], np.float64), n_actions=np.array(N_ACTIONS, np.int32),
                  offsets=np.array(offsets, np.int64), b_offsets=np.array(b_offsets, np.int64),
                  r_offsets=np.array(r_offsets, np.int64))
    for name, parts in flat.items():
        arrays[name] = np.concatenate(parts)
    out = os.path.join(HERE, "gae_multi_cases.npz")
    write_npz(out, arrays)
    size = os.path.getsize(out)
    print("gae_multi_cases: %d cases, %d rows, %.1f %% inactive, %d bytes" % (len(meta["T"]), len(valid), 100 * frac, size))
    assert size < 1024 * 1024


if __name__ == "__main__":
    main()
