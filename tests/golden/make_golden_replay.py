#!/usr/bin/env python3
"""
Writes tests/golden/replay_cases.npz by RUNNING THE REFERENCE's DQN (training/dqn.py: take_one_step, add_to_replay,
ReplayBuffer) on the CPU: what slhip_replay_add and tests/replay_ref.py are held to, bit for bit.

    python tests/golden/make_golden_replay.py

Runs where make_golden.py runs (it needs the reference's Python, loaded through make_golden.import_reference()).  The
reference's trainer is driven with scripted envs and a table model:

  - env b returns the recorded reward R[t,b] (a numpy scalar of the case's dtype) and done flag D[t,b] at its t-th step,
    whatever the action; its observation is the tag (b, t) with t the number of steps it has taken in all (a reset does
    not rewind it), so the observation of step t is (b, t) and its next observation (b, t + 1) -- for a finished env that
    is the first observation of its next episode, which is what the fused runner hands over too;
  - the model returns fixed Q-values Q[t,b,:]; epsilon is 0.3, the global generator is seeded, and the actions the
    reference drew are recorded (A[t,b]).

After steps DUMP[0] <= DUMP[1] <= DUMP[2] = T the replay buffer and the per-agent windows are dumped.

Per case i (flat arrays):
    n, B, T, reward_f64, capacity, gamma, dump_steps [3]      the case
    R32 / R64, D, A     [T,B] rewards (in the array of the case's dtype, T * B values from r_offsets[i]), done uint8,
                        actions int32; T * B values from step_offsets[i]
    per dump j (index 3 * i + j):
        idx                      ReplayBuffer.idx
        e_* [min(idx, capacity)] the ring, slot by slot, from entry_offsets[3 i + j]: obs tag (e_obs_b, e_obs_t), e_action,
                                 e_reward (float64, the n-step sum), next-obs tag (e_next_b, e_next_t), e_done
        w_fill [B], w_reward / w_action / w_obs_t [n,B]   the windows, from win_offsets[3 i + j] (winn_offsets for the [n,B] ones):
                                 slots filled, and slot k = the step k steps back (0 / 0 / -1 where empty)

Cases: n in {1, 2, 5} x T in {1, n-1, n, n+1, 3n+2} (distinct, >= 1) x B in {1, 63, 64, 65, 257}; reward dtype, capacity
(exactly B * (n+1), so the ring wraps, or large enough never to wrap) and gamma in {0.97, 1, 0, 0.5} cycle so that every
value meets every n and every B.  Columns 0-4 of a case (B = 1: the one column takes them in turn, case after case) are:
never done, done at every step, done at the last step only, done at step n-1 only, done at t = 0 only; the others draw
done with probability 0.3.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

N_ACTIONS = 9
EPSILON = 0.3
GAMMAS = (0.97, 1.0, 0.0, 0.5)
NS, BS = (1, 2, 5), (1, 63, 64, 65, 257)


def special_column(kind, T, n):
    d = np.zeros(T, np.uint8)
    if kind == 1:
        d[:] = 1
    elif kind == 2:
        d[T - 1] = 1
    elif kind == 3 and 0 <= n - 1 < T:
        d[n - 1] = 1
    elif kind == 4:
        d[0] = 1
    return d


def make_cases():
    rng = np.random.default_rng(20261019)
    singles = count = 0
    for n in NS:
        for T in sorted({t for t in (1, n - 1, n, n + 1, 3 * n + 2) if t >= 1}):
            for bi, B in enumerate(BS):
                f64 = bool((count + bi) % 2)
                wraps = bool(((count + bi) // 2) % 2)
                gamma = GAMMAS[(count + 2 * bi) % 4]
                count += 1
                D = (rng.random((T, B)) < 0.3).astype(np.uint8)
                for k in range(min(5, B)):
                    D[:, k] = special_column(k if B > 1 else singles % 5, T, n)
                R = rng.normal(0.0, 1.0, (T, B))
                R[rng.random((T, B)) < 0.2] = 0.0                  # most steps of the game score nothing
                R = R.astype(np.float64 if f64 else np.float32)
                Q = rng.normal(0.0, 1.0, (T, B, N_ACTIONS)).astype(np.float32)
                capacity = B * (n + 1) if wraps else B * (T + 1) + 7
                capacity = max(capacity, B * (n + 1))
                dumps = (max(1, T // 3), max(1, (2 * T) // 3), T)
                yield dict(n=n, B=B, T=T, f64=f64, gamma=gamma, capacity=capacity, R=R, D=D, Q=Q, dumps=dumps,
                           seed=1000 + count)
                singles += B == 1
        count += 1                  # (shifts the cycles between the blocks of n)


def dump_state(algo, envs, case):
    n, B = case["n"], case["B"]
    rb = algo.replay_buffer
    size = len(rb)
    e = dict(obs_b=np.zeros(size, np.int16), obs_t=np.zeros(size, np.int16), action=np.zeros(size, np.int32),
             reward=np.zeros(size, np.float64), next_b=np.zeros(size, np.int16), next_t=np.zeros(size, np.int16),
             done=np.zeros(size, np.uint8))
    for s in range(size):
        obs, act, reward, next_obs, done = rb.buffer[s]
        assert isinstance(reward, (float, np.float64)), type(reward)
        e["obs_b"][s], e["obs_t"][s] = int(obs[0]), int(obs[1])
        e["next_b"][s], e["next_t"][s] = int(next_obs[0]), int(next_obs[1])
        e["action"][s], e["reward"][s], e["done"][s] = int(act), reward, bool(done)
    w = dict(fill=np.zeros(B, np.int8), reward=np.zeros((n, B), np.float64), action=np.zeros((n, B), np.int32),
             obs_t=np.full((n, B), -1, np.int16))
    for b, env in enumerate(envs):
        key = (id(env), env.num_resets, 0)
        if key not in algo.agent_trajectories:
            continue
        traj = algo.agent_trajectories[key]
        for k in range(n):
            if traj[k]["obs"] is None:
                break
            assert int(traj[k]["obs"][0]) == b
            w["fill"][b] = k + 1
            w["reward"][k, b], w["action"][k, b], w["obs_t"][k, b] = traj[k]["reward"], traj[k]["action"], traj[k]["obs"][1]
    return dict(idx=rb.idx, e=e, w=w)


def run_reference(DQN, set_rng, torch, case):
    n, B, T, R, D, Q = case["n"], case["B"], case["T"], case["R"], case["D"], case["Q"]

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
            self.table = torch.from_numpy(Q)

        def forward(self, obs):
            b, t = obs[:, 0].to(torch.int64), obs[:, 1].to(torch.int64)
            return self.table[t, b]

    set_rng(np.random.default_rng(case["seed"]))
    envs = [ScriptedEnv(b) for b in range(B)]
    algo = DQN(TableModel(), TableModel(), training_envs=envs, gamma=case["gamma"], multi_step_learning=n,
               replay_size=case["capacity"])
    algo.epsilon = EPSILON
    A = np.zeros((T, B), np.int32)
    dumps = []
    for t in range(T):
        step = algo.take_one_step(envs)
        assert len(step.obs) == B and step.rewards.dtype == R.dtype
        assert np.array_equal(step.obs, np.stack([np.arange(B), np.full(B, t)], 1).astype(np.float32))
        assert np.array_equal(step.next_obs, np.stack([np.arange(B), np.full(B, t + 1)], 1).astype(np.float32))
        assert np.array_equal(step.rewards, R[t]) and np.array_equal(step.done, D[t] != 0)
        A[t] = step.actions
        algo.add_to_replay(step)
        for s in case["dumps"]:
            if s == t + 1:
                dumps.append(dump_state(algo, envs, case))
    assert len(dumps) == 3
    greedy = A == Q.argmax(axis=2)
    assert T * B < 50 or (0.55 < greedy.mean() < 0.95)      # epsilon 0.3: about 73 % of the actions are the argmax
    return A, dumps


def main():
    import make_golden
    from make_golden_gae import write_npz
    make_golden.import_reference()
    import torch
    from safelife.random import set_rng
    from training.dqn import DQN
    DQN.compute_device = torch.device("cpu")
    torch.set_num_threads(1)

    meta = {k: [] for k in ("n", "B", "T", "reward_f64", "capacity", "gamma", "dump_steps")}
    flat = {k: [] for k in ("R32", "R64", "D", "A", "idx", "e_obs_b", "e_obs_t", "e_action", "e_reward", "e_next_b",
                            "e_next_t", "e_done", "w_fill", "w_reward", "w_action", "w_obs_t")}
    step_offsets, r_offsets, entry_offsets, win_offsets, winn_offsets = [0], [], [0], [0], [0]
    for case in make_cases():
        A, dumps = run_reference(DQN, set_rng, torch, case)
        n, B, T = case["n"], case["B"], case["T"]
        for k in ("n", "B", "T", "capacity", "gamma"):
            meta[k].append(case[k])
        meta["reward_f64"].append(int(case["f64"])), meta["dump_steps"].append(case["dumps"])
        key = "R64" if case["f64"] else "R32"
        r_offsets.append(sum(len(x) for x in flat[key]))
        flat[key].append(case["R"].ravel())
        flat["D"].append(case["D"].ravel()), flat["A"].append(A.ravel())
        step_offsets.append(step_offsets[-1] + T * B)
        for d in dumps:
            flat["idx"].append(np.array([d["idx"]], np.int64))
            for name, a in d["e"].items():
                flat["e_" + name].append(a)
            for name, a in d["w"].items():
                flat["w_" + name].append(a.ravel())
            entry_offsets.append(entry_offsets[-1] + len(d["e"]["done"]))
            win_offsets.append(win_offsets[-1] + B)
            winn_offsets.append(winn_offsets[-1] + n * B)
        print("n=%d T=%2d B=%3d %s gamma=%-4g capacity=%5d idx=%5d done %.2f" % (
            n, T, B, "f64" if case["f64"] else "f32", case["gamma"], case["capacity"], dumps[-1]["idx"], case["D"].mean()),
            flush=True)
    arrays = dict(n=np.array(meta["n"], np.int32), B=np.array(meta["B"], np.int32), T=np.array(meta["T"], np.int32),
                  reward_f64=np.array(meta["reward_f64"], np.uint8), capacity=np.array(meta["capacity"], np.int64),
                  gamma=np.array(meta["gamma"], np.float64), dump_steps=np.array(meta["dump_steps"], np.int32),
                  n_actions=np.array(N_ACTIONS, np.int32), epsilon=np.array(EPSILON, np.float64),
                  step_offsets=np.array(step_offsets, np.int64), r_offsets=np.array(r_offsets, np.int64),
                  entry_offsets=np.array(entry_offsets, np.int64), win_offsets=np.array(win_offsets, np.int64),
                  winn_offsets=np.array(winn_offsets, np.int64))
    for name, parts in flat.items():
        arrays[name] = np.concatenate(parts)
    out = os.path.join(HERE, "replay_cases.npz")
    write_npz(out, arrays)
    print("replay_cases: %d cases, %d bytes" % (len(meta["n"]), os.path.getsize(out)))


if __name__ == "__main__":
    main()
