#!/usr/bin/env python3
"""
Writes tests/golden/replay_multi_cases.npz by RUNNING THE REFERENCE's DQN (training/dqn.py: take_one_step, add_to_replay,
ReplayBuffer, over training/base_algo.py:152-244) on the CPU with MULTI-AGENT envs: what slhip_replay_add_masked and
tests/replay_multi_ref.py are held to, bit for bit.

    python tests/golden/make_golden_replay_multi.py

Runs where make_golden_replay.py runs.  The reference's trainer is driven with scripted envs (single_agent = False) and a
table model:

  - env b has A agents.  At its t-th step (t counts all its steps: a reset does not rewind it) agent a leaves if F[t,b,a]
    is set and it is still there; from then on its done flag stays 1, as the real env's does.  reset() -- which the
    reference calls once all agents are done -- brings everybody back.  The env asserts that it is handed action 0 for
    every agent that is gone.  Rewards are R[t,b,:], an array of the case's dtype; the observation of agent a is the tag
    (b, a, t), so the observation of step t is (b, a, t) and its next observation (b, a, t + 1);
  - the model looks Q[t,b,a,:] up from the tag; epsilon is 0.3, the global generator is seeded, and the actions the
    reference drew are recorded.

After steps DUMP[0] <= DUMP[1] <= DUMP[2] = T the replay buffer, the per-agent windows and the envs' reset counts are
dumped.  A COLUMN is c = b * A + a.

Per case i (flat arrays):
    n, B, A, T, reward_f64, capacity, gamma, dump_steps [3]      the case
    R32 / R64, D, ACT, active    [T,B,A]: rewards (in the array of the case's dtype, from r_offsets[i]; 0 where the agent
                        sat the step out), the ENV's done flags uint8 (1 for an agent that is gone), the actions the
                        reference drew int32 (0 where inactive) and who took part uint8; from step_offsets[i]
    per dump j (index 3 * i + j):
        idx                      ReplayBuffer.idx
        e_* [min(idx, capacity)] the ring, slot by slot, from entry_offsets[3 i + j]: obs tag (e_obs_c, e_obs_t), e_action,
                                 e_reward (float64, the n-step sum), next-obs tag (e_next_c, e_next_t), e_done
        w_fill [B*A], w_reward / w_action / w_obs_t [n,B*A]   the windows, from win_offsets[3 i + j] (winn_offsets for the
                                 [n,B*A] ones): slots filled, and slot k = the step k steps back (0 / 0 / -1 where empty)
        resets [B]               env.num_resets, from res_offsets[3 i + j]

Cases.  SMALL: (B, A) in {(1,4), (21,3), (32,2), (8,8), (65,1)} -- 4, 63, 64, 64 and 65 columns -- x n in {1, 2, 5} x T
in {1, n, n+1, 3n+2} (distinct).  WIDE: (341,3), (512,2), (513,2), (129,8) -- 1023, 1024, 1026 and 1032 columns, the
last with a boundary between two chunks of 1024 columns inside an env's group of agents -- with two (n, T) each, one of
them n = 5 (the whole grid at that width would not fit below 1 MiB).  Reward dtype, capacity (exactly B * A * (n+1), so the
ring wraps, or large enough never to wrap) and gamma in {0.97, 1, 0, 0.5} cycle.  Scripted envs of a case with B >= 4
(B = 1: env 3's script): env 0 -- nobody ever leaves; env 1 -- everybody leaves at every step (the env reloads every
step); env 2 -- everybody leaves at the last step only; env 3 and every env b = 7 mod 8 -- agent 0 leaves at t = 0, its
partners stay for n + 1 steps and leave at step n + 1 (with A = 1 the column is done at t = 0 and at t = n + 1): a long
inactive stretch followed by a reload.  Everything else leaves with a probability per step that depends on A (where a tight ring is
to wrap more than twice in 3n + 2 steps: a quarter of it, and all agents of an env together with probability 0.3).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

N_ACTIONS = 9
EPSILON = 0.3
GAMMAS = (0.97, 1.0, 0.0, 0.5)
LEAVE_P = {1: 0.3, 2: 0.2, 3: 0.25, 4: 0.3, 8: 0.45}
SMALL = ((1, 4), (21, 3), (32, 2), (8, 8), (65, 1))
# (B, A, ((n, T), (n, T)))
WIDE = ((341, 3, ((5, 6), (1, 5))), (512, 2, ((5, 5), (2, 8))), (513, 2, ((5, 6), (2, 3))), (129, 8, ((5, 6), (1, 2))))


def case_list():
    out = []
    for n in (1, 2, 5):
        for T in sorted({1, n, n + 1, 3 * n + 2}):
            for B, A in SMALL:
                out.append((n, T, B, A))
    for B, A, pairs in WIDE:
        for n, T in pairs:
            out.append((n, T, B, A))
    return out


def script(F, T, n, kind):
    """One env's leaving flags F [T, A]."""
    if kind == 0:
        F[:] = 0
    elif kind == 1:
        F[:] = 1
    elif kind == 2:
        F[:] = 0
        F[T - 1] = 1
    elif kind == 3:
        F[:n + 1] = 0
        F[0, 0] = 1
        if T > n + 1:
            F[n + 1] = 1


def make_cases():
    rng = np.random.default_rng(20261020)
    for i, (n, T, B, A) in enumerate(case_list()):
        f64 = bool(i % 2)
        wraps = bool((i // 2) % 2)
        gamma = GAMMAS[(i + i // 4) % 4]
        # (a ring of exactly B * A * (n+1) slots wraps more than twice in 3n + 2 steps only if most agents take most steps
        # and few steps wait in the windows at the end: there the agents of an env mostly leave together)
        together = wraps and T == 3 * n + 2
        F = (rng.random((T, B, A)) < LEAVE_P[A] * (0.25 if together else 1.0)).astype(np.uint8)
        if together:
            F |= (rng.random((T, B, 1)) < 0.3).astype(np.uint8)
        if B == 1:
            script(F[:, 0], T, n, 3)
        elif B >= 4:
            for b in range(B):
                if b < 4 or b % 8 == 7:
                    script(F[:, b], T, n, b if b < 4 else 3)
        R = rng.normal(0.0, 1.0, (T, B, A))
        R[rng.random((T, B, A)) < 0.2] = 0.0                       # most steps of the game score nothing
        R = R.astype(np.float64 if f64 else np.float32)
        Q = rng.normal(0.0, 1.0, (T, B, A, N_ACTIONS)).astype(np.float32)
        cols = B * A
        capacity = cols * (n + 1) if wraps else cols * (T + 1) + 7
        capacity = max(capacity, cols * (n + 1))
        dumps = (max(1, T // 3), max(1, (2 * T) // 3), T)
        yield dict(n=n, B=B, A=A, T=T, f64=f64, gamma=gamma, capacity=capacity, F=F, R=R, Q=Q, dumps=dumps, seed=3000 + i)


def dump_state(algo, envs, case):
    n, B, A = case["n"], case["B"], case["A"]
    cols = B * A
    rb = algo.replay_buffer
    size = len(rb)
    e = dict(obs_c=np.zeros(size, np.int16), obs_t=np.zeros(size, np.int16), action=np.zeros(size, np.int32),
             reward=np.zeros(size, np.float64), next_c=np.zeros(size, np.int16), next_t=np.zeros(size, np.int16),
             done=np.zeros(size, np.uint8))
    for s in range(size):
        obs, act, reward, next_obs, done = rb.buffer[s]
        assert isinstance(reward, (float, np.float64)), type(reward)
        e["obs_c"][s], e["obs_t"][s] = int(obs[0]) * A + int(obs[1]), int(obs[2])
        e["next_c"][s], e["next_t"][s] = int(next_obs[0]) * A + int(next_obs[1]), int(next_obs[2])
        e["action"][s], e["reward"][s], e["done"][s] = int(act), reward, bool(done)
    w = dict(fill=np.zeros(cols, np.int8), reward=np.zeros((n, cols), np.float64), action=np.zeros((n, cols), np.int32),
             obs_t=np.full((n, cols), -1, np.int16))
    live = 0
    for b, env in enumerate(envs):
        for a in range(A):
            key = (id(env), env.num_resets, a)
            if key not in algo.agent_trajectories:
                continue
            live += 1
            traj, c = algo.agent_trajectories[key], b * A + a
            for k in range(n):
                if traj[k]["obs"] is None:
                    break
                assert int(traj[k]["obs"][0]) == b and int(traj[k]["obs"][1]) == a
                w["fill"][c] = k + 1
                w["reward"][k, c], w["action"][k, c], w["obs_t"][k, c] = traj[k]["reward"], traj[k]["action"], traj[k]["obs"][2]
    assert live == len(algo.agent_trajectories)         # no window of an earlier episode is left behind
    return dict(idx=rb.idx, e=e, w=w, resets=np.array([env.num_resets for env in envs], np.int64))


def run_reference(DQN, set_rng, torch, case):
    n, B, A, T, F, R, Q = case["n"], case["B"], case["A"], case["T"], case["F"], case["R"], case["Q"]
    D = np.zeros((T, B, A), np.uint8)
    active = np.zeros((T, B, A), np.uint8)

    class ScriptedEnv(object):
        single_agent = False

        def __init__(self, b):
            self.b, self.t, self.gone = b, 0, np.zeros(A, bool)

        def obs(self):
            return np.array([[self.b, a, self.t] for a in range(A)], np.float32)

        def reset(self):
            self.gone[:] = False
            return self.obs()

        def step(self, actions):
            actions = np.asarray(actions)
            assert actions.shape == (A,) and not actions[self.gone].any()       # a gone agent is handed 0
            active[self.t, self.b] = ~self.gone
            self.gone = self.gone | (F[self.t, self.b] != 0)
            D[self.t, self.b] = self.gone
            r = R[self.t, self.b].copy()
            self.t += 1
            return self.obs(), r, self.gone.copy(), {}

    class TableModel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.unused = torch.nn.Parameter(torch.zeros(1))       # (the trainer builds an optimiser)
            self.table = torch.from_numpy(Q)

        def forward(self, obs):
            b, a, t = (obs[:, k].to(torch.int64) for k in range(3))
            return self.table[t, b, a]

    set_rng(np.random.default_rng(case["seed"]))
    envs = [ScriptedEnv(b) for b in range(B)]
    algo = DQN(TableModel(), TableModel(), training_envs=envs, gamma=case["gamma"], multi_step_learning=n,
               replay_size=case["capacity"])
    algo.epsilon = EPSILON
    ACT = np.zeros((T, B, A), np.int32)
    dumps = []
    for t in range(T):
        step = algo.take_one_step(envs)
        on = active[t] != 0
        b, a = np.nonzero(on)                                   # env-major, agent-minor: the reference's order
        assert len(step.obs) == len(b) and step.rewards.dtype == R.dtype and on.any(axis=1).all()
        assert np.array_equal(step.obs, np.stack([b, a, np.full(len(b), t)], 1).astype(np.float32))
        # the next observation of an agent whose env has reloaded is the new episode's first: the same tag (b, a, t + 1)
        assert np.array_equal(step.next_obs, np.stack([b, a, np.full(len(b), t + 1)], 1).astype(np.float32))
        assert np.array_equal(step.rewards, R[t][on]) and np.array_equal(step.done, D[t][on] != 0)
        ACT[t][on] = step.actions
        algo.add_to_replay(step)
        for s in case["dumps"]:
            if s == t + 1:
                dumps.append(dump_state(algo, envs, case))
    assert len(dumps) == 3
    return ACT, D, active, dumps


def main():
    import make_golden
    from make_golden_gae import write_npz
    make_golden.import_reference()
    import torch
    from safelife.random import set_rng
    from training.dqn import DQN
    DQN.compute_device = torch.device("cpu")
    torch.set_num_threads(1)

    meta = {k: [] for k in ("n", "B", "A", "T", "reward_f64", "capacity", "gamma", "dump_steps")}
    flat = {k: [] for k in ("R32", "R64", "D", "ACT", "active", "idx", "e_obs_c", "e_obs_t", "e_action", "e_reward",
                            "e_next_c", "e_next_t", "e_done", "w_fill", "w_reward", "w_action", "w_obs_t", "resets")}
    step_offsets, r_offsets, entry_offsets, win_offsets, winn_offsets, res_offsets = [0], [], [0], [0], [0], [0]
    pushes = inactive = total = wrapped_twice = 0
    for case in make_cases():
        ACT, D, active, dumps = run_reference(DQN, set_rng, torch, case)
        n, B, A, T = case["n"], case["B"], case["A"], case["T"]
        cols = B * A
        on = active != 0
        # what a test could otherwise pass without
        if A >= 2 and T > n + 2:
            gone_at_0 = ~on[1:n + 1, :, 0].any(axis=0) & on[1:n + 1, :, 1].all(axis=0)
            assert gone_at_0.any() and on[n + 2:, gone_at_0, 0].any(), (n, T, B, A)    # away for n + 1 steps, then back
        if A == 1:
            assert on.all()
        for k in ("n", "B", "A", "T", "capacity", "gamma"):
            meta[k].append(case[k])
        meta["reward_f64"].append(int(case["f64"])), meta["dump_steps"].append(case["dumps"])
        key = "R64" if case["f64"] else "R32"
        r_offsets.append(sum(len(x) for x in flat[key]))
        # (rewards of steps the reference never saw are zeroed: they carry no information, and zeros pack well)
        flat[key].append(np.where(on, case["R"], 0).astype(case["R"].dtype).ravel())
        flat["D"].append(D.ravel()), flat["ACT"].append(ACT.ravel()), flat["active"].append(active.ravel())
        step_offsets.append(step_offsets[-1] + T * cols)
        for d in dumps:
            flat["idx"].append(np.array([d["idx"]], np.int64))
            for name, a in d["e"].items():
                flat["e_" + name].append(a)
            for name, a in d["w"].items():
                flat["w_" + name].append(a.ravel())
            flat["resets"].append(d["resets"])
            entry_offsets.append(entry_offsets[-1] + len(d["e"]["done"]))
            win_offsets.append(win_offsets[-1] + cols)
            winn_offsets.append(winn_offsets[-1] + n * cols)
            res_offsets.append(res_offsets[-1] + B)
        pushes += dumps[-1]["idx"]
        wrapped_twice += A >= 2 and dumps[-1]["idx"] > 2 * case["capacity"]
        inactive += int((~on).sum())
        total += on.size
        print("n=%d T=%2d B=%3d A=%d %s gamma=%-4g capacity=%5d idx=%5d inactive %.2f resets %d" % (
            n, T, B, A, "f64" if case["f64"] else "f32", case["gamma"], case["capacity"], dumps[-1]["idx"],
            1.0 - on.mean(), dumps[-1]["resets"].sum()), flush=True)
    arrays = dict(n=np.array(meta["n"], np.int32), B=np.array(meta["B"], np.int32), A=np.array(meta["A"], np.int32),
                  T=np.array(meta["T"], np.int32), reward_f64=np.array(meta["reward_f64"], np.uint8),
                  capacity=np.array(meta["capacity"], np.int64), gamma=np.array(meta["gamma"], np.float64),
                  dump_steps=np.array(meta["dump_steps"], np.int32), n_actions=np.array(N_ACTIONS, np.int32),
                  epsilon=np.array(EPSILON, np.float64), step_offsets=np.array(step_offsets, np.int64),
                  r_offsets=np.array(r_offsets, np.int64), entry_offsets=np.array(entry_offsets, np.int64),
                  win_offsets=np.array(win_offsets, np.int64), winn_offsets=np.array(winn_offsets, np.int64),
                  res_offsets=np.array(res_offsets, np.int64))
    for name, parts in flat.items():
        arrays[name] = np.concatenate(parts)
    out = os.path.join(HERE, "replay_multi_cases.npz")
    write_npz(out, arrays)
    size = os.path.getsize(out)
    print("replay_multi_cases: %d cases, %d pushes, %.1f %% of the agent steps inactive, %d bytes"
          % (len(meta["n"]), pushes, 100.0 * inactive / total, size))
    assert size < 1024 * 1024 and wrapped_twice >= 3, wrapped_twice


if __name__ == "__main__":
    main()
