#!/usr/bin/env python
"""
Times the multi-agent DQN replay (safelife_amd.replay.MultiAgentReplayBuffer -> slhip_replay_add_masked, and
slhip_sample_actions_eps_masked; csrc/sl_replay.hip) at 8192 envs x 2 agents = 16384 columns, n = 5, the 10x25x25 uint8
policy observation (6250-byte rows), a ring of 100000 slots:

    add (a)   every column active
    add (b)   the active masks and done flags of a real run: MultiAgentDQNRunner on the 26x26 multi-agent levels of
              tests/golden/trace_multi_*.npz (time limit 100, a Q-model that walks towards the exits it sees, epsilon 0.1),
              the last 20 of --run-steps steps
    add (c)   the existing ReplayBuffer.add (no mask) on 16384 columns, the same rows and flags as (a), in the same process
    draw      slhip_sample_actions_eps_masked with the run's last mask against slhip_sample_actions_eps on the same rows

(a) and (c) are first checked to leave the same ring.  What (a) costs over (c) is what the mask costs when nobody is ever
away; (b) moves fewer rows.  Device time: HIP events around a loop of 20 calls, every buffer allocated before the events,
one loop of warm-up, the variants alternating, medians of 9 loops.  The span includes the gaps the host leaves between
launches.  (The recorded masks of (b) are replayed loop after loop: a column that is away at the loop's first step may
have steps waiting in its window from the loop before, which a real run never has -- the kernels do the same work.)
Writes profiles/replay_multi_bench.json.

    python tools/replay_multi_bench.py [--envs 8192] [--run-steps 300] [--repeats 9] [--out DIR]
"""
import argparse
import collections
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

Step = collections.namedtuple("Step", "obs actions rewards done next_obs active")
A, N, GAMMA, N_ACTIONS, P_DONE, LOOP, CAPACITY = 2, 5, 0.97, 9, 0.01, 20, 100000
OBS_SHAPE = (10, 25, 25)


class ExitSeeker(object):
    """obs uint8 [rows, 10, 25, 25] -> qvals [rows, 9]: 1 for the move towards the nearest exit in view (channel 8 without the
    agent's channel 1), else for an action hashed from the row; what makes agents of one env finish at different steps."""

    def __init__(self, torch, device):
        self.torch = torch
        W = H = 25
        x = torch.arange(W, dtype=torch.int64).view(W, 1).expand(W, H) - W // 2
        y = torch.arange(H, dtype=torch.int64).view(1, H).expand(W, H) - H // 2
        self.key = ((x.abs() + y.abs()) * 4096 + torch.arange(W * H, dtype=torch.int64).view(W, H)).to(device)
        self.dx, self.dy = x.reshape(-1).to(device), y.reshape(-1).to(device)

    def __call__(self, obs):
        torch = self.torch
        rows = obs.shape[0]
        hashed = obs[:, 0].reshape(rows, -1).sum(dim=1, dtype=torch.int64) % 9
        exits = (obs[:, 8] != 0) & (obs[:, 1] == 0)
        far = 1 << 40
        key = torch.where(exits, self.key, torch.full_like(self.key, far)).view(rows, -1).min(dim=1).values
        seen = key < far
        cell = torch.where(seen, key % 4096, torch.zeros_like(key))
        dx, dy = self.dx[cell], self.dy[cell]
        move = torch.where(dx.abs() >= dy.abs(), torch.where(dx > 0, 2, 4), torch.where(dy > 0, 3, 1))
        q = torch.zeros((rows, N_ACTIONS), dtype=torch.float32, device=obs.device)
        q[torch.arange(rows, device=obs.device), torch.where(seen, move, hashed)] = 1.0
        return q


def real_run(torch, B, steps):
    """(active, done) uint8 [B, A] of the last LOOP steps of a run of ``steps`` steps, and the run's last Q-values."""
    from safelife_amd.levels import LevelPool, _device_counts
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    from safelife_amd.runner import MultiAgentDQNRunner
    from tests import util
    levels = []
    for name in ("multi_asym1", "multi_build_coop", "multi_build_compete"):
        levels += util.levels_from_trace(util.load_trace(name))
    pool = LevelPool(levels, counts_fn=_device_counts, n_agents=A, min_performance_fraction=0.0)
    env = SafeLifeMultiAgentVectorEnv(pool, B, time_limit=100, view_shape=OBS_SHAPE[1:], output_channels=tuple(range(OBS_SHAPE[0])),
                                      first_level=np.arange(B) % len(levels), auto_reset=True, with_obs=False,
                                      policy_layout="uint8")
    assert tuple(env.policy_tensor.shape[2:]) == OBS_SHAPE
    model = ExitSeeker(torch, env.device)
    qvals = []

    def q_model(obs):
        qvals[:] = [model(obs)]
        return qvals[0]
    runner = MultiAgentDQNRunner(env, q_model, seed=1, cast_obs=False)
    kept = []
    for t in range(steps):
        step = runner.take_one_step(0.1)
        if t >= steps - LOOP:
            kept.append((step.active.clone(), step.done.to(torch.uint8)))
    agent_steps = int(runner.num_agent_steps.item())
    return kept, qvals[0], {"run_steps": steps, "inactive_fraction_of_run": round(1.0 - agent_steps / (steps * B * A), 4),
                            "envs_reloaded": int((runner.num_resets > 0).sum().item())}


def alternate(torch, variants, repeats):
    """variants: name -> callable that makes LOOP calls; -> name -> {us_per_call_runs, us_per_call_median}."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    runs = {name: [] for name in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            runs[name].append(e0.elapsed_time(e1) * 1e3 / LOOP)
    return {name: {"us_per_call_runs": [round(x, 1) for x in r], "us_per_call_median": round(statistics.median(r), 1)}
            for name, r in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--run-steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of replay_multi_bench.json")
    args = ap.parse_args()
    import torch
    from safelife_amd import _hip
    from safelife_amd.replay import MultiAgentReplayBuffer, ReplayBuffer
    dev, lib = _hip.device(), _hip.lib()
    B = args.envs
    cols = B * A
    capacity = max(CAPACITY, cols * (N + 1))
    report = {"envs": B, "agents": A, "columns": cols, "n": N, "capacity": capacity, "obs_bytes": int(np.prod(OBS_SHAPE)),
              "p_done_a_c": P_DONE, "calls_per_loop": LOOP, "device": torch.cuda.get_device_name(dev)}
    masks, last_q, run = real_run(torch, B, max(args.run_steps, LOOP))
    report["real_run"] = run
    report["real_run"]["inactive_fraction_timed"] = round(1.0 - float(torch.stack([m for m, _ in masks]).float().mean().item()), 4)
    torch.cuda.empty_cache()

    g = torch.Generator(device="cpu").manual_seed(16384)
    frames = [torch.randint(0, 256, (B, A) + OBS_SHAPE, generator=g, dtype=torch.uint8).to(dev) for _ in range(LOOP + 1)]
    ones = torch.ones((B, A), dtype=torch.uint8, device=dev)
    all_on, flat, real = [], [], []
    for t in range(LOOP):
        actions = torch.randint(0, N_ACTIONS, (B, A), generator=g, dtype=torch.int32).to(dev)
        rewards = torch.randn((B, A), generator=g).to(dev)
        done = (torch.rand((B, A), generator=g) < P_DONE).to(torch.uint8).to(dev)
        all_on.append(Step(frames[t], actions, rewards, done, frames[t + 1], ones))
        flat.append(Step(frames[t].view((cols,) + OBS_SHAPE), actions.view(cols), rewards.view(cols), done.view(cols),
                         frames[t + 1].view((cols,) + OBS_SHAPE), None))
        real.append(Step(frames[t], actions, rewards, masks[t][1], frames[t + 1], masks[t][0]))
    kw = dict(multi_step=N, gamma=GAMMA, obs_shape=OBS_SHAPE, obs_dtype=torch.uint8, reward_dtype=torch.float32, device=dev)
    buf_a, buf_b = MultiAgentReplayBuffer(capacity, B, A, **kw), MultiAgentReplayBuffer(capacity, B, A, **kw)
    buf_c = ReplayBuffer(capacity, cols, **kw)
    for sa, sc in zip(all_on, flat):
        buf_a.add(sa), buf_c.add(sc)
    torch.cuda.synchronize()
    same = int(buf_a.idx.item()) == int(buf_c.idx.item()) and all(
        torch.equal(getattr(buf_a, name), getattr(buf_c, name)) for name in ("obs", "next_obs", "action", "reward", "done", "fill"))
    report["all_active_equals_unmasked"] = bool(same)
    if not same:
        raise SystemExit("replay_multi_bench: the masked add with everybody active and the unmasked add disagree; nothing timed")
    report["add"] = alternate(torch, {"a_masked_all_active": lambda: [buf_a.add(s) for s in all_on],
                                      "c_unmasked_16384_columns": lambda: [buf_c.add(s) for s in flat],
                                      "b_masked_real_run": lambda: [buf_b.add(s) for s in real]}, args.repeats)
    add = report["add"]
    add["a_over_c"] = round(add["a_masked_all_active"]["us_per_call_median"] / add["c_unmasked_16384_columns"]["us_per_call_median"], 3)
    add["b_over_c"] = round(add["b_masked_real_run"]["us_per_call_median"] / add["c_unmasked_16384_columns"]["us_per_call_median"], 3)
    for buf in (buf_a, buf_b, buf_c):
        buf.check_status()

    actions = torch.zeros(cols, dtype=torch.int32, device=dev)
    mask = masks[-1][0].contiguous()
    counter = [0]

    def masked():
        for _ in range(LOOP):
            lib.slhip_sample_actions_eps_masked(_hip.ptr(last_q), _hip.ptr(mask), cols, N_ACTIONS, 0.03, 5, counter[0],
                                                _hip.ptr(actions), _hip.current_stream_ptr())
            counter[0] += 1

    def plain():
        for _ in range(LOOP):
            lib.slhip_sample_actions_eps(_hip.ptr(last_q), cols, N_ACTIONS, 0.03, 5, counter[0], _hip.ptr(actions),
                                         _hip.current_stream_ptr())
            counter[0] += 1
    report["epsilon_draw"] = alternate(torch, {"masked_real_mask": masked, "unmasked": plain}, args.repeats)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "replay_multi_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
