#!/usr/bin/env python
"""
Times the device-side DQN replay (safelife_amd.replay.ReplayBuffer -> slhip_replay_add / slhip_replay_sample /
slhip_replay_gather, and slhip_sample_actions_eps; csrc/sl_replay.hip) at 8192 envs, n = 5, the 25x25x10 uint8 policy
observation (6250-byte rows, which move 2 bytes per lane), k = 96, against the same operations written with torch ops in
the same process:

    add      torch: the window as [n,B] tensors, n-1 masked reward updates, a cumsum for the slots, and index_copy_ of
             whole batches of rows into a ring with one spare slot that takes the rows of envs that push nothing (the
             sync-free way to scatter a data-dependent subset: 2 + 2n batches of rows per step)
    sample   torch: randperm(N)[:k], index_select of the five arrays, the casts of DQN.optimize
    epsilon  torch: argmax, rand < eps, randint, where

Ring capacities: 100000 (the reference's replay_size; B * (n+1) = 49152 fits) and 2^19.  A third run stores the same
observation in 6256-byte rows (padded to a multiple of 16), which is what the 16-byte-per-lane path costs.

Before anything is timed the torch add is checked against the kernels: the same steps through both, rings equal.  Device
time: HIP events around a loop of calls, every buffer allocated before the events, the window full and one loop of
warm-up first, median of five loops.  The span includes the gaps the host leaves between launches.  Bytes per add are
counted from the flags of the timed steps: obs read + window write per env, window read + two ring writes per push,
next_obs read once + a window read and two ring writes per flushed row.

    python tools/replay_bench.py [--envs 8192] [--repeats 5] [--out DIR]
"""
import argparse
import collections
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

Step = collections.namedtuple("Step", "obs actions rewards done next_obs")
N, GAMMA, K, N_ACTIONS, P_DONE, LOOP = 5, 0.97, 96, 9, 0.01, 20


class TorchReplay(object):
    """DQN.add_to_replay with torch ops, no host visit.  Ring arrays have capacity + 1 rows: the last takes what envs
    that push nothing write."""

    def __init__(self, torch, capacity, B, n, gamma, obs_shape, dev):
        import numpy as np
        self.torch, self.cap, self.B, self.n = torch, capacity, B, n
        self.G = [float(g) for g in gamma ** np.arange(1, n)]
        z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)    # noqa: E731
        self.obs, self.next_obs = z((capacity + 1,) + obs_shape, torch.uint8), z((capacity + 1,) + obs_shape, torch.uint8)
        self.action, self.reward, self.done = z(capacity + 1, torch.int32), z(capacity + 1, torch.float64), z(capacity + 1, torch.uint8)
        self.win_obs, self.win_action = z((n, B) + obs_shape, torch.uint8), z((n, B), torch.int32)
        self.win_reward, self.fill = z((n, B), torch.float64), z(B, torch.int64)
        self.idx, self.t = z(1, torch.int64), 0
        self.trash = torch.full((B,), capacity, dtype=torch.int64, device=dev)

    def add(self, s):
        torch, n, cap = self.torch, self.n, self.cap
        cur = self.t % n
        r, d = s.rewards.double(), s.done != 0
        full = self.fill == n
        fill_new = torch.clamp(self.fill + 1, max=n)
        count = full.long() + torch.where(d, fill_new, torch.zeros_like(fill_new))
        base = self.idx + torch.cumsum(count, 0) - count
        dest = torch.where(full, base % cap, self.trash)
        for ring, src in ((self.obs, self.win_obs[cur]), (self.next_obs, s.obs), (self.action, self.win_action[cur]),
                          (self.reward, self.win_reward[cur]), (self.done, s.done)):
            ring.index_copy_(0, dest, src)
        for k in range(1, n):
            slot = (cur - k) % n
            self.win_reward[slot] += torch.where(self.fill >= k, r * self.G[k - 1], torch.zeros_like(r))
        self.win_obs[cur].copy_(s.obs), self.win_action[cur].copy_(s.actions), self.win_reward[cur].copy_(r)
        first = base + full.long()
        for k in range(n):
            slot = (cur - k) % n
            dest = torch.where(d & (fill_new > k), (first + k) % cap, self.trash)
            for ring, src in ((self.obs, self.win_obs[slot]), (self.next_obs, s.next_obs), (self.action, self.win_action[slot]),
                              (self.reward, self.win_reward[slot]), (self.done, s.done)):
                ring.index_copy_(0, dest, src)
        self.fill = torch.where(d, torch.zeros_like(fill_new), fill_new)
        self.idx += count.sum()
        self.t += 1

    def sample(self, k, size):
        torch = self.torch
        index = torch.randperm(size, device=self.obs.device)[:k]
        return (self.obs.index_select(0, index).float(), self.action.index_select(0, index).long(),
                self.reward.index_select(0, index).float(), self.next_obs.index_select(0, index).float(),
                self.done.index_select(0, index).float())


def timed(torch, fn, repeats, calls):
    fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / calls)
    return {"us_per_call_runs": [round(x, 1) for x in runs], "us_per_call_median": round(statistics.median(runs), 1)}


def bytes_per_add(steps, n, obs_bytes):
    """Observation bytes an add has to move (reads + writes), averaged over `steps`, for a window that starts full."""
    import numpy as np
    B = steps[0].done.numel()
    fill, total = np.full(B, n), 0
    for s in steps:
        d = s.done.cpu().numpy() != 0
        push, fill_new = fill == n, np.minimum(fill + 1, n)
        flushed = np.where(d, fill_new, 0)
        rows = 2 * B + 3 * push.sum() + d.sum() + (np.maximum(flushed - 1, 0) + 2 * flushed).sum()
        total += int(rows) * obs_bytes
        fill = np.where(d, 0, fill_new)
    return total / len(steps)


def run_add(torch, ReplayBuffer, dev, B, capacity, obs_shape, repeats, check):
    g = torch.Generator(device="cpu").manual_seed(capacity % 1000 + obs_shape[0])
    frames = [torch.randint(0, 256, (B,) + obs_shape, generator=g, dtype=torch.uint8).to(dev) for _ in range(LOOP + 1)]
    steps = [Step(frames[t], torch.randint(0, N_ACTIONS, (B,), generator=g, dtype=torch.int32).to(dev),
                  torch.randn(B, generator=g).to(dev), (torch.rand(B, generator=g) < P_DONE).to(torch.uint8).to(dev),
                  frames[t + 1]) for t in range(LOOP)]
    buf = ReplayBuffer(capacity, B, multi_step=N, gamma=GAMMA, obs_shape=obs_shape, obs_dtype=torch.uint8,
                       reward_dtype=torch.float32, device=dev)
    ref = TorchReplay(torch, capacity, B, N, GAMMA, obs_shape, dev)
    out = {"capacity": capacity, "obs_bytes": buf.obs_bytes, "ring_bytes": 2 * capacity * buf.obs_bytes}
    if check:
        for s in steps:
            buf.add(s), ref.add(s)
        torch.cuda.synchronize()
        out["torch_add_equals_kernel"] = bool(
            int(buf.idx.item()) == int(ref.idx.item()) and all(torch.equal(getattr(buf, name), getattr(ref, name)[:capacity])
                                                                for name in ("obs", "next_obs", "action", "reward", "done")))
        if not out["torch_add_equals_kernel"]:
            raise SystemExit("replay_bench: the torch add and the kernels disagree; nothing timed")
    else:
        for s in steps[:N + 1]:
            buf.add(s), ref.add(s)
    # (the window is full from here on; the byte count assumes that -- a done flag empties an env's window for n steps,
    # which the count of the first loop does not see: it is an upper bound by about n * P_DONE)
    out["bytes_per_add"] = round(bytes_per_add(steps, N, buf.obs_bytes))
    out["hip_add"] = timed(torch, lambda: [buf.add(s) for s in steps], repeats, LOOP)
    out["torch_add"] = timed(torch, lambda: [ref.add(s) for s in steps], repeats, LOOP)
    us = out["hip_add"]["us_per_call_median"]
    out["hip_add_GBps"] = round(out["bytes_per_add"] / us / 1e3, 1)
    out["torch_over_hip_add"] = round(out["torch_add"]["us_per_call_median"] / us, 2)
    size = len(buf)
    out["rows_held"] = size
    out["hip_sample_gather"] = timed(torch, lambda: [buf.sample(K) for _ in range(LOOP)], repeats, LOOP)
    out["hip_sample_only"] = timed(torch, lambda: [buf.sample_indices(K) for _ in range(LOOP)], repeats, LOOP)
    out["torch_sample_gather"] = timed(torch, lambda: [ref.sample(K, size) for _ in range(LOOP)], repeats, LOOP)
    out["torch_over_hip_sample"] = round(out["torch_sample_gather"]["us_per_call_median"]
                                         / out["hip_sample_gather"]["us_per_call_median"], 2)
    buf.check_status()
    return out


def run_eps(torch, _hip, dev, B, repeats):
    lib = _hip.lib()
    g = torch.Generator(device="cpu").manual_seed(1)
    q = torch.randn((B, N_ACTIONS), generator=g).to(dev)
    actions = torch.zeros(B, dtype=torch.int32, device=dev)
    counter = [0]

    def hip():
        for _ in range(LOOP):
            lib.slhip_sample_actions_eps(_hip.ptr(q), B, N_ACTIONS, 0.03, 5, counter[0], _hip.ptr(actions),
                                         _hip.current_stream_ptr())
            counter[0] += 1

    def plain():
        for _ in range(LOOP):
            greedy = torch.argmax(q, dim=1)
            rnd = torch.randint(0, N_ACTIONS, (B,), device=dev)
            actions.copy_(torch.where(torch.rand(B, device=dev) < 0.03, rnd, greedy))

    out = {"hip_eps_draw": timed(torch, hip, repeats, LOOP), "torch_eps_draw": timed(torch, plain, repeats, LOOP)}
    out["torch_over_hip_eps"] = round(out["torch_eps_draw"]["us_per_call_median"] / out["hip_eps_draw"]["us_per_call_median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of replay_bench.json")
    args = ap.parse_args()
    import torch
    from safelife_amd import _hip
    from safelife_amd.replay import ReplayBuffer
    dev = _hip.device()
    B = args.envs
    report = {"envs": B, "n": N, "k": K, "p_done": P_DONE, "calls_per_loop": LOOP, "device": torch.cuda.get_device_name(dev),
              "min_capacity": B * (N + 1)}
    for name, capacity, shape, check in (("capacity_100000", max(100000, B * (N + 1)), (10, 25, 25), True),
                                         ("capacity_2p19", max(2 ** 19, B * (N + 1)), (10, 25, 25), False),
                                         ("capacity_100000_rows_6256", max(100000, B * (N + 1)), (6256,), True)):
        report[name] = run_add(torch, ReplayBuffer, dev, B, capacity, shape, args.repeats, check)
        print(name, json.dumps(report[name], sort_keys=True), flush=True)
        torch.cuda.empty_cache()
    report["epsilon"] = run_eps(torch, _hip, dev, B, args.repeats)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "replay_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
