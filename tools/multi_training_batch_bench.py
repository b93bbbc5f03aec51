#!/usr/bin/env python
"""
Times the multi-agent PPO batch builder (the masked window of csrc/sl_rollout.hip) at T = 20 and 8192 / 16384 columns, float32 rewards:

    (a) slhip_training_batch_multi with every row active against slhip_training_batch on the same window (the outputs
        are checked to be bit-equal first): what the mask costs when nobody is ever away
    (b) the same with about half of the rows inactive -- envs of 8 agents that leave with probability 0.45 per step and
        come back when the last one is gone -- against the single-agent kernel on a window of equal size
    (c) slhip_rollout_compact + the host read of N + slhip_rollout_gather of the six tensors (observation rows of
        15 x 11 x 7 bytes) on the window of (b), against torch: x[mask] for each of the six tensors, and one nonzero()
        followed by six index_select calls.  All three are checked to give the same rows first.

Device time: HIP events around LAUNCHES back-to-back calls of a variant (one call of a kernel is a few tens of
microseconds: shorter than an event's resolution likes), divided by LAUNCHES; the variants of a comparison alternate,
REPEATS times each after one warm-up; medians.  Every buffer is allocated before the events.  Writes
profiles/multi_training_batch_bench.json.

    python tools/multi_training_batch_bench.py [--repeats 9] [--launches 20] [--out DIR]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

GAMMA, LMDA, T, OBS_BYTES = 0.97, 0.95, 20, 15 * 11 * 7


def leaving_window(rng, envs, agents, p_leave):
    """active, done [T, envs * agents] of envs whose agents leave with probability p_leave per step."""
    now = np.ones((envs, agents), bool)
    active, done = np.zeros((T, envs, agents), np.uint8), np.zeros((T, envs, agents), np.uint8)
    for t in range(T):
        leave = rng.random((envs, agents)) < p_leave
        active[t], done[t] = now, now & leave
        now = now & ~leave
        now[~now.any(axis=1)] = True
    return active.reshape(T, -1), done.reshape(T, -1)


def alternate(torch, variants, repeats, launches):
    """variants: name -> callable; -> name -> {us_runs, us_median} per call."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    runs = {name: [] for name in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            e1.synchronize()
            runs[name].append(e0.elapsed_time(e1) * 1e3 / launches)
    return {name: {"us_runs": [round(x, 2) for x in r], "us_median": round(statistics.median(r), 2)}
            for name, r in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of multi_training_batch_bench.json")
    args = ap.parse_args()
    import torch
    from safelife_amd import _hip
    dev, lib = _hip.device(), _hip.lib()
    rng = np.random.default_rng(0)
    report = {"steps": T, "reward_dtype": "float32", "gamma": GAMMA, "lmda": LMDA, "obs_bytes": OBS_BYTES,
              "launches_per_timing": args.launches, "device": torch.cuda.get_device_name(dev), "columns": {}}

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    for N in (8192, 2 * 8192):
        R, V = up(rng.normal(size=(T, N)).astype(np.float32)), up(rng.normal(size=(T, N)).astype(np.float32))
        fv = up(rng.normal(size=N).astype(np.float32))
        D1 = up((rng.random((T, N)) < 0.05).astype(np.uint8))
        ones = torch.ones((T, N), dtype=torch.uint8, device=dev)
        half_active, half_done = leaving_window(rng, N // 8, 8, 0.45)
        A2, D2 = up(half_active), up(half_done)
        outs = {k: (torch.zeros((T, N), device=dev), torch.zeros((T, N), device=dev),
                    torch.zeros((T, N), dtype=torch.uint8, device=dev)) for k in ("single", "multi", "half")}
        single = _hip.Rollout()
        single.T, single.B, single.row_stride, single.out_stride, single.reward_dtype = T, N, N, N, _hip.REWARD_F32
        single.rewards, single.values, single.done = R.data_ptr(), V.data_ptr(), D1.data_ptr()

        def multi_struct(done, active, agents):
            m = _hip.RolloutMulti()
            m.w.T, m.w.B, m.w.row_stride, m.w.out_stride, m.w.reward_dtype = T, N, N, N, _hip.REWARD_F32
            m.w.rewards, m.w.values, m.w.done = R.data_ptr(), V.data_ptr(), done.data_ptr()
            m.n_agents, m.active = agents, active.data_ptr()
            return m
        all_on, half = multi_struct(D1, ones, 1), multi_struct(D2, A2, 8)
        stream = _hip.current_stream_ptr()

        def run_single():
            o = outs["single"]
            _hip.check(lib.slhip_training_batch(C.byref(single), _hip.ptr(fv), GAMMA, LMDA, _hip.ptr(o[0]), _hip.ptr(o[1]),
                                                _hip.ptr(o[2]), stream))

        def run_multi(m, key):
            o = outs[key]
            _hip.check(lib.slhip_training_batch_multi(C.byref(m), _hip.ptr(fv), GAMMA, LMDA, _hip.ptr(o[0]), _hip.ptr(o[1]),
                                                      _hip.ptr(o[2]), stream))
        run_single(), run_multi(all_on, "multi")
        torch.cuda.synchronize()
        if not all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs["single"], outs["multi"])):
            raise SystemExit("multi_training_batch_bench: the two kernels disagree with every row active; nothing timed")
        entry = {"inactive_fraction_half": round(1.0 - float(half_active.mean()), 4)}
        entry["a_all_active"] = alternate(torch, {"single_agent_kernel": run_single,
                                                  "multi_kernel": lambda: run_multi(all_on, "multi")},
                                          args.repeats, args.launches)
        entry["b_half_inactive"] = alternate(torch, {"single_agent_kernel": run_single,
                                                     "multi_kernel": lambda: run_multi(half, "half")},
                                             args.repeats, args.launches)
        for part in ("a_all_active", "b_half_inactive"):
            e = entry[part]
            e["multi_over_single"] = round(e["multi_kernel"]["us_median"] / e["single_agent_kernel"]["us_median"], 3)

        # (c) the active rows of the half-inactive window as flat tensors
        src = dict(actions=up(rng.integers(0, 9, (T, N)).astype(np.int32)), action_prob=up(rng.random((T, N)).astype(np.float32)),
                   values=V, returns=outs["half"][0], advantages=outs["half"][1])
        obs = torch.randint(0, 256, (T * N, OBS_BYTES), dtype=torch.uint8, device=dev)
        half.w.actions, half.w.action_prob = src["actions"].data_ptr(), src["action_prob"].data_ptr()
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        half.w.status = status.data_ptr()
        rows = torch.zeros(T * N, dtype=torch.int64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        work = torch.zeros(lib.slhip_rollout_compact_chunks(C.byref(half)), dtype=torch.int32, device=dev)
        n_rows = int(half_active.sum())
        g = dict(obs=torch.zeros((n_rows, OBS_BYTES), dtype=torch.uint8, device=dev),
                 actions=torch.zeros(n_rows, dtype=torch.int64, device=dev))
        for k in ("action_prob", "returns", "advantages", "values"):
            g[k] = torch.zeros(n_rows, device=dev)
        mask = A2.view(-1) != 0
        flat = {k: v.view(-1) for k, v in src.items()}

        def hip_gather():
            _hip.check(lib.slhip_rollout_compact(C.byref(half), _hip.ptr(rows), _hip.ptr(count), _hip.ptr(work), stream))
            n = int(count.item())
            _hip.check(lib.slhip_rollout_gather(C.byref(half), _hip.ptr(rows), n, _hip.ptr(src["returns"]),
                                                _hip.ptr(src["advantages"]), _hip.ptr(obs), OBS_BYTES, _hip.ptr(g["obs"]),
                                                _hip.ptr(g["actions"]), _hip.ptr(g["action_prob"]), _hip.ptr(g["returns"]),
                                                _hip.ptr(g["advantages"]), _hip.ptr(g["values"]), stream))
            return n

        def torch_mask():
            return dict(obs=obs[mask], actions=flat["actions"][mask].to(torch.int64), action_prob=flat["action_prob"][mask],
                        returns=flat["returns"][mask], advantages=flat["advantages"][mask], values=flat["values"][mask])

        def torch_nonzero_once():
            idx = mask.nonzero().view(-1)
            return dict(obs=obs.index_select(0, idx), actions=flat["actions"].index_select(0, idx).to(torch.int64),
                        action_prob=flat["action_prob"].index_select(0, idx), returns=flat["returns"].index_select(0, idx),
                        advantages=flat["advantages"].index_select(0, idx), values=flat["values"].index_select(0, idx))
        n = hip_gather()
        t1, t2 = torch_mask(), torch_nonzero_once()
        torch.cuda.synchronize()
        if n != n_rows or int(status.item()) or not all(torch.equal(g[k], t1[k]) and torch.equal(g[k], t2[k]) for k in g):
            raise SystemExit("multi_training_batch_bench: the gather and torch's indexing disagree; nothing timed")
        entry["c_compact_gather"] = alternate(torch, {"hip_compact_count_gather": hip_gather, "torch_boolean_mask": torch_mask,
                                                      "torch_nonzero_index_select": torch_nonzero_once},
                                              args.repeats, max(1, args.launches // 4))
        c = entry["c_compact_gather"]
        c["rows"], c["bytes_moved"] = n_rows, 2 * n_rows * (OBS_BYTES + 4 * 4 + 4 + 8)
        c["torch_mask_over_hip"] = round(c["torch_boolean_mask"]["us_median"] / c["hip_compact_count_gather"]["us_median"], 2)
        c["torch_nonzero_over_hip"] = round(c["torch_nonzero_index_select"]["us_median"]
                                            / c["hip_compact_count_gather"]["us_median"], 2)
        report["columns"][str(N)] = entry
        del obs, g, t1, t2
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "multi_training_batch_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
