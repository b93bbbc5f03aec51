#!/usr/bin/env python
"""
Times the batched earth-mover distances (SideEffectBatch.scores_all -> slhip_emd_batch) against the host LP path
(SideEffectBatch.scores(i): one HiGHS transportation LP per cell type) on queues that replay the committed
side-effect fixtures: tests/golden/side_effect_inputs.npz (25x25, life-blue: 80 differing cells) and
side_effect_inputs_64.npz (64x64, life-yellow: 1735), every entry of the queue the same episode.

Device time: HIP events around the launch, median of --repeats fresh batches (the pass itself is outside the
events).  Host time: wall clock of scores(i) on --host-entries entries of the same batch (64x64: one entry, minutes);
"host_batch_s_extrapolated" is that per-entry time multiplied by the number of entries -- an extrapolation, labelled
as such.  Writes profiles/emd_bench.json.

    python tools/emd_bench.py [--cap25 2048] [--cap64 256] [--repeats 5] [--host-entries 3] [--skip-host-64]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def replay_batch(d, cap, num_samples=1000):
    """A SideEffectBatch whose `cap` entries all replay the fixture's episode (recorded generator state)."""
    import torch
    from safelife_amd import _hip, speedups as sp
    from safelife_amd.levels import Level, LevelPool, _device_counts
    from safelife_amd.vector_env import SafeLifeVectorEnv, SideEffectBatch
    start = Level(d["b0"], agent_locs=np.zeros((0, 2), int), spawn_prob=float(d["spawn_prob"]))
    env = SafeLifeVectorEnv(LevelPool([start], counts_fn=_device_counts), 4, with_obs=False)
    dev = env.device
    H, W = d["b0"].shape
    rec = np.zeros((cap, 8), np.int32)
    rec[:, 0], rec[:, 2] = np.arange(cap), int(d["num_steps"])
    rec[:, 4] = np.float32(d["spawn_prob"]).view(np.int32)
    bufs = dict(count=torch.tensor([cap], dtype=torch.int32, device=dev), records=torch.from_numpy(rec).to(dev),
                boards=torch.from_numpy(np.broadcast_to(d["b2"], (cap, H, W)).copy().view(np.int16)).to(dev))
    q = _hip.EpisodeQueue()
    q.capacity, q.env_base = cap, 0
    q.count, q.records, q.boards = (bufs[k].data_ptr() for k in ("count", "records", "boards"))
    K = _hip.SL_SE_MAX_KEYS
    out = dict(work_boards=torch.zeros((2 * cap, H, W), dtype=torch.int16, device=dev),
               work_prob=torch.zeros(2 * cap, dtype=torch.float32, device=dev),
               work_steps=torch.zeros(2 * cap, dtype=torch.int32, device=dev),
               work_rng=sp._to_device(np.broadcast_to(d["rng0"], (2 * cap, 4)).copy(), np.uint64),
               counts=torch.zeros((2, cap, H, W, 8), dtype=torch.int32, device=dev),
               keys=torch.zeros((cap, K), dtype=torch.int16, device=dev),
               life_dist=torch.zeros((cap, 2, 8, H, W), dtype=torch.float64, device=dev),
               type_masks=torch.zeros((cap, 2, K - 8, H, W), dtype=torch.uint8, device=dev))
    _hip.check(_hip.lib().slhip_side_effects(env._sref, C.byref(q), num_samples, 0,
                                             *[_hip.ptr(out[k]) for k in ("work_boards", "work_prob", "work_steps",
                                                                          "work_rng", "counts", "keys", "life_dist",
                                                                          "type_masks")],
                                             _hip.current_stream_ptr()))
    return SideEffectBatch(env, bufs, out, num_samples)


def bench(fixture, cap, repeats, host_entries):
    import torch
    with np.load(os.path.join(REPO, "tests", "golden", fixture)) as d:
        d = {k: d[k] for k in d.files}
    batch = replay_batch(d, cap)
    torch.cuda.synchronize()
    times = []
    for r in range(repeats + 1):                 # (run 0 warms up: allocations, the table upload)
        batch._emd = None
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        all_ = batch.scores_all()
        t1.record()
        t1.synchronize()
        if r:
            times.append(t0.elapsed_time(t1))
    device = batch.scores(0, device=True)
    n_cells = all_["n_cells"][0].cpu().numpy()
    keys = batch.keys[0].cpu().numpy().view(np.uint16)
    from safelife_amd.side_effects import cell_name
    res = dict(fixture=fixture, shape=list(d["b0"].shape), entries=cap, repeats=repeats,
               device_ms_runs=[round(t, 3) for t in times], device_ms_median=round(statistics.median(times), 3),
               device_us_per_entry=round(1e3 * statistics.median(times) / cap, 3),
               n_cells={cell_name(k): int(n) for k, n in zip(keys, n_cells) if k != 0xFFFF}, device_scores=device)
    print(json.dumps(res), flush=True)
    if host_entries > 0:
        host_times, host = [], None
        for i in range(host_entries):
            print("host LP path, entry %d of %s ..." % (i, fixture), flush=True)
            t = time.perf_counter()
            host = batch.scores(i)
            host_times.append(time.perf_counter() - t)
        per = statistics.median(host_times)
        res.update(host_s_per_entry_runs=[round(t, 3) for t in host_times], host_s_per_entry=round(per, 3),
                   host_entries_timed=host_entries, host_batch_s_extrapolated=round(per * cap, 1), host_scores=host,
                   speedup_per_entry_extrapolated=round(per * cap / (statistics.median(times) * 1e-3), 1),
                   max_abs_difference=max(abs(device[k][0] - host[k][0]) for k in host))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap25", type=int, default=2048)
    ap.add_argument("--cap64", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-entries", type=int, default=3)
    ap.add_argument("--skip-host-64", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "emd_bench.json"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build(quiet=True)
    import torch
    results = dict(device=torch.cuda.get_device_name(0),
                   note="device: HIP events around scores_all(), median; host: wall clock of scores(i) per entry, "
                        "extrapolated to the batch")
    results["25x25"] = bench("side_effect_inputs.npz", args.cap25, args.repeats, args.host_entries)
    results["64x64"] = bench("side_effect_inputs_64.npz", args.cap64, args.repeats, 0 if args.skip_host_64 else 1)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(results, sort_keys=True))


if __name__ == "__main__":
    main()
