"""Throughput of the batched region partition: partitions per second of the device kernel (slhip_partition_batch) at 1, 64,
2048 and 16384 problems per launch beside ``proc_gen.partition`` on ONE CPU core, timed in this script; and levels per
second of ``proc_gen.gen_games(prune-still)`` with the device partition against ``partition_backend=host_partition_backend``
(what generation did before the kernel), the seconds inside the partition backend split out.

    python tools/partition_bench.py [--out profiles/partition_bench.json] [--quick]

The problem is the specs' own: 26x26 with 2 to 3 regions, every problem of a launch on a generator of its own, so the
partitions' lengths differ as real ones do.  A kernel run is bracketed by device synchronisations, its inputs are on the
device before it, and it is repeated until a shape has been timed for a fifth of a second at least; the figure is the
median, the range beside it.  The two whole-level configurations alternate, --repeats times each after one warm-up of
each, on the same seeds; their levels are compared byte for byte; ``device_default`` says whether the ranges of the
repeats at the largest count leave the device ahead without overlapping -- the condition for it being gen_games' default.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from safelife_amd import proc_gen, speedups      # noqa: E402

SPECS = os.path.join(REPO, "tests", "golden", "procgen")
SHAPE, BOUNDS = (26, 26), (2, 3)


def words_for(n, base=0):
    return np.stack([speedups.pcg64_words6(np.random.PCG64(base + k)) for k in range(n)]).astype(np.uint64)


def spread(times):
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times)), "runs": len(times)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "partition_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small sizes only (a functional check)")
    args = ap.parse_args()
    sizes = (1, 64) if args.quick else (1, 64, 2048, 16384)
    level_counts = (8,) if args.quick else (64, 2048)
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "bounds": list(BOUNDS), "repeats": args.repeats,
              "partitions": {}, "levels": {}}

    # ---- the kernel alone ----
    for n in sizes:
        w0 = torch.from_numpy(words_for(n).view(np.int64)).to(dev)
        out = (torch.empty((n,) + SHAPE, dtype=torch.int16, device=dev), torch.empty((n, 6), dtype=torch.int64, device=dev),
               torch.empty((n,), dtype=torch.int32, device=dev))

        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            speedups.partition_batch(w0, SHAPE, BOUNDS[0], BOUNDS[1], out=out)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        run()
        times = []
        while len(times) < args.repeats or (sum(times) < 0.2 and len(times) < 2000):
            times.append(run())
        assert int(out[2].abs().max()) == 0
        row = spread(times)
        row["partitions_per_s"] = n / row["median"]
        row["mean_labelled_cells"] = float((out[0] != 0).sum()) / n
        result["partitions"][str(n)] = row
        print("device  %6d partitions  %12.1f partitions/s  (median %.3f ms, %.3f .. %.3f, %d runs)"
              % (n, row["partitions_per_s"], row["median"] * 1e3, row["min"] * 1e3, row["max"] * 1e3, row["runs"]), flush=True)
    n = 16 if args.quick else 128
    w = words_for(n)
    bg = np.random.PCG64(0)

    def run_host():
        t0 = time.perf_counter()
        for j in range(n):
            speedups.pcg64_set_words6(bg, w[j])
            proc_gen.partition(np.random.Generator(bg), SHAPE, BOUNDS[0], BOUNDS[1])
        return time.perf_counter() - t0
    run_host()
    row = spread([run_host() for _ in range(args.repeats)])
    row["partitions_per_s"] = n / row["median"]
    result["host_one_core"] = row
    print("host    %6d partitions  %12.1f partitions/s  (proc_gen.partition, one CPU core)" % (n, row["partitions_per_s"]),
          flush=True)

    # ---- whole levels ----
    params = proc_gen.load_params(os.path.join(SPECS, "prune-still.yaml"), defaults=os.path.join(SPECS, "_defaults.yaml"))
    backends = {"device_partition": proc_gen.device_partition_backend, "host_partition": proc_gen.host_partition_backend}
    for n in level_counts:
        runs = {name: [] for name in backends}
        levels = {}

        def once(name):
            spent = {"partition": 0.0, "pattern": 0.0}

            def timed_partition(requests):
                t0 = time.perf_counter()
                out = backends[name](requests)
                spent["partition"] += time.perf_counter() - t0
                return out

            def timed_pattern(requests):
                t0 = time.perf_counter()
                out = proc_gen.device_backend(requests)
                spent["pattern"] += time.perf_counter() - t0
                return out
            t0 = time.perf_counter()
            levels[name] = proc_gen.gen_games(params, range(n), backend=timed_pattern, partition_backend=timed_partition)
            return {"seconds": time.perf_counter() - t0, "seconds_in_partition_backend": spent["partition"],
                    "seconds_in_pattern_backend": spent["pattern"]}
        for name in backends:
            once(name)                                      # warm-up: code objects, allocator
        for _ in range(args.repeats):
            for name in backends:                           # alternating
                runs[name].append(once(name))
        same = all(a.board.tobytes() == b.board.tobytes() and a.goals.tobytes() == b.goals.tobytes()
                   and a.regions.tobytes() == b.regions.tobytes()
                   for a, b in zip(levels["device_partition"], levels["host_partition"]))
        row = {"levels_equal": bool(same)}
        for name in backends:
            secs = [r["seconds"] for r in runs[name]]
            row[name] = {"seconds": spread(secs), "levels_per_s": n / float(np.median(secs)),
                         "levels_per_s_range": [n / max(secs), n / min(secs)],
                         "seconds_in_partition_backend": float(np.median([r["seconds_in_partition_backend"] for r in runs[name]])),
                         "seconds_in_pattern_backend": float(np.median([r["seconds_in_pattern_backend"] for r in runs[name]]))}
            print("gen_games(prune-still) %5d levels  %-17s %8.1f levels/s  (%.2f .. %.2f s; %.3f s in the partition backend, "
                  "%.2f s in the pattern backend)" % (n, name, row[name]["levels_per_s"], min(secs), max(secs),
                                                       row[name]["seconds_in_partition_backend"],
                                                       row[name]["seconds_in_pattern_backend"]), flush=True)
        row["device_ahead_without_overlap"] = bool(row["device_partition"]["seconds"]["max"] < row["host_partition"]["seconds"]["min"])
        print("levels equal: %s; device partition ahead, ranges apart: %s" % (same, row["device_ahead_without_overlap"]), flush=True)
        result["levels"][str(n)] = row
    result["device_default"] = bool(result["levels"][str(level_counts[-1])]["device_ahead_without_overlap"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
