"""Throughput of procedural generation: Metropolis chains per second of the device kernel (slhip_gen_pattern_batch) at
1, 64, 2048 and 16384 problems per launch, and levels per second of proc_gen.gen_games, each beside the yardstick: the
compiled reference gen_pattern on ONE CPU core, timed in this script (oracle/_ref; skipped when it has not been built).

Two problem kinds, both 26x26 with a fenced region mask: the green layer of the "prune medium" region at period 1, and the
same at period 2 with max_iter cut to 5 (a period-2 chain at the default limit mostly runs to it).

    python tools/procgen_bench.py [--out profiles/procgen_bench.json] [--quick]

Every figure is the best of --repeats timed runs after one warm-up; a run is bracketed by device synchronisations and its
inputs are built outside it.  Chains of one launch differ in their generator only, so their lengths differ as real ones do.
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
KINDS = {
    "26x26 period 1 (prune medium, green layer)": dict(period=1, kw=dict(min_fill=0.1, wall=(1, 20), tree=(1, 20))),
    "26x26 period 2, max_iter 5": dict(period=2, kw=dict(min_fill=0.1, wall=(1, 20), tree=(1, 20), max_iter=5)),
}


def problem(period):
    """a 26x26 board with one fenced region of about a third of it, as proc_gen would hand it to the sampler"""
    rng = np.random.default_rng(1)
    regions = proc_gen.partition(rng, (26, 26), 2, 3)
    region = regions == 1
    rim = proc_gen._grow(region) & ~region
    mask = (region * 7 + rim * 4).astype(np.int32)
    fence = region & ~proc_gen._shrink(region)
    board = np.zeros((26, 26), np.uint16)
    board[fence] = 16
    mask[fence] &= ~3
    if period == 1:
        mask &= ~2
    return board, mask


def words_for(n, base=0):
    return np.stack([speedups.pcg64_words6(np.random.PCG64(base + k)) for k in range(n)]).astype(np.uint64)


def best_of(fn, repeats):
    fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "procgen_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small sizes only (a functional check)")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import oracle
    ref = oracle.load_ref()
    ref = ref if ref is not None and hasattr(ref, "gen_pattern") else None
    sizes = (1, 64) if args.quick else (1, 64, 2048, 16384)
    level_counts = (8,) if args.quick else (64, 2048)
    result = {"device": torch.cuda.get_device_name(0), "chains": {}, "levels": {}, "repeats": args.repeats,
              "yardstick": "compiled reference gen_pattern, one CPU core" if ref else None}
    dev = torch.device("cuda", 0)
    for kind, k in KINDS.items():
        board, mask = problem(k["period"])
        params = speedups.gen_pattern_params(**k["kw"])
        row = {"device_chains_per_s": {}, "mean_iterations": {}}
        for n in sizes:
            d_b = torch.from_numpy(np.repeat(board[None], n, 0).view(np.int16)).to(dev)
            d_m = torch.from_numpy(np.repeat(mask[None], n, 0)).to(dev)
            d_p = torch.from_numpy(np.repeat(params[None], n, 0)).to(dev)
            w0 = torch.from_numpy(words_for(n).view(np.int64)).to(dev)
            state = {}

            def run():
                rng = w0.clone()
                torch.cuda.synchronize()
                state["out"] = speedups.gen_pattern_batch(d_b, d_m, k["period"], None, d_p, rng)
                torch.cuda.synchronize()
            dt = best_of(run, args.repeats)
            row["device_chains_per_s"][str(n)] = n / dt
            row["mean_iterations"][str(n)] = float(state["out"][2].float().mean())
            print("%-44s %6d chains  %10.1f chains/s  (%.2f ms, mean %.0f iterations)"
                  % (kind, n, n / dt, dt * 1e3, row["mean_iterations"][str(n)]), flush=True)
        if ref is not None:
            n = 16 if args.quick else 256
            bg = np.random.PCG64(0)
            ref.set_bit_generator(bg)
            w = words_for(n)

            def run_ref():
                for j in range(n):
                    speedups.pcg64_set_words6(bg, w[j])
                    try:
                        ref.gen_pattern(board, mask, k["period"], **k["kw"])
                    except ref.MaxIterException:
                        pass
            dt = best_of(run_ref, args.repeats)
            row["reference_cpu_chains_per_s"] = n / dt
            print("%-44s %6d chains  %10.1f chains/s  (compiled reference, one CPU core)" % (kind, n, n / dt), flush=True)
        result["chains"][kind] = row
    params = proc_gen.load_params(os.path.join(SPECS, "prune-still.yaml"), defaults=os.path.join(SPECS, "_defaults.yaml"))
    backends = {"device": None}
    if ref is not None:
        backends["reference_cpu"] = proc_gen.function_backend(ref)
    for n in level_counts:
        row = {}
        for name, backend in backends.items():
            calls = {"n": 0, "t": 0.0}

            def timed(requests, backend=backend):
                t0 = time.perf_counter()
                out = (backend or proc_gen.device_backend)(requests)
                calls["n"] += len(requests)
                calls["t"] += time.perf_counter() - t0
                return out
            t0 = time.perf_counter()
            proc_gen.gen_games(params, range(n), backend=timed)
            dt = time.perf_counter() - t0
            row[name] = {"levels_per_s": n / dt, "seconds": dt, "pattern_calls": calls["n"], "seconds_in_backend": calls["t"]}
            print("gen_games(prune-still) %5d levels  %-14s %8.1f levels/s  (%.2f s, %.2f s of it in the backend, %d chains)"
                  % (n, name, n / dt, dt, calls["t"], calls["n"]), flush=True)
        result["levels"][str(n)] = row
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
