#!/usr/bin/env python
"""
Times the device renderer (safelife_amd.render.render_batch -> slhip_render_boards, csrc/sl_render.hip) on

    a  1000 frames of 25x25 boards             (a 1000-step board history)
    b  8192 envs of 25x25, view 15x15, 3 exits (a frame of every env of a training batch)
    c  200 frames of 64x64 boards

for both kernel variants (cells staged in LDS per workgroup / decoded by every lane), each in a child process of its
own (SAFELIFE_RENDER_VARIANT is read once per process).  Device time: HIP events around the launch, buffers allocated
before timing, one full-size warm-up, median of five.  Reports us per frame and output GB/s, and beside them the
store-side figure of tools/ubench/copy_bw.hip from the same session: that kernel writes one byte for every two it
reads, so its store side is a third of the best rate it prints for its largest arrays.  Writes profiles/render_bench.json.

    python tools/render_bench.py [--repeats 5] [--skip-copy-bw]

Every child runs under a time limit; the first one that fails, faults or runs over ends the run (exit status 1).
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
COPY_BW_SRC = os.path.join(REPO, "tools", "ubench", "copy_bw.hip")
COPY_BW_BIN = os.path.join(REPO, "tools", "ubench", "copy_bw.bin")
CHILD_LIMIT_S = 120


def workloads():
    rng = np.random.default_rng(0)
    cells = np.array([0, 0, 0, 9, 9, 16, 17, 32788, 152, 272, 122], np.uint16)

    def boards(n, h, w):
        b = cells[rng.integers(0, len(cells), (n, h, w))] | (rng.integers(0, 8, (n, h, w)).astype(np.uint16) << 9)
        return b, rng.integers(0, 8, (n, h, w)).astype(np.uint16) << 9
    yield "a_1000x25x25", boards(1000, 25, 25), None
    yield "b_8192x25x25_view15", boards(8192, 25, 25), (15, 15)
    yield "c_200x64x64", boards(200, 64, 64), None


def child(repeats):
    import torch
    from safelife_amd import _hip, render
    dev = _hip.device()
    sheet = render.device_sheet()
    rng = np.random.default_rng(1)
    result = {}
    for name, (b, g), view in workloads():
        n, h, w = b.shape
        bt = torch.from_numpy(b.view(np.int16)).to(dev)
        gt = torch.from_numpy(g.view(np.int16)).to(dev)
        kw = {}
        if view is not None:
            centers = np.stack([rng.integers(0, h, n), rng.integers(0, w, n)], axis=1).astype(np.int32)
            kw = dict(view_size=view, centers=torch.from_numpy(centers).to(dev),
                      exits=torch.from_numpy(rng.integers(0, h * w, (n, 3)).astype(np.int32)).to(dev))
        vh, vw = view or (h, w)
        out = torch.empty((n, vh * 14, vw * 14, 3), dtype=torch.uint8, device=dev)
        render.render_batch(bt, gt, sheet, out=out, **kw)          # full-size warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            render.render_batch(bt, gt, sheet, out=out, **kw)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = statistics.median(times)
        result[name] = {"frames": n, "out_bytes": out.numel(), "device_ms_runs": [round(t, 4) for t in times],
                        "device_ms_median": round(ms, 4), "us_per_frame": round(ms * 1e3 / n, 3),
                        "out_GBps": round(out.numel() / ms * 1e-6, 1)}
        del out
    print("RENDER_BENCH " + json.dumps(result))


def run_child(variant, repeats):
    env = dict(os.environ, SAFELIFE_RENDER_VARIANT=variant)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(repeats)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_LIMIT_S)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        raise SystemExit("render_bench: variant %s ended with status %d; stopping" % (variant, p.returncode))
    line = [l for l in p.stdout.splitlines() if l.startswith("RENDER_BENCH ")][-1]
    return json.loads(line[len("RENDER_BENCH "):])


def copy_bw():
    if not os.path.exists(COPY_BW_BIN):
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3",
                               COPY_BW_SRC, "-o", COPY_BW_BIN])
    p = subprocess.run([COPY_BW_BIN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_LIMIT_S)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        raise SystemExit("render_bench: copy_bw ended with status %d; stopping" % p.returncode)
    sections = p.stdout.split("---- ")
    lines = [l for l in sections[-1].splitlines() if "GB/s" in l and "read-only" not in l]
    best = max(float(re.search(r"([0-9.]+) GB/s", l).group(1)) for l in lines)
    return {"largest_arrays_best_GBps_moved": best, "store_side_GBps": round(best / 3.0, 1),
            "note": "copy_bw moves 2 bytes read + 1 written; the store side is a third of its rate"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--skip-copy-bw", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.repeats)
    report = {"variants": {}}
    if not args.skip_copy_bw:
        report["copy_bw"] = copy_bw()
    for variant in ("stage", "direct"):
        report["variants"][variant] = run_child(variant, args.repeats)
    store = report.get("copy_bw", {}).get("store_side_GBps")
    if store:
        for variant, r in report["variants"].items():
            for name, w in r.items():
                w["fraction_of_copy_bw_store_side"] = round(w["out_GBps"] / store, 3)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    path = os.path.join(REPO, "profiles", "render_bench.json")
    with open(path, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
