"""life_occupancy on board shapes without row kernels: this tree's LDS-counter kernel (k_occupancy_generic, reached through
slhip_life_occupancy in a timing-only build of this tree's library, -DSL_LIFE_OCCUPANCY_LDS: csrc/sl_abi.hip) against the
parent commit's library, same inputs, same process, runs alternated; and the derived-stream episode-end pass on a 13x17
queue (this tree's shipped library only: the parent refuses the shape).

    python tools/occupancy_generic_bench.py [--lds-lib PATH] [--parent-lib PATH] [--out profiles/occupancy_generic_bench.json]
    python tools/occupancy_generic_bench.py --build-lds             # builds the timing-only library first (needs build())
    python tools/occupancy_generic_bench.py --build-parent REV      # builds REV's library from a git worktree first

Boards: random palette cells with spawners (tests/util.random_boards kind 0 plus one spawner per 50 cells), spawn_prob
0.3, 1000 steps.  Timing: HIP events around the one call, one warm-up call per library and shape, then 5 timed calls
per library, alternating between the two; the median is quoted and every run is kept.  The two libraries' counts and
generators are compared bit for bit before anything is timed.
"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = (((13, 17), 4096), ((33, 64), 1024))
STEPS, REPEATS = 1000, 5


def build_parent(rev, dest):
    """REV's library, built in a detached worktree under a temporary directory, copied to `dest`."""
    tmp = tempfile.mkdtemp(prefix="occ_parent_")
    tree = os.path.join(tmp, "tree")
    subprocess.check_call(["git", "-C", REPO, "worktree", "add", "--detach", tree, rev])
    try:
        subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build(quiet=True)"], cwd=tree)
        os.makedirs(os.path.dirname(dest), exist_ok=True)
        shutil.copy(os.path.join(tree, "safelife_amd", "libsafelife_hip.so"), dest)
    finally:
        subprocess.call(["git", "-C", REPO, "worktree", "remove", "--force", tree])
        shutil.rmtree(tmp, ignore_errors=True)
    return dest


def build_lds(dest):
    """This tree's library with slhip_life_occupancy routed to k_occupancy_generic: sl_abi.hip compiled again with
    -DSL_LIFE_OCCUPANCY_LDS, linked with the objects build() left under build/obj."""
    import __graft_entry__ as g
    g.build(quiet=True)
    objdir = os.path.join(REPO, "build", "obj")
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    abi = os.path.join(os.path.dirname(dest), "sl_abi_lds.hip.o")
    flags = [f for f in g.HIP_FLAGS if f != "-shared"]
    subprocess.check_call([g.HIPCC] + flags + ["-DSL_LIFE_OCCUPANCY_LDS", "-c", os.path.join(g.CSRC, "sl_abi.hip"), "-o", abi])
    objs = [abi] + sorted(os.path.join(objdir, n) for n in os.listdir(objdir) if n.endswith(".o") and n != "sl_abi.hip.o")
    subprocess.check_call([g.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-fno-gpu-rdc"] + objs + ["-o", dest])
    return dest


def occupancy_fn(lib):
    f = lib.slhip_life_occupancy
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    return f


def make_boards(rng, B, H, W):
    from tests import util
    b = util.random_boards(rng, B, H, W, 0)
    spawn = np.array([152, 152 | 0x200, 152 | 0x600, 144 | 0x800], np.uint16)
    for k in range(B):
        cells = rng.integers(0, H * W, max(2, H * W // 50))
        b[k].reshape(-1)[cells] = spawn[np.arange(len(cells)) % 4]
    return b


def time_call(torch, call):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    call()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def bench_occupancy(torch, here, parent, shape, B):
    from safelife_amd import _hip, speedups as sp
    from tests import util
    H, W = shape
    rng = np.random.default_rng(H * 100 + W)
    d_b = sp._to_device(make_boards(rng, B, H, W), np.uint16)
    d_p = torch.full((B,), 0.3, dtype=torch.float32, device=d_b.device)
    words = sp._to_device(util.random_rng_words(rng, B), np.uint64)
    st = _hip.current_stream_ptr()
    outs = {}

    def run(fn, name):
        d_rng = words.clone()
        counts = outs.setdefault(name, torch.empty((B, H, W, 8), dtype=torch.int32, device=d_b.device))
        torch.cuda.synchronize()

        def call():
            rc = fn(d_b.data_ptr(), counts.data_ptr(), B, H, W, d_p.data_ptr(), STEPS, d_rng.data_ptr(), st)
            assert rc == 0, rc
        return time_call(torch, call), d_rng

    libs = (("this_tree", here), ("parent", parent))
    after = {name: run(fn, name)[1] for name, fn in libs}           # warm-up, and the outputs to compare
    same = bool(torch.equal(outs["this_tree"], outs["parent"]) and torch.equal(after["this_tree"], after["parent"]))
    if not same or int(outs["this_tree"].sum().item()) <= 0:       # different (or no) work: the timings would mean nothing
        sys.exit("%dx%d: the two libraries' counts or generators differ, or nothing was counted" % (H, W))
    runs = {name: [] for name, _ in libs}
    for _ in range(REPEATS):
        for name, fn in libs:
            runs[name].append(round(run(fn, name)[0], 3))
    res = dict(shape=[H, W], boards=B, steps=STEPS, outputs_identical=same,
               counted=int(outs["this_tree"].sum().item()))
    for name, _ in libs:
        res[name + "_ms_runs"] = runs[name]
        res[name + "_ms_median"] = round(statistics.median(runs[name]), 3)
    res["parent_over_this_tree"] = round(res["parent_ms_median"] / res["this_tree_ms_median"], 3)
    return res


def bench_pass(torch, capacity=2048, n_samples=1000):
    """The derived-stream pass (slhip_side_effects, derive_streams = 1) on a full 13x17 queue of `capacity` entries."""
    from safelife_amd import _hip
    from safelife_amd.levels import Level, LevelPool, _device_counts
    from safelife_amd.vector_env import SafeLifeVectorEnv
    H, W = 13, 17
    rng = np.random.default_rng(1317)
    boards = make_boards(rng, 16, H, W)
    pool = LevelPool([Level(b, agent_locs=np.zeros((0, 2), int), spawn_prob=0.3) for b in boards], counts_fn=_device_counts)
    env = SafeLifeVectorEnv(pool, 8, with_obs=False)
    dev, K = env.device, _hip.SL_SE_MAX_KEYS
    rec = np.zeros((capacity, 8), np.int32)
    rec[:, 0] = np.arange(capacity)
    rec[:, 1] = np.arange(capacity) % 16
    rec[:, 2] = 100
    rec[:, 4] = np.float32(0.3).view(np.int32)
    finals = make_boards(rng, capacity, H, W)
    bufs = dict(count=torch.tensor([capacity], dtype=torch.int32, device=dev), records=torch.from_numpy(rec).to(dev),
                boards=torch.from_numpy(finals.view(np.int16)).to(dev))
    q = _hip.EpisodeQueue()
    q.capacity, q.env_base = capacity, 0
    q.count, q.records, q.boards = (bufs[k].data_ptr() for k in ("count", "records", "boards"))
    out = dict(work_boards=torch.empty((2 * capacity, H, W), dtype=torch.int16, device=dev),
               work_prob=torch.empty(2 * capacity, dtype=torch.float32, device=dev),
               work_steps=torch.empty(2 * capacity, dtype=torch.int32, device=dev),
               work_rng=torch.empty((2 * capacity, 4), dtype=torch.int64, device=dev),
               counts=torch.empty((2, capacity, H, W, 8), dtype=torch.int32, device=dev),
               keys=torch.empty((capacity, K), dtype=torch.int16, device=dev),
               life_dist=torch.empty((capacity, 2, 8, H, W), dtype=torch.float64, device=dev),
               type_masks=torch.empty((capacity, 2, K - 8, H, W), dtype=torch.uint8, device=dev))
    args = [_hip.ptr(out[k]) for k in ("work_boards", "work_prob", "work_steps", "work_rng", "counts", "keys", "life_dist",
                                       "type_masks")]

    def call():
        _hip.check(_hip.lib().slhip_side_effects(env._sref, C.byref(q), n_samples, 1, *args, _hip.current_stream_ptr()))
    torch.cuda.synchronize()
    time_call(torch, call)
    runs = [round(time_call(torch, call), 3) for _ in range(REPEATS)]
    if int(out["counts"].sum().item()) <= 0:
        sys.exit("pass: nothing was counted")
    return dict(shape=[H, W], entries=capacity, num_steps=100, num_samples=n_samples, pass_ms_runs=runs,
                pass_ms_median=round(statistics.median(runs), 3),
                pass_us_per_entry=round(1000 * statistics.median(runs) / capacity, 3),
                counted=int(out["counts"].sum().item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.path.join(REPO, "build", "parent", "libsafelife_hip_parent.so"))
    ap.add_argument("--build-parent", metavar="REV", default=None)
    ap.add_argument("--lds-lib", default=os.path.join(REPO, "build", "parent", "libsafelife_hip_occlds.so"))
    ap.add_argument("--build-lds", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occupancy_generic_bench.json"))
    a = ap.parse_args()
    if a.build_parent:
        build_parent(a.build_parent, a.parent_lib)
    if a.build_lds:
        build_lds(a.lds_lib)
    if not os.path.exists(a.parent_lib):
        sys.exit("no parent library at %s (--build-parent REV builds one)" % a.parent_lib)
    if not os.path.exists(a.lds_lib):
        sys.exit("no timing-only library at %s (--build-lds builds one)" % a.lds_lib)
    import safelife_amd  # noqa: F401  (ahead of torch)
    import torch
    here = occupancy_fn(C.CDLL(a.lds_lib))
    parent = occupancy_fn(C.CDLL(a.parent_lib))
    res = dict(device=torch.cuda.get_device_name(0),
               note="HIP events around one call, 1 warm-up + %d alternated runs per library, median; this_tree = "
                    "k_occupancy_generic (uint16 counters in LDS) through slhip_life_occupancy of the timing-only build; "
                    "parent = the parent commit's library (global read-modify-write per counted cell); both loaded by "
                    "path in one process; first measurement of these shapes" % REPEATS)
    for shape, B in SHAPES:
        res["%dx%d" % shape] = bench_occupancy(torch, here, parent, shape, B)
        print(json.dumps(res["%dx%d" % shape]), flush=True)
    res["pass_13x17"] = bench_pass(torch)
    print(json.dumps(res["pass_13x17"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
