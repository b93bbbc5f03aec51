"""CPU suite for the batched region partition: the host-compilable half of the kernel (safelife_amd/csrc/sl_partition_core.h)
run on the CPU under AddressSanitizer against ``proc_gen.partition``, the model of numpy's draws held to numpy itself, the
request protocol of ``proc_gen.gen_games``, and the host side of the two entry points.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from safelife_amd import _hip, proc_gen, speedups
from tests import gen_pattern_ref as gpr
from tests import partition_cases as pc
from tests import util

REPO = util.REPO
SPECS = os.path.join(REPO, "tests", "golden", "procgen")


def spec(name):
    return proc_gen.load_params(os.path.join(SPECS, name + ".yaml"), defaults=os.path.join(SPECS, "_defaults.yaml"))


_memo = {}


def restated_backend(requests):
    """gen_pattern_ref.gen_pattern per request; equal requests (a pure function's argument) are answered from a memo"""
    out = []
    for rq in requests:
        assert type(rq) is proc_gen.PatternRequest          # a pattern backend never sees another kind of request
        key = (rq.board.tobytes(), rq.mask.tobytes(), None if rq.seeds is None else rq.seeds.tobytes(), rq.period,
               tuple(sorted(rq.kwargs.items())), np.asarray(rq.words).tobytes())
        if key not in _memo:
            g = gpr.gen_pattern(rq.board, rq.mask, rq.period, seeds=rq.seeds, words=rq.words, **rq.kwargs)
            _memo[key] = (g["board"], g["status"], g["words"])
        b, st, w = _memo[key]
        out.append((b.copy(), st, w.copy()))
    return out


# ---- the draws ---------------------------------------------------------------------------------------------------------------------

def test_draw_model_follows_numpy():
    """integers(0, n) and random() of the model against numpy's Generator, interleaved, the six words after every draw: 50
    generators x 400 draws with n up to 5000, starting with and without a buffered half."""
    pick = np.random.RandomState(1)
    for g in range(50):
        bg = np.random.PCG64(1000 + g)
        gen = np.random.Generator(bg)
        if g % 2:
            gen.integers(0, 1 << 32, dtype=np.uint32)
        mine = pc.Draws(speedups.pcg64_words6(bg))
        for k in range(400):
            kind = pick.randint(0, 4)
            if kind == 0:
                assert mine.random() == gen.random()
            else:
                n = 1 if kind == 1 and k % 5 == 0 else int(pick.randint(1, 5001))
                assert mine.integers(0, n) == int(gen.integers(0, n)), (g, k, n)
            assert np.array_equal(mine.words(), speedups.pcg64_words6(bg)), (g, k)


def test_draw_model_redraws_where_numpy_does():
    """The recipe's generators: the first 32-bit draw lands under Lemire's threshold, numpy draws a second one (the buffered
    half goes: has_uint32 is 0 after ONE call), and the model does the same."""
    found = pc.redraw_cases()
    assert len(found[(61, 59)]) == 19 and len(found[(63, 63)]) == 5 and len(found[(26, 26)]) == 3
    assert found[(61, 59)][0] == 4449616
    for (H, W), idx in found.items():
        for i in idx:
            w0 = pc.words_of(12345, advance=i)
            assert int(w0[4]) == 0
            bg = np.random.PCG64(0)
            speedups.pcg64_set_words6(bg, w0)
            got = int(np.random.Generator(bg).integers(0, H * W))
            w1 = speedups.pcg64_words6(bg)
            assert int(w1[4]) == 0 and not np.array_equal(w1[:2], w0[:2])       # two halves of one output: it redrew
            mine = pc.Draws(w0)
            assert mine.integers(0, H * W) == got and mine.redraws == 1 and np.array_equal(mine.words(), w1)


def test_partition_under_the_draw_model():
    """proc_gen.partition makes two kinds of draws; with the model in the generator's place it gives the same labels and
    leaves the same words, so the model is all a restatement needs."""
    for H, W, lo, hi in pc.SHAPES[:8]:
        w0 = pc.words_of(H * 100 + W + hi, buffered=bool(hi % 2))
        labels, w1 = pc.host(w0, (H, W), lo, hi)
        mine = pc.Draws(w0)
        assert np.array_equal(proc_gen.partition(mine, (H, W), min_regions=lo, max_regions=hi), labels)
        assert np.array_equal(mine.words(), w1)


# ---- the kernel's core on the host -------------------------------------------------------------------------------------------------

def host_cases():
    cases = []

    def add(shape, lo, hi, w0, room=None):
        labels, w1 = pc.host(w0, shape, lo, hi)
        cases.append({"shape": shape, "lo": lo, "hi": hi, "room": pc.room_for(lo, hi) if room is None else room, "w0": w0,
                      "w1": w1, "labels": labels})
        return cases[-1]

    for H, W, lo, hi in pc.SHAPES:
        for s in range(3 if H * W > 2000 else 6):
            add((H, W), lo, hi, pc.words_of(7000 + 10 * s + H, buffered=bool(s % 2)))
    for (H, W), idx in pc.redraw_cases().items():
        for i in idx[:3]:
            add((H, W), 3, 3, pc.words_of(12345, advance=i))
    add((64, 64), 7, 7, pc.words_of(5))                 # the largest state that still fits LDS
    add((26, 26), 0, -3, pc.words_of(6), room=1)        # clamped to one region
    add((26, 26), 4, 2, pc.words_of(7), room=8)         # max below min: min regions, more room than needed
    return cases


def test_kernel_core_on_the_host_under_sanitizers(tmp_path):
    """The functions the kernel is made of, compiled for the CPU with -fsanitize=address,undefined into a stand-alone program
    and put together as the kernel puts them together: validation, workspace sizing, the layout, the bounded draw, the region
    pick with crafted values that reach its fall-back, made-up problems at the extreme shapes, refusals -- and partitions of
    every shape under test, the redraw cases among them, against proc_gen.partition."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "partition_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "partition_host_check.cpp"),
                           "-o", exe])
    cases = host_cases()
    assert {int(c["w0"][4]) for c in cases} == {0, 1} and {int(c["w1"][4]) for c in cases} == {0, 1}
    assert any(c["labels"].max() < c["lo"] for c in cases)                  # fewer regions than drawn: no free seed cell
    assert any((c["labels"] != 0).sum() == (4 * 26 * 26) // 5 for c in cases if c["hi"] == 1)     # the lone region's stop
    blob = str(tmp_path / "cases.bin")
    pc.write_cases_bin(blob, cases)
    run = subprocess.run([exe, blob], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "all checks held" in run.stdout, run.stdout[-4000:]
    assert "%d recorded cases" % len(cases) in run.stdout


# ---- the entry points' host side ----------------------------------------------------------------------------------------------------

def layout_bytes(H, W, room):
    """the state's size as sl_partition_core.h lays it out: ctrl, a bitmap and a frontier per region, the labels"""
    cells = H * W
    return (64 + 8 * room * ((cells + 63) // 64) + 2 * room * cells + cells + 15) // 16 * 16


def test_library_exports_the_entry_points():
    header = open(os.path.join(REPO, "include", "safelife_hip.h")).read()
    lib = _hip.lib()
    for name in ("slhip_partition_workspace_bytes", "slhip_partition_batch"):
        assert name in _hip.EXPORTS and hasattr(lib, name) and name + "(" in header
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13
    # sizing and the call's own errors are host code: no device is touched
    size = lib.slhip_partition_workspace_bytes
    assert size(8, 26, 26, 5) == 0 and size(8, 26, 26, 8) == 0 and size(8, 64, 64, 7) == 0
    assert size(8, 64, 64, 8) == 8 * layout_bytes(64, 64, 8) > 8 * 65536
    assert size(8, 65, 64, 8) == 0 and size(8, 64, 2, 8) == 0 and size(8, 64, 64, 9) == 0 and size(0, 64, 64, 8) == 0
    for H in (3, 26, 48, 57, 60, 63, 64):
        for W in (3, 59, 61, 64):
            for room in range(1, 9):
                b = layout_bytes(H, W, room)
                assert size(3, H, W, room) == (3 * b if b > 65536 else 0), (H, W, room)
    assert layout_bytes(26, 26, 5) <= 8192 and layout_bytes(64, 64, 8) <= 73 * 1024
    args = [None] * 5
    assert lib.slhip_partition_batch(*args, -1, 26, 26, 3, None, 0, None) == _hip.SL_E_ARG
    assert lib.slhip_partition_batch(*args, 1, 26, 26, 0, None, 0, None) == _hip.SL_E_ARG
    assert lib.slhip_partition_batch(*args, 1, 26, 26, 9, None, 0, None) == _hip.SL_E_ARG
    assert lib.slhip_partition_batch(*args, 1, 26, 26, 3, None, 0, None) == _hip.SL_E_ARG         # null pointers
    assert lib.slhip_partition_batch(*args, 0, 26, 26, 3, None, 0, None) == 0
    assert (_hip.PARTITION_REFUSED, _hip.PARTITION_CAPPED) == (-4, -5)
    for text in ("#define SL_PARTITION_REFUSED (-4)", "#define SL_PARTITION_CAPPED (-5)", "#define SL_PARTITION_MAX_REGIONS 8"):
        assert text in header


# ---- the request protocol ----------------------------------------------------------------------------------------------------------

class RecordingPartition(object):
    def __init__(self):
        self.calls = []

    def __call__(self, requests):
        assert all(type(rq) is proc_gen.PartitionRequest for rq in requests)
        self.calls.append(len(requests))
        return proc_gen.host_partition_backend(requests)


def same_level(a, b):
    return (a.board.tobytes() == b.board.tobytes() and a.goals.tobytes() == b.goals.tobytes()
            and a.regions.tobytes() == b.regions.tobytes() and np.array_equal(a.agent_locs, b.agent_locs)
            and np.array_equal(a.initial_rng_words(), b.initial_rng_words()))


def test_partition_requests_go_out_once_per_round():
    params = spec("prune-still")
    seeds = list(range(300, 316))
    plain = proc_gen.gen_games(params, seeds, backend=restated_backend)         # no partition_backend: the host's
    recorder = RecordingPartition()
    got = proc_gen.gen_games(params, seeds, backend=restated_backend, partition_backend=recorder)
    assert recorder.calls == [len(seeds)]               # every level's partition, in ONE call, and never again
    for s, a, b in zip(seeds, plain, got):
        assert same_level(a, b), s
        assert a.regions.dtype == np.int16 and a.regions.shape == a.board.shape
        # the level's partition is what the host function makes of the level's generator at that point
        rng = np.random.default_rng(s)
        proc_gen._resolve(params.get("board_shape", (25, 25)), rng)
        proc_gen._resolve(params.get("min_performance", -1), rng)
        want = proc_gen.partition(rng, a.board.shape, **proc_gen._resolve(params.get("partitioning") or {}, rng))
        assert np.array_equal(a.regions, want), s


def test_request_and_host_backend():
    w0 = pc.words_of(77, buffered=True)
    rq = proc_gen.PartitionRequest(w0, (13, 20), 2, 4)
    (labels, w1), (labels2, w2) = proc_gen.host_partition_backend([rq, rq])
    want, want_w = pc.host(w0, (13, 20), 2, 4)
    assert np.array_equal(labels, want) and np.array_equal(w1, want_w) and labels.dtype == np.int16
    assert np.array_equal(labels2, want) and np.array_equal(w2, want_w)         # a request is a pure function's argument
    assert np.array_equal(rq.words, w0)
    d = proc_gen.PartitionRequest(w0, [26, 26])
    assert (d.shape, d.min_regions, d.max_regions) == ((26, 26), 2, 5)


def test_fill_pool_takes_a_partition_backend():
    from safelife_amd import levels
    params = spec("prune-still")
    first = proc_gen.gen_games(params, [300, 301], backend=restated_backend)
    pool = levels.LevelPool(first, counts_fn=util.oracle_counts, refreshable=True)
    recorder = RecordingPartition()
    new = proc_gen.fill_pool(pool, [0], params, [301], backend=restated_backend, partition_backend=recorder)
    assert recorder.calls == [1] and same_level(new[0], first[1])
