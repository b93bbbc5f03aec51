"""CPU suite for the pattern generator: the fixture of the compiled reference's gen_pattern against the plain-Python
restatement (tests/gen_pattern_ref.py), the wrong readings the fixture tells apart, the host-compilable half of the kernel
(safelife_amd/csrc/sl_gen_pattern_core.h) run on the CPU under AddressSanitizer, and the argument checks of
speedups.gen_pattern.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from safelife_amd import _hip, speedups
from tests import gen_pattern_ref as gpr
from tests import util

REPO = util.REPO
FIXTURE = os.path.join(REPO, "tests", "golden", "gen_pattern_cases.npz")
MIN_MARGIN = 1e-12


@pytest.fixture(scope="module")
def cases():
    return gpr.load_cases(FIXTURE)


@pytest.fixture(scope="module")
def restated(cases):
    """every case through the restatement, once"""
    return [gpr.run_case(c) for c in cases]


def test_fixture_covers_what_it_should(cases):
    names = [c["name"] for c in cases]
    assert len(names) == len(set(names)) and len(names) >= 55
    shapes = {(c["period"],) + c["board"].shape for c in cases}
    assert {(1, 3, 3), (1, 4, 5), (1, 8, 8), (1, 10, 10), (1, 26, 26), (2, 3, 3), (2, 5, 5), (2, 10, 10), (3, 4, 5)} <= shapes
    assert {c["status"] for c in cases} == {0, -1}
    for period in (1, 2, 3):
        assert {c["status"] for c in cases if c["period"] == period} == {0, -1}, period
    assert {int(c["w1"][4]) for c in cases} == {0, 1}               # both end states of the buffered half
    assert any(int(c["w0"][4]) == 1 for c in cases)                 # and a generator that starts with one
    assert any(c["seeds"] is None for c in cases) and any(c["seeds"] is not None and not c["seeds"].any() for c in cases)
    assert any(c["seeds"] is not None and c["seeds"].any() for c in cases)
    assert any(not c["mask"].any() for c in cases)                  # all-zero mask: max-iter having drawn nothing
    for c in cases:
        if not (c["mask"] & gpr.NEW_CELL).any():
            assert c["status"] == -1 and c["iters"] == 0 and (c["period"] > 1 or np.array_equal(c["w0"], c["w1"]))
    assert any((c["mask"] == gpr.INCLUDE_VIOLATIONS).any() for c in cases)
    assert any(not (c["mask"] & gpr.CAN_OSCILLATE).any() and c["mask"].any() for c in cases)
    assert any(c["kwargs"]["min_fill"] == 0 for c in cases)
    assert {0.1, 1.5} <= {c["kwargs"]["temperature"] for c in cases}
    assert any(c["period"] > 1 and (c["board"] & 128).any() for c in cases)      # a spawner under the layer pass
    for c in cases:
        if c["status"] == -1:
            assert np.array_equal(c["out"], c["board"]), c["name"]
        if c["period"] > 1:
            assert c["iters"] <= 400, c["name"]


def test_every_case_keeps_the_exp_margin(cases, restated):
    """exp() is not bit-defined across libraries: a pick can differ only within a few ulps times the number of candidates
    (about 1e-14) of a cumulative probability, so every case must stay 1e-12 clear of one."""
    for c, got in zip(cases, restated):
        assert c["margin"] >= MIN_MARGIN, c["name"]
        assert got["margin"] >= MIN_MARGIN, c["name"]
        assert got["margin"] == c["margin"] or got["margin"] == pytest.approx(c["margin"], rel=1e-6), c["name"]


def test_restatement_reproduces_every_case(cases, restated):
    for c, got in zip(cases, restated):
        assert got["status"] == c["status"], c["name"]
        assert np.array_equal(got["board"], c["out"]), c["name"]
        assert np.array_equal(got["words"], c["w1"]), c["name"]
        assert got["iterations"] == c["iters"], c["name"]


@pytest.mark.parametrize("reading", [r for r in gpr.WRONG_READINGS if r != "empty_set_size0"])
def test_fixture_tells_a_wrong_reading_apart(cases, reading):
    order = sorted(cases, key=lambda c: c["iters"])
    for c in order:
        if c["iters"] == 0 and c["period"] == 1:
            continue
        if not gpr.same_as_recorded(c, gpr.run_case(c, readings=(reading,))):
            return
    pytest.fail("no case of the fixture differs under the wrong reading %r" % reading)


def test_an_empty_set_is_never_sampled(cases):
    """iset_sample hands out any index of the backing array when its set is empty, and a restatement that sampled such a set
    as "size 0" would be wrong -- but no call of gen_pattern can tell: BAD and SEEDS are only sampled when they have members,
    and UNMASKED is empty only when no cell carries NEW_CELL, where max_iter * 0 iterations run.  So this reading cannot
    be told apart by ANY fixture of this function; what is pinned instead is that the cases with empty sets (an all-zero
    mask, empty seeds) come out the same under it, and that the empty-area cases run no iteration."""
    picked = [c for c in cases if not c["mask"].any() or (c["seeds"] is not None and not c["seeds"].any())]
    assert len(picked) >= 4
    for c in picked:
        assert gpr.same_as_recorded(c, gpr.run_case(c, readings=("empty_set_size0",))), c["name"]


def test_draw_paths_follow_numpy():
    """The restated 32-bit / 64-bit draws against numpy's own generator, interleaved."""
    bg = np.random.PCG64(7)
    gen = np.random.Generator(bg)
    mine = gpr.Pcg64(gpr.words6(bg))
    for k in range(200):
        if k % 3 == 0:
            assert mine.next_double() == gen.random()
        else:
            assert mine.next32() == int(gen.integers(0, 1 << 32, dtype=np.uint32))
        assert np.array_equal(mine.words(), gpr.words6(bg))
    assert mine.random_int(0) == 0
    for high in (1, 2, 3, 4, 5, 8, 9, 100, 676):
        assert 0 <= mine.random_int(high) < high


def test_six_word_helpers_round_trip():
    bg = np.random.PCG64(11)
    np.random.Generator(bg).integers(0, 1 << 32, dtype=np.uint32)
    w = speedups.pcg64_words6(bg)
    assert w.dtype == np.uint64 and w.shape == (6,) and int(w[4]) == 1
    assert np.array_equal(w, gpr.words6(bg)) and np.array_equal(w[:4], speedups.pcg64_words(bg))
    other = np.random.PCG64(12)
    speedups.pcg64_set_words6(other, w)
    assert other.state == bg.state
    assert np.random.Generator(other).integers(0, 1 << 32, dtype=np.uint32) == np.random.Generator(bg).integers(
        0, 1 << 32, dtype=np.uint32)


def test_penalty_mapping():
    p = speedups.gen_pattern_params(40, 0.2, 0.5, 0.3, alive=(1, 4), wall=(2, 7), tree=(3, 3.5))
    assert p.dtype == np.float64 and p.tolist() == [40, 0.2, 0.5, 0.3, 0, 0, 2, 5, 1, 3, 3, 0.5]
    assert np.array_equal(p[4:], gpr.penalties(alive=(1, 4), wall=(2, 7), tree=(3, 3.5)))
    with pytest.raises(TypeError):
        speedups.gen_pattern_params(alive=1.0)


def test_gen_pattern_argument_errors_and_exceptions():
    assert issubclass(speedups.BoardGenException, Exception)
    for cls in (speedups.MaxIterException, speedups.BadProbabilityException, speedups.InsufficientAreaException):
        assert issubclass(cls, speedups.BoardGenException)
    b, m = np.zeros((5, 5), np.uint16), np.ones((5, 5), np.int32)
    with pytest.raises(ValueError, match="Pattern period must be larger than 0."):
        speedups.gen_pattern(b, m, 0)
    with pytest.raises(ValueError, match="must all be dimension 2"):
        speedups.gen_pattern(b[0], m, 1)
    with pytest.raises(ValueError, match="must all be dimension 2"):
        speedups.gen_pattern(b, m, 1, seeds=m[0])
    with pytest.raises(ValueError, match="Board must be at least 3x3."):
        speedups.gen_pattern(b[:2], m[:2], 1)
    with pytest.raises(ValueError, match="must all have the same shape"):
        speedups.gen_pattern(b, m[:4], 1)
    with pytest.raises(ValueError, match="must all have the same shape"):
        speedups.gen_pattern(b, m, 1, seeds=np.ones((5, 6), np.int32))
    with pytest.raises(TypeError):
        speedups.gen_pattern(b, m, 1.5)
    with pytest.raises(TypeError):
        speedups.gen_pattern(b, m, 1, wall=100)
    with pytest.raises(ValueError, match="supports boards from 3x3 to 64x64 and periods 1 to 4"):
        speedups.gen_pattern(b, m, 5)
    with pytest.raises(ValueError, match="supports boards"):
        speedups.gen_pattern(np.zeros((65, 5), np.uint16), np.ones((65, 5), np.int32), 1)
    with pytest.raises(ValueError, match="supports boards"):
        speedups.gen_pattern_batch(np.zeros((2, 5, 70), np.uint16), np.ones((2, 5, 70), np.int32), 1,
                                   rng=np.zeros((2, 6), np.uint64))


def test_library_exports_the_entry_points():
    header = open(os.path.join(REPO, "include", "safelife_hip.h")).read()
    lib = _hip.lib()
    for name in ("slhip_gen_pattern_workspace_bytes", "slhip_gen_pattern_batch"):
        assert name in _hip.EXPORTS and hasattr(lib, name) and name + "(" in header
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13
    # sizing and refusals are host code: no device is touched
    assert lib.slhip_gen_pattern_workspace_bytes(8, 26, 26, 1) == 0
    assert lib.slhip_gen_pattern_workspace_bytes(8, 64, 64, 4) > 8 * 65536
    assert lib.slhip_gen_pattern_workspace_bytes(8, 65, 64, 4) == 0
    args = [None] * 8
    assert lib.slhip_gen_pattern_batch(*args, 1, 2, 3, 1, None, 0, None) == _hip.SL_E_SHAPE
    assert lib.slhip_gen_pattern_batch(*args, 1, 3, 3, 0, None, 0, None) == _hip.SL_E_ARG
    assert lib.slhip_gen_pattern_batch(*args, 1, 3, 65, 1, None, 0, None) == _hip.SL_E_UNSUPPORTED
    assert lib.slhip_gen_pattern_batch(*args, 1, 3, 3, 5, None, 0, None) == _hip.SL_E_UNSUPPORTED
    assert lib.slhip_gen_pattern_batch(*args, 1, 3, 3, 1, None, 0, None) == _hip.SL_E_ARG       # null pointers
    assert lib.slhip_gen_pattern_batch(*args, 0, 3, 3, 1, None, 0, None) == 0


def _write_cases_bin(path, cases):
    """the recorded cases in the flat layout tests/gen_pattern_host_check.cpp reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            H, W = c["board"].shape
            layers, w_after_layers = gpr.layers_of(c["board"], c["period"], c["w0"])
            params = speedups.gen_pattern_params(**c["kwargs"])
            f.write(struct.pack("<6i", H, W, c["period"], int(c["seeds"] is not None), c["status"], c["iters"]))
            f.write(params.astype("<f8").tobytes())
            f.write(np.asarray(w_after_layers, "<u8").tobytes())
            f.write(np.asarray(c["w1"], "<u8").tobytes())
            f.write(np.stack(layers).astype("<u2").tobytes())
            f.write(np.asarray(c["mask"], "<i4").tobytes())
            if c["seeds"] is not None:
                f.write(np.asarray(c["seeds"], "<i4").tobytes())
            f.write(np.asarray(c["out"], "<u2").tobytes())


def test_kernel_core_on_the_host_under_sanitizers(cases, tmp_path):
    """The functions the kernel is made of, compiled for the CPU with -fsanitize=address,undefined into a stand-alone program:
    validation, workspace sizing, the state layout, made-up chains at the extreme shapes, and EVERY recorded case -- walking
    the candidates one by one, and (depth 1) slot by slot as the wavefront's lanes do."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gen_pattern_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "gen_pattern_host_check.cpp"),
                           "-o", exe])
    blob = str(tmp_path / "cases.bin")
    _write_cases_bin(blob, cases)
    run = subprocess.run([exe, blob], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "all checks held" in run.stdout, run.stdout[-4000:]
    assert "%d recorded cases" % len(cases) in run.stdout
