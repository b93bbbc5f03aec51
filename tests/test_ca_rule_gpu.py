"""GPU suite: the Life rule on every kernel family against its restatement (tests/ca_ref.py) -- boards, occupancy counts
and generator words, bit for bit -- on the constructed cases of tests/ca_rule_cases.py: every neighbourhood class as a
tile, the seam subset on every edge of every layout, the rule soup.  What the cases reach is asserted on the restatement
alone by tests/test_ca_rule_host.py, which also holds the restatement to the reference's recorded output and the oracle to
the restatement.  Where whole-array numpy would be slow (boards of more than 4096 cells past 7 steps, 300 steps, the fused
step's env) the oracle stands in.  Each test launches all of a shape's boards in one call, names the kernel family it
expects -- for advance_board on a row shape also WHICH row kernel, the one-wave k_advance_small or the four-wave
k_advance_rowlane, by the launcher's own rule and this device's CU count -- and compares exactly: no tolerance anywhere.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ca_ref as ref
from tests import ca_rule_cases as crc
from tests import util

pytestmark = pytest.mark.gpu

FORCED_GENERIC = os.environ.get("SAFELIFE_HIP_FORCE_GENERIC") == "1"
CASES = crc.cases()
CASE_IDS = ["%s-%s" % (crc.case_id(c), crc.family(c[1], c[2])) for c in CASES]       # "seam-25x25-row", "soup-3x3-generic"
ROW_CASES = [c for c in CASES if crc.family(c[1], c[2]) == "row"]


def case_family(case):
    """The family a case was listed under: the last word of its test id."""
    return CASE_IDS[CASES.index(case)].rsplit("-", 1)[1]


@pytest.fixture(scope="module")
def sp():
    from safelife_amd import speedups
    return speedups


def kernel_family(H, W, *tensors):
    """The family slhip_advance_board / slhip_advance_board_each take (sl_abi.hip): the row kernels where the shape has
    them, every board pointer is 16-byte aligned and the process does not force the size-generic ones."""
    aligned = all(t.data_ptr() % 16 == 0 for t in tensors)
    return "row" if crc.family(H, W) == "row" and aligned and not FORCED_GENERIC else "generic"


def advance_kernel(H, W, B):
    """Which row kernel launch_advance_t gives a batch on THIS device: the one-wave k_advance_small, or from 2 * n_cu
    workgroups of four waves on k_advance_rowlane."""
    import torch
    return crc.advance_kernel(H, W, B, torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


ROW_SIZES = (8, 10, 12, 15, 16, 20, 24, 25, 26, 30, 32, 40, 48, 64)    # SL_ROWLANE_SHAPES of sl_rowlane.hip, written out


def occupancy_family(H, W, n_steps):
    """slhip_life_occupancy's choice (sl_abi.hip), restated: the row kernels on a row shape for up to 65535 steps unless
    the process forces the size-generic ones -- whatever the alignment."""
    return "row" if H == W and H in ROW_SIZES and n_steps <= 65535 and not FORCED_GENERIC else "generic"


def _differing(got, want, w_dev, w_cpu):
    return np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1) | (w_dev != w_cpu).any(axis=1)).tolist()


def _advance(sp, d_b, b, n, want, want_w, what, family, kernel="small"):
    import torch
    H, W = b.boards.shape[1:]
    if family == "row":
        assert advance_kernel(H, W, len(b.boards)) == kernel, what
    d_r = sp._to_device(np.array(b.words), np.uint64)
    d_p = torch.from_numpy(np.array(b.p)).to(d_b.device)
    if not isinstance(n, int):
        n = torch.from_numpy(np.ascontiguousarray(n, dtype=np.int32)).to(d_b.device)
    out = sp.advance_board_batch(d_b, d_p, d_r, n)
    assert kernel_family(H, W, d_b, out) == family, what
    got, w_dev = sp._to_host(out, np.uint16), sp._to_host(d_r, np.uint64)
    bad = _differing(got, want, w_dev, want_w)
    assert not bad, "%dx%d %s on the %s kernels: boards %r of %d differ" % (H, W, what, family, bad[:20], len(got))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_advance_board_cases(sp, case):
    """advance_board_batch at n = 1 and n = 3, and slhip_advance_board_each with step counts 0-3 mixed in the batch."""
    kind, H, W = case
    b, r = crc.BATCHES[kind](H, W), crc.run(kind, H, W)
    d_b = sp._to_device(np.array(b.boards), np.uint16)
    family = "generic" if FORCED_GENERIC else crc.family(H, W)
    for n in (1, 3):
        _advance(sp, d_b, b, n, r["boards"][n], r["words"][n], "n = %d" % n, family)
    each = crc.each_steps(len(b.boards))
    want, want_w = crc.each_from(r, each)
    _advance(sp, d_b, b, each, want, want_w, "one step count per board", family)


@pytest.mark.parametrize("case", ROW_CASES, ids=[crc.case_id(c) for c in ROW_CASES])
def test_advance_board_off_alignment(sp, case):
    """The same boards behind a pointer 2 bytes past a 16-byte boundary: a row shape then falls to the size-generic
    kernel (slhip_advance_board's `aligned` test)."""
    import torch
    kind, H, W = case
    b, r = crc.BATCHES[kind](H, W), crc.run(kind, H, W)
    flat = sp._to_device(np.array(b.boards), np.uint16).reshape(-1)
    store = torch.zeros(flat.numel() + 8, dtype=flat.dtype, device=flat.device)
    d_b = store[1:1 + flat.numel()].view(b.boards.shape)
    d_b.copy_(flat.view(b.boards.shape))
    assert d_b.data_ptr() % 16 == 2 and d_b.is_contiguous()
    for n in (1, 3):
        _advance(sp, d_b, b, n, r["boards"][n], r["words"][n], "off alignment, n = %d" % n, "generic")


FOUR_WAVE = [(kind, H) for kind in ("seam", "soup") for H in crc.FOUR_WAVE_SHAPES]


@pytest.mark.parametrize("kind,H", FOUR_WAVE, ids=["%s-%dx%d" % (k, H, H) for k, H in FOUR_WAVE])
def test_four_wave_advance_kernel_cases(sp, kind, H):
    """Up to two workgroups per CU a batch runs on one-wave workgroups (launch_advance_t): the batches above never reach
    k_advance_rowlane -- the LDS board image, read_row / write_row, the halo refreshed through LDS between steps, boards
    wave * G + g of a workgroup.  The seam and soup batches repeated to 2 * 256 * NB + 1 boards do, on one shape per
    layout and per way a lane reaches its neighbour rows: n = 1, n = 3 and one step count per board.  What is expected
    of a copy is what the restatement expects of the board it copies."""
    if FORCED_GENERIC:
        return
    b, idx = crc.four_wave_batch(kind, H)
    r = crc.run(kind, H, H)
    d_b = sp._to_device(np.array(b.boards), np.uint16)
    for n in (1, 3):
        _advance(sp, d_b, b, n, r["boards"][n][idx], r["words"][n][idx], "four-wave kernel, n = %d" % n, "row", "four-wave")
    each = crc.each_steps(len(b.boards))
    want = np.stack([r["boards"][s] for s in range(4)])[each, idx]
    want_w = np.stack([r["words"][s] for s in range(4)])[each, idx]
    _advance(sp, d_b, b, each, want, want_w, "four-wave kernel, one step count per board", "row", "four-wave")


def _occupancy(sp, d_b, b, n, want, want_w, family):
    import torch
    H, W = b.boards.shape[1:]
    assert occupancy_family(H, W, n) == family
    d_r = sp._to_device(np.array(b.words), np.uint64)
    d_p = torch.from_numpy(np.array(b.p)).to(d_b.device)
    got = sp.life_occupancy_batch(d_b, d_p, d_r, n).cpu().numpy()
    w_dev = sp._to_host(d_r, np.uint64)
    bad = _differing(got, want, w_dev, want_w)
    assert not bad, "%dx%d occupancy over %d steps on the %s kernels: boards %r of %d differ" % (
        H, W, n, family, bad[:20], len(got))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_life_occupancy_cases(sp, case):
    """life_occupancy_batch over 1, 2 and 7 steps and over 20 (past the 15-step flush of the register counters); the
    64x64 seam and soup boards also over 300 (past the drain of the 8-bit counters; the oracle's counts).  The row
    kernels take every row shape (slhip_life_occupancy does not look at the alignment)."""
    kind, H, W = case
    b = crc.BATCHES[kind](H, W)
    d_b = sp._to_device(np.array(b.boards), np.uint16)
    family = "generic" if FORCED_GENERIC else case_family(case)
    steps = (1, 2, 7, crc.N_LONG) + ((300,) if (H, W) == (64, 64) and kind != "tile" else ())
    for n in steps:
        want, want_w = crc.expected_occupancy(kind, H, W, n)
        _occupancy(sp, d_b, b, n, want, want_w, family)
    if kind == "soup" and (H, W) == (64, 64):       # both instantiations of the 64-wide kernel in this launch
        vary = [crc.varying_colour_bits(x) for x in b.boards]
        assert 3 in vary and min(vary) <= 2


def test_the_generic_family_on_the_row_shapes():
    """The advance and occupancy cases of the row shapes once more with the row kernels switched off (the switch is read
    once per process, hence the subprocess)."""
    if FORCED_GENERIC:
        return
    env = dict(os.environ, SAFELIFE_HIP_FORCE_GENERIC="1")
    subprocess.check_call([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k",
                           "(test_advance_board_cases or test_life_occupancy_cases) and row"], env=env, cwd=util.REPO)


# ------------------------------------------------------------------------------- the side-effect pass's occupancy kernel

@pytest.mark.parametrize("kind", ("seam", "soup"))
@pytest.mark.parametrize("H,W", crc.PASS_SHAPES, ids=["%dx%d" % s for s in crc.PASS_SHAPES])
def test_side_effect_pass_occupancy(H, W, kind):
    """k_occupancy_generic (reached only through the pass): the boards as queue entries -- entry i has board 2 i as its
    level and board 2 i + 1 as its terminal board, no roll-forward, the caller's generator (derive_streams = 0) -- so
    counts[0, i] is life_occupancy of the one and counts[1, i] that of the other further along the same generator."""
    from safelife_amd.levels import Level, LevelPool
    from tests import test_side_effects_generic as seg
    assert crc.family(H, W) == "generic"            # (no row kernel: the pass takes the size-generic launcher)
    b = crc.BATCHES[kind](H, W)
    n = len(b.boards) // 2
    first, second = np.array(b.boards[0:2 * n:2]), np.array(b.boards[1:2 * n:2])
    p, words = np.array(b.p[0:2 * n:2]), np.array(b.words[0:2 * n:2])
    pool = LevelPool([Level(first[i], agent_locs=np.zeros((0, 2), int), spawn_prob=float(p[i])) for i in range(n)],
                     counts_fn=seg._device_counts)
    env = seg.quiet_env(pool)
    recs = np.zeros((n, 8), np.int32)
    recs[:, 0], recs[:, 1], recs[:, 4] = 3 * np.arange(n) + 1, np.arange(n), p.view(np.int32)
    for ns in (1, 2, 7):
        rc, got = seg.run_pass(env, H, W, recs, second, n, n, ns, 0, work_rng=words)
        assert rc == 0
        c0, w1 = ref.occupancy(first, p, ns, words)
        c1, w2 = ref.occupancy(second, p, ns, w1)
        assert np.array_equal(got["work_boards"][:n], first), ns
        bad = _differing(got["counts"][0], c0, got["work_rng"][:n], w2) + _differing(got["counts"][1], c1, w2, w2)
        assert not bad, "%dx%d %s through the pass, %d samples: entries %r differ" % (H, W, kind, ns, sorted(set(bad))[:20])


# ------------------------------------------------------------------------------------------------- the fused step

STATE = ("board", "goals", "rng", "agent_loc", "num_steps", "episode_idx", "level_idx", "exit_locs")
RECORDS = ("reward", "done", "success", "times_up", "episode_reward", "episode_length")
STEP_SHAPES = ((25, 25), (64, 64), (40, 40), (30, 30), (31, 33))       # draw_deal_cases.STEP_SHAPES


@pytest.mark.parametrize("wrapped", (False, True), ids=["plain", "inaction"])
@pytest.mark.parametrize("kind", crc.STEP_KINDS)
@pytest.mark.parametrize("H,W", STEP_SHAPES, ids=["%dx%d" % s for s in STEP_SHAPES])
def test_fused_step_cases(H, W, kind, wrapped):
    """Tile and soup boards as the levels of a hand-made pool, the real agent walled in: three single no-op steps, then
    one T-step launch; with the training wrappers the inaction baseline advances a second board by the same rule.
    Boards, generators, rewards and records equal the oracle env's after every launch."""
    from safelife_amd._hip import SafeLifeHipError
    from safelife_amd.levels import LevelPool
    from tests import draw_deal_cases as ddc
    assert STEP_SHAPES == ddc.STEP_SHAPES
    levels, B, kw, actions = crc.step_case(kind, H, W, wrapped)
    pool = LevelPool(levels, counts_fn=util.oracle_counts, min_performance_fraction=1.0)
    assert pool.exit_slots <= crc.MAX_EXITS
    dev = util.DeviceBackend(pool, B, **kw)
    cpu = util.OracleBackend(pool, B, **kw)
    env = dev.env
    assert env.row_kernels() == (crc.family(H, W) == "row")
    last_done = np.ones(B, np.uint8)

    def same(where, names):
        for name in names:
            got, want = dev.get(name), cpu.get(name)
            if name == "inaction_board":    # (the oracle copies the board when it resets an env, the library when the
                got, want = got[last_done == 0], want[last_done == 0]   # env next steps: the envs that did not just finish)
            assert got.shape == want.shape and np.array_equal(got, want), "%s %dx%d %s, %s: envs %r differ" % (
                kind, H, W, where, name, np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1)).tolist()[:20])

    extra = ("shaped_reward", "inaction_rng", "inaction_board") if wrapped else ()
    env.reset()
    cpu.env.reset()
    same("reset", STATE)
    T1 = crc.STEP_SINGLE
    for t in range(T1):
        env.step(actions[t])
        last_done = cpu.step(actions[t])[2]
        same("step %d" % t, STATE + RECORDS + extra)
    if wrapped and not env.row_kernels():       # the size-generic T-step launch cannot advance the baseline between steps
        with pytest.raises(SafeLifeHipError, match="T must be 1"):
            env.rollout(actions[T1:])
        for t in range(T1, len(actions)):
            env.step(actions[t])
            last_done = cpu.step(actions[t])[2]
            same("step %d" % t, STATE + RECORDS + extra)
        return
    r_t, d_t = env.rollout(actions[T1:])
    want = [cpu.step(a) for a in actions[T1:]]
    last_done = want[-1][2]
    assert np.array_equal(r_t.cpu().numpy(), np.stack([w[1] for w in want])), "reward_t"
    assert np.array_equal(d_t.cpu().numpy(), np.stack([w[2] for w in want])), "done_t"
    same("rollout", STATE + RECORDS + extra)
