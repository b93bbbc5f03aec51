"""GPU suite: the spawner draw deal in every draw-count regime, on every kernel family, against the oracle -- boards and
generator words, bit for bit.  The boards make an exact number of draws (tests/draw_deal_cases.py: every threshold of
resolve_draws_planes from both sides, rows in which all 64 cells draw, two boards of a wave on different counts and
probabilities); what regimes the cases reach is asserted on the oracle alone by tests/test_draw_deal_host.py.  Integer
work: every comparison is np.array_equal.
"""
import numpy as np
import pytest

import oracle
from tests import draw_deal_cases as ddc
from tests import util

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["%dx%d" % s for s in ddc.ADVANCE_SHAPES]


@pytest.fixture(scope="module")
def sp():
    from safelife_amd import speedups
    return speedups


def _dev_advance(sp, boards, p, n, words):
    import torch
    d_b = sp._to_device(np.array(boards), np.uint16)       # (a copy: the shared batch is read-only)
    d_r = sp._to_device(words, np.uint64)
    d_p = torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).to(d_b.device)
    if not isinstance(n, int):
        n = torch.from_numpy(np.ascontiguousarray(n, dtype=np.int32)).to(d_b.device)
    out = sp.advance_board_batch(d_b, d_p, d_r, n)
    return sp._to_host(out, np.uint16), sp._to_host(d_r, np.uint64)


def _dev_occupancy(sp, boards, p, n, words):
    import torch
    d_r = sp._to_device(words, np.uint64)
    d_p = torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).to(d_r.device)
    got = sp.life_occupancy_batch(sp._to_device(np.array(boards), np.uint16), d_p, d_r, n)
    return got.cpu().numpy(), sp._to_host(d_r, np.uint64)


def _same_boards(H, W, got, want, w_dev, w_cpu, totals, what):
    """Bit exact; a mismatch names the boards, their draw counts at step 0 and the regimes of their waves."""
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1) | (w_dev != w_cpu).any(axis=1))
    if len(bad):
        G = ddc.boards_per_wave(H, W) if ddc.family(H, W) == "row" else 1
        labels = ddc.wave_regimes(H, W, totals)
        raise AssertionError("%dx%d %s: boards %r differ (draws at step 0 %r, regimes %r)" % (
            H, W, what, bad.tolist(), [int(totals[b]) for b in bad], [labels[b // G] for b in bad]))


@pytest.mark.parametrize("rot", (0, 1))
@pytest.mark.parametrize("H,W", ddc.ADVANCE_SHAPES, ids=SHAPE_IDS)
def test_advance_board_in_every_regime(sp, H, W, rot):
    """advance_board_batch on the shape's case list, one launch per step count: n = 1 (the exact regime of each case and
    the dealing of outcomes to cells), n = 3 (the rows stay bit planes between the steps), and one count per board, 0, 1
    and 3 mixed inside the waves.  rot: which boards have which spawn_prob -- under one of the two every board has a
    fractional one, and the two boards of a wave always differ."""
    boards, totals = ddc.advance_batch(H, W)
    B = len(boards)
    p, words = ddc.spawn_probs(B, rot), ddc.rng_words(H + rot, B)
    for n in (1, 3, ddc.each_steps(B)):
        w_cpu = words.copy()
        if isinstance(n, int):
            want = oracle.advance_board_batch(boards, p, n, w_cpu, n_threads=8)
        else:
            _, want, w_cpu = ddc.oracle_trace(boards, p, words, n)
        got, w_dev = _dev_advance(sp, boards, p, n, words)
        _same_boards(H, W, got, want, w_dev, w_cpu, totals, "n = %s" % (n if isinstance(n, int) else "each"))


@pytest.mark.parametrize("H,boards", [(64, ddc.mixed_batch_64), (25, ddc.mixed_batch_25)], ids=["64x64", "25x25"])
def test_one_launch_mixes_regimes(sp, H, boards):
    """Consecutive waves of one launch in different regimes (the paths are wave-uniform branches next to each other), at a
    fractional probability on every board, and the same batch reversed: every regime at another place of the grid."""
    boards = boards()
    for order in (slice(None), slice(None, None, -1)):
        b = np.ascontiguousarray(boards[order])
        B = len(b)
        p = np.where(np.arange(B) % 2 == 0, 0.5, 0.3).astype(np.float32)
        words = ddc.rng_words(77 + H, B)
        for n in (1, 2):
            w_cpu = words.copy()
            want = oracle.advance_board_batch(b, p, n, w_cpu, n_threads=8)
            got, w_dev = _dev_advance(sp, b, p, n, words)
            _same_boards(H, H, got, want, w_dev, w_cpu, ddc.draws(b), "mixed, n = %d" % n)


@pytest.mark.parametrize("H,B", [(64, 2079), (25, 4118)], ids=["64x64", "25x25"])
def test_four_wave_advance_kernel_in_every_regime(sp, H, B):
    """Up to two workgroups of the four-wave kernel per CU a batch runs on one-wave workgroups (rowlane_advance_t): the
    batches above never reach k_advance_rowlane.  The case list repeated to 2 * 256 * NB boards and more does -- an odd
    list on a shape of two boards per wave pairs the boards the other way round in every second copy."""
    boards, totals = ddc.advance_batch(H, H)
    reps = -(-B // len(boards))
    boards, totals = np.tile(boards, (reps, 1, 1))[:B], np.tile(totals, reps)[:B]
    assert B >= 2 * 256 * 4 * ddc.boards_per_wave(H, H)
    p, words = ddc.spawn_probs(B, 1), ddc.rng_words(H, B)
    for n in (1, 2):
        w_cpu = words.copy()
        want = oracle.advance_board_batch(boards, p, n, w_cpu, n_threads=8)
        got, w_dev = _dev_advance(sp, boards, p, n, words)
        _same_boards(H, H, got, want, w_dev, w_cpu, totals, "four-wave kernel, n = %d" % n)


@pytest.mark.parametrize("H", ddc.OCCUPANCY_SHAPES)
def test_life_occupancy_stays_in_a_regime(sp, H):
    """The occupancy kernels (they keep a lane's jump from step to step) for 12 steps at spawn_prob = 0: every board stays
    on its count, the generators move on by 12 times that -- and once more at the cases' own probabilities."""
    boards, totals = ddc.advance_batch(H, H)
    B = len(boards)
    for p in (np.zeros(B, np.float32), ddc.spawn_probs(B, 1)):
        words = ddc.rng_words(40 + H, B)
        w_cpu = words.copy()
        want = oracle.life_occupancy_batch(boards, p, 12, w_cpu, n_threads=8)
        got, w_dev = _dev_occupancy(sp, boards, p, 12, words)
        _same_boards(H, H, got, want, w_dev, w_cpu, totals, "occupancy, 12 steps, p %s" % ("= 0" if not p.any() else "mixed"))


@pytest.mark.parametrize("case", ddc.TRANSITIONS, ids=["%d-%s-p%s" % (c[0], c[1][0], c[2][0]) for c in ddc.TRANSITIONS])
def test_life_occupancy_across_regime_changes(sp, case):
    """Boards whose count crosses a regime boundary from one step to the next, in both directions: the cached jump must
    be refilled.  Every prefix of the steps as a launch of its own, so that a wrong step is named."""
    H, targets, ps, seed, steps = case
    boards, p, words = ddc.transition_case(H, targets, ps, seed)
    counts = ddc.oracle_trace(boards, p, words, steps)[0]
    for n in sorted({steps, steps // 2, 2, 3, 4}):
        w_cpu = words.copy()
        want = oracle.life_occupancy_batch(boards, p, n, w_cpu, n_threads=2)
        got, w_dev = _dev_occupancy(sp, boards, p, n, words)
        labels = [ddc.regime(H, H, row) for row in counts[:n]]
        assert np.array_equal(w_dev, w_cpu), "generator after %d steps, regimes %r" % (n, labels)
        assert np.array_equal(got, want), "counts after %d steps, regimes %r" % (n, labels)


# ------------------------------------------------------------------------------------------------- the fused step

STATE = ("board", "goals", "rng", "agent_loc", "num_steps", "episode_idx", "level_idx", "exit_locs")
RECORDS = ("reward", "done", "success", "times_up", "episode_reward", "episode_length")


@pytest.mark.parametrize("wrapped", (False, True), ids=["plain", "wrappers"])
@pytest.mark.parametrize("H,W", ddc.STEP_SHAPES, ids=["%dx%d" % s for s in ddc.STEP_SHAPES])
def test_fused_step_in_every_regime(H, W, wrapped):
    """A pool of levels with exact draw counts, env e on level e, time limit 5: eight single steps (the first action is 0:
    step 0 makes exactly the levels' counts), then six steps in one launch.  With the training wrappers the inaction
    baseline advances a second board on the same counts from a generator of its own."""
    from safelife_amd._hip import SafeLifeHipError
    from safelife_amd.levels import LevelPool
    levels, B, kw, actions = ddc.step_case(H, W, wrapped)
    pool = LevelPool(levels, counts_fn=util.oracle_counts, min_performance_fraction=1.0)
    dev = util.DeviceBackend(pool, B, **kw)
    cpu = util.OracleBackend(pool, B, **kw)
    env = dev.env
    assert env.row_kernels() == (ddc.family(H, W) == "row")
    last_done = np.ones(B, np.uint8)

    def same(where, names):
        for name in names:
            got, want = dev.get(name), cpu.get(name)
            if name == "inaction_board":    # (the oracle copies the board when it resets an env, the library when the
                got, want = got[last_done == 0], want[last_done == 0]   # env next steps: the envs that did not just finish)
            assert got.shape == want.shape and np.array_equal(got, want), "%dx%d %s, %s: envs %r differ" % (
                H, W, where, name, np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1)).tolist())

    extra = ("shaped_reward", "inaction_rng", "inaction_board") if wrapped else ()
    env.reset()
    cpu.env.reset()
    same("reset", STATE)
    T1 = ddc.STEP_SINGLE
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
