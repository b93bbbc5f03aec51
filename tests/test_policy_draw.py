"""
The device action draw (slhip_sample_actions) pinned to an exact host model and, through the model, to a float64
reference of the reference's own draw (tests/policy_ref.py).

CPU part: the model against ``choice_reference`` inside a DERIVED window, the uniformity and independence of the
splitmix64 uniforms, the identity that makes a draw a function of the global env index, the 64-bit edges.
GPU part: kernel == model bit for bit over sizes, row families, the two ends of u, rows that are no distributions,
seed and counter edges; PipelinedRunner driven by a stochastic policy whose every draw is predicted on the host and
fed to the oracle, in three ways of cutting the same batch; slhip_obs_to_policy at its edges.

The window of the model against the float64 reference (a row may only disagree inside it): every fp32 add of a running
sum <= 2 rounds by at most 2^-24, so cum_k is off the exact partial sum by at most k * 2^-24 <= A * 2^-24; normalising
the float64 cdf by its last entry moves a boundary by at most the row's own fp32 sum error, another A * 2^-24; together
A * 2^-23.  A disagreement needs u inside that window of one of the row's A boundaries, a set of measure at most
A * 2 * A * 2^-23 -- the bound on the share of disagreeing rows.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import policy_ref as pr
from tests import util

gpu = pytest.mark.gpu
TWO24 = 1 << 24
# (counter, env) of a run seeded 5 at which the 24-bit uniform takes its largest and its smallest value
SEED_ENDS = 5
U_MAX_AT = ((398, 4983), (3005, 7197), (8566, 7438))
U_ZERO_AT = ((6036, 6044), (9673, 5975), (14611, 7616))


# ------------------------------------------------------------------------------------------------ row families

def _softmax32(logits, mask=None):
    """fp32 softmax rows; `mask` (bool, True = action masked) entries are exactly 0 and the rest is renormalised in fp32."""
    z = np.exp((logits - logits.max(axis=1, keepdims=True)).astype(np.float32))
    if mask is not None:
        z = np.where(mask, np.float32(0), z)
    return (z / z.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)


def _dyadic(rng, n, A, parts=None):
    """Rows of multiples of 1/64 that sum to exactly 1 (every fp32 partial sum is exact); zeros occur.  `parts`: only
    the first `parts` entries take mass."""
    parts = A if parts is None else parts
    rows = np.zeros((n, A), np.float32)
    rows[:, :parts] = rng.multinomial(64, np.full(parts, 1.0 / parts), size=n).astype(np.float32) / np.float32(64)
    return rows


def _bump_last_positive(rows, delta):
    """Dyadic rows with `delta` added to their last positive entry: the fp32 running sum ends at exactly 1 + delta
    (delta = -2^-24: one ulp below 1; +2^-23: one ulp above)."""
    rows = rows.copy()
    last = rows.shape[1] - 1 - np.argmax(rows[:, ::-1] > 0, axis=1)
    rows[np.arange(len(rows)), last] += np.float32(delta)
    return rows


def _zero_mask(n, A, where):
    m = np.zeros((n, A), bool)
    w = max(1, A // 4)
    if where == "start":
        m[:, :w] = True
    elif where == "end":
        m[:, A - w:] = True
    else:
        m[:, A // 2:A // 2 + w] = True
    if m.all(axis=1).any():             # (A = 1: nothing can be masked)
        m[:] = False
    return m


def _fp32_running_sum(rows, upto=None):
    s = np.zeros(len(rows), np.float32)
    for k in range(rows.shape[1] if upto is None else upto):
        s = s + rows[:, k]
    return s


def _families(rng, n, A):
    """name -> float32 [n, A]: the row families of the device tests."""
    logits = rng.standard_normal((n, A))
    fam = {"uniform": np.full((n, A), np.float32(1) / np.float32(A), np.float32)}
    for temp in (0.1, 1.0, 8.0, 30.0):
        fam["softmax_x%g" % temp] = _softmax32(logits * temp)
    onehot = np.zeros((n, A), np.float32)
    onehot[np.arange(n), np.arange(n) % A] = 1.0
    fam["onehot"] = onehot
    fam["dyadic"] = _dyadic(rng, n, A)
    fam["sum_1_minus_ulp"] = _bump_last_positive(_dyadic(rng, n, A), -2.0 ** -24)
    fam["sum_1_plus_ulp"] = _bump_last_positive(_dyadic(rng, n, A), 2.0 ** -23)
    for where in ("start", "middle", "end"):
        fam["zeros_" + where] = _softmax32(logits * 2.0, _zero_mask(n, A, where))
    if A >= 2:
        last = np.zeros((n, A), bool)
        last[:, -1] = True
        fam["masked_last_softmax"] = _softmax32(logits, last)
        fam["masked_last_short"] = _bump_last_positive(_dyadic(rng, n, A, parts=A - 1), -2.0 ** -24)
    return fam


def _mixed_rows(rng, B, A):
    """B rows that cycle through every family."""
    fam = _families(rng, -(-B // 8), A)
    rows = np.concatenate(list(fam.values()))           # (12 families or more: at least B rows)
    return np.ascontiguousarray(rows[rng.permutation(len(rows))[:B]])


# ------------------------------------------------------------------------------------------------ CPU: the model

def _splitmix_python(seed, counter, env):
    """draw_u24 once more in Python integers (nothing shared with the numpy version but the constants' values)."""
    m = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (counter * 0x100000001B3 + env + 1)) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return (z ^ (z >> 31)) >> 40


def test_draw_u24_arithmetic_edges():
    """Seeds 0 and 2^64-1, counters 0, 2^32 and 2^63 (counter * K wraps), Python integers against np.uint64 inputs --
    each against splitmix64 in Python's unbounded integers."""
    envs = [0, 1, 255, 4097, 2 ** 31, 2 ** 32 + 3]
    for seed in (0, 1, 5, 2 ** 63, 2 ** 64 - 1):
        for counter in (0, 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1):
            want = np.array([_splitmix_python(seed, counter, e) for e in envs], np.uint32)
            got_py = pr.draw_u24(seed, counter, envs)
            got_np = pr.draw_u24(np.uint64(seed), np.uint64(counter), np.array(envs, np.uint64))
            assert got_py.dtype == np.uint32 and got_py.shape == (len(envs),)
            assert np.array_equal(got_py, want) and np.array_equal(got_np, want), (seed, counter)
            assert int(pr.draw_u24(seed, counter, envs[3])) == int(want[3])            # scalars in, scalar out
    assert np.array_equal(pr.draw_u24(2 ** 64 + 5, 2 ** 64 + 7, [3]), pr.draw_u24(5, 7, [3]))   # inputs reduce mod 2^64
    assert np.array_equal(pr.draw_u24(-1, 0, [3]), pr.draw_u24(2 ** 64 - 1, 0, [3]))
    u = pr.uniform_f32(np.array([0, 1, TWO24 - 1], np.uint32))
    assert u.dtype == np.float32 and [float(v) for v in u] == [0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]


def test_draw_u24_takes_both_ends_where_the_device_tests_expect_them():
    for counter, env in U_MAX_AT:
        assert int(pr.draw_u24(SEED_ENDS, counter, env)) == 0xFFFFFF
    for counter, env in U_ZERO_AT:
        assert int(pr.draw_u24(SEED_ENDS, counter, env)) == 0


def test_seed_identity_makes_the_draw_a_function_of_the_global_index():
    """seed + G * lo (mod 2^64) shifts the env index by lo; seed + lo does not."""
    e = np.arange(1000)
    for seed in (0, 5, 2 ** 64 - 1):
        for lo in (1, 256, 4096, 2 ** 33 + 1):
            for c in (0, 7, 2 ** 32):
                want = pr.draw_u24(seed, c, e + lo)
                assert np.array_equal(pr.draw_u24((seed + pr.G * lo) % 2 ** 64, c, e), want)
                assert np.array_equal(pr.draw_u24(seed + pr.G * lo, c, e), want)        # (reduced inside as well)
                assert (pr.draw_u24(seed + lo, c, e) == want).mean() < 0.01
    p = _softmax32(np.random.default_rng(3).standard_normal((1000, 9)))
    assert np.array_equal(pr.sample_model(p, 5 + pr.G * 256, 11), pr.sample_model(p, 5, 11, first_env=256))


def _chi2_p(counts):
    """Two-sided: the smaller tail probability of Pearson's statistic against the uniform expectation."""
    from scipy.stats import chi2
    counts = np.asarray(counts, np.float64).ravel()
    expected = counts.sum() / counts.size
    assert expected >= 5
    stat = ((counts - expected) ** 2).sum() / expected
    return min(chi2.sf(stat, counts.size - 1), chi2.cdf(stat, counts.size - 1))


def _joint(a, b):
    return np.bincount(((a >> 16).astype(np.int64) << 8 | (b >> 16).astype(np.int64)).ravel(), minlength=65536)


def test_uniforms_are_uniform_and_independent():
    """Chi-square on the top 8 bits (fixed seeds, so the outcome is fixed): over envs at one counter, over counters for
    one env, and on the 8x8-bit joint bins of neighbouring envs, of consecutive counters and of two groups whose seeds
    differ by G * lo.  Every p-value (either tail) above 1e-6."""
    seed = 20240917
    top = lambda u: np.bincount((u >> 16).ravel(), minlength=256)
    e, c = np.arange(1 << 16), np.arange(1 << 16)
    ps = {"envs": _chi2_p(top(pr.draw_u24(seed, 7, e))),
          "counters": _chi2_p(top(pr.draw_u24(seed, c, 3))),
          "counters_x_envs": _chi2_p(top(pr.draw_u24(seed, np.arange(4096)[:, None], np.arange(64)[None, :])))}
    cc, ee = np.arange(1024)[:, None], np.arange(1024)[None, :]
    grid = pr.draw_u24(seed, cc, ee)
    ps["env_pairs"] = _chi2_p(_joint(grid, pr.draw_u24(seed, cc, ee + 1)))
    ps["counter_pairs"] = _chi2_p(_joint(grid, pr.draw_u24(seed, cc + 1, ee)))
    for lo in (256, 192):
        ps["groups_%d" % lo] = _chi2_p(_joint(grid, pr.draw_u24(seed + pr.G * lo, cc, ee)))
    print(ps)
    assert min(ps.values()) > 1e-6, ps


MODEL_FAMILIES = ("uniform", "uniform_random", "softmax_sharp", "softmax_flat", "zeros_start", "zeros_middle", "zeros_end")


def _model_family(rng, name, n, A):
    if name == "uniform":
        return np.full((n, A), np.float32(1) / np.float32(A), np.float32)
    if name == "uniform_random":
        w = rng.random((n, A)).astype(np.float32) + np.float32(1e-3)
        return (w / w.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)
    logits = rng.standard_normal((n, A))
    if name == "softmax_sharp":
        return _softmax32(logits * 8.0)
    if name == "softmax_flat":
        return _softmax32(logits * 0.1)
    return _softmax32(logits * 2.0, _zero_mask(n, A, name.split("_")[1]))


@pytest.mark.parametrize("A", [2, 9, 64])
def test_model_against_choice_reference(A):
    """7 families x 2^16 rows per A (3 x 458752 > 2^20 draws in all), one draw per row: the fp32 model may leave the
    float64 reference only inside the derived window (module docstring), and never returns a zero-probability action."""
    n = 1 << 16
    rng = np.random.default_rng(1000 + A)
    probs = np.concatenate([_model_family(rng, name, n, A) for name in MODEL_FAMILIES])
    N = len(probs)
    u24 = pr.draw_u24(77 + A, np.arange(N) // 4096, np.arange(N) % 4096)
    u32 = pr.uniform_f32(u24)
    model = pr.model_with_u(probs, u32).astype(np.int64)
    ref, cdf = pr.choice_reference(probs, u32)
    some = rng.integers(0, N, 2048)             # the all-rows-at-once search is numpy's searchsorted(side="right")
    assert all(int(ref[i]) == int(np.searchsorted(cdf[i], np.float64(u32[i]), side="right")) for i in some)
    rows = np.arange(N)
    assert model.min() >= 0 and model.max() < A and ref.max() < A
    assert (probs[rows, model] > 0).all() and (probs[rows, ref] > 0).all()
    window = A * 2.0 ** -23
    bad = np.flatnonzero(model != ref)
    print("A=%d: %d of %d rows differ (bound %.1f)" % (A, len(bad), N, 2 * A * A * 2.0 ** -23 * N))
    assert len(bad) <= 2 * A * A * 2.0 ** -23 * N
    for i in bad:
        lo, hi = sorted((int(model[i]), int(ref[i])))
        assert np.abs(cdf[i, lo:hi] - np.float64(u32[i])).min() <= window, (i, lo, hi)
        assert (probs[i, lo + 1:hi] <= window).all(), (i, lo, hi)


def test_model_rule_on_hand_made_rows():
    """The contract, case by case, at the two ends of u."""
    f = np.float32
    top, zero = f(1 - 2.0 ** -24), f(0)
    short = np.array([[0.5, 0.25, f(0.25) - f(2.0 ** -24), 0, 0]], f)          # fp32 sum 1 - 2^-24, two trailing zeros
    assert pr.model_with_u(short, [top])[0] == 2 and pr.model_with_u(short, [zero])[0] == 0
    assert pr.model_with_u(np.array([[0, 0, 1, 0]], f), [zero])[0] == 2          # p_0 = 0 is skipped at u = 0
    assert pr.model_with_u(np.array([[1e-40, 1, 0]], f), [zero])[0] == 0         # an fp32 subnormal is positive
    assert pr.model_with_u(np.zeros((1, 4), f), [top])[0] == 3                   # no positive entry: A-1
    assert pr.model_with_u(np.array([[-1, -1, -1]], f), [zero])[0] == 2
    assert pr.model_with_u(np.array([[np.nan, 0.5, np.nan, 0]], f), [zero])[0] == 1     # NaN sum: the last positive entry
    assert pr.model_with_u(np.array([[0.25, np.inf, 0]], f), [top])[0] == 1
    assert pr.model_with_u(np.array([[1]], f), [top])[0] == 0 and pr.model_with_u(np.array([[0]], f), [top])[0] == 0


def test_row_families_hold_what_their_names_say():
    rng = np.random.default_rng(8)
    for A in (1, 2, 9, 17, 64):
        fam = _families(rng, 512, A)
        assert (_fp32_running_sum(fam["dyadic"]) == 1).all()
        assert (_fp32_running_sum(fam["sum_1_minus_ulp"]) == np.float32(1 - 2.0 ** -24)).all()
        assert (_fp32_running_sum(fam["sum_1_plus_ulp"]) == np.float32(1 + 2.0 ** -23)).all()
        if A >= 2:
            assert (fam["zeros_start"][:, 0] == 0).all() and (fam["zeros_end"][:, -1] == 0).all()
            assert (fam["zeros_middle"][:, A // 2] == 0).all()
            short = fam["masked_last_short"]
            assert (short[:, -1] == 0).all() and (_fp32_running_sum(short, A - 1) < 1).all()
        if A == 9:          # masked softmax rows: a good part of them stays below 1 by itself
            soft = fam["masked_last_softmax"]
            assert (soft[:, -1] == 0).all() and (_fp32_running_sum(soft, A - 1) < 1).mean() > 0.1
        assert all(v.dtype == np.float32 and v.shape == (512, A) for v in fam.values())


# ------------------------------------------------------------------------------------------------ GPU: kernel == model

CANARY = -1515870811            # 0xA5A5A5A5
PAD = 1024                      # int32 slots of canary on either side: more than one block of the kernel


def _kernel(probs, seed, counter):
    """slhip_sample_actions into the middle of a canary buffer; nothing outside [0, B) may be written."""
    import torch
    from safelife_amd import _hip
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    B, A = probs.shape
    dev = _hip.device()
    d_p = torch.from_numpy(probs).to(dev)
    buf = torch.full((B + 2 * PAD,), CANARY, dtype=torch.int32, device=dev)
    _hip.check(_hip.lib().slhip_sample_actions(d_p.data_ptr(), B, A, seed, counter, buf.data_ptr() + 4 * PAD,
                                               _hip.current_stream_ptr()))
    out = buf.cpu().numpy()
    assert (out[:PAD] == CANARY).all() and (out[PAD + B:] == CANARY).all(), "written outside [0, B)"
    return out[PAD:PAD + B]


def _assert_kernel_is_model(probs, seed, counter, what=None):
    got, want = _kernel(probs, seed, counter), pr.sample_model(probs, seed, counter)
    assert got.min() >= 0 and got.max() < probs.shape[1], what
    assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8])
    return got


@gpu
@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_kernel_equals_model_sizes(B):
    for A in (1, 2, 9, 17, 64):
        rng = np.random.default_rng(B * 100 + A)
        _assert_kernel_is_model(_mixed_rows(rng, B, A), 1234567 + A, 3 + B, (B, A))


@gpu
@pytest.mark.parametrize("A", [2, 9, 64])
def test_kernel_equals_model_row_families(A):
    rng = np.random.default_rng(50 + A)
    for i, (name, rows) in enumerate(sorted(_families(rng, 4099, A).items())):
        got = _assert_kernel_is_model(rows, 99, i, name)
        assert (rows[np.arange(len(rows)), got] > 0).all(), name


def _at(env, counter):
    assert int(pr.draw_u24(SEED_ENDS, counter, env)) in (0, 0xFFFFFF)
    return env


@gpu
def test_kernel_at_the_largest_uniform():
    """u = 1 - 2^-24 on a row whose last action is masked and whose other entries sum below 1 in fp32: the action is the
    row's last POSITIVE one, not A-1."""
    B = 8192
    rng = np.random.default_rng(61)
    for A, (counter, env) in zip((9, 2, 64), U_MAX_AT):
        rows = _bump_last_positive(_dyadic(rng, B, A, parts=A - 1), -2.0 ** -24)
        got = _assert_kernel_is_model(rows, SEED_ENDS, counter, (A, counter))
        last_positive = int(np.flatnonzero(rows[_at(env, counter)] > 0)[-1])
        assert last_positive < A - 1 and got[env] == last_positive, (A, got[env], last_positive)
        assert (rows[np.arange(B), got] > 0).all()
    soft = _families(rng, B, 9)["masked_last_softmax"]       # the rows a masked policy head really emits
    soft[U_MAX_AT[0][1]] = soft[np.flatnonzero(_fp32_running_sum(soft, 8) < 1)[0]]
    got = _assert_kernel_is_model(soft, SEED_ENDS, U_MAX_AT[0][0])
    assert got[U_MAX_AT[0][1]] == 7 and (soft[np.arange(B), got] > 0).all()


@gpu
def test_kernel_at_the_smallest_uniform():
    """u = 0: a row with p_0 = 0 skips action 0; a row with p_0 = 1e-40, an fp32 subnormal, returns it (0 < 1e-40 must
    hold on the device: subnormals are not flushed)."""
    B = 8192
    rng = np.random.default_rng(62)
    for A, (counter, env) in zip((9, 2, 64), U_ZERO_AT):
        rows = _dyadic(rng, B, A)
        rows[:, 1] += rows[:, 0]                            # (multiples of 1/64: exact)
        rows[:, 0] = 0
        first = np.argmax(rows > 0, axis=1)                 # the first positive entry of each row
        assert (_fp32_running_sum(rows) == 1).all() and first.min() >= 1
        got = _assert_kernel_is_model(rows, SEED_ENDS, counter, (A, counter))
        assert got[_at(env, counter)] == first[env] and (got >= first).all()
        tiny = _dyadic(rng, B, A)
        tiny[:, 0] = np.float32(1e-40)
        tiny[:, 1:] = _dyadic(rng, B, A - 1) if A > 2 else 1.0
        assert 0 < tiny[0, 0] < np.finfo(np.float32).tiny
        got = _assert_kernel_is_model(tiny, SEED_ENDS, counter, (A, counter, "subnormal"))
        assert got[env] == 0 and np.array_equal(got == 0, pr.draw_u24(SEED_ENDS, counter, np.arange(B)) == 0)


@gpu
def test_kernel_on_rows_that_are_no_distributions():
    """NaN, +inf and negative entries: the action lies in [0, A) and is the model's."""
    rng = np.random.default_rng(63)
    for A in (1, 2, 9, 64):
        B = 2051
        rows = _mixed_rows(rng, B, A)
        kind = rng.integers(0, 6, B)
        col = rng.integers(0, A, B)
        r = np.arange(B)
        rows[r[kind == 0], col[kind == 0]] = np.nan
        rows[r[kind == 1], col[kind == 1]] = np.inf
        rows[r[kind == 2], col[kind == 2]] = -np.inf
        rows[r[kind == 3], col[kind == 3]] = -0.75
        rows[kind == 4] *= np.float32(-1)
        rows[5 % B], rows[6 % B], rows[7 % B] = np.nan, 0.0, np.inf
        rows[8 % B] = -0.0
        if A >= 2:
            rows[9, 0], rows[9, 1] = np.inf, -np.inf
            rows[10, 0], rows[10, 1] = 3e38, 3e38
        _assert_kernel_is_model(rows, 17, A, A)


@gpu
def test_kernel_seed_and_counter_edges():
    rng = np.random.default_rng(64)
    rows = _softmax32(rng.standard_normal((257, 9)))
    seen = []
    for seed in (0, 2 ** 64 - 1):
        for counter in (0, 2 ** 32, 2 ** 63):
            seen.append(_assert_kernel_is_model(rows, seed, counter, (seed, counter)))
    assert len({a.tobytes() for a in seen}) == len(seen)
    # the kernel under seed + G * lo draws what envs lo + e draw under seed
    for lo in (1, 256, 4096):
        assert np.array_equal(_kernel(rows, (5 + pr.G * lo) % 2 ** 64, 9), pr.sample_model(rows, 5, 9, first_env=lo))


# ------------------------------------------------------------------------------------------------ GPU: the runner

def _device_counts(boards, goals):
    from safelife_amd.levels import _device_counts as f
    return f(boards, goals)


ENV_STATE = ("board", "goals", "agent_loc", "exit_locs", "rng", "num_steps", "old_value", "required_points",
             "initial_points", "goals_static", "is_active", "episode_reward", "episode_length", "level_idx",
             "episode_idx", "success", "times_up")
RUN_B, RUN_T, RUN_SEED = 448, 40, 0xC0FFEE
RUN_CHANNELS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 25, 26, 27)
# 64ths per action: every row sums to 64, so every fp32 partial sum is exact and the host's prediction is too
POLICY_TABLE_64 = np.array([
    [8, 8, 8, 8, 8, 8, 8, 4, 4],
    [32, 0, 0, 16, 0, 8, 8, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0, 64],
    [1, 1, 1, 1, 1, 1, 1, 1, 56],
    [0, 16, 16, 0, 16, 16, 0, 0, 0],
    [7, 9, 5, 11, 3, 13, 1, 15, 0],
    [0, 0, 0, 0, 32, 0, 0, 0, 32],
    [16, 16, 16, 16, 0, 0, 0, 0, 0],
    [2, 4, 8, 16, 2, 4, 8, 16, 4],
    [0, 21, 0, 21, 0, 22, 0, 0, 0],
    [64, 0, 0, 0, 0, 0, 0, 0, 0],
    [10, 10, 10, 10, 10, 10, 2, 1, 1],
    [0, 0, 0, 1, 0, 0, 0, 63, 0],
    [4, 4, 4, 4, 4, 4, 4, 4, 32],
    [0, 0, 20, 20, 20, 0, 0, 4, 0],
    [12, 0, 12, 0, 12, 0, 12, 0, 16],
], np.float32)


def _policy_row(total, t):
    return (total * 7 + t * 3) % len(POLICY_TABLE_64)


def _run_pool():
    pool, _ = util.pool_from_fixture("append_spawn_25", _device_counts, min_performance_fraction=0.05)
    common = dict(auto_reset=True, level_stride=3, time_limit=15, view_shape=(9, 9), output_channels=RUN_CHANNELS)
    return pool, common, np.arange(RUN_B) % len(pool)


@functools.lru_cache(maxsize=None)
def _oracle_run():
    """The oracle stepped with the actions the host PREDICTS for a runner seeded RUN_SEED: the draw of global env e at
    step t is sample_model(table[row(obs, t)], seed, counter=t) at env index e.  Computed once, never changed."""
    assert (POLICY_TABLE_64.sum(axis=1) == 64).all() and (POLICY_TABLE_64[:, -1] == 0).sum() >= 3
    table = POLICY_TABLE_64 / np.float32(64)
    pool, common, first = _run_pool()
    cpu = util.OracleBackend(pool, RUN_B, first_level=first, **common)
    obs = cpu.reset()
    actions, rewards, dones = [], [], []
    for t in range(RUN_T):
        total = obs.reshape(RUN_B, -1).sum(axis=1).astype(np.int64)
        a = pr.sample_model(table[_policy_row(total, t)], RUN_SEED, t)
        obs, r, d = cpu.step(a)
        actions.append(a), rewards.append(r), dones.append(d.astype(bool))
    state = {name: cpu.get(name) for name in ENV_STATE}
    assert state["episode_idx"].min() >= 1 and len({a.tobytes() for a in actions}) == RUN_T
    for v in actions + rewards + dones + list(state.values()):
        v.setflags(write=False)
    return actions, rewards, dones, state


RUN_LAYOUTS = {
    "slices2": [dict(lo=0, n=RUN_B, slices=2, bounds=(0, 256, 448))],
    "slices3": [dict(lo=0, n=RUN_B, slices=3, bounds=(0, 192, 384, 448))],
    "two_shards": [dict(lo=0, n=RUN_B // 2, slices=2, bounds=(0, 128, 224)),
                   dict(lo=RUN_B // 2, n=RUN_B // 2, slices=2, bounds=(0, 128, 224))],
}


@gpu
@pytest.mark.parametrize("layout", sorted(RUN_LAYOUTS))
def test_pipelined_runner_draws_by_global_env_and_step(layout):
    """PipelinedRunner with a policy whose draws matter (a table of dyadic rows, gathered on the device by the
    observation's bit count and the step) against the oracle stepped with the host's predictions: the actions, rewards
    and dones of every group step, then the full state.  A counter that does not advance or is shared between groups, a
    wrong seed offset, a wrong pointer into the action tensor all show.  The same batch cut into 2 slices, into 3, and
    dealt to two shards with env_offset 0 and B/2 is compared with the SAME prediction: the draw of an env at a step
    does not depend on how the batch is cut."""
    import torch
    from safelife_amd.runner import PipelinedRunner
    want_a, want_r, want_d, want_state = _oracle_run()
    pool, common, first = _run_pool()
    final = {name: [] for name in ENV_STATE}
    for part in RUN_LAYOUTS[layout]:
        lo, n = part["lo"], part["n"]
        dev = util.DeviceBackend(pool, n, first_level=first[lo:lo + n], slices=part["slices"], env_offset=lo,
                                 policy_layout="uint8", **common)
        env = dev.env
        assert env.slice_bounds == part["bounds"] and env.env_offset == lo
        table = torch.from_numpy(POLICY_TABLE_64 / np.float32(64)).to(env.device)
        steps, seen = {}, []

        def policy(obs):                        # obs: one group's [n, C, W, H] uint8, a view of the env's policy tensor
            t = steps.get(obs.data_ptr(), 0)    # (one view per group: its address tells the groups apart)
            steps[obs.data_ptr()] = t + 1
            total = obs.to(torch.int64).sum(dim=(1, 2, 3))
            return torch.zeros(obs.shape[0], device=obs.device), table[_policy_row(total, t)]

        def on_step(g, glo, ghi):
            seen.append((g, glo, ghi, runner.actions[glo:ghi].clone(), env.reward[glo:ghi].clone(), env.done[glo:ghi].clone()))
        runner = PipelinedRunner(env, policy, seed=RUN_SEED, on_step=on_step)
        runner.run(RUN_T)
        runner.finish()
        torch.cuda.synchronize()
        assert len(seen) == RUN_T * env.slices and len(steps) == env.slices
        for k, (g, glo, ghi, a, r, d) in enumerate(seen):
            t = k // env.slices
            assert g == k % env.slices and (glo, ghi) == env.slice_bounds[g:g + 2]
            where = slice(lo + glo, lo + ghi)
            assert np.array_equal(a.cpu().numpy(), want_a[t][where]), (t, g, "actions")
            assert np.array_equal(r.cpu().numpy(), want_r[t][where]), (t, g, "reward")
            assert np.array_equal(d.cpu().numpy().astype(bool), want_d[t][where]), (t, g, "done")
        assert np.array_equal(runner.actions.cpu().numpy(), want_a[RUN_T - 1][lo:lo + n])
        for name in ENV_STATE:
            final[name].append(dev.get(name))
    for name in ENV_STATE:
        assert np.array_equal(np.concatenate(final[name]), want_state[name]), name


# ------------------------------------------------------------------------------------------------ GPU: obs_to_policy

@gpu
def test_obs_to_policy_edges():
    """slhip_obs_to_policy against ((view[b,y,x] >> ch[c]) & 1) transposed to [B,C,vw,vh]: views with all 32 bits in
    use, degenerate shapes, channel 31, channel 0, a repeated channel, SL_MAX_CHANNELS channels, both output types, the
    output inside a canary buffer; bad arguments are SL_E_ARG."""
    import torch
    from safelife_amd import _hip
    lib, dev, st = _hip.lib(), _hip.device(), _hip.current_stream_ptr()
    assert _hip.SL_MAX_CHANNELS == 32
    rng = np.random.default_rng(65)
    pad = 4096
    lists = [(31,), (0,), (3, 31, 3, 0, 3), tuple(range(32)), tuple(reversed(range(32)))]
    for B, vh, vw in ((1, 1, 1), (3, 5, 7), (2, 1, 9), (5, 9, 1)):
        view = rng.integers(0, 2 ** 32, (B, vh, vw), dtype=np.uint64).astype(np.uint32)
        view.flat[-1] = 0x80000001
        view.flat[0] = 0xFFFFFFFF
        assert np.bitwise_or.reduce(view.ravel()) == 0xFFFFFFFF
        d_view = torch.from_numpy(view.view(np.int32)).to(dev)
        for chans in lists:
            ch = (C.c_int32 * len(chans))(*chans)
            want = np.stack([(view >> np.uint32(c)) & np.uint32(1) for c in chans], axis=1).transpose(0, 1, 3, 2)
            total = want.size
            assert want.shape == (B, len(chans), vw, vh) and (total % 256 != 0 or total < 256)
            for dtype, tdt, canary in ((0, torch.uint8, 0xA5), (1, torch.float32, -7.5)):
                buf = torch.full((total + 2 * pad,), canary, dtype=tdt, device=dev)
                out_ptr = buf.data_ptr() + pad * buf.element_size()
                _hip.check(lib.slhip_obs_to_policy(d_view.data_ptr(), B, vh, vw, ch, len(chans), out_ptr, dtype, st))
                got = buf.cpu().numpy()
                assert (got[:pad] == canary).all() and (got[pad + total:] == canary).all(), (B, vh, vw, chans, dtype)
                assert np.array_equal(got[pad:pad + total].reshape(want.shape), want.astype(got.dtype)), (B, vh, vw, chans, dtype)
    out = torch.zeros(64, dtype=torch.float32, device=dev)
    d_view = torch.zeros((1, 1, 1), dtype=torch.int32, device=dev)
    one = (C.c_int32 * 1)(0)
    assert lib.slhip_obs_to_policy(d_view.data_ptr(), 1, 1, 1, (C.c_int32 * 1)(32), 1, out.data_ptr(), 0, st) == _hip.SL_E_ARG
    assert lib.slhip_obs_to_policy(d_view.data_ptr(), 1, 1, 1, (C.c_int32 * 1)(-1), 1, out.data_ptr(), 0, st) == _hip.SL_E_ARG
    assert lib.slhip_obs_to_policy(d_view.data_ptr(), 1, 1, 1, one, 0, out.data_ptr(), 0, st) == _hip.SL_E_ARG
    assert lib.slhip_obs_to_policy(d_view.data_ptr(), 1, 1, 1, one, _hip.SL_MAX_CHANNELS + 1, out.data_ptr(), 0, st) == _hip.SL_E_ARG
    assert lib.slhip_obs_to_policy(d_view.data_ptr(), 1, 1, 1, one, 1, out.data_ptr(), 2, st) == _hip.SL_E_ARG
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0
