"""DQN replay, the part that needs no GPU: the numpy restatement (tests/replay_ref.py) against what the reference's DQN
left in its replay buffer (tests/golden/replay_cases.npz), the bookkeeping identities, the exact models of the Floyd
sampler and of the epsilon-greedy draw, and the C ABI: symbols, struct layout, argument errors (refused before anything
touches a device)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from safelife_amd import _hip
from tests import replay_ref as rr
from tests import util

CASES = rr.load_cases() if os.path.exists(os.path.join(util.GOLDEN, "replay_cases.npz")) else []
RING_COLUMNS = ("obs_b", "obs_t", "action", "reward", "next_b", "next_t", "done")


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def test_fixture_covers_the_issue():
    assert os.path.getsize(os.path.join(util.GOLDEN, "replay_cases.npz")) < 1024 * 1024
    want = {(n, T, B) for n in (1, 2, 5) for T in (1, n - 1, n, n + 1, 3 * n + 2) if T >= 1 for B in (1, 63, 64, 65, 257)}
    assert {(c["n"], c["T"], c["B"]) for c in CASES} == want
    for key in ("n", "B"):
        for v in {c[key] for c in CASES}:
            mine = [c for c in CASES if c[key] == v]
            assert {c["R"].dtype for c in mine} == {np.dtype(np.float32), np.dtype(np.float64)}
            assert {c["capacity"] == c["B"] * (c["n"] + 1) for c in mine} == {True, False}
            assert {c["gamma"] for c in mine} == {0.97, 1.0, 0.0, 0.5}
    assert sum(c["dumps"][2]["idx"] > 2 * c["capacity"] for c in CASES) >= 5        # rings that wrap more than twice
    for c in CASES:
        n, T, B, D = c["n"], c["T"], c["B"], c["D"]
        assert c["capacity"] >= B * (n + 1) and c["dump_steps"][2] == T
        if c["capacity"] != B * (n + 1):
            assert c["dumps"][2]["idx"] <= c["capacity"]                            # large enough never to wrap
        if B >= 5:                              # the five scripted columns
            assert not D[:, 0].any() and D[:, 1].all()
            assert D[T - 1, 2] and D[:, 2].sum() == 1
            assert D[:, 3].sum() == (1 if n - 1 < T else 0) and (n - 1 >= T or D[n - 1, 3])
            assert D[0, 4] and D[:, 4].sum() == 1
    assert {int(c["D"][:, 0].sum()) for c in CASES if c["B"] == 1} >= {0, 1}


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_restatement_reproduces_the_reference(case):
    """Ring contents, idx, the windows and the float64 rewards bit for bit, at the three dumps; and at every step
    idx == steps * B - pending and the min_len bound."""
    n, B, cap = case["n"], case["B"], case["capacity"]
    seen = 0
    for steps, rep in rr.replay_case(case):
        assert rep.idx == steps * B - rep.pending()
        assert rep.pending() <= n * B
        assert rr.min_len(cap, B, n, steps) <= len(rep)
        for j, s in enumerate(case["dump_steps"]):
            if s != steps:
                continue
            seen += 1
            dump, cols = case["dumps"][j], rr.ring_columns(rep)
            assert rep.idx == dump["idx"] and len(rep) == len(dump["done"])
            for name in RING_COLUMNS:
                if name == "reward":
                    assert np.array_equal(bits64(cols[name]), bits64(dump[name])), (j, name)
                else:
                    assert np.array_equal(cols[name], dump[name]), (j, name)
            assert np.array_equal(rep.fill(), dump["fill"])
            assert np.array_equal(bits64(rep.window_rewards()), bits64(dump["w_reward"]))
            for b, w in enumerate(rep.windows):
                assert [e[1] for e in w] == dump["w_action"][:len(w), b].tolist()
                assert [e[0][1] for e in w] == dump["w_obs_t"][:len(w), b].tolist()
    assert seen == 3


# ------------------------------------------------------------------------------------------------ the sampler's model

def test_sampler_model_is_distinct_and_in_range():
    for N, k in ((1, 1), (2, 1), (2, 2), (40, 8), (95, 64), (96, 96), (97, 65), (4096, 96), (4096, 4096), (100000, 96)):
        for seed, counter in ((0, 0), (5, 17), (2 ** 64 - 1, 2 ** 64 - 1), (2 ** 63, 1)):
            out = rr.sample_model(N, k, seed, counter)
            assert out.dtype == np.int64 and out.shape == (k,)
            assert out.min() >= 0 and out.max() < N and len(set(out.tolist())) == k
            if k == N:
                assert sorted(out.tolist()) == list(range(N))
    assert not np.array_equal(rr.sample_model(4096, 96, 5, 0), rr.sample_model(4096, 96, 5, 1))
    assert not np.array_equal(rr.sample_model(4096, 96, 5, 0), rr.sample_model(4096, 96, 6, 0))


def test_sampler_model_is_uniform():
    """N = 40, k = 8 over 20000 counters with a fixed seed: the inclusion counts of the 40 rows against the 0.999 quantile
    of chi-square with 39 degrees of freedom.  (The counts of a k-subset are negatively correlated: Pearson's statistic
    on them is (N-k)/(N-1) of a chi-square variable in expectation, so the bound holds with room.)"""
    from scipy.stats import chi2
    N, k, draws = 40, 8, 20000
    counts = np.zeros(N, np.int64)
    for c in range(draws):
        counts[rr.sample_model(N, k, 20261018, c)] += 1
    expected = draws * k / N
    stat = ((counts - expected) ** 2).sum() / expected
    print("chi-square", stat)
    assert counts.sum() == draws * k
    assert stat < chi2.ppf(0.999, N - 1)


# --------------------------------------------------------------------------------------------- the epsilon draw's model

def test_eps_model_extremes_ties_and_nan():
    rng = np.random.default_rng(4)
    q = rng.standard_normal((257, 9)).astype(np.float32)
    a0, r0 = rr.eps_model(q, 0.0, 5, 3)
    assert not r0.any() and np.array_equal(a0, np.argmax(q, axis=1))
    a1, r1 = rr.eps_model(q, 1.0, 5, 3)
    assert r1.all() and a1.min() >= 0 and a1.max() < 9
    ties = np.zeros((4, 9), np.float32)
    ties[1, 3] = ties[1, 7] = 2.0
    ties[2, :] = -np.inf
    ties[3, 8] = ties[3, 2] = np.inf
    assert rr.eps_model(ties, 0.0, 1, 1)[0].tolist() == [0, 3, 0, 2]
    nan = rng.standard_normal((3, 9)).astype(np.float32)
    nan[0, 4] = nan[0, 6] = np.nan
    nan[1, 0] = np.nan
    nan[2, 8] = np.nan
    nan[2, 1] = np.inf
    assert rr.eps_model(nan, 0.0, 1, 1)[0].tolist() == [4, 0, 8]
    # the sub-batch rule
    whole = rr.eps_model(q, 0.3, 5, 11)[0]
    assert np.array_equal(rr.eps_model(q[100:], 0.3, 5 + rr.policy_ref.G * 100, 11)[0], whole[100:])
    assert np.array_equal(rr.eps_model(q[100:], 0.3, 5, 11, first_env=100)[0], whole[100:])


def test_eps_model_fraction_and_uniformity():
    """At epsilon 0.03 and 0.5 over 200000 envs: the number of random draws inside 4.9 standard deviations of the binomial
    (two-sided 1e-6), and the random actions uniform over 9 by chi-square at the 0.999 quantile, 8 degrees of freedom."""
    from scipy.stats import chi2
    n, A = 200000, 9
    q = np.zeros((n, A), np.float32)
    q[:, 0] = 1.0
    for eps in (0.03, 0.5):
        a, rnd = rr.eps_model(q, eps, 99, 7)
        sd = (n * eps * (1 - eps)) ** 0.5
        assert abs(rnd.sum() - n * eps) < 4.9 * sd, (eps, rnd.sum())
        assert (a[~rnd] == 0).all()
        counts = np.bincount(a[rnd], minlength=A)
        expected = rnd.sum() / A
        stat = ((counts - expected) ** 2).sum() / expected
        print(eps, rnd.sum(), stat)
        assert stat < chi2.ppf(0.999, A - 1)


# ------------------------------------------------------------------------------------------------------------- the ABI

NAMES = ("slhip_replay_add", "slhip_replay_sample", "slhip_replay_gather", "slhip_sample_actions_eps")


def test_symbols_and_version():
    lib = _hip.lib()
    for name in NAMES:
        assert name in _hip.EXPORTS and hasattr(lib, name)
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13


def test_replay_layout_matches_header(tmp_path):
    """ctypes mirror of struct sl_replay against gcc's offsetof / sizeof, and the constants."""
    st = _hip.Replay
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "safelife_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(sl_replay));',
             'printf("consts %d %d %d %d\\n", SL_REPLAY_MAX_N, SL_REPLAY_MAX_K, SL_REPLAY_SHORT, SL_REPLAY_BAD_INDEX);']
    want = ["size %d" % C.sizeof(st), "consts %d %d %d %d" % (_hip.REPLAY_MAX_N, _hip.REPLAY_MAX_K, _hip.REPLAY_SHORT,
                                                              _hip.REPLAY_BAD_INDEX)]
    for name, ctype in st._fields_:
        lines.append('printf("%s %%zu %%zu\\n", offsetof(sl_replay, %s), sizeof(((sl_replay *)0)->%s));'
                     % (name, name, name))
        want.append("%s %d %d" % (name, getattr(st, name).offset, C.sizeof(ctype)))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(util.REPO, "include"), str(src), "-o", exe])
    got = [g for g in subprocess.check_output([exe]).decode().split("\n") if g]
    assert got == want
    assert C.sizeof(st) == 264 and _hip.REPLAY_MAX_N == 16


def _replay(**kw):
    """A description whose pointers are non-null but never dereferenced: every call below is refused first."""
    s = _hip.Replay()
    s.capacity, s.obs_bytes, s.B, s.n, s.reward_dtype = 48, 16, 8, 5, _hip.REWARD_F32
    for name, ctype in _hip.Replay._fields_:
        if ctype is C.c_void_p:
            setattr(s, name, 0x1000)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


BAD_STRUCTS = [dict(B=0), dict(n=0), dict(n=17), dict(obs_bytes=0), dict(capacity=47), dict(reward_dtype=2),
               dict(reward_dtype=-1), dict(obs=None), dict(next_obs=None), dict(action=None), dict(reward=None),
               dict(done=None), dict(idx=None), dict(status=None)]


@pytest.mark.parametrize("bad", BAD_STRUCTS, ids=[str(b) for b in BAD_STRUCTS])
def test_bad_descriptions_are_refused_by_all(bad):
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    s = _replay(**bad)
    assert lib.slhip_replay_add(C.byref(s), p, p, p, p, p, None) == _hip.SL_E_ARG
    assert b"replay" in lib.slhip_last_error()
    assert lib.slhip_replay_sample(C.byref(s), 4, 0, 0, p, None) == _hip.SL_E_ARG
    assert lib.slhip_replay_gather(C.byref(s), p, 4, p, p, 0, p, p, p, None) == _hip.SL_E_ARG
    with pytest.raises(ValueError):
        _hip.check(_hip.SL_E_ARG)


def test_entry_point_argument_errors():
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    assert lib.slhip_replay_add(None, p, p, p, p, p, None) == _hip.SL_E_ARG
    for name in ("win_obs", "win_action", "win_reward", "fill", "head", "plan_base", "plan_code"):
        assert lib.slhip_replay_add(C.byref(_replay(**{name: None})), p, p, p, p, p, None) == _hip.SL_E_ARG
        assert b"window" in lib.slhip_last_error()
    s = _replay()
    for k in range(5):
        args = [p] * 5
        args[k] = None
        assert lib.slhip_replay_add(C.byref(s), *args, None) == _hip.SL_E_ARG
        assert b"null pointer" in lib.slhip_last_error()
    for k in (0, -1, _hip.REPLAY_MAX_K + 1):
        assert lib.slhip_replay_sample(C.byref(s), k, 0, 0, p, None) == _hip.SL_E_ARG
        assert b"k outside" in lib.slhip_last_error()
    assert lib.slhip_replay_sample(C.byref(s), 4, 0, 0, None, None) == _hip.SL_E_ARG
    assert lib.slhip_replay_gather(C.byref(s), p, 0, p, p, 0, p, p, p, None) == _hip.SL_E_ARG
    for k in range(6):
        args = [p] * 6
        args[k] = None
        assert lib.slhip_replay_gather(C.byref(s), args[0], 4, args[1], args[2], 0, args[3], args[4], args[5], None) \
            == _hip.SL_E_ARG
    assert lib.slhip_sample_actions_eps(p, -1, 9, 0.1, 0, 0, p, None) == _hip.SL_E_ARG
    assert lib.slhip_sample_actions_eps(p, 4, 0, 0.1, 0, 0, p, None) == _hip.SL_E_ARG
    assert lib.slhip_sample_actions_eps(p, 4, 9, float("nan"), 0, 0, p, None) == _hip.SL_E_ARG
    assert lib.slhip_sample_actions_eps(None, 4, 9, 0.1, 0, 0, p, None) == _hip.SL_E_ARG
    assert lib.slhip_sample_actions_eps(p, 4, 9, 0.1, 0, 0, None, None) == _hip.SL_E_ARG
    assert lib.slhip_sample_actions_eps(None, 0, 9, 0.1, 0, 0, None, None) == 0         # nothing to draw


def test_replay_buffer_argument_errors():
    """Refused in Python, before any device is looked for."""
    import torch
    from safelife_amd.replay import ReplayBuffer
    ok = dict(capacity=48, num_envs=8, multi_step=5, obs_shape=(4,), obs_dtype=torch.uint8, device="cpu")
    for bad in (dict(capacity=47), dict(multi_step=17), dict(multi_step=0), dict(reward_dtype=torch.float16),
                dict(reward_dtype=torch.int32), dict(num_envs=0), dict(obs_shape=(0,))):
        with pytest.raises(ValueError):
            ReplayBuffer(**dict(ok, **bad))
