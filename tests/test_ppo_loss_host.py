"""The PPO update, the part that needs no GPU: the numpy restatement of the loss and its hand-written gradients
(tests/ppo_loss_ref.py) against what the reference's PPO.calculate_loss and torch's autograd computed
(tests/golden/ppo_loss_cases.npz), the deal's host model against the reference's split points and numpy's own, five
deliberately wrong readings of the rule that the fixture must tell apart, and the C ABI: symbols, struct layout, argument
errors (all refused before anything touches a device).

Bounds of the float64 comparison -- measured; the bound is twice that.  Over the fixture's 28 cases the float64 restatement
deviates from the reference's float64 run by at most 1.4e-15 in a row's entropy (values up to 3.4: three ulps, the nine
terms are added in index order here and in torch's order there), by 3.4e-16 relative in the loss, and not at all in either
gradient (they contain no sum).  Twice that, because another summation order can only cost a few ulps of float64 and the
factor keeps the test from pinning one order; and never below four ulps of the value, because numpy's and torch's `log`
are two libraries, each correct to an ulp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from safelife_amd import _hip
from tests import ppo_loss_ref as ref
from tests import util

HAVE = os.path.exists(os.path.join(util.GOLDEN, "ppo_loss_cases.npz"))
CASES = ref.load_cases() if HAVE else []
SPLITS = ref.load_splits() if HAVE else []
IDS = [c["id"] for c in CASES]

#: measured maximal deviation of the float64 restatement from the fixture's float64 run (absolute; the loss relative)
MEASURED = dict(entropy=1.4e-15, loss=3.4e-16, dvalues=0.0, dpolicy=0.0)


def within(got, want, measured, relative=False):
    """|got - want| <= max(2 * measured, 4 ulp of want), elementwise."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    floor = 4 * np.spacing(np.abs(want))
    bound = np.maximum(2 * measured * (np.abs(want) if relative else 1.0), floor)
    return bool(np.all(np.abs(got - want) <= bound))


def agrees64(case, out):
    return (within(out["entropy"], case["entropy64"], MEASURED["entropy"])
            and within(out["loss"], case["loss64"], MEASURED["loss"], relative=True)
            and within(out["dvalues"], case["dvalues64"], MEASURED["dvalues"])
            and within(out["dpolicy"], case["dpolicy64"], MEASURED["dpolicy"]))


def test_fixture_covers_the_issue():
    assert os.path.getsize(os.path.join(util.GOLDEN, "ppo_loss_cases.npz")) < 1024 * 1024
    plain = [c for c in CASES if not c["kink"]]
    assert {c["n"] for c in plain if c["n_actions"] == 9} == {1, 63, 64, 65, 257, 4099}
    assert {c["n_actions"] for c in plain if c["n"] == 65} == {2, 9, 32}
    for n in (1, 63, 64, 65, 257):              # the bonus on and off at every row count up to two workgroups
        assert {int(c["flag32"]) for c in plain if c["n"] == n} == {0, 1}
    kinks = [c for c in CASES if c["kink"]]
    assert len(kinks) == 3 and all(c["hyper"][0] == c["hyper"][1] == 0.25 for c in kinks)
    b = np.concatenate([c["branch64"] for c in kinks])
    assert {0, 1, 2} <= set(b[:, 0]) and {0, 1, 2, 3, 4} <= set(b[:, 1]) and {0, 1, 2, 3} <= set(b[:, 2])
    assert any((c["advantages"] == 0).any() for c in kinks) and any((c["policy"] == 0).any() for c in kinks)
    assert {int(c["flag32"]) for c in kinks} == {0, 1}
    at_clip = [c for c in kinks if c["means32"][2] == c["hyper"][4]]
    assert len(at_clip) == 1 and at_clip[0]["flag32"] == 1 and at_clip[0]["flag64"] == 1
    for c in kinks:                             # dyadic: multiples of 2^-6
        for k in ("policy", "values", "returns", "old_values"):
            assert np.array_equal(c[k] * 64, np.round(c[k] * 64))
    for c in CASES:
        assert np.array_equal(c["branch32"], c["branch64"]) and c["flag32"] == c["flag64"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float64_restatement_reproduces_the_reference(case):
    out = ref.loss_and_grads(case["hyper"], **ref.inputs(case, np.float64))
    for name, want, measured, rel in (("entropy", case["entropy64"], MEASURED["entropy"], False),
                                      ("loss", case["loss64"], MEASURED["loss"], True),
                                      ("dvalues", case["dvalues64"], MEASURED["dvalues"], False),
                                      ("dpolicy", case["dpolicy64"], MEASURED["dpolicy"], False)):
        dev = float(np.max(np.abs(np.asarray(out[name], np.float64) - want)))
        print("%s %s: max deviation %.3g" % (case["id"], name, dev))
        assert within(out[name], want, measured, rel), name
    assert within(out["means"], case["means64"], MEASURED["entropy"])
    assert np.array_equal(out["branch"], case["branch64"]) and out["flag"] == case["flag64"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float32_restatement_takes_the_reference_branches(case):
    out = ref.loss_and_grads(case["hyper"], **ref.inputs(case, np.float32))
    assert out["entropy"].dtype == out["dvalues"].dtype == out["dpolicy"].dtype == np.float32
    assert np.array_equal(out["branch"], case["branch32"])
    assert out["flag"] == case["flag32"]
    # a gradient that is exactly zero in the reference's float32 run is exactly zero here
    assert np.all(out["dvalues"][case["dvalues32"] == 0] == 0)
    assert np.all(out["dpolicy"][case["dpolicy32"] == 0] == 0)
    if case["kink"]:            # dyadic inputs: the value gradient has no rounding at all
        assert np.array_equal(out["dvalues"], case["dvalues32"])


@pytest.mark.parametrize("variant", ref.WRONG_VARIANTS)
def test_fixture_tells_a_wrong_reading_apart(variant):
    failing = [c["id"] for c in CASES
               if not agrees64(c, ref.loss_and_grads(c["hyper"], **ref.inputs(c, np.float64), **{variant: True}))]
    print(variant, "fails on", failing)
    assert failing, variant
    assert all(agrees64(c, ref.loss_and_grads(c["hyper"], **ref.inputs(c, np.float64))) for c in CASES)


def test_grad_loss_and_grad_entropy_in_the_restatement():
    """grad_loss scales both gradients; grad_entropy adds the per-row entropy's own gradient -log(p + e) - p / (p + e)."""
    c = next(c for c in CASES if c["id"] == "n65-a9-on-0")
    x = ref.inputs(c, np.float64)
    one, half = ref.loss_and_grads(c["hyper"], **x), ref.loss_and_grads(c["hyper"], **x, grad_loss=0.5)
    assert np.array_equal(half["dvalues"], 0.5 * one["dvalues"]) and np.allclose(half["dpolicy"], 0.5 * one["dpolicy"], rtol=1e-14)
    w = np.linspace(-1.0, 1.0, c["n"])
    both = ref.loss_and_grads(c["hyper"], **x, grad_entropy=w)
    p = x["policy"]
    own = -np.log(p + 1e-12) - p / (p + 1e-12)
    assert np.allclose(both["dpolicy"] - one["dpolicy"], w[:, None] * own, rtol=1e-9, atol=1e-12)
    assert np.array_equal(both["dvalues"], one["dvalues"])


# -------------------------------------------------------------------------------------------------------------- the deal

def test_split_points_are_the_references():
    assert SPLITS
    for N, m, want in SPLITS:
        assert len(want) == m                   # m cuts: m + 1 pieces
        assert ref.split_points(N, m) == want, (N, m)
        from safelife_amd import ppo
        assert ppo.split_points(N, m) == want, (N, m)


def test_split_points_equal_numpy():
    from safelife_amd import ppo
    for N in range(1, 201):
        idx = np.arange(N)
        for m in range(1, 9):
            want = np.linspace(0, N, m + 2, dtype=int)[1:-1]
            assert ref.split_points(N, m) == want.tolist() == ppo.split_points(N, m)
            pieces = [p for p in np.split(idx, want) if len(p)]
            bounds = [0] + ref.split_points(N, m) + [N]
            mine = [idx[lo:hi] for lo, hi in zip(bounds[:-1], bounds[1:]) if hi > lo]
            assert len(pieces) == len(mine) and all(np.array_equal(a, b) for a, b in zip(pieces, mine))


def test_pieces_equal_minibatches_is_told_apart():
    """The fifth wrong reading: num_minibatches pieces instead of num_minibatches + 1."""
    failing = [(N, m) for N, m, want in SPLITS if ref.split_points(N, m, pieces_equal_minibatches=True) != want]
    assert failing


def test_keys_are_the_documented_mix():
    for seed, epoch in ((0, 0), (12345, 7), ((1 << 64) - 1, (1 << 40) + 3)):
        k = ref.keys(300, seed, epoch)
        assert k.dtype == np.uint64
        assert [int(x) for x in k[:5]] == [ref.key(seed, epoch, i) for i in range(5)]
        assert int(k[299]) == ref.key(seed, epoch, 299)
    assert ref.key(0, 0, 0) == 0xE220A8397B1DCDAF           # splitmix64's first output for seed 0


def test_host_model_is_a_permutation_that_depends_on_seed_and_epoch():
    from safelife_amd import ppo
    for N in (1, 5, 257, 4099):
        perms = {}
        for seed in (0, 1):
            for epoch in (0, 1, 2):
                p = ref.permutation(N, seed, epoch)
                assert np.array_equal(np.sort(p), np.arange(N))
                perms[seed, epoch] = p
                for m in (1, 4, 8):
                    pieces = ref.deal(N, m, seed, epoch)
                    assert all(len(x) for x in pieces) and len(pieces) == min(m + 1, len(pieces))
                    assert np.array_equal(np.concatenate(pieces), p)
                    theirs = ppo.deal_host(N, m, seed, epoch)
                    assert len(theirs) == len(pieces) and all(np.array_equal(a, b) for a, b in zip(theirs, pieces))
        if N >= 257:
            assert not np.array_equal(perms[0, 0], perms[0, 1]) and not np.array_equal(perms[0, 0], perms[1, 0])
            assert not np.array_equal(perms[0, 1], perms[0, 2])
    assert len(ref.deal(3, 4, 0, 0)) == 3       # N < num_minibatches + 1: the zero-row pieces are left out


# ------------------------------------------------------------------------------------------------------------- the ABI

NEW = ("slhip_ppo_workspace_bytes", "slhip_ppo_loss_forward", "slhip_ppo_loss_backward", "slhip_minibatch_obs",
       "slhip_minibatch_keys")


def test_symbols_and_version():
    lib = _hip.lib()
    for name in NEW:
        assert name in _hip.EXPORTS and hasattr(lib, name)
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13
    assert lib.slhip_ppo_workspace_bytes(1) == 24 and lib.slhip_ppo_workspace_bytes(257) == 48
    assert lib.slhip_ppo_workspace_bytes(0) == 0


def test_ppo_loss_layout_matches_header(tmp_path):
    """ctypes mirror of struct sl_ppo_loss against gcc's offsetof / sizeof, and the constants."""
    st = _hip.PpoLoss
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "safelife_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(sl_ppo_loss));',
             'printf("consts %d %d %d %d\\n", SL_PPO_BAD_ACTION, SL_PPO_BAD_INDEX, SL_PPO_SUMS, SL_PPO_SUM_LOSS_F32);',
             'printf("sums %d %d %d %d %d %d %d\\n", SL_PPO_SUM_POLICY, SL_PPO_SUM_VALUE, SL_PPO_SUM_ENTROPY, '
             'SL_PPO_SUM_ENTROPY_TERM, SL_PPO_SUM_LOSS, SL_PPO_SUM_FLAG, SL_PPO_SUM_N);']
    want = ["size %d" % C.sizeof(st),
            "consts %d %d 8 %d" % (_hip.PPO_BAD_ACTION, _hip.PPO_BAD_INDEX, _hip.PPO_SUM_LOSS_F32),
            "sums " + " ".join(str(i) for i in range(len(_hip.PPO_SUMS)))]
    for name, ctype in st._fields_:
        lines.append('printf("%s %%zu %%zu\\n", offsetof(sl_ppo_loss, %s), sizeof(((sl_ppo_loss *)0)->%s));'
                     % (name, name, name))
        want.append("%s %d %d" % (name, getattr(st, name).offset, C.sizeof(ctype)))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(util.REPO, "include"), str(src), "-o", exe])
    got = [g for g in subprocess.check_output([exe]).decode().split("\n") if g]
    assert got == want
    assert C.sizeof(st) == 136
    assert _hip.PPO_SUMS == ("policy", "value", "entropy", "entropy_term", "loss", "flag", "n")


def _loss(**kw):
    """A description whose pointers are non-null but never dereferenced: every call below is refused first."""
    s = _hip.PpoLoss()
    s.n, s.N, s.n_actions = 8, 32, 9
    for name in ("values", "policy", "actions", "action_prob", "old_values", "returns", "advantages", "rows", "status"):
        setattr(s, name, 0x1000)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


BAD = [dict(n=0), dict(N=0), dict(n_actions=1), dict(n_actions=33), dict(rows=None), dict(values=None), dict(policy=None),
       dict(actions=None), dict(action_prob=None), dict(old_values=None), dict(returns=None), dict(advantages=None),
       dict(status=None)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_bad_descriptions_are_refused_by_both(bad):
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    s = _loss(**bad)
    assert lib.slhip_ppo_loss_forward(C.byref(s), p, p, p, None) == _hip.SL_E_ARG
    assert b"ppo_loss" in lib.slhip_last_error()
    assert lib.slhip_ppo_loss_backward(C.byref(s), p, None, p, p, p, None) == _hip.SL_E_ARG
    assert b"ppo_loss" in lib.slhip_last_error()


def test_argument_errors():
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    s = _loss()
    assert lib.slhip_ppo_loss_forward(None, p, p, p, None) == _hip.SL_E_ARG
    for k in range(3):
        args = [p] * 3
        args[k] = None
        assert lib.slhip_ppo_loss_forward(C.byref(s), *args, None) == _hip.SL_E_ARG
        assert b"null pointer" in lib.slhip_last_error()
    assert lib.slhip_ppo_loss_forward(C.byref(s), p, C.c_void_p(0x1004), p, None) == _hip.SL_E_ARG
    assert b"aligned" in lib.slhip_last_error()
    for k in (0, 2, 3, 4):                      # grad_entropy (1) may be null
        args = [p] * 5
        args[k] = None
        assert lib.slhip_ppo_loss_backward(C.byref(s), *args, None) == _hip.SL_E_ARG
        assert b"null pointer" in lib.slhip_last_error()
    # minibatch_obs(obs, obs_bytes, N, rows, n, out, out_float32, status, stream)
    assert lib.slhip_minibatch_obs(p, 0, 4, p, 2, p, 0, p, None) == _hip.SL_E_ARG
    assert lib.slhip_minibatch_obs(p, 16, 0, p, 2, p, 0, p, None) == _hip.SL_E_ARG
    assert lib.slhip_minibatch_obs(p, 16, 4, p, -1, p, 0, p, None) == _hip.SL_E_ARG
    assert lib.slhip_minibatch_obs(p, 16, 4, p, 0, p, 0, p, None) == 0          # nothing to move
    for k in range(4):
        args = [p] * 4
        args[k] = None
        assert lib.slhip_minibatch_obs(args[0], 16, 4, args[1], 2, args[2], 0, args[3], None) == _hip.SL_E_ARG
        assert b"null pointer" in lib.slhip_last_error()
    assert lib.slhip_minibatch_obs(p, 16, 4, p, 2, C.c_void_p(0x1002), 1, p, None) == _hip.SL_E_ARG
    assert lib.slhip_minibatch_keys(-1, 0, 0, p, None) == _hip.SL_E_ARG
    assert lib.slhip_minibatch_keys(0, 0, 0, None, None) == 0
    assert lib.slhip_minibatch_keys(4, 0, 0, None, None) == _hip.SL_E_ARG
    with pytest.raises(ValueError):
        _hip.check(_hip.SL_E_ARG)
