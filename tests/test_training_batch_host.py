"""PPO training batches, the part that needs no GPU: the numpy restatement of the returns / GAE contract
(tests/gae_ref.py) against what the reference's PPO.gen_training_batch computed (tests/golden/gae_cases.npz), four
deliberately wrong readings of the contract that the fixture must tell apart, and the C ABI of slhip_rollout_record /
slhip_training_batch: symbols, struct layout, argument errors (all refused before anything touches a device)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from safelife_amd import _hip
from tests import gae_ref, util

CASES = gae_ref.load_cases() if os.path.exists(os.path.join(util.GOLDEN, "gae_cases.npz")) else []


def test_fixture_covers_the_issue():
    assert os.path.getsize(os.path.join(util.GOLDEN, "gae_cases.npz")) < 1024 * 1024
    for dt in (np.float32, np.float64):
        mine = [c for c in CASES if c["R"].dtype == dt]
        assert {(c["T"], c["B"]) for c in mine} == {(T, B) for T in (1, 2, 3, 20) for B in (1, 63, 64, 65, 257)}
        assert {(c["gamma"], c["lmda"]) for c in mine} == {(0.97, 0.95), (1.0, 1.0), (0.0, 0.0), (0.5, 0.999)}
    for c in CASES:
        T, B, D = c["T"], c["B"], c["D"]
        assert np.array_equal(c["values"], c["V"][:T])
        assert np.all(c["action_prob"] == np.float32(1.0 / c["n_actions"]))
        if B >= 5:                              # the five scripted columns
            assert not D[:, 0].any() and D[:, 1].all()
            assert D[T - 1, 2] and D[:, 2].sum() == 1
            assert D[:, 3].sum() == (1 if T >= 2 else 0) and (T < 2 or D[T - 2, 3])
            assert D[0, 4] and D[:, 4].sum() == 1
    assert {int(c["D"][:, 0].sum()) for c in CASES if c["B"] == 1} >= {0, 1}


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_restatement_reproduces_the_reference(case):
    ret, adv, start = gae_ref.training_batch(case["R"], case["D"], case["V"][:-1], case["V"][-1], case["gamma"], case["lmda"])
    assert ret.dtype == adv.dtype == np.float32
    assert np.array_equal(gae_ref.bits(ret), gae_ref.bits(case["returns"]))
    assert np.array_equal(gae_ref.bits(adv), gae_ref.bits(case["advantages"]))
    want = np.ones_like(case["D"])
    want[1:] = case["D"][:-1] != 0
    assert np.array_equal(start, want)


@pytest.mark.parametrize("variant", gae_ref.WRONG_VARIANTS)
def test_fixture_tells_a_wrong_reading_apart(variant):
    """Each of the plausible misreadings differs from the reference on at least one case."""
    failing = []
    for c in CASES:
        ret, adv, _ = gae_ref.training_batch(c["R"], c["D"], c["V"][:-1], c["V"][-1], c["gamma"], c["lmda"], **{variant: True})
        if not (np.array_equal(gae_ref.bits(ret), gae_ref.bits(c["returns"]))
                and np.array_equal(gae_ref.bits(adv), gae_ref.bits(c["advantages"]))):
            failing.append(c["id"])
    assert failing, variant


def test_worked_example():
    """Two columns by hand: a closed trajectory followed by a one-step open tail, and an open three-step trajectory."""
    f32 = np.float32
    R = np.array([[1.0, 0.5], [2.0, 0.25], [4.0, 0.125]], f32)
    D = np.array([[0, 0], [1, 0], [0, 0]], np.uint8)
    V = np.array([[0.5, 1.0], [0.25, 2.0], [0.125, 3.0]], f32)
    fv = np.array([8.0, 4.0], f32)
    ret, adv, start = gae_ref.training_batch(R, D, V, fv, 0.5, 0.5)
    # column 0: steps 0-1 closed (no bootstrap), step 2 open with one step (bootstrapped with fv)
    assert list(ret[:, 0]) == [1.0 + 0.5 * 2.0, 2.0, 4.0 + 0.5 * 8.0]
    assert list(adv[:, 0]) == [(1.0 + 0.5 * 0.25 - 0.5) + 0.5 * (2.0 - 0.25), 2.0 - 0.25, 4.0 + 0.5 * 8.0 - 0.125]
    # column 1: one open trajectory
    assert list(ret[:, 1]) == [0.5 + 0.5 * (0.25 + 0.5 * (0.125 + 2.0)), 0.25 + 0.5 * (0.125 + 2.0), 0.125 + 2.0]
    a2 = 0.125 + 0.5 * 4.0 - 3.0
    a1 = 0.25 + 0.5 * 3.0 - 2.0 + 0.5 * a2
    assert list(adv[:, 1]) == [0.5 + 0.5 * 2.0 - 1.0 + 0.5 * a1, a1, a2]
    assert start.tolist() == [[1, 1], [0, 0], [1, 0]]


# ------------------------------------------------------------------------------------------------------------- the ABI

def test_symbols_and_version():
    lib = _hip.lib()
    for name in ("slhip_rollout_record", "slhip_training_batch"):
        assert name in _hip.EXPORTS and hasattr(lib, name)
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13


def test_rollout_layout_matches_header(tmp_path):
    """ctypes mirror of struct sl_rollout against gcc's offsetof / sizeof, and the constants."""
    st = _hip.Rollout
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "safelife_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(sl_rollout));',
             'printf("consts %d %d %d\\n", SL_REWARD_F32, SL_REWARD_F64, SL_ROLLOUT_BAD_ACTION);']
    want = ["size %d" % C.sizeof(st), "consts %d %d %d" % (_hip.REWARD_F32, _hip.REWARD_F64, _hip.ROLLOUT_BAD_ACTION)]
    for name, ctype in st._fields_:
        lines.append('printf("%s %%zu %%zu\\n", offsetof(sl_rollout, %s), sizeof(((sl_rollout *)0)->%s));'
                     % (name, name, name))
        want.append("%s %d %d" % (name, getattr(st, name).offset, C.sizeof(ctype)))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(util.REPO, "include"), str(src), "-o", exe])
    got = [g for g in subprocess.check_output([exe]).decode().split("\n") if g]
    assert got == want
    assert C.sizeof(st) == 80


def _rollout(**kw):
    """A description whose pointers are non-null but never dereferenced: every call below is refused first."""
    s = _hip.Rollout()
    s.T, s.B, s.reward_dtype, s.row_stride, s.out_stride = 4, 8, _hip.REWARD_F32, 8, 8
    for name in ("actions", "action_prob", "rewards", "values", "done", "status"):
        setattr(s, name, 0x1000)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


BAD_STRUCTS = [dict(T=0), dict(T=-1), dict(B=0), dict(reward_dtype=2), dict(reward_dtype=-1), dict(row_stride=7),
               dict(rewards=None), dict(values=None), dict(done=None)]


@pytest.mark.parametrize("bad", BAD_STRUCTS, ids=[str(b) for b in BAD_STRUCTS])
def test_bad_descriptions_are_refused_by_both(bad):
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    s = _rollout(**bad)
    assert lib.slhip_rollout_record(C.byref(s), 0, p, p, 9, p, p, p, None) == _hip.SL_E_ARG
    assert b"rollout" in lib.slhip_last_error()
    assert lib.slhip_training_batch(C.byref(s), p, 0.97, 0.95, p, p, None, None) == _hip.SL_E_ARG
    assert b"rollout" in lib.slhip_last_error()
    with pytest.raises(ValueError):
        _hip.check(_hip.SL_E_ARG)


def test_record_argument_errors():
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    assert lib.slhip_rollout_record(None, 0, p, p, 9, p, p, p, None) == _hip.SL_E_ARG
    for bad in (dict(actions=None), dict(action_prob=None), dict(status=None)):
        assert lib.slhip_rollout_record(C.byref(_rollout(**bad)), 0, p, p, 9, p, p, p, None) == _hip.SL_E_ARG
    s = _rollout()
    for t in (-1, 4):
        assert lib.slhip_rollout_record(C.byref(s), t, p, p, 9, p, p, p, None) == _hip.SL_E_ARG
        assert b"t outside" in lib.slhip_last_error()
    assert lib.slhip_rollout_record(C.byref(s), 0, p, p, 0, p, p, p, None) == _hip.SL_E_ARG
    for k in range(5):
        args = [p] * 5
        args[k] = None
        assert lib.slhip_rollout_record(C.byref(s), 0, args[0], args[1], 9, args[2], args[3], args[4], None) == _hip.SL_E_ARG
        assert b"null pointer" in lib.slhip_last_error()


def test_training_batch_argument_errors():
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    assert lib.slhip_training_batch(None, p, 0.97, 0.95, p, p, None, None) == _hip.SL_E_ARG
    assert lib.slhip_training_batch(C.byref(_rollout(out_stride=7)), p, 0.97, 0.95, p, p, None, None) == _hip.SL_E_ARG
    assert b"out_stride" in lib.slhip_last_error()
    s = _rollout(actions=None, action_prob=None, status=None)       # not needed by this entry point
    for k in range(3):
        args = [p] * 3
        args[k] = None
        assert lib.slhip_training_batch(C.byref(s), args[0], 0.97, 0.95, args[1], args[2], None, None) == _hip.SL_E_ARG
        assert b"null pointer" in lib.slhip_last_error()
