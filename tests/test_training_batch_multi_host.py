"""Multi-agent PPO training batches, the part that needs no GPU: the numpy restatement of the masked-window contract
(tests/gae_multi_ref.py) against what the reference's PPO.gen_training_batch computed over two consecutive windows of
multi-agent envs (tests/golden/gae_multi_cases.npz), against the single-agent restatement and its fixture where there is
one agent, five deliberately wrong readings that the fixture must tell apart, and the C ABI of the new entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from safelife_amd import _hip
from tests import gae_multi_ref, gae_ref, util

CASES = gae_multi_ref.load_cases()
bits = gae_multi_ref.bits


def test_fixture_covers_the_issue():
    assert os.path.getsize(os.path.join(util.GOLDEN, "gae_multi_cases.npz")) < 1024 * 1024
    for dt in (np.float32, np.float64):
        mine = [c for c in CASES if c["R"].dtype == dt]
        assert {(c["T"], c["A"]) for c in mine} == {(T, A) for T in (1, 2, 3, 20) for A in (1, 2, 3, 8)}
        assert {(c["gamma"], c["lmda"]) for c in mine} == {(0.97, 0.95), (1.0, 1.0), (0.0, 0.0), (0.5, 0.999)}
    assert {c["B"] * c["A"] for c in CASES} >= {1, 2, 3, 63, 64, 65, 255, 256, 257, 258}
    valid = np.concatenate([c["valid"].ravel() for c in CASES])
    assert 0.15 <= 1.0 - valid.mean() <= 0.60
    for c in CASES:
        T, A, v, D = c["T"], c["A"], c["valid"], c["D"]
        assert np.all(c["action_prob"][v != 0] == np.float32(1.0 / c["n_actions"]))
        for name in ("returns", "advantages", "values", "action_prob"):
            assert not c[name][v == 0].any()
        if A == 1:
            assert v.all()
            continue
        # an env reloads on the step where its last agent is done; anywhere but on a window's last step that is mid-window
        all_done = D.all(axis=3)
        if T >= 3:
            assert (v == 0).any() and all_done[:, :T - 1].any(), c["id"]
        if c["B"] >= 4:
            assert v[:, :, 0, 0].all()                              # never leaves
            assert v[0, 0, 0, 1] and v[:, :, 0, 1].sum() == 1       # leaves at t = 0, away for the rest and all of window 2
            assert all_done[0, T // 2, 1] and not all_done[0, :T // 2, 1].any()      # everybody leaves together
            assert all_done[0, T - 1, 2] and not all_done[0, :T - 1, 2].any()        # reloads exactly at the end of window 1
            if T >= 2:
                assert D[0, T - 2, 2, 1] and not D[0, T - 2, 2, 0]  # one leaves at T-2, one at T-1


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_restatement_reproduces_the_reference(case):
    for w, res in enumerate(gae_multi_ref.two_windows(case)):
        assert np.array_equal(res.active, case["valid"][w]), w
        assert np.array_equal(bits(res.returns), bits(case["returns"][w])), w
        assert np.array_equal(bits(res.advantages), bits(case["advantages"][w])), w
        T, B, A = case["T"], case["B"], case["A"]
        assert np.array_equal(res.rows, np.flatnonzero(case["valid"][w].ravel()))
        assert res.traj_start.sum() == len({tuple(x) for x in res.agent_ids.tolist()})      # one start per agent id
        assert not res.traj_start[res.active == 0].any()


@pytest.mark.parametrize("case", [c for c in CASES if c["A"] == 1], ids=[c["id"] for c in CASES if c["A"] == 1])
def test_one_agent_is_the_single_agent_contract(case):
    for w, res in enumerate(gae_multi_ref.two_windows(case)):
        ret, adv, start = gae_ref.training_batch(case["R"][w, :, :, 0], case["D"][w, :, :, 0], case["values"][w, :, :, 0],
                                                 case["V_boot"][w, :, 0], case["gamma"], case["lmda"])
        assert np.array_equal(bits(res.returns[:, :, 0]), bits(ret))
        assert np.array_equal(bits(res.advantages[:, :, 0]), bits(adv))
        assert np.array_equal(res.traj_start[:, :, 0], start)
        assert res.active.all()


SINGLE = gae_ref.load_cases()


@pytest.mark.parametrize("case", SINGLE, ids=[c["id"] for c in SINGLE])
def test_reproduces_the_single_agent_goldens(case):
    res = gae_multi_ref.window(case["R"][:, :, None], case["D"][:, :, None], case["V"][:-1, :, None], case["V"][-1][:, None],
                               case["gamma"], case["lmda"])
    assert np.array_equal(bits(res.returns[:, :, 0]), bits(case["returns"]))
    assert np.array_equal(bits(res.advantages[:, :, 0]), bits(case["advantages"]))
    assert np.array_equal(res.agent_ids[:, 2], np.zeros(len(res.rows), np.int64))
    # resets so far: the done steps of the env in front of the row
    before = np.cumsum(case["D"] != 0, axis=0) - (case["D"] != 0)
    assert np.array_equal(res.agent_ids[:, 1], before.ravel())


@pytest.mark.parametrize("variant", gae_multi_ref.WRONG_VARIANTS)
def test_fixture_tells_a_wrong_reading_apart(variant):
    """Each of the plausible misreadings differs from the reference on at least one case."""
    failing = []
    for c in CASES:
        for w, res in enumerate(gae_multi_ref.two_windows(c, **{variant: True})):
            v = c["valid"][w] != 0
            same = (np.array_equal(res.active != 0, v)
                    and np.array_equal(bits(res.returns)[v], bits(c["returns"][w])[v])
                    and np.array_equal(bits(res.advantages)[v], bits(c["advantages"][w])[v]))
            if not same:
                failing.append((c["id"], w))
    assert failing, variant


def test_worked_example():
    """One env, two agents, by hand: agent 1 leaves at t = 0 and is away until the env reloads at t = 2."""
    f32 = np.float32
    R = np.array([[[1.0, 0.5]], [[2.0, 9.0]], [[4.0, 9.0]], [[8.0, 0.25]]], f32)
    D = np.array([[[0, 1]], [[0, 1]], [[1, 1]], [[0, 0]]], np.uint8)
    V = np.array([[[0.5, 1.0]], [[0.25, 7.0]], [[0.125, 7.0]], [[2.0, 3.0]]], f32)
    fv = np.array([[16.0, 32.0]], f32)
    res = gae_multi_ref.window(R, D, V, fv, 0.5, 0.5)
    assert res.active[:, 0].tolist() == [[1, 1], [1, 0], [1, 0], [1, 1]]
    assert res.traj_start[:, 0].tolist() == [[1, 1], [0, 0], [0, 0], [1, 1]]
    assert res.rows.tolist() == [0, 1, 2, 4, 6, 7]
    assert res.agent_ids.tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 1, 1]]
    assert res.resets_end.tolist() == [1] and res.active_end.all()
    # agent 0: steps 0-2 closed, step 3 open with one step
    assert list(res.returns[:, 0, 0]) == [1.0 + 0.5 * (2.0 + 0.5 * 4.0), 2.0 + 0.5 * 4.0, 4.0, 8.0 + 0.5 * 16.0]
    a2 = 4.0 - 0.125
    a1 = 2.0 + 0.5 * 0.125 - 0.25 + 0.5 * a2
    assert list(res.advantages[:, 0, 0]) == [1.0 + 0.5 * 0.25 - 0.5 + 0.5 * a1, a1, a2, 8.0 + 0.5 * 16.0 - 2.0]
    # agent 1: one closed step, a gap of two rows (left at zero), one open step
    assert list(res.returns[:, 0, 1]) == [0.5, 0.0, 0.0, 0.25 + 0.5 * 32.0]
    assert list(res.advantages[:, 0, 1]) == [0.5 - 1.0, 0.0, 0.0, 0.25 + 0.5 * 32.0 - 3.0]
    # the next window starts with agent 1 gone if it was gone at the end of this one
    res2 = gae_multi_ref.window(R[:2], D[:2], V[:2], fv, 0.5, 0.5)
    assert res2.active_end.tolist() == [[True, False]] and res2.resets_end.tolist() == [0]
    res3 = gae_multi_ref.window(R[2:], D[2:], V[2:], fv, 0.5, 0.5, res2.active_end, res2.resets_end)
    assert res3.active[:, 0].tolist() == [[1, 0], [1, 1]] and res3.agent_ids.tolist() == [[0, 0, 0], [0, 1, 0], [0, 1, 1]]


# ------------------------------------------------------------------------------------------------------------- the ABI

NEW_SYMBOLS = ("slhip_sample_actions_masked", "slhip_rollout_record_multi", "slhip_training_batch_multi",
               "slhip_rollout_compact_chunks", "slhip_rollout_compact", "slhip_rollout_gather")


def test_symbols_and_version():
    lib = _hip.lib()
    for name in NEW_SYMBOLS:
        assert name in _hip.EXPORTS and hasattr(lib, name)
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13


def test_rollout_multi_layout_matches_header(tmp_path):
    """ctypes mirror of struct sl_rollout_multi against gcc's offsetof / sizeof, and the constants."""
    st = _hip.RolloutMulti
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "safelife_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(sl_rollout_multi));',
             'printf("consts %d %d %d\\n", SL_ROLLOUT_BAD_ACTION, SL_ROLLOUT_BAD_INDEX, SL_ROLLOUT_SCAN_CHUNK);']
    want = ["size %d" % C.sizeof(st),
            "consts %d %d %d" % (_hip.ROLLOUT_BAD_ACTION, _hip.ROLLOUT_BAD_INDEX, _hip.ROLLOUT_SCAN_CHUNK)]
    for name, ctype in st._fields_:
        lines.append('printf("%s %%zu %%zu\\n", offsetof(sl_rollout_multi, %s), sizeof(((sl_rollout_multi *)0)->%s));'
                     % (name, name, name))
        want.append("%s %d %d" % (name, getattr(st, name).offset, C.sizeof(ctype)))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(util.REPO, "include"), str(src), "-o", exe])
    got = [g for g in subprocess.check_output([exe]).decode().split("\n") if g]
    assert got == want
    assert C.sizeof(st) == 96 and C.sizeof(_hip.Rollout) == 80


def _multi(**kw):
    """A description whose pointers are non-null but never dereferenced: every call below is refused first."""
    s = _hip.RolloutMulti()
    s.w.T, s.w.B, s.w.reward_dtype, s.w.row_stride, s.w.out_stride = 4, 8, _hip.REWARD_F32, 8, 8
    for name in ("actions", "action_prob", "rewards", "values", "done", "status"):
        setattr(s.w, name, 0x1000)
    s.n_agents, s.active = 2, 0x1000
    for k, v in kw.items():
        setattr(s if k in ("n_agents", "active") else s.w, k, v)
    return s


BAD_STRUCTS = [dict(T=0), dict(B=0), dict(reward_dtype=2), dict(row_stride=7), dict(rewards=None), dict(values=None),
               dict(done=None), dict(n_agents=0), dict(n_agents=9), dict(n_agents=3), dict(active=None)]


@pytest.mark.parametrize("bad", BAD_STRUCTS, ids=[str(b) for b in BAD_STRUCTS])
def test_bad_descriptions_are_refused_by_all(bad):
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    s = C.byref(_multi(**bad))
    assert lib.slhip_rollout_record_multi(s, 0, p, p, 9, p, p, p, p, p, None) == _hip.SL_E_ARG
    assert b"rollout" in lib.slhip_last_error()
    assert lib.slhip_training_batch_multi(s, p, 0.97, 0.95, p, p, None, None) == _hip.SL_E_ARG
    assert lib.slhip_rollout_compact(s, p, p, p, None) == _hip.SL_E_ARG
    assert lib.slhip_rollout_gather(s, p, 1, p, p, None, 0, None, p, p, p, p, p, None) == _hip.SL_E_ARG
    assert lib.slhip_rollout_compact_chunks(s) == 0


def test_argument_errors():
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    s = C.byref(_multi())
    assert lib.slhip_rollout_compact_chunks(s) == 1
    assert lib.slhip_rollout_compact_chunks(C.byref(_multi(T=20, B=2 * 8192, row_stride=2 * 8192, out_stride=2 * 8192))) == 80
    for t in (-1, 4):
        assert lib.slhip_rollout_record_multi(s, t, p, p, 9, p, p, p, p, p, None) == _hip.SL_E_ARG
        assert b"t outside" in lib.slhip_last_error()
    assert lib.slhip_rollout_record_multi(s, 0, p, p, 0, p, p, p, p, p, None) == _hip.SL_E_ARG
    for k in range(7):
        args = [p] * 7
        args[k] = None
        assert lib.slhip_rollout_record_multi(s, 0, args[0], args[1], 9, *args[2:], None) == _hip.SL_E_ARG
        assert b"null pointer" in lib.slhip_last_error()
    assert lib.slhip_training_batch_multi(C.byref(_multi(out_stride=7)), p, 0.97, 0.95, p, p, None, None) == _hip.SL_E_ARG
    assert b"out_stride" in lib.slhip_last_error()
    for k in range(3):
        args = [p] * 3
        args[k] = None
        assert lib.slhip_rollout_compact(s, *args, None) == _hip.SL_E_ARG
    assert lib.slhip_rollout_gather(s, p, 33, p, p, None, 0, None, p, p, p, p, p, None) == _hip.SL_E_ARG      # n > T * B
    assert lib.slhip_rollout_gather(s, p, -1, p, p, None, 0, None, p, p, p, p, p, None) == _hip.SL_E_ARG
    assert lib.slhip_rollout_gather(s, p, 1, p, p, p, 0, p, p, p, p, p, p, None) == _hip.SL_E_ARG             # obs_bytes 0
    assert lib.slhip_rollout_gather(s, p, 1, p, p, p, 16, None, p, p, p, p, p, None) == _hip.SL_E_ARG         # no obs_out
    assert lib.slhip_rollout_gather(s, None, 1, p, p, None, 0, None, p, p, p, p, p, None) == _hip.SL_E_ARG
    assert lib.slhip_rollout_gather(s, p, 0, p, p, None, 0, None, p, p, p, p, p, None) == 0                    # nothing to do
    assert lib.slhip_sample_actions_masked(p, p, 4, 0, 0, 0, p, None) == _hip.SL_E_ARG
    assert lib.slhip_sample_actions_masked(p, p, 4, 65, 0, 0, p, None) == _hip.SL_E_ARG
    assert lib.slhip_sample_actions_masked(None, p, 4, 9, 0, 0, p, None) == _hip.SL_E_ARG
    assert lib.slhip_sample_actions_masked(p, p, 0, 9, 0, 0, p, None) == 0
