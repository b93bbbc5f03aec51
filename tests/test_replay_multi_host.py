"""Multi-agent DQN replay, the part that needs no GPU: the masked numpy restatement (tests/replay_multi_ref.py) against what
the reference's DQN left in its replay buffer when driven with multi-agent envs (tests/golden/replay_multi_cases.npz), its
agreement with the single-agent restatement when there is one agent and everybody is active, the carried state, the model
of the masked epsilon-greedy draw, the min_len bound, and the argument errors of the new entry points and classes (refused
before anything touches a device)."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

from safelife_amd import _hip
from tests import replay_multi_ref as mr
from tests import replay_ref as rr
from tests import util

CASES = mr.load_cases()
SINGLE = rr.load_cases()
RING_COLUMNS = ("obs_c", "obs_t", "action", "reward", "next_c", "next_t", "done")
Step = collections.namedtuple("Step", "obs actions rewards done next_obs active")


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def test_fixture_covers_the_issue():
    assert os.path.getsize(os.path.join(util.GOLDEN, "replay_multi_cases.npz")) < 1024 * 1024
    assert {c["A"] for c in CASES} >= {1, 2, 3, 8}
    assert {c["columns"] for c in CASES} == {4, 63, 64, 65, 1023, 1024, 1026, 1032}
    assert {(c["B"], c["A"]) for c in CASES if c["columns"] > 1000} == {(341, 3), (512, 2), (513, 2), (129, 8)}
    assert (1, 4) in {(c["B"], c["A"]) for c in CASES}
    small = {(c["n"], c["T"]) for c in CASES if c["columns"] < 100}
    assert small == {(n, T) for n in (1, 2, 5) for T in (1, n, n + 1, 3 * n + 2)}
    for cols in (4, 63, 64, 65):
        assert {(c["n"], c["T"]) for c in CASES if c["columns"] == cols} == small
    for cols in (1023, 1024, 1026, 1032):
        assert 5 in {c["n"] for c in CASES if c["columns"] == cols}
    assert {c["R"].dtype for c in CASES} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert {c["gamma"] for c in CASES} == {0.97, 1.0, 0.0, 0.5}
    tight = [c for c in CASES if c["capacity"] == c["columns"] * (c["n"] + 1)]
    assert sum(c["A"] >= 2 and c["dumps"][2]["idx"] > 2 * c["capacity"] for c in tight) >= 3    # wrap more than twice
    loose = [c for c in CASES if c["capacity"] != c["columns"] * (c["n"] + 1)]
    assert len(loose) > 10 and all(c["dumps"][2]["idx"] <= c["capacity"] for c in loose)        # never wrap
    away_and_back = 0
    for c in CASES:
        n, T, B, A, D, on = c["n"], c["T"], c["B"], c["A"], c["D"] != 0, c["active"] != 0
        assert c["capacity"] >= c["columns"] * (n + 1) and c["dump_steps"][2] == T
        assert on.any(axis=2).all() and on[0].all()                     # every env step has somebody in it
        assert not c["ACT"][~on].any() and not c["R"][~on].any()
        assert D[~on].all()                                             # done stays 1 for an agent that has left
        if B >= 4:                                                      # the scripted envs
            assert not D[:, 0].any() and D[:, 1].all() and on[:, 1].all()
            assert D[T - 1, 2].all() and not D[:T - 1, 2].any()
        if A >= 2 and T > n + 2:
            b = 3 if B >= 4 else 0
            assert D[0, b, 0] and not on[1:n + 2, b, 0].any() and on[1:n + 2, b, 1:].all() and on[n + 2, b].all()
            away_and_back += 1
    assert away_and_back >= 10
    frac = 1.0 - np.concatenate([c["active"].ravel() for c in CASES]).mean()
    assert 0.1 < frac < 0.5


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_restatement_reproduces_the_reference(case):
    """Ring contents and order, idx, the windows, the float64 rewards bit for bit and the envs' reset counts at the three
    dumps; the carried state restated here is the mask the reference implied, step by step; the min_len bound."""
    n, B, A, N, cap = case["n"], case["B"], case["A"], case["columns"], case["capacity"]
    seen, agent_steps = 0, 0
    assert case["active"][0].all()
    for steps, rep, active, resets in mr.replay_case(case):
        agent_steps += int(case["active"][steps - 1].sum())
        assert rep.idx == agent_steps - rep.pending() and rep.pending() <= n * N
        assert mr.min_len(cap, B, A, n, steps) <= len(rep)
        if steps < case["T"]:
            assert np.array_equal(active, case["active"][steps] != 0), steps
        for j, s in enumerate(case["dump_steps"]):
            if s != steps:
                continue
            seen += 1
            dump, cols = case["dumps"][j], mr.ring_columns(rep)
            assert rep.idx == dump["idx"] and len(rep) == len(dump["done"])
            for name in RING_COLUMNS:
                if name == "reward":
                    assert np.array_equal(bits64(cols[name]), bits64(dump[name])), (j, name)
                else:
                    assert np.array_equal(cols[name], dump[name]), (j, name)
            assert np.array_equal(rep.fill(), dump["fill"])
            assert np.array_equal(bits64(rep.window_rewards()), bits64(dump["w_reward"]))
            for c, w in enumerate(rep.windows):
                assert [e[1] for e in w] == dump["w_action"][:len(w), c].tolist()
                assert [e[0] for e in w] == [(c, t) for t in dump["w_obs_t"][:len(w), c].tolist()]
            assert np.array_equal(resets, dump["resets"])
    assert seen == 3


@pytest.mark.parametrize("case", SINGLE, ids=[c["id"] for c in SINGLE])
def test_one_agent_all_active_is_the_single_agent_restatement(case):
    n, B, T = case["n"], case["B"], case["T"]
    multi = mr.MultiReplay(case["capacity"], B, 1, n, case["gamma"])
    on = np.ones((B, 1), np.uint8)
    for t, (steps, single) in enumerate(rr.replay_case(case)):
        multi.add([(b, t) for b in range(B)], case["A"][t], case["R"][t], case["D"][t], [(b, t + 1) for b in range(B)], on)
        assert multi.idx == single.idx and multi.ring == single.ring and multi.windows == single.windows
    dump, cols = case["dumps"][2], rr.ring_columns(multi)
    assert multi.idx == dump["idx"] and np.array_equal(bits64(cols["reward"]), bits64(dump["reward"]))
    for name in ("obs_b", "obs_t", "action", "next_b", "next_t", "done"):
        assert np.array_equal(cols[name], dump[name])


def test_carried_state():
    active = np.array([[1, 1, 1], [1, 0, 1], [0, 0, 1], [1, 1, 1]], bool)
    done = np.array([[0, 1, 0], [1, 1, 0], [1, 1, 1], [1, 1, 1]], np.uint8)         # (1 for whoever is gone already)
    now, resets = mr.carried_state(active, np.array([0, 2, 5, 7]), done)
    assert now.tolist() == [[True, False, True], [False, False, True], [True, True, True], [True, True, True]]
    assert resets.tolist() == [0, 2, 6, 8] and resets.dtype == np.int64
    assert active[2].tolist() == [False, False, True]                               # the inputs are left alone


def test_masked_eps_model():
    rng = np.random.default_rng(8)
    for B in (1, 255, 1032):
        q = rng.standard_normal((B, 9)).astype(np.float32)
        active = (rng.random(B) < 0.6).astype(np.uint8)
        active[0] = 0 if B > 1 else 1
        poisoned = q.copy()
        poisoned[active == 0] = np.nan
        for eps in (0.0, 0.3, 1.0):
            want, _ = rr.eps_model(q, eps, 77, 5)
            got = mr.eps_model_masked(poisoned, active, eps, 77, 5)
            assert got.dtype == np.int32 and np.array_equal(got[active != 0], want[active != 0])
            assert not got[active == 0].any()
        assert np.array_equal(mr.eps_model_masked(q, np.ones(B, np.uint8), 0.3, 77, 5), rr.eps_model(q, 0.3, 77, 5)[0])
        if B > 1:           # the shard rule: rows [lo, B) drawn on their own
            lo = B // 3
            whole = mr.eps_model_masked(poisoned, active, 0.3, 77, 5)
            assert np.array_equal(mr.eps_model_masked(poisoned[lo:], active[lo:], 0.3, 77 + rr.policy_ref.G * lo, 5), whole[lo:])
            assert np.array_equal(mr.eps_model_masked(poisoned[lo:], active[lo:], 0.3, 77, 5, first_row=lo), whole[lo:])


# ------------------------------------------------------------------------------------------------------------- the ABI

NAMES = ("slhip_replay_add_masked", "slhip_sample_actions_eps_masked")


def test_symbols_and_version():
    lib = _hip.lib()
    header = open(os.path.join(util.REPO, "include", "safelife_hip.h")).read()
    for name in NAMES:
        assert name in _hip.EXPORTS and hasattr(lib, name) and name + "(" in header
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13
    assert C.sizeof(_hip.Replay) == 264


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


def test_entry_point_argument_errors():
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    assert lib.slhip_replay_add_masked(None, p, p, p, p, p, p, None) == _hip.SL_E_ARG
    for bad in (dict(B=0), dict(n=17), dict(capacity=47), dict(reward_dtype=2), dict(obs=None), dict(idx=None)):
        assert lib.slhip_replay_add_masked(C.byref(_replay(**bad)), p, p, p, p, p, p, None) == _hip.SL_E_ARG
        assert b"replay" in lib.slhip_last_error()
    for name in ("win_obs", "win_action", "win_reward", "fill", "head", "plan_base", "plan_code"):
        assert lib.slhip_replay_add_masked(C.byref(_replay(**{name: None})), p, p, p, p, p, None, None) == _hip.SL_E_ARG
        assert b"window" in lib.slhip_last_error()
    s = _replay()
    for k in range(5):              # (the mask is the one pointer that may be null)
        args = [p] * 5
        args[k] = None
        assert lib.slhip_replay_add_masked(C.byref(s), *args, p, None) == _hip.SL_E_ARG
        assert b"null pointer" in lib.slhip_last_error()
    for active in (p, None):
        assert lib.slhip_sample_actions_eps_masked(p, active, -1, 9, 0.1, 0, 0, p, None) == _hip.SL_E_ARG
        assert lib.slhip_sample_actions_eps_masked(p, active, 4, 0, 0.1, 0, 0, p, None) == _hip.SL_E_ARG
        assert lib.slhip_sample_actions_eps_masked(p, active, 4, 9, float("nan"), 0, 0, p, None) == _hip.SL_E_ARG
        assert lib.slhip_sample_actions_eps_masked(None, active, 4, 9, 0.1, 0, 0, p, None) == _hip.SL_E_ARG
        assert lib.slhip_sample_actions_eps_masked(p, active, 4, 9, 0.1, 0, 0, None, None) == _hip.SL_E_ARG
        assert lib.slhip_sample_actions_eps_masked(None, active, 0, 9, 0.1, 0, 0, None, None) == 0      # nothing to draw


def test_buffer_argument_errors():
    """Refused in Python, before any device is looked for."""
    import torch
    from safelife_amd.replay import MultiAgentReplayBuffer, ReplayBuffer
    ok = dict(capacity=96, num_envs=8, n_agents=2, multi_step=5, obs_shape=(4,), obs_dtype=torch.uint8, device="cpu")
    for bad in (dict(capacity=95), dict(n_agents=0), dict(n_agents=9), dict(multi_step=17), dict(multi_step=0),
                dict(reward_dtype=torch.float16), dict(num_envs=0), dict(obs_shape=(0,))):
        with pytest.raises(ValueError):
            MultiAgentReplayBuffer(**dict(ok, **bad))
    buf = MultiAgentReplayBuffer(**ok)
    assert isinstance(buf, ReplayBuffer) and buf.columns == 16 and buf.win_obs.shape == (5, 16, 4) and buf.fill.shape == (16,)
    assert (buf.num_envs, buf.n_agents, buf.struct.B, buf.struct.n) == (8, 2, 16, 5)
    z = torch.zeros((8, 2), dtype=torch.uint8)
    obs = torch.zeros((8, 2, 4), dtype=torch.uint8)
    no_active = collections.namedtuple("S", "obs actions rewards done next_obs")(obs, z, torch.zeros((8, 2)), z, obs)
    with pytest.raises(ValueError, match="active"):
        buf.add(no_active)
    with pytest.raises(ValueError, match="rewards"):
        buf.add(Step(obs, z, torch.zeros((8, 2), dtype=torch.float64), z, obs, z))
    with pytest.raises(RuntimeError):                   # a field of the wrong size
        buf.add(Step(obs[:7], z, torch.zeros((8, 2)), z, obs, z))
    assert buf.steps_added == 0
    # the bound: B env steps in, at most n per column pending
    for steps in (0, 5, 10, 11, 40):
        buf.steps_added = steps
        assert buf.min_len() == mr.min_len(96, 8, 2, 5, steps) == min(96, max(0, 8 * steps - 80))
    assert ReplayBuffer(48, 8, multi_step=5, obs_shape=(4,), obs_dtype=torch.uint8, device="cpu").columns == 8


def test_runner_argument_errors():
    from safelife_amd.runner import MultiAgentDQNRunner, MultiAgentDQNStep

    class NotMulti(object):
        policy_tensor = object()

    with pytest.raises(ValueError, match="SafeLifeMultiAgentVectorEnv"):
        MultiAgentDQNRunner(NotMulti(), None)
    assert MultiAgentDQNStep._fields == ("obs", "actions", "rewards", "done", "next_obs", "agent_ids", "active")
