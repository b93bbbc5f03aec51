"""
Level schedules for multi-agent envs without a GPU: the ABI of slhip_schedule_required_multi / _harvest_multi, the host
restatement (tests/schedule_multi_ref.py) against what the reference computes (tests/golden/schedule_multi_cases.npz,
written by tests/golden/make_golden_schedule_multi.py), and the argument checks of safelife_amd.schedule for multi-agent
pools.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from safelife_amd import _hip, levels, schedule
from tests import schedule_multi_ref as smr
from tests import schedule_ref as sr
from tests import util

#: The largest |restatement - reference| over EVERY curriculum probability of the multi-agent golden cases (1720 episodes;
#: 2, 3 and 8 agents; 2 and 3 groups; lookback 100 and 5), measured on the CPU: 1.6542323066914832e-14 (per case 1.9e-15,
#: 1.5e-14, 1.7e-14, 1.7e-15, 3.1e-15, 7.8e-16).  The performances that enter are the reference's bit for bit
#: (test_performances_equal_the_reference_bit_for_bit), so -- as in the single-agent test -- this is the reference's
#: polyfit against the closed-form slope, amplified by the division by the smallest |progress|.
CURRICULUM_MULTI_MEASURED = 1.6542323066914832e-14
#: The bound of the tests, derived as test_level_schedule_host.CURRICULUM_BOUND is: the measured value times 2.  The only
#: operation that is not exactly specified is exp(), whose last-ulp differences between libms (or the device's) move a
#: probability by a few 1e-16.
CURRICULUM_MULTI_BOUND = 2 * CURRICULUM_MULTI_MEASURED

TRACES = ("multi_asym1", "multi_build_coop", "multi_build_compete", "multi_hand_exit")


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "schedule_multi_cases.npz")) as d:
        return {k: d[k] for k in d.files}


def synthetic_levels(g, agents):
    """The fixture's synthetic levels with `agents` agents, as Level objects."""
    out = []
    for k in np.flatnonzero(g["syn_agents"] == agents):
        out.append(levels.Level(g["syn_board"][k], g["syn_goals"][k], g["syn_agent_locs"][k, :agents].astype(np.int64), 0.0,
                                float(g["syn_min_performance"][k]), g["syn_points_table"][k, :agents].astype(np.int64),
                                rng_words=np.arange(4, dtype=np.uint64) + 1))
    return out


# ------------------------------------------------------------------------------------------------------------- the ABI

NAMES = ("slhip_schedule_required_multi", "slhip_schedule_harvest_multi")


def test_symbols_and_version():
    lib = _hip.lib()
    for name in NAMES:
        assert name in _hip.EXPORTS and hasattr(lib, name)
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13


def test_multi_layout_matches_header(tmp_path):
    """ctypes mirror of struct sl_level_schedule_multi against gcc's offsetof / sizeof; the inner struct keeps its size."""
    st = _hip.LevelScheduleMulti
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "safelife_hip.h"', 'int main(void) {',
             'printf("size %zu %zu %zu %d\\n", sizeof(sl_level_schedule_multi), sizeof(sl_level_schedule), '
             'sizeof(sl_level_agent), SL_MAX_AGENTS);']
    want = ["size %d 168 32 %d" % (C.sizeof(st), _hip.SL_MAX_AGENTS)]
    for name, ctype in st._fields_:
        lines.append('printf("%s %%zu %%zu\\n", offsetof(sl_level_schedule_multi, %s), sizeof(((sl_level_schedule_multi *)0)->%s));'
                     % (name, name, name))
        want.append("%s %d %d" % (name, getattr(st, name).offset, C.sizeof(ctype)))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(util.REPO, "include"), str(src), "-o", exe])
    got = [x for x in subprocess.check_output([exe]).decode().split("\n") if x]
    assert got == want
    assert C.sizeof(st) == 208 and C.sizeof(_hip.LevelSchedule) == 168


def _multi(n_agents=2, **kw):
    """A description whose pointers are non-null but never dereferenced: every call below is refused first."""
    m = _hip.LevelScheduleMulti()
    m.s.G, m.s.lookback, m.s.L = 2, 100, 64
    m.s.start[0], m.s.len[0], m.s.start[1], m.s.len[1] = 0, 10, 10, 54
    for name, ctype in _hip.LevelSchedule._fields_:
        if ctype is C.c_void_p:
            setattr(m.s, name, 0x1000)
    m.n_agents = n_agents
    for name in ("available", "reward_possible", "pool_agents", "out"):
        setattr(m, name, 0x1000)
    for k, v in kw.items():
        if k in ("G", "lookback", "L"):
            setattr(m.s, k, v)
        elif k.startswith("s_"):
            setattr(m.s, k[2:], v)
        else:
            setattr(m, k, v)
    return m


def test_entry_point_argument_errors():
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    ok = _multi()
    for f in (float("nan"), float("inf"), -float("inf")):
        assert lib.slhip_schedule_required_multi(C.byref(ok), f, None) == _hip.SL_E_SHAPE
    assert b"fraction" in lib.slhip_last_error()
    for A in (0, -1, 9):
        assert lib.slhip_schedule_required_multi(C.byref(_multi(A)), 0.5, None) == _hip.SL_E_SHAPE, A
        assert b"n_agents" in lib.slhip_last_error()
        assert lib.slhip_schedule_harvest_multi(C.byref(_multi(A)), p, 8, None) == _hip.SL_E_SHAPE, A
    assert lib.slhip_schedule_required_multi(C.byref(_multi(L=0)), 0.5, None) == _hip.SL_E_SHAPE
    assert lib.slhip_schedule_required_multi(C.byref(_multi(8, L=2 ** 31 - 1)), 0.5, None) == _hip.SL_E_SHAPE
    assert lib.slhip_schedule_required_multi(None, 0.5, None) == _hip.SL_E_ARG
    for name in ("s_min_performance", "available", "pool_agents"):
        assert lib.slhip_schedule_required_multi(C.byref(_multi(**{name: None})), 0.5, None) == _hip.SL_E_ARG, name
    assert lib.slhip_schedule_harvest_multi(None, p, 8, None) == _hip.SL_E_ARG
    assert lib.slhip_schedule_harvest_multi(C.byref(ok), p, 0, None) == _hip.SL_E_SHAPE
    assert lib.slhip_schedule_harvest_multi(C.byref(ok), None, 8, None) == _hip.SL_E_ARG
    for bad in (dict(G=0), dict(G=9), dict(lookback=1), dict(lookback=1025), dict(L=0)):
        assert lib.slhip_schedule_harvest_multi(C.byref(_multi(**bad)), p, 8, None) == _hip.SL_E_SHAPE, bad
        assert b"schedule" in lib.slhip_last_error()
    for name in ("reward_possible", "out", "s_cur_slot", "s_ring", "s_count", "s_episodes", "s_pos", "s_best", "s_mean"):
        assert lib.slhip_schedule_harvest_multi(C.byref(_multi(**{name: None})), p, 8, None) == _hip.SL_E_ARG, name


# ------------------------------------------------------------------------------------- the restatement against the reference

def test_required_points_equal_the_reference(golden):
    g = golden
    n, F = len(g["req_level"]), len(g["req_fraction"])
    assert g["req_points"].shape == (n, F, 8) and F == 9
    assert sorted(set(g["req_agents"].tolist())) == [1, 2, 3, 8] and set(g["req_source"].tolist()) == {0, 1, 2, 3, 4}
    pairs = 0
    for k in range(n):
        A, mp = int(g["req_agents"][k]), g["req_min_performance"][k]
        for j, f in enumerate(g["req_fraction"]):
            want = g["req_points"][k, j, :A]
            assert np.array_equal(smr.required_points_multi(mp, f, g["req_available"][k, :A]), want), (k, f)
            assert [levels.required_points(np.float64(mp) * f, int(a)) for a in g["req_available"][k, :A]] == want.tolist()
            assert (g["req_points"][k, j, A:] == 0).all()
            pairs += A
    assert pairs == 9 * int(g["req_agents"].sum())
    # the agents of a level do ask for different amounts (or the per-agent path would show nothing)
    assert any(len(set(g["req_points"][k, 6, :g["req_agents"][k]].tolist())) > 1 for k in range(n))


def test_schedule_inputs_are_the_reference_per_agent(golden):
    """LevelSchedule.available is [L, A] and the reference's initial_available_points() for every agent; reward_possible
    adds the exit's points; LevelPool's own per-agent required points follow from it."""
    g = golden
    pools = [(s, util.levels_from_trace(util.load_trace(name)), 2) for s, name in enumerate(TRACES)]
    pools += [(4, synthetic_levels(g, A), A) for A in (3, 8)]
    for s, lvls, A in pools:
        pool = levels.LevelPool(lvls, counts_fn=util.oracle_counts, n_agents=A)
        sched = schedule.LevelSchedule(pool, [(0, len(lvls))], mode="uniform", seed=0)
        sel = (g["req_source"] == s) & (g["req_agents"] == A)
        assert sel.sum() == len(lvls) and sched.n_agents == A
        assert sched.available.shape == (len(lvls), A) == pool.pool_agent_required_step.shape
        assert sched.available.dtype == np.int32
        assert np.array_equal(sched.available, g["req_available"][sel][:, :A])
        assert np.array_equal(sched.min_performance, g["req_min_performance"][sel])
        assert np.array_equal(sched.reward_possible(1), sched.available + 1) and sched.reward_possible(3).dtype == np.int32
        for l, lv in enumerate(lvls):
            assert np.array_equal(pool.pool_agent_required_reset[l],
                                  smr.required_points_multi(lv.min_performance, 1.0, sched.available[l]))
        j = g["req_fraction"].tolist().index(1.0)
        assert np.array_equal(pool.pool_agent_required_step, g["req_points"][sel][:, j, :A])
    # one agent: the shapes a single-agent pool always had
    one = levels.LevelPool(synthetic_levels(g, 1), counts_fn=util.oracle_counts)
    s1 = schedule.LevelSchedule(one, [(0, 1)], mode="uniform", seed=0)
    assert s1.n_agents == 1 and s1.available.shape == (1,)
    assert np.array_equal(s1.available, g["req_available"][(g["req_source"] == 4) & (g["req_agents"] == 1)][:, 0])


def test_performances_equal_the_reference_bit_for_bit(golden):
    """np.average(reward / reward_possible) of every golden episode, A = 8 included -- where numpy's eight-accumulator tree
    and a plain running sum differ on some episodes, so the comparison tells them apart."""
    g = golden
    tree_matters = 0
    for i in range(len(g["cur_agents"])):
        A = int(g["cur_agents"][i])
        for e in range(g["cur_offsets"][i], g["cur_offsets"][i + 1]):
            got = smr.performance_multi(g["cur_reward"][e, :A], g["cur_possible"][e, :A])
            assert np.float64(got).view(np.int64) == g["cur_perf"][e].view(np.int64), (i, e, got, g["cur_perf"][e])
            if A == 8:
                with np.errstate(all="ignore"):
                    q = g["cur_reward"][e].astype(np.float64) / g["cur_possible"][e]
                s = 0.0
                for v in q.tolist():
                    s = s + v
                tree_matters += int(np.isfinite(s) and s / 8.0 != got)
    assert tree_matters > 0
    # the model's identity: an all -0.0 row averages to +0.0, as numpy's reduction does
    assert np.signbit(np.average(np.array([-0.0, -0.0]))) == np.signbit(smr.add_reduce([-0.0, -0.0])) == False  # noqa: E712
    assert smr.performance_multi([3.0, 1.0], [0, 5]) == 0.0 and smr.performance_multi([0.0, 1.0], [0, 5]) == 0.0


def test_golden_inputs_are_what_the_issue_asks_for(golden):
    g = golden
    cases = set(zip(g["cur_agents"].tolist(), g["cur_groups"].tolist(), g["cur_lookback"].tolist()))
    assert {c[0] for c in cases} == {2, 3, 8} and {c[1] for c in cases} == {2, 3} and {c[2] for c in cases} == {5, 100}
    assert len(cases) == 6 and all((A, lb) in {(c[0], c[2]) for c in cases} for A in (2, 3, 8) for lb in (5, 100))
    for i in range(len(g["cur_agents"])):
        A = int(g["cur_agents"][i])
        lo, hi = g["cur_offsets"][i], g["cur_offsets"][i + 1]
        r, p = g["cur_reward"][lo:hi, :A], g["cur_possible"][lo:hi, :A]
        assert 100 <= hi - lo and ((p == 0) & (r == 0)).any() and ((p == 0) & (r != 0)).any()     # NaN and inf averages
        assert (r < 0).any() and ((r == 0).sum(axis=1) == 1).any()


def feed_golden(g, i):
    """Case i of the golden curricula through the model, one episode per harvest: yields (episode, model)."""
    A, G, n = int(g["cur_agents"][i]), int(g["cur_groups"][i]), int(g["cur_lookback"][i])
    groups = [(3 * k, 3) for k in range(G)]
    m = smr.ScheduleModelMulti(groups, n, np.ones((3 * G, A), np.int32), np.zeros(1, np.int32))
    for e in range(g["cur_offsets"][i], g["cur_offsets"][i + 1]):
        slot = 3 * int(g["cur_group"][e]) + e % 3
        m.cur_slot[0] = slot
        m.reward_possible[slot] = g["cur_possible"][e, :A]
        m.harvest(np.ones((1, A), np.uint8), g["cur_reward"][e:e + 1, :A], np.zeros(1, np.int32))
        yield e, m


def test_curriculum_probabilities_within_the_measured_bound(golden):
    """The restatement against CurricularLevelIterator.get_next_parameters on every golden episode.  Measured here, on the
    CPU: the largest absolute difference is 1.6542323066914832e-14 (CURRICULUM_MULTI_MEASURED); the bound is twice that.  best_perf_lvl* is exact; recent*_perf_lvl* is numpy's
    pairwise mean there and a sequential one here: a few ulps."""
    g = golden
    worst, n = 0.0, 0
    for i in range(len(g["cur_agents"])):
        G, case = int(g["cur_groups"][i]), 0.0
        for e, m in feed_golden(g, i):
            case = max(case, np.abs(m.curriculum() - g["cur_probs"][e, :G]).max())
            n += 1
            assert np.array_equal(m.best, g["cur_best"][e, :G]), e
            assert np.abs(m.mean - g["cur_recent"][e, :G])[m.episodes > 0].max() < 1e-15 * 8, e
        assert (m.count > m.lookback).all()             # every ring filled and wrapped
        print("case %d: largest |restatement - reference| %r" % (i, case))
        worst = max(worst, case)
    print("largest |restatement - reference| over %d episodes: %r" % (n, worst))
    assert n == len(g["cur_group"]) == 1720
    assert worst <= CURRICULUM_MULTI_BOUND, worst


def test_harvest_model_files_one_record_per_episode():
    """Agents that finish on different steps: nothing is filed until the last one is done, then one record -- the average
    -- and cur_slot follows level_idx on every step."""
    m = smr.ScheduleModelMulti([(0, 2), (2, 2)], 4, [[10, 20], [10, 20], [5, 5], [1, 1]], [1, 3, 2])
    done = np.array([[1, 0], [0, 0], [0, 1]], np.uint8)
    ep = np.array([[5.0, np.nan], [np.nan, np.nan], [np.nan, 2.0]], np.float32)       # (unfinished agents are not read)
    m.harvest(done, ep, [1, 3, 2])
    assert m.episodes.tolist() == [0, 0] and m.count.tolist() == [1, 1] and m.cur_slot.tolist() == [1, 3, 2]
    done[0, 1], ep[0, 1] = 1, 10.0
    done[2, 0], ep[2, 0] = 1, 1.0
    m.harvest(done, ep, [0, 3, 3])
    assert m.episodes.tolist() == [1, 1] and m.cur_slot.tolist() == [0, 3, 3]
    assert m.ring[0, 1] == (5.0 / 10 + 10.0 / 20) / 2 and m.ring[1, 1] == (1.0 / 5 + 2.0 / 5) / 2
    assert m.best.tolist() == [0.5, m.ring[1, 1]]


# ------------------------------------------------------------------------------------------------------- LevelSchedule

@pytest.fixture(scope="module")
def pool2():
    lvls = []
    for name in TRACES[:3]:
        lvls += util.levels_from_trace(util.load_trace(name))
    return levels.LevelPool(lvls, counts_fn=util.oracle_counts, n_agents=2)


def test_level_schedule_argument_checks_for_multi_agent_pools(pool2):
    LS = schedule.LevelSchedule
    L = len(pool2)
    ok = dict(mode="uniform", seed=1)
    s = LS(pool2, [(0, 3), (3, L - 3)], **ok)
    assert s.n_agents == 2 and s.available.shape == (L, 2)
    LS(pool2, [range(0, 3), range(4, L)], mode="curriculum", seed=1, lookback=5)
    LS(pool2, [(0, 3), (3, 3)], mode="switching", seed=1, p_switch=0.5, min_performance_fraction=0.25)
    for groups in ([], [(0, 0)], [(-1, 3)], [(0, L + 1)], [(0, 4), (3, 3)], [range(0, 6, 2)]):
        with pytest.raises(ValueError):
            LS(pool2, groups, **ok)
    for kw in (dict(mode="cycle", seed=1), dict(mode="switching", seed=1), dict(mode="uniform", seed=1, p_switch=0.5),
               dict(mode="uniform", seed=1, lookback=1), dict(mode="uniform", seed=1, lookback=1025)):
        with pytest.raises(ValueError):
            LS(pool2, [(0, 3), (3, 3)], **kw)
    with pytest.raises(ValueError, match="not attached"):
        s.stats()
    # first_levels is the draw's model by global env index, whatever the agent count
    want = sr.draw_many(s.groups, [0.5, 0.5], 1, np.uint64(schedule.FIRST_LEVELS_COUNTER), np.arange(40))[1]
    assert np.array_equal(s.first_levels(40), want) and np.array_equal(s.first_levels(10, env_offset=30), want[30:])


def test_the_wrong_env_class_is_refused(pool2, golden):
    """Both refusals come before anything is allocated on a device."""
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    from safelife_amd.vector_env import SafeLifeVectorEnv
    multi = schedule.LevelSchedule(pool2, [(0, len(pool2))], mode="uniform", seed=1)
    with pytest.raises(ValueError, match="SafeLifeMultiAgentVectorEnv"):
        SafeLifeVectorEnv(pool2, 4, level_schedule=multi)
    one = levels.LevelPool(synthetic_levels(golden, 1), counts_fn=util.oracle_counts)
    single = schedule.LevelSchedule(one, [(0, 1)], mode="uniform", seed=1)
    with pytest.raises(ValueError, match="1 agent per level"):
        SafeLifeMultiAgentVectorEnv(pool2, 4, level_schedule=single)
    three = levels.LevelPool(synthetic_levels(golden, 3), counts_fn=util.oracle_counts, n_agents=3)
    with pytest.raises(ValueError, match="3 agents per level"):
        SafeLifeMultiAgentVectorEnv(pool2, 4, level_schedule=schedule.LevelSchedule(three, [(0, 2)], mode="uniform", seed=1))
    other = levels.LevelPool(pool2.levels, counts_fn=util.oracle_counts, n_agents=2)
    with pytest.raises(ValueError, match="another pool"):
        SafeLifeMultiAgentVectorEnv(other, 4, level_schedule=multi)
    assert multi.env is None and single.env is None        # nothing was attached
