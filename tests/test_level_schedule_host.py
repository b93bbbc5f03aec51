"""
Level schedules without a GPU: the ABI of the four slhip_schedule_* entry points, the host restatement
(tests/schedule_ref.py) against what the reference computes (tests/golden/schedule_cases.npz, written by
tests/golden/make_golden_schedule.py), the draw's model, and the argument checks of safelife_amd.schedule.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from safelife_amd import _hip, levels, schedule
from tests import schedule_ref as sr
from tests import util

#: The largest |restatement - reference| over EVERY curriculum probability of the golden cases (2600 episodes, 2 and 3
#: groups, lookback 100 and 5), measured on the CPU: 3.430589146091734e-14.  It is the reference's polyfit (a scaled
#: Vandermonde least-squares solve) against the closed-form slope, amplified by the division by the smallest |progress|.
CURRICULUM_MEASURED = 3.430589146091734e-14
#: The bound of the tests: the measured value times 2.  The only operation of the restatement that is not exactly
#: specified is exp(); another libm's -- or the device's -- exp may differ from this one's by an ulp or two per term,
#: which moves a probability by at most a few 1e-16: a factor 2 on 3.4e-14 leaves that room many times over and no more.
CURRICULUM_BOUND = 2 * CURRICULUM_MEASURED


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "schedule_cases.npz")) as d:
        return {k: d[k] for k in d.files}


# ------------------------------------------------------------------------------------------------------------- the ABI

NAMES = ("slhip_schedule_draw", "slhip_schedule_required", "slhip_schedule_harvest", "slhip_schedule_curriculum")


def test_symbols_and_version():
    lib = _hip.lib()
    for name in NAMES:
        assert name in _hip.EXPORTS and hasattr(lib, name)
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13


def test_schedule_layout_matches_header(tmp_path):
    """ctypes mirror of struct sl_level_schedule against gcc's offsetof / sizeof, and the constants."""
    st = _hip.LevelSchedule
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "safelife_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(sl_level_schedule));',
             'printf("consts %d %d %d\\n", SL_SCHEDULE_MAX_GROUPS, SL_SCHEDULE_MAX_LOOKBACK, SL_SCHEDULE_BAD_PROBS);',
             'printf("others %zu %zu %zu\\n", sizeof(sl_env_scalars), sizeof(sl_level_scalars), sizeof(sl_step_out));']
    want = ["size %d" % C.sizeof(st), "consts %d %d %d" % (_hip.SCHEDULE_MAX_GROUPS, _hip.SCHEDULE_MAX_LOOKBACK,
                                                           _hip.SCHEDULE_BAD_PROBS), "others 64 32 16"]
    for name, ctype in st._fields_:
        lines.append('printf("%s %%zu %%zu\\n", offsetof(sl_level_schedule, %s), sizeof(((sl_level_schedule *)0)->%s));'
                     % (name, name, name))
        want.append("%s %d %d" % (name, getattr(st, name).offset, C.sizeof(ctype)))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(util.REPO, "include"), str(src), "-o", exe])
    got = [g for g in subprocess.check_output([exe]).decode().split("\n") if g]
    assert got == want
    assert C.sizeof(st) == 168


def _sched(**kw):
    """A description whose pointers are non-null but never dereferenced: every call below is refused first."""
    s = _hip.LevelSchedule()
    s.G, s.lookback, s.L = 2, 100, 64
    s.start[0], s.len[0], s.start[1], s.len[1] = 0, 10, 10, 54
    for name, ctype in _hip.LevelSchedule._fields_:
        if ctype is C.c_void_p:
            setattr(s, name, 0x1000)
    for k, v in kw.items():
        if k in ("start", "len"):
            for i, x in enumerate(v):
                getattr(s, k)[i] = x
        else:
            setattr(s, k, v)
    return s


BAD_SHAPES = [dict(G=0), dict(G=9), dict(lookback=1), dict(lookback=1025), dict(L=0), dict(len=(0, 54)), dict(start=(-1, 10)),
              dict(start=(0, 9)), dict(len=(10, 55)), dict(start=(20, 10), len=(10, 30))]


@pytest.mark.parametrize("bad", BAD_SHAPES, ids=[str(b) for b in BAD_SHAPES])
def test_bad_descriptions_are_refused_before_any_launch(bad):
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    s = _sched(**bad)
    probs = (C.c_double * 2)(0.5, 0.5)
    assert lib.slhip_schedule_draw(C.byref(s), probs, None, 1, 0, p, s.L, None) == _hip.SL_E_SHAPE
    assert b"schedule" in lib.slhip_last_error()
    assert lib.slhip_schedule_harvest(C.byref(s), p, p, 8, None) == _hip.SL_E_SHAPE
    assert lib.slhip_schedule_curriculum(C.byref(s), p, None) == _hip.SL_E_SHAPE
    with pytest.raises(ValueError):
        _hip.check(_hip.SL_E_SHAPE)


def test_entry_point_argument_errors():
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    s = _sched()
    ok = (C.c_double * 2)(0.5, 0.5)
    for bad in ((-0.1, 1.1), (float("nan"), 1.0), (float("inf"), 1.0), (0.0, 0.0), (1e308, 1e308)):
        assert lib.slhip_schedule_draw(C.byref(s), (C.c_double * 2)(*bad), None, 1, 0, p, 64, None) == _hip.SL_E_SHAPE, bad
        assert b"probabilit" in lib.slhip_last_error()
    assert lib.slhip_schedule_draw(C.byref(s), ok, None, 1, 0, p, 63, None) == _hip.SL_E_SHAPE      # not the schedule's L
    assert lib.slhip_schedule_draw(C.byref(s), ok, None, 1, 0, None, 64, None) == _hip.SL_E_ARG
    assert lib.slhip_schedule_draw(C.byref(s), None, None, 1, 0, p, 64, None) == _hip.SL_E_ARG     # no probabilities at all
    assert lib.slhip_schedule_draw(None, ok, None, 1, 0, p, 64, None) == _hip.SL_E_ARG
    assert lib.slhip_schedule_draw(C.byref(_sched(status=None)), ok, None, 1, 0, p, 64, None) == _hip.SL_E_ARG
    for f in (float("nan"), float("inf")):
        assert lib.slhip_schedule_required(C.byref(s), f, p, 64, None) == _hip.SL_E_SHAPE
    assert lib.slhip_schedule_required(C.byref(s), 0.5, p, 65, None) == _hip.SL_E_SHAPE
    assert lib.slhip_schedule_required(C.byref(s), 0.5, None, 64, None) == _hip.SL_E_ARG
    for name in ("min_performance", "available"):
        assert lib.slhip_schedule_required(C.byref(_sched(**{name: None})), 0.5, p, 64, None) == _hip.SL_E_ARG
    assert lib.slhip_schedule_harvest(C.byref(s), p, p, 0, None) == _hip.SL_E_SHAPE
    assert lib.slhip_schedule_harvest(C.byref(s), None, p, 8, None) == _hip.SL_E_ARG
    assert lib.slhip_schedule_harvest(C.byref(s), p, None, 8, None) == _hip.SL_E_ARG
    for name in ("reward_possible", "cur_slot", "ring", "count", "episodes", "pos", "best", "mean"):
        assert lib.slhip_schedule_harvest(C.byref(_sched(**{name: None})), p, p, 8, None) == _hip.SL_E_ARG, name
    assert lib.slhip_schedule_curriculum(C.byref(s), None, None) == _hip.SL_E_ARG
    assert lib.slhip_schedule_curriculum(C.byref(_sched(ring=None)), p, None) == _hip.SL_E_ARG


# ------------------------------------------------------------------------------------- the restatement against the reference

def test_linear_schedule_equals_the_reference(golden):
    g = golden
    n = 0
    for i in range(len(g["lin_knots"]) - 1):
        t = g["lin_t"][g["lin_knots"][i]:g["lin_knots"][i + 1]]
        y = g["lin_y"][g["lin_knots"][i]:g["lin_knots"][i + 1]]
        mine = schedule.LinearSchedule(t, y)
        for j in range(g["lin_offsets"][i], g["lin_offsets"][i + 1]):
            x, want = g["lin_x"][j], g["lin_value"][j]
            assert sr.linear_schedule(t, y, x) == want, (i, x)
            assert mine(x) == want, (i, x)
            n += 1
        assert mine(t[0] - 5) == y[0] and mine(t[-1] + 5) == y[-1] and mine(t[0]) == y[0] and mine(t[-1]) == y[-1]
    assert n == len(g["lin_x"]) > 100


def test_linear_schedule_argument_errors():
    for t, y in (([1.0], [1.0]), ([0, 1], [1]), ([0, 0], [1, 2]), ([1, 0], [1, 2])):
        with pytest.raises(ValueError):
            schedule.LinearSchedule(t, y)


def test_required_points_equal_the_reference(golden):
    g = golden
    assert g["req_points"].shape == (len(g["req_level"]), len(g["req_fraction"])) and len(g["req_level"]) >= 100
    for k in range(len(g["req_level"])):
        mp, avail = g["req_min_performance"][k], int(g["req_available"][k])
        for j, f in enumerate(g["req_fraction"]):
            assert sr.required_points(mp, f, avail) == g["req_points"][k, j], (k, f)
            assert levels.required_points(np.float64(mp) * f, avail) == g["req_points"][k, j], (k, f)
    # the schedule's own per-slot inputs are the reference's
    for p, name in enumerate(("prune_still_25", "append_spawn_25")):
        pool, _ = util.pool_from_fixture(name, util.oracle_counts)
        s = schedule.LevelSchedule(pool, [(0, len(pool))], mode="uniform", seed=0)
        sel = g["req_pool"] == p
        assert np.array_equal(s.available, g["req_available"][sel])
        assert np.array_equal(s.min_performance, g["req_min_performance"][sel])


def _feed_golden(g, i):
    """Case i of the golden curricula through the model, one episode per harvest: yields (episode, model)."""
    G, n = int(g["cur_groups"][i]), int(g["cur_lookback"][i])
    groups = [(3 * k, 3) for k in range(G)]
    m = sr.ScheduleModel(groups, n, np.zeros(3 * G, np.int32), np.zeros(1, np.int32))
    for e in range(g["cur_offsets"][i], g["cur_offsets"][i + 1]):
        slot = 3 * int(g["cur_group"][e]) + e % 3
        m.cur_slot[0] = slot
        m.reward_possible[slot] = g["cur_possible"][e]
        m.harvest(np.ones(1, np.uint8), g["cur_reward"][e:e + 1], np.zeros(1, np.int32))
        yield e, m


def test_curriculum_probabilities_within_the_measured_bound(golden):
    """The restatement against CurricularLevelIterator.get_next_parameters on every golden episode -- none is left out.
    Measured here, on the CPU: the largest absolute difference is 3.430589146091734e-14 (CURRICULUM_MEASURED; per case
    4.8e-15, 1.2e-14, 9.4e-15, 3.4e-14); the bound is twice that (CURRICULUM_BOUND says why).  best_perf_lvl* is exact;
    recent*_perf_lvl* is numpy's pairwise mean there and a sequential one here: a few ulps."""
    g = golden
    worst, n = 0.0, 0
    for i in range(len(g["cur_groups"])):
        G = int(g["cur_groups"][i])
        for e, m in _feed_golden(g, i):
            d = np.abs(m.curriculum() - g["cur_probs"][e, :G]).max()
            worst = max(worst, d)
            n += 1
            assert np.array_equal(m.best, g["cur_best"][e, :G]), e
            assert np.abs(m.mean - g["cur_recent"][e, :G])[m.episodes > 0].max() < 1e-15 * 8, e
        assert (m.count > 2 * m.lookback).all()         # every ring wrapped more than twice
    print("largest |restatement - reference| over %d episodes: %r" % (n, worst))
    assert n == len(g["cur_group"]) == 2600
    assert worst <= CURRICULUM_BOUND, worst


def test_golden_inputs_are_what_the_issue_asks_for(golden):
    g = golden
    assert sorted(set(g["cur_groups"].tolist())) == [2, 3] and sorted(set(g["cur_lookback"].tolist())) == [5, 100]
    ratio_zero = g["cur_possible"] == 0
    assert (ratio_zero & (g["cur_reward"] == 0)).any() and (ratio_zero & (g["cur_reward"] != 0)).any()   # NaN and inf
    assert (g["cur_reward"] < 0).any()


def test_curriculum_degenerate_inputs():
    """All records equal: the closed form's slope is exactly 0 (the reference's polyfit returns rounding noise there, which
    its division by `scale` blows up -- a degenerate input, kept out of the comparison).  Every progress <= 0 becomes 0;
    a scale of 0 turns every entry into NaN or inf -> 0 and the probabilities are equal."""
    assert sr.slope([0.25] * 100) == 0.0 and sr.slope([0.0] * 5) == 0.0
    assert sr.softmax_of_progress([0.0, 0.0, 0.0]) == [1 / 3, 1 / 3, 1 / 3]
    assert sr.softmax_of_progress([0.0, 0.3]) == [0.5, 0.5]
    assert sr.softmax_of_progress([float("nan"), 0.3]) == [0.5, 0.5]
    p = sr.softmax_of_progress([-0.5, 0.25])            # scale 0.25: (0, 1) -> softmax
    assert p[0] == np.exp(-1.0) / (np.exp(-1.0) + 1.0) and abs(sum(p) - 1) < 1e-15
    assert sr.slope([0.0, 1.0, 2.0, 3.0]) == 1.0 and sr.slope([3.0, 1.0]) == -2.0


# --------------------------------------------------------------------------------------------------------- the draw's model

GROUPS3 = [(2, 5), (9, 1), (16, 10)]


def test_draw_models_agree():
    """draw_one (Python ints), draw_many (wrapping uint64) and the package's own model (first_levels) are one function."""
    for seed, counter in ((0, 0), (2 ** 64 - 1, 2 ** 64 - 1), (12345, 7), (2 ** 63, 2 ** 64 - 1)):
        for groups, probs in ((GROUPS3, [0.2, 0.3, 0.5]), (GROUPS3, [0.0, 1.0, 0.0]), ([(0, 1)], [3.0]),
                              ([(k, 1) for k in range(8)], [1, 2, 3, 4, 0, 6, 7, 8])):
            one = np.array([sr.draw_one(groups, probs, seed, counter, s) for s in range(70)])
            g, slot = sr.draw_many(groups, probs, seed, np.uint64(counter), np.arange(70))
            assert np.array_equal(one[:, 0], g) and np.array_equal(one[:, 1], slot)
            assert np.array_equal(schedule.draw_model(groups, probs, seed, counter, np.arange(70)), slot)
            assert np.array_equal(sr.draw(groups, probs, seed, counter, 70), slot)


def test_draw_stays_in_its_groups_and_never_draws_probability_zero():
    idx = np.arange(20000)
    g, slot = sr.draw_many(GROUPS3, [0.5, 0.0, 0.5], 9, np.uint64(3), idx)
    assert set(g.tolist()) == {0, 2}
    for k, (a, n) in enumerate(GROUPS3):
        assert ((slot[g == k] >= a) & (slot[g == k] < a + n)).all()
    assert set(slot[g == 0].tolist()) == set(range(2, 7)) and set(slot[g == 2].tolist()) == set(range(16, 26))
    # p = 0 and p = 1 are exact: [1 - p, p] of a switching schedule
    for p, only in ((0.0, 0), (1.0, 1)):
        g, slot = sr.draw_many([(0, 4), (4, 4)], [1.0 - p, p], 9, np.arange(64, dtype=np.uint64)[:, None], idx[None, :1000])
        assert (g == only).all() and (slot // 4 == only).all()
    # rounding can leave no group with cum > t only at the top end; the rule then takes the last POSITIVE group
    assert sr.draw_one([(0, 1), (1, 1), (2, 1)], [0.3, 0.7, 0.0], 1, 1, 5)[0] in (0, 1)


def _chi2_two_sided(counts, expected):
    from scipy.stats import chi2
    counts, expected = np.asarray(counts, np.float64).ravel(), np.asarray(expected, np.float64).ravel()
    assert expected.min() >= 5
    stat = ((counts - expected) ** 2 / expected).sum()
    return min(chi2.sf(stat, counts.size - 1), chi2.cdf(stat, counts.size - 1))


def test_draw_frequencies_and_independence():
    """Pearson's chi-square at fixed seeds (so the outcome is fixed), the smaller tail probability of each: the group
    frequencies against the probabilities, the member frequencies against uniform (the member draw's bias is at most
    len / 2^64: stated, not tested), and -- the sense the action draw's tests use -- the joint bins of the draws of
    (counter, slot) and (counter + 1, slot), and of (counter, slot) and (counter, slot + 1).  Threshold: a correct
    generator gives a two-sided tail below q with probability 2q, so with the seven statistics here q = 1e-6 fails a
    correct one about once in 70000 choices of seed, while a wrong frequency of a few percent at these counts (65536 to
    a million draws) pushes the tail below 1e-20."""
    seed = 20261019
    probs = [0.1, 0.25, 0.05, 0.6]
    groups = [(0, 4), (4, 3), (7, 1), (8, 8)]
    c, s = np.arange(256, dtype=np.uint64)[:, None], np.arange(1024)[None, :]
    g, slot = sr.draw_many(groups, probs, seed, c, s)
    n = g.size
    ps = {"groups": _chi2_two_sided(np.bincount(g.ravel(), minlength=4), n * np.array(probs))}
    for k, (a, m) in enumerate(groups):
        if m > 1:
            cnt = np.bincount(slot[g == k] - a, minlength=m)
            ps["members_%d" % k] = _chi2_two_sided(cnt, np.full(m, cnt.sum() / m))
    uni = [(0, 16)]
    a = sr.draw_many(uni, [1.0], seed, c, s)[1]
    for name, b in (("counter_pairs", sr.draw_many(uni, [1.0], seed, c + np.uint64(1), s)[1]),
                    ("slot_pairs", sr.draw_many(uni, [1.0], seed, c, s + 1)[1])):
        joint = np.bincount((a * 16 + b).ravel(), minlength=256)
        ps[name] = _chi2_two_sided(joint, np.full(256, a.size / 256))
    # the group draws of consecutive counters as well (word 1), two groups of equal probability
    two = [(0, 1), (1, 1)]
    ga = sr.draw_many(two, [0.5, 0.5], seed, c, s)[0]
    gb = sr.draw_many(two, [0.5, 0.5], seed, c + np.uint64(1), s)[0]
    ps["group_counter_pairs"] = _chi2_two_sided(np.bincount((ga * 2 + gb).ravel(), minlength=4), np.full(4, ga.size / 4))
    print(ps)
    assert len(ps) == 7 and min(ps.values()) > 1e-6, ps


def test_device_probabilities_fall_back_to_uniform():
    assert sr.device_probs([0.2, 0.8]) == ([0.2, 0.8], 0)
    for bad in ([0.0, 0.0], [float("nan"), 1.0], [float("inf"), 1.0], [-0.1, 1.1], [1e308, 1e308]):
        assert sr.device_probs(bad) == ([1.0, 1.0], sr.BAD_PROBS)


# ------------------------------------------------------------------------------------------------------- LevelSchedule

@pytest.fixture(scope="module")
def pool():
    return util.pool_from_fixture("prune_still_25", util.oracle_counts, n=12)[0]


def test_level_schedule_argument_errors(pool):
    LS = schedule.LevelSchedule
    ok = dict(mode="uniform", seed=1)
    LS(pool, [(0, 6), (6, 6)], **ok)
    LS(pool, [range(0, 6), range(8, 12)], **ok)
    for groups in ([], [(0, 0)], [(-1, 3)], [(0, 13)], [(0, 6), (5, 3)], [(k, 1) for k in range(9)], [range(0, 6, 2)]):
        with pytest.raises(ValueError):
            LS(pool, groups, **ok)
    with pytest.raises(TypeError):
        LS(None, [(0, 6)], **ok)
    for kw in (dict(mode="cycle", seed=1), dict(mode="switching", seed=1), dict(mode="uniform", seed=1, p_switch=0.5),
               dict(mode="uniform", seed=1, curriculum="uniform"), dict(mode="curriculum", seed=1, curriculum="greedy"),
               dict(mode="uniform", seed=1, lookback=1), dict(mode="uniform", seed=1, lookback=1025)):
        with pytest.raises(ValueError):
            LS(pool, [(0, 6), (6, 6)], **kw)
    with pytest.raises(ValueError, match="two groups"):
        LS(pool, [(0, 4), (4, 4), (8, 4)], mode="switching", seed=1, p_switch=0.5)
    s = LS(pool, [(0, 6), (6, 6)], mode="switching", seed=1, p_switch=lambda t: 2.0)
    with pytest.raises(ValueError, match="p_switch"):
        s.group_probs()
    s = LS(pool, [(0, 6)], mode="uniform", seed=1, min_performance_fraction=lambda t: float("nan"))
    with pytest.raises(ValueError, match="finite"):
        s.fraction()
    with pytest.raises(ValueError, match="not attached"):
        s.stats()


def test_refreshable_and_multi_agent_pools_are_refused():
    refreshable = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=4, refreshable=True)[0]
    with pytest.raises(ValueError, match="pool_next"):
        schedule.LevelSchedule(refreshable, [(0, 4)], mode="uniform", seed=1)


def test_schedules_follow_the_training_step(pool):
    p = schedule.LinearSchedule([100, 200], [0.1, 1.0])
    s = schedule.LevelSchedule(pool, [(0, 6), (6, 6)], mode="switching", seed=3, p_switch=p,
                               min_performance_fraction=schedule.LinearSchedule([0, 1000], [0.001, 1.0]))
    assert s.group_probs().tolist() == [0.9, 0.1] and s.fraction() == 0.001
    s.training_steps = 150
    assert s.group_probs().tolist() == [1.0 - p(150), p(150)] and s.fraction() == sr.linear_schedule([0, 1000], [0.001, 1.0], 150)
    s.training_steps = 10 ** 9
    assert s.group_probs().tolist() == [0.0, 1.0] and s.fraction() == 1.0
    u = schedule.LevelSchedule(pool, [(0, 4), (4, 4), (8, 4)], mode="curriculum", seed=3, curriculum="uniform")
    assert u.group_probs().tolist() == [1 / 3] * 3 and u.fraction() is None
    assert schedule.LevelSchedule(pool, [(0, 4), (4, 8)], mode="curriculum", seed=3).group_probs() is None


def test_first_levels_are_the_model_by_global_env_index(pool):
    groups = [(0, 6), (6, 6)]
    s = schedule.LevelSchedule(pool, groups, mode="switching", seed=77, p_switch=schedule.LinearSchedule([1e5, 1.5e6], [0.1, 1.0]))
    first = s.first_levels(2000)
    want = sr.draw_many(groups, [0.9, 0.1], 77, np.uint64(schedule.FIRST_LEVELS_COUNTER), np.arange(2000))[1]
    assert np.array_equal(first, want) and first.dtype == np.int32
    assert abs((first >= 6).mean() - 0.1) < 4.9 * (0.1 * 0.9 / 2000) ** 0.5          # not spread evenly over both families
    assert np.array_equal(s.first_levels(500, env_offset=1500), first[1500:])        # shards: the global index counts
    c = schedule.LevelSchedule(pool, groups, mode="curriculum", seed=77)
    assert np.array_equal(c.first_levels(64), sr.draw_many(groups, [0.5, 0.5], 77, np.uint64(2 ** 64 - 1), np.arange(64))[1])


def test_from_pools_remembers_the_ranges():
    a = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=5)[0].levels
    b = util.pool_from_fixture("append_spawn_25", util.oracle_counts, n=7)[0].levels
    s = schedule.LevelSchedule.from_pools([a, b], pool_args=dict(counts_fn=util.oracle_counts), mode="switching", seed=1,
                                          p_switch=0.25)
    assert s.groups == ((0, 5), (5, 7)) and len(s.pool) == 12 and s.pool.has_spawner
    assert np.array_equal(s.pool.pool_board[5:], np.stack([lv.board for lv in b]))
