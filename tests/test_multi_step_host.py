"""The multi-agent step from 1 to 8 agents, on the CPU: the fixture tests/golden/multi_step_cases.npz (the reference's
SafeLifeEnv(single_agent=False) on scripted agent clashes, dense random boards and block-size edges) holds the events it is
there for; the plain restatement of the serial action loop reproduces the reference's boards and can tell six wrong
readings apart; the oracle equals the reference on every case and array, and its one-agent multi env equals its
single-agent env.  (The device's half is tests/test_multi_step_gpu.py.)"""
import os

import numpy as np
import pytest

import oracle
from tests import multi_step_cases as msc
from tests import util

SCRIPTED, DENSE, EDGE = msc.names("scripted"), msc.names("dense"), msc.names("edge")

# the scripted case each wrong reading of the action loop must fail on (it may fail on more)
CAUGHT_BY = {
    "reverse_order": "scripted/same_cell/plain/fwd",
    "stale_board": "scripted/follow_leader/plain/rev",
    "kill_keeps_agent": "scripted/kill/plain/fwd",
    "kill_keeps_destructible": "scripted/mutual_toggle/plain/fwd",
    "exit_into_agent": "scripted/leaver_at_leaver/plain/fwd",
    "dead_agent_acts": "scripted/done_agents_act/plain/fwd",
    "crate_over_agent": "scripted/crate_into_agent/plain/fwd",
}


def test_fixture_size_and_cases():
    assert os.path.getsize(msc.FIXTURE) < 1000 * 1000
    base = sorted(set(n.split("/")[1] for n in SCRIPTED))
    assert len(base) == 23 and len(SCRIPTED) == 6 * len(base)          # 3 placements x 2 index orders each
    agents = {b: msc.agents_of(msc.case("scripted/%s/plain/fwd" % b)) for b in base}
    assert sum(a == 3 for a in agents.values()) >= 2 and sum(a == 8 for a in agents.values()) >= 2
    for n in SCRIPTED:
        tr = msc.case(n)
        assert max(tr["level0_board"].shape) <= 8 and 2 <= len(tr["trace_reward"]) <= 6, n
    assert [n.split("/")[1] for n in DENSE] == ["1x4x4", "2x3x4", "3x5x5", "5x4x5", "8x6x7"]
    assert [n.split("/")[1] for n in EDGE] == ["8x16x16", "8x16x17", "8x32x32", "8x25x41", "3x32x33"]
    for n in EDGE:
        tr = msc.case(n)
        assert len(tr["trace_reward"]) == 40 and int(tr["env_time_limit"]) == 10
        for lv in msc.levels_of(tr):            # one spawner, the agents within one 4 x 4 patch of the torus
            assert int(((lv.board & 0x80) != 0).sum()) == 1
            H, W = lv.shape
            assert any(all((y - y0) % H < 4 and (x - x0) % W < 4 for y, x in lv.agent_locs)
                       for y0 in range(H) for x0 in range(W))


@pytest.mark.parametrize("name", DENSE + EDGE)
def test_random_cases_hold_kills_exits_and_time_limits(name):
    tr = msc.case(name)
    kills, exits, ends, idle = msc.event_counts(tr)
    if msc.agents_of(tr) > 1:
        assert kills > 0 and exits > 0 and ends > 0 and idle > 0, (kills, exits, ends, idle)
    else:
        assert exits > 0 and ends > 0


def _scripted(base, order="fwd", placement="plain"):
    return msc.case("scripted/%s/%s/%s" % (base, placement, order))


def test_scripted_cases_show_their_events():
    """The events, asserted again on the file for the cases recorded as drawn (the generator asserts them for every
    placement): who is killed, who leaves, who stays, in either index order."""
    def kills(tr):
        return tr["trace_done"] & ~tr["trace_success"] & ~tr["trace_times_up"][:, None] & msc.active_before(tr)
    for order, ix in (("fwd", lambda a, A: a), ("rev", lambda a, A: A - 1 - a)):
        fwd = order == "fwd"
        tr = _scripted("head_on", order)
        assert all(np.array_equal(l, tr["trace_pre_locs"][0]) for l in tr["trace_act_locs"])
        tr = _scripted("follow_leader", order)
        assert (tr["trace_act_locs"][0][ix(0, 2)][1] != tr["trace_pre_locs"][0][ix(0, 2)][1]) == (not fwd)
        tr = _scripted("same_cell", order)
        assert tuple(tr["trace_act_locs"][0][0]) == (2, 2)
        assert np.array_equal(tr["trace_act_locs"][0][1], tr["trace_pre_locs"][0][1])
        tr = _scripted("create_destroy", order)
        assert tr["trace_act_board"][0][2, 2] == 0 and tr["trace_act_board"][1][2, 2] & 1
        tr = _scripted("kill", order)
        assert kills(tr)[0, ix(1, 2)] and kills(tr).sum() == 1 and (tr["trace_act_board"][0][3, 2] != 0) == (not fwd)
        assert not tr["trace_act_board"][0][2, 2] & (msc.AGENT | msc.DESTRUCTIBLE)
        tr = _scripted("kill_then_exit", order)
        assert kills(tr)[0, ix(1, 2)] and tr["trace_success"][1, ix(0, 2)] and tr["trace_done"][1].all()
        assert list(tr["trace_reset_at"]) == [0, 2] and not tr["trace_times_up"][1]
        tr = _scripted("mutual_toggle", order)
        assert kills(tr)[0].tolist() == [False, True]
        tr = _scripted("done_agents_act", order)
        act = msc.active_before(tr)
        for a in (1, 2):
            assert not act[1:, ix(a, 3)].any() and (tr["trace_actions"][1:, ix(a, 3)] != 0).all()
            assert (tr["trace_reward"][1:, ix(a, 3)] == 0).all()
        assert kills(tr)[0, ix(1, 3)] and tr["trace_success"][0, ix(2, 3)] and act[:, ix(0, 3)].all()
        tr = _scripted("walk_into_corpse", order)
        assert kills(tr)[0].sum() == (2 if fwd else 1) and not tr["trace_success"].any()
        tr = _scripted("crate_into_agent", order)
        assert np.array_equal(tr["trace_act_locs"][0], tr["trace_pre_locs"][0]) and tr["trace_act_board"][0][2, 2] == 0x8014
        assert not tr["trace_pre_board"][0][2, 3] & msc.EXIT
        tr = _scripted("crate_into_leaving_agent", order)
        assert tr["trace_pre_board"][0][2, 3] & msc.EXIT and not (tr["trace_act_board"][0] == 0x8014).any()
        tr = _scripted("crate_into_exit", order)
        assert not (tr["trace_act_board"][0] == 0x8014).any() and tuple(tr["trace_act_locs"][0][ix(0, 2)]) == (2, 2)
        tr = _scripted("crate_shove", order)
        assert tr["trace_act_board"][0][2, 3] == 0x8014 and np.array_equal(tr["trace_act_locs"][0], tr["trace_pre_locs"][0])
        tr = _scripted("crate_pull", order)
        assert tr["trace_act_board"][0][2, 3] == 0x8014 and (tuple(tr["trace_act_locs"][0][ix(1, 2)]) == (2, 2)) == fwd
        tr = _scripted("leaver_at_leaver", order)
        assert tr["trace_pre_board"][0][2, 1] & tr["trace_pre_board"][0][2, 2] & msc.EXIT
        assert np.array_equal(tr["trace_act_locs"][0], tr["trace_pre_locs"][0]) and not tr["trace_done"].any()
        tr = _scripted("same_exit_same_step", order)
        assert tr["trace_success"][0].all() and np.array_equal(tr["trace_act_locs"][0][0], tr["trace_act_locs"][0][1])
        tr = _scripted("same_exit_successive", order)
        assert tr["trace_success"][:2, ix(0, 2)].all() and tr["trace_success"][:2, ix(1, 2)].tolist() == [False, True]
        tr = _scripted("over_under", order)     # index 0 is over its requirement, index 1 under it
        b, locs = tr["trace_board"][0], tr["trace_agent_locs"][0]
        assert b[tuple(locs[0])] & msc.EXIT and not b[tuple(locs[1])] & msc.EXIT and b[3, 1] == 0x110 | 0x200
        assert tr["trace_reset_board"][0][3, 1] == 0x110
        assert tr["trace_success"][4].tolist() == [True, False] and not tr["trace_done"][:, 1].any()
        assert np.array_equal(tr["trace_act_locs"][3][1], tr["trace_act_locs"][4][1]) and tr["trace_actions"][4, 1] != 0
        tr = _scripted("alias_3x3", order)
        assert (tr["trace_act_board"][0][1, 0] == 0x8014) == fwd
        tr = _scripted("time_limit_mixed", order)
        assert kills(tr)[0, ix(1, 3)] and tr["trace_success"][1, ix(2, 3)]
        assert tr["trace_times_up"].tolist()[:3] == [False, False, True]
        assert tr["trace_done"][2].all() and tr["trace_success"][2].sum() == 1 and not tr["trace_done"][1, ix(0, 3)]
        tr = _scripted("inactive_value", order)
        assert tr["trace_success"][0, ix(1, 2)]
        assert tr["trace_reward"][1, ix(0, 2)] != 0 and tr["trace_reward"][1, ix(1, 2)] == 0
        table = tr["level0_points_table"][ix(1, 2)]
        assert table[1, 1] - table[0, 1] != 0       # the push moves the leaver's own table score: its reward is still 0
        tr = _scripted("train8", order)
        assert kills(tr)[0].sum() == (1 if fwd else 2) and kills(tr)[0, ix(3, 8)]
        tr = _scripted("melee8", order)
        assert kills(tr)[0].tolist() == [False] * 4 + [True] * 4


def _restated_mismatches(tr, wrong):
    bad = 0
    for t in range(len(tr["trace_reward"])):
        board, locs = msc.execute_actions(tr["trace_pre_board"][t], tr["trace_pre_locs"][t], tr["trace_actions"][t], wrong)
        bad += not (np.array_equal(board, tr["trace_act_board"][t]) and np.array_equal(locs, tr["trace_act_locs"][t]))
    return bad


@pytest.mark.parametrize("name", SCRIPTED)
def test_restatement_reproduces_reference_action_boards(name):
    assert _restated_mismatches(msc.case(name), None) == 0


@pytest.mark.parametrize("wrong", msc.WRONG_READINGS)
def test_wrong_readings_are_caught(wrong):
    """Every wrong reading of the action loop differs from the reference on the case named for it in CAUGHT_BY."""
    caught = [n for n in SCRIPTED if _restated_mismatches(msc.case(n), wrong)]
    assert CAUGHT_BY[wrong] in caught, caught


@pytest.mark.parametrize("name", SCRIPTED)
def test_oracle_execute_actions_on_scripted_boards(name):
    tr = msc.case(name)
    for t in range(len(tr["trace_reward"])):
        board = np.ascontiguousarray(tr["trace_pre_board"][t], np.uint16).copy()
        locs = np.ascontiguousarray(tr["trace_pre_locs"][t], np.int64).copy()
        oracle.execute_actions(board, locs, tr["trace_actions"][t].astype(np.int64))
        assert np.array_equal(board, tr["trace_act_board"][t]) and np.array_equal(locs, tr["trace_act_locs"][t]), t


@pytest.mark.parametrize("name", SCRIPTED + DENSE + EDGE)
def test_oracle_replays_case(name):
    """OracleMultiEnv against the reference: every recorded array of every step and reset."""
    tr = msc.case(name)
    assert util.replay_trace_multi(tr, util.OracleMultiBackend, util.oracle_counts) == len(tr["trace_reward"])


@pytest.mark.parametrize("name", DENSE[:1] + EDGE[:1])
def test_one_agent_multi_oracle_equals_single_agent_oracle(name):
    """slo_env_step_multi with A = 1 against slo_env_step on the same levels and actions (the first agent's of the case):
    state, outputs and observation, array for array."""
    from safelife_amd.levels import LevelPool
    tr = msc.case(name)
    levels = msc.levels_of(tr)
    for lv in levels:
        lv.agent_locs, lv.points_table = lv.agent_locs[:1], lv.points_table[:1]
        lv.board[(lv.board & msc.AGENT) != 0] = 0
        lv.board[tuple(lv.agent_locs[0])] = 0x7A | 0x200
    B = 7
    kw = dict(first_level=np.arange(B) % len(levels), auto_reset=True, level_stride=3, time_limit=9, view_shape=(5, 7),
              output_channels=None)
    pool = LevelPool(levels, counts_fn=util.oracle_counts, min_performance_fraction=0.5)
    multi, single = util.OracleMultiBackend(pool, B, **kw), util.OracleBackend(pool, B, **kw)
    assert np.array_equal(multi.reset()[:, 0], single.reset())
    rng = np.random.default_rng(5)
    for t in range(40):
        acts = rng.integers(0, 9, B).astype(np.int32)
        om, rm, dm = multi.step(acts[:, None])
        o1, r1, d1 = single.step(acts)
        assert np.array_equal(om[:, 0], o1) and np.array_equal(rm[:, 0], r1) and np.array_equal(dm[:, 0], d1), t
        for name_ in ("board", "goals", "rng", "num_steps", "level_idx", "episode_idx", "goals_static", "exit_locs"):
            assert np.array_equal(multi.get(name_), single.get(name_)), (t, name_)
        assert np.array_equal(multi.get("agent_locs")[:, 0], single.get("agent_loc")), t
        for name_ in ("old_value", "required_points", "initial_points", "table_idx", "is_active", "episode_reward",
                      "episode_length", "success"):
            assert np.array_equal(multi.get(name_)[:, 0], single.get(name_)), (t, name_)
    assert single.get("episode_idx").min() >= 2
