#!/usr/bin/env python3
"""
Writes tests/golden/multi_step_cases.npz by RUNNING THE REFERENCE on the CPU: what the fused multi-agent step
(csrc/sl_generic.hip: k_env_step_multi, k_env_reset_multi), the oracle's slo_env_step_multi and the plain restatement of
the serial action loop in tests/multi_step_cases.py are held to, from 1 to 8 agents.

    python tests/golden/make_golden_multi_step.py

Runs where make_golden.py runs.  Every case is one run of the reference's SafeLifeEnv(single_agent=False) through
make_golden.run_trace_multi: the arrays of a trace_multi_*.npz file (level records, reset and per-step outputs, the
actions AS GIVEN -- agents that are done keep receiving non-zero actions).  The cases of a family are padded to a common
shape and stacked, `<key>` next to `<key>__shape` (tests/multi_step_cases.py cuts them apart again); the levels of a case
are stacked as lv_<key> [n_levels, ...].

  scripted/*  hand-made boards up to 8 x 8, 2 to 6 steps, one event each (scripted_cases() below).  Every base case is
              recorded in three placements -- as drawn, rolled so that the event straddles the column seam of the torus, transposed
              and rolled so that it straddles the row seam -- and in both index orders (the agent list and the action
              columns reversed).  These also hold, per step, the board and locations right before execute_actions
              (pre_board, pre_locs) and right after it, before advance_board (act_board, act_locs).
  dense/*     dense random boards (15 % life, 10 % crates, 5 % walls, goals, two exits), 10 levels with min_performance
              alternating -1 / 0.3, time_limit 12, 120 uniformly random actions 0..8 for every agent, done or not.
  edge/*      the same on boards at the edges of the generic kernels' block sizes (HW = 256 / 272 / 1024 / 1025 / 1056),
              the agents starting in one 4 x 4 patch together with the exits, one spawner per level, 40 steps, time_limit 10.

Agent a plays on the default points table with its colour columns rolled by a and one entry changed, as
make_golden_schedule_multi.synthetic_levels does.  The script asserts on the reference's own output that every scripted
case shows the event it is named for and that every multi-agent random case holds a kill, an exit and a time-limit end
(tests/test_multi_step_host.py asserts it again on the file).
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

AGENT, PUSHABLE, DESTRUCTIBLE, FROZEN, EXIT = 2, 4, 8, 16, 256
PLAYER = 2 | 8 | 16 | 32 | 64
WALL, CRATE, LEVEL_EXIT, SPAWNER = 16, 16 | 4 | 0x8000, 16 | 256, 16 | 128 | 8
PLANT = 16 | 1 | 4 | 0x8000
RED, GREEN = 1 << 9, 2 << 9
TRANSPOSED_ACTION = np.array([0, 4, 3, 2, 1, 8, 7, 6, 5])
DENSE = ((1, 4, 4), (2, 3, 4), (3, 5, 5), (5, 4, 5), (8, 6, 7))
EDGE = ((8, 16, 16), (8, 16, 17), (8, 32, 32), (8, 25, 41), (3, 32, 33))
RAW_VIEW = dict(view_shape=(5, 5), output_channels=None, should_calculate_side_effects=False)


def agent_cell(a):
    return PLAYER | (((a % 7) + 1) << 9)


def agent_tables(default_table, A):
    tables = np.zeros((A, 8, 9), np.int64)
    for a in range(A):
        t = np.array(default_table, np.int64)
        t[:, :8] = np.roll(t[:, :8], a, axis=1)
        t[1 + a % 7, (a * 3) % 8] += a + 1
        tables[a] = t
    return tables


# ------------------------------------------------------------------------------------------------ scripted cases
#
# A base case: board size, agents [(y, x)], cells {(y, x): value}, goals {(y, x): colour}, actions [T][A], and
# `locked` (min_performance 1 with goals in a corner: no agent may leave, so no agent cell carries the EXIT bit) or open
# (min_performance -1: every agent may leave and carries it).  `event(c)` is asserted on the reference's output; c maps
# the case's own coordinates and agent numbers onto the recorded placement and index order (class Ctx).

def kills(c):
    return c.done & ~c.success & ~c.times_up[:, None] & c.was_active


def ev_head_on(c):
    for t in range(c.T):
        assert np.array_equal(c.act_locs_l[t], c.start), "both stay"
    for a in (0, 1):            # blocked, but turned to face the way it was told to go
        assert (c.cell(c.act_board[0], c.start[a]) >> 12) & 3 == (int(c.actions[0, c.ix(a)]) - 1) & 3


def ev_follow(c):
    # the follower is agent 0: as the lower index it finds the leader still there on step 0; as the higher one it follows
    moved = c.act_locs_l[0][0][1] != c.start[0][1]
    assert moved == (c.order == "rev") and c.act_locs_l[0][1][1] == c.start[1][1] + 1


def ev_same_cell(c):
    winner = 0 if c.order == "fwd" else 1
    assert tuple(c.act_locs_l[0][winner]) == (2, 2) and tuple(c.act_locs_l[0][1 - winner]) == tuple(c.start[1 - winner])


def ev_create_destroy(c):
    assert c.cell(c.pre_board[0], (2, 2)) == 0 and c.cell(c.act_board[0], (2, 2)) == 0
    assert c.cell(c.act_board[1], (2, 2)) == (1 | 8 | (agent_cell(c.ix(0)) & 0xE00))


def ev_kill(c):
    k = kills(c)
    assert k[0, c.ix(1)] and k.sum() == 1
    dead = c.cell(c.act_board[0], (2, 2))
    assert not dead & (AGENT | DESTRUCTIBLE) and dead & FROZEN
    # the victim's own action (a life cell below it) is lost when it is the higher index, carried out when the lower
    assert (c.cell(c.act_board[0], (3, 2)) != 0) == (c.order == "rev")
    assert (c.actions[1:, c.ix(1)] != 0).all()


def ev_kill_then_exit(c):
    k = kills(c)
    assert k[0, c.ix(1)] and c.success[1, c.ix(0)] and c.done[1].all() and not c.times_up[1]
    assert len(c.tr["reset_at"]) == 2 and c.tr["reset_at"][1] == 2


def ev_mutual(c):
    k = kills(c)
    assert k[0].sum() == 1 and k[0, 1], "the lower index kills, whoever it is"
    assert c.cell(c.act_board[0], c.start[c.lx(0)]) & AGENT


def ev_done_actions(c):
    k = kills(c)
    assert k[0, c.ix(1)] and c.success[0, c.ix(2)]
    for a in (1, 2):
        assert (c.actions[1:, c.ix(a)] != 0).all() and c.done[:, c.ix(a)].all()
        assert (c.reward[1:, c.ix(a)] == 0).all()
    assert not c.done[:, c.ix(0)].any()
    for t in range(1, c.T):     # nothing but agent 0 acts: the block (its EXIT bit gone with the first recolouring) stays
        assert c.cell(c.act_board[t], (2, 2)) == c.cell(c.act_board[0], (2, 2)) & ~EXIT
        assert tuple(c.act_locs_l[t][2]) == (4, 4)


def ev_crate_blocked(c):
    assert np.array_equal(c.act_locs_l[0], c.start) and c.cell(c.act_board[0], (2, 2)) == CRATE
    assert not c.cell(c.pre_board[0], (2, 3)) & EXIT and c.cell(c.act_board[0], (2, 3)) & AGENT


def ev_crate_into_leaving_agent(c):
    # an agent that may leave carries the EXIT bit, so the crate is "pushed out the exit" (advance_board.c:276-278)
    assert c.cell(c.pre_board[0], (2, 3)) & EXIT and c.cell(c.pre_board[0], (2, 3)) & AGENT
    assert tuple(c.act_locs_l[0][0]) == (2, 2) and (c.act_board[0] == CRATE).sum() == 0


def ev_crate_into_exit(c):
    assert tuple(c.act_locs_l[0][0]) == (2, 2) and (c.act_board[0] == CRATE).sum() == 0
    assert c.cell(c.act_board[0], (2, 3)) & EXIT and not c.success[0].any()


def ev_crate_shove(c):
    assert np.array_equal(c.act_locs_l[0], c.start)
    assert c.cell(c.act_board[0], (2, 2)) == 0 and c.cell(c.act_board[0], (2, 3)) == CRATE


def ev_crate_pull(c):
    assert c.cell(c.act_board[0], (2, 3)) == CRATE and tuple(c.act_locs_l[0][0]) == (2, 4)
    # the other agent walks into the cell the crate left when it acts second; acting first it pushes at a crate that has
    # an agent behind it, and stays
    assert (tuple(c.act_locs_l[0][1]) == (2, 2)) == (c.order == "fwd")


def ev_leaver_at_leaver(c):
    assert c.cell(c.pre_board[0], c.start[0]) & EXIT and c.cell(c.pre_board[0], c.start[1]) & EXIT
    assert np.array_equal(c.act_locs_l[0], c.start) and not c.done.any()


def ev_same_exit_same_step(c):
    assert c.success[0].all() and np.array_equal(c.act_locs_l[0][0], c.act_locs_l[0][1])
    assert c.cell(c.act_board[0], (2, 2)) & EXIT and not c.cell(c.act_board[0], (2, 2)) & AGENT


def ev_same_exit_successive(c):
    assert c.success[0, c.ix(0)] and not c.done[0, c.ix(1)] and c.success[1].all()
    assert np.array_equal(c.tr["agent_locs"][0][c.ix(0)], c.act_locs[1][c.ix(1)])


def ev_over_under(c):
    # the push is worth +4 on the table of index 0 and -3 on that of index 1: whoever has index 0 is over its requirement
    over, under = c.lx(0), c.lx(1)
    b = c.tr["board"][0]
    assert c.cell(b, c.act_locs_l[0][over]) & EXIT and not c.cell(b, c.act_locs_l[0][under]) & EXIT
    assert c.cell(b, (3, 1)) == LEVEL_EXIT | RED, "any agent may leave: red exits"
    assert c.cell(c.tr["reset_board"][0], (3, 1)) == LEVEL_EXIT
    for a in (0, 1):
        assert not c.cell(c.tr["reset_board"][0], c.start[a]) & EXIT
    # the agent under its requirement stands in front of the exit, is told to walk in twice and stays
    front = (3, 2) if under == 1 else (2, 1)
    assert tuple(c.act_locs_l[3][under]) == front and tuple(c.act_locs_l[4][under]) == front
    assert c.actions[4, c.ix(under)] != 0 and not c.done[:, c.ix(under)].any()
    assert c.success[4, c.ix(over)]


def ev_alias(c):
    # 3 wide: the cell two ahead IS the cell behind.  The first to act wins (2, 2)'s neighbourhood
    if c.order == "fwd":        # the crate is pushed to (1, 2) = the cell behind the agent's old place, and pulled along
        assert tuple(c.act_locs_l[0][0]) == (1, 1) and c.cell(c.act_board[0], (1, 0)) == CRATE
    else:
        assert tuple(c.act_locs_l[0][1]) == (1, 2) and tuple(c.act_locs_l[0][0]) == (1, 0)


def ev_time_limit(c):
    k = kills(c)
    assert k[0, c.ix(1)] and c.success[1, c.ix(2)] and c.times_up[2] and not c.times_up[:2].any()
    assert c.done[2].all() and not c.done[1, c.ix(0)] and list(c.success[2]) == [a == c.ix(2) for a in range(3)]


def ev_inactive_value(c):
    assert c.success[0, c.ix(1)]
    assert c.reward[1, c.ix(0)] != 0 and c.reward[1, c.ix(1)] == 0
    assert c.points_table[c.ix(1)][1, 1] - c.points_table[c.ix(1)][0, 1] != 0, "its own table does move on that push"


def ev_train8(c):
    k = kills(c)
    moved = (c.act_locs_l[0][:7, 1] != c.start[:7, 1])
    if c.order == "fwd":        # in index order only the head of the train finds its cell free; then agent 3 is killed
        assert k[0].sum() == 1 and k[0, c.ix(3)] and moved[6] and moved.sum() == 1
    else:
        # in reverse order agent 3 is killed first and the train moves up from the head.  Agent 2 then walks at the block
        # agent 3 left, which still carries the EXIT bit agent 3 had: it "leaves" through it (advance_board.c:282) and is
        # gone -- the recolouring takes the bit off, so it has not exited -- and agents 1 and 0 move up behind it
        assert k[0].sum() == 2 and k[0, c.ix(3)] and k[0, c.ix(2)] and not c.success.any()
        assert list(moved) == [True, True, True, False, True, True, True]
        assert tuple(c.act_locs_l[0][2]) == tuple(c.start[3])


def ev_corpse(c):
    k = kills(c)
    if c.order == "fwd":        # killed first, then walked into: the walker is gone too (see ev_train8)
        assert k[0, c.ix(1)] and k[0, c.ix(2)] and tuple(c.act_locs_l[0][2]) == (2, 2)
        assert c.cell(c.act_board[0], (2, 1)) == 0 and not c.cell(c.act_board[0], (2, 2)) & AGENT
    else:                       # the walker acts first and finds a live agent that may leave: it stays
        assert k[0].sum() == 1 and k[0, c.ix(1)] and tuple(c.act_locs_l[0][2]) == (2, 1)
    assert not c.success.any()


def ev_melee8(c):
    k = kills(c)
    assert k[0].sum() == 4 and k[0, 4:].all(), "the four lower indices kill the four higher ones"
    assert c.times_up[-1] or not c.done[-1].all()


def scripted_cases():
    S = []

    def add(name, h, w, agents, cells, actions, event, goals=None, locked=False, time_limit=20, min_perf=None):
        S.append(dict(name=name, h=h, w=w, agents=agents, cells=cells, actions=actions, event=event, goals=goals or {},
                      locked=locked, time_limit=time_limit,
                      min_perf=(1.0 if locked else -1.0) if min_perf is None else min_perf))

    add("head_on", 6, 6, [(2, 1), (2, 2)], {}, [[2, 4], [2, 4]], ev_head_on)
    add("follow_leader", 6, 7, [(2, 1), (2, 2)], {}, [[2, 2], [2, 2], [2, 2]], ev_follow)
    add("same_cell", 6, 6, [(2, 1), (2, 3)], {}, [[2, 4], [0, 0]], ev_same_cell)
    add("create_destroy", 6, 6, [(2, 1), (2, 3)], {}, [[6, 8], [6, 0], [0, 0]], ev_create_destroy)
    add("kill", 6, 6, [(2, 1), (2, 2)], {}, [[6, 7], [0, 2], [1, 7], [0, 3]], ev_kill)
    add("kill_then_exit", 6, 6, [(2, 1), (2, 2)], {(3, 1): LEVEL_EXIT}, [[6, 5], [3, 4], [0, 0], [2, 2]], ev_kill_then_exit)
    add("mutual_toggle", 6, 6, [(2, 1), (2, 2)], {}, [[6, 8], [6, 8]], ev_mutual)
    add("done_agents_act", 7, 7, [(2, 1), (2, 2), (4, 3)], {(4, 4): LEVEL_EXIT},
        [[6, 0, 2], [0, 2, 4], [1, 7, 6], [0, 4, 1], [3, 5, 8], [0, 1, 3]], ev_done_actions)
    add("walk_into_corpse", 6, 6, [(1, 2), (2, 2), (2, 1)], {}, [[7, 0, 2], [0, 3, 4], [2, 2, 2]], ev_corpse)
    add("crate_into_agent", 6, 6, [(2, 1), (2, 3)], {(2, 2): CRATE}, [[2, 0], [2, 0]], ev_crate_blocked, locked=True)
    add("crate_into_leaving_agent", 6, 6, [(2, 1), (2, 3)], {(2, 2): CRATE}, [[2, 0], [0, 0]], ev_crate_into_leaving_agent)
    add("crate_into_exit", 6, 6, [(2, 1), (4, 4)], {(2, 2): CRATE, (2, 3): LEVEL_EXIT}, [[2, 0], [0, 1]], ev_crate_into_exit)
    add("crate_shove", 6, 6, [(2, 1), (4, 4)], {(2, 2): CRATE}, [[6, 0], [0, 1]], ev_crate_shove)
    add("crate_pull", 6, 7, [(2, 3), (2, 1)], {(2, 2): CRATE}, [[2, 2], [0, 0]], ev_crate_pull, locked=True)
    add("leaver_at_leaver", 6, 6, [(2, 1), (2, 2)], {(4, 4): LEVEL_EXIT}, [[2, 0], [2, 4]], ev_leaver_at_leaver)
    add("same_exit_same_step", 6, 6, [(2, 1), (2, 3)], {(2, 2): LEVEL_EXIT}, [[2, 4], [1, 2], [3, 3]],
        ev_same_exit_same_step)
    add("same_exit_successive", 6, 7, [(2, 1), (2, 4)], {(2, 2): LEVEL_EXIT}, [[2, 4], [5, 4], [1, 1]],
        ev_same_exit_successive)
    add("over_under", 6, 6, [(1, 1), (3, 3)], {(1, 2): PLANT | RED, (3, 1): LEVEL_EXIT},
        [[2, 0], [3, 4], [4, 4], [3, 4], [3, 4]], ev_over_under, goals={(1, 3): RED}, min_perf=0.5)
    add("alias_3x3", 3, 3, [(1, 0), (2, 2)], {(1, 1): CRATE}, [[2, 1], [0, 0]], ev_alias, locked=True)
    add("time_limit_mixed", 7, 7, [(2, 1), (2, 2), (4, 3)], {(4, 4): LEVEL_EXIT},
        [[6, 0, 0], [1, 3, 2], [2, 2, 2], [0, 0, 0]], ev_time_limit, time_limit=3)
    add("inactive_value", 6, 7, [(1, 1), (3, 3)], {(1, 2): PLANT | RED, (3, 4): LEVEL_EXIT}, [[0, 2], [2, 6], [0, 0]],
        ev_inactive_value, goals={(1, 3): RED})
    add("train8", 8, 8, [(2, x) for x in range(7)] + [(3, 3)], {}, [[2] * 7 + [5], [2] * 7 + [1], [2, 3, 2, 1, 2, 4, 2, 6]],
        ev_train8)
    add("melee8", 8, 8, [(2, x) for x in range(1, 5)] + [(3, x) for x in range(1, 5)], {},
        [[7] * 4 + [5] * 4, [2, 1, 4, 6, 1, 2, 3, 4], [1] * 8], ev_melee8, time_limit=3)
    return S


class Ctx(object):
    """A recorded scripted case seen in the base case's own coordinates and agent numbers."""

    def __init__(self, case, placement, order, tr, shape, shift):
        self.tr, self.order, self.placement = tr, order, placement
        self.A = A = len(case["agents"])
        self.T = len(tr["reward"])
        self.shape, self.shift = shape, shift
        self.start = np.array(case["agents"])
        self.actions = tr["actions"]
        self.done, self.success, self.times_up, self.reward = tr["done"], tr["success"], tr["times_up"], tr["reward"]
        active = np.ones((self.T, A), bool)
        for t in range(1, self.T):
            active[t] = True if t in tr["reset_at"] else active[t - 1] & ~self.done[t - 1]
        self.was_active = active
        self.pre_board, self.act_board, self.act_locs = tr["pre_board"], tr["act_board"], tr["act_locs"]
        by_agent = [self.ix(a) for a in range(A)]
        self.act_locs_l = np.array([[self.unplace(l) for l in locs[by_agent]] for locs in self.act_locs])
        self.points_table = tr["points_table"]

    def ix(self, a):            # the base case's agent a -> recorded index
        return a if self.order == "fwd" else self.A - 1 - a

    lx = ix                     # (an involution: recorded index -> the base case's agent)

    def place(self, p):
        return place(p, self.placement, self.shape, self.shift)

    def unplace(self, q):
        H, W = self.shape
        if self.placement == "plain":
            return (int(q[0]), int(q[1]))
        if self.placement == "colseam":
            return (int(q[0]), int(q[1] - self.shift) % W)
        return (int(q[1]), int(q[0] - self.shift) % H)

    def cell(self, board, p):
        return int(board[self.place(tuple(int(v) for v in p))])


def place(p, placement, shape, shift):
    """The base case's cell (y, x) on the recorded board (shape: the recorded board's)."""
    H, W = shape
    if placement == "plain":
        return (p[0], p[1])
    if placement == "colseam":
        return (p[0], (p[1] + shift) % W)
    return ((p[1] + shift) % H, p[0])           # rowseam: transposed, then rolled down the rows


def build_scripted(R, case, placement, order):
    Game = R.game.SafeLifeGame
    h, w, A = case["h"], case["w"], len(case["agents"])
    shape = (h, w) if placement != "rowseam" else (w, h)
    # the seam falls between the base case's columns 1 and 2, where every case has its event (3 wide: between 0 and 1)
    shift = 0 if placement == "plain" else (shape[1] if placement == "colseam" else shape[0]) - (2 if w > 3 else 1)
    perm = list(range(A)) if order == "fwd" else list(range(A))[::-1]
    board, goals = np.zeros(shape, np.uint16), np.zeros(shape, np.uint16)
    for p, v in case["cells"].items():
        board[place(p, placement, shape, shift)] = v
    for p, v in case["goals"].items():
        goals[place(p, placement, shape, shift)] = v
    if case["locked"]:          # goals nobody fills, in the far corner: every agent has points to earn
        far = [(h - 1, w - 1), (h - 1, w - 2)] if h > 3 else [(0, 2), (0, 1)]
        goals[place(far[0], placement, shape, shift)] = RED
        goals[place(far[1], placement, shape, shift)] = GREEN
    locs = np.zeros((A, 2), np.int64)
    for i, a in enumerate(perm):    # recorded index i is the base case's agent a; the colour goes with the index
        locs[i] = place(case["agents"][a], placement, shape, shift)
        board[tuple(locs[i])] = agent_cell(i)
    actions = np.array(case["actions"], np.int64)[:, perm]
    if placement == "rowseam":
        actions = TRANSPOSED_ACTION[actions]
    tables = agent_tables(Game.default_points_table, A)

    def games():
        out = []
        for k in range(2):          # the same level twice: an episode that ends reloads inside the step
            g = Game(board_size=shape)
            g.board, g.goals, g.agent_locs = board.copy(), goals.copy(), locs.copy()
            g.min_performance = case["min_perf"]
            g.spawn_prob = 0.3
            g.points_table = tables.copy()
            g.update_exit_locs()
            out.append(make_golden.seeded(Game.loaddata(g.serialize()), 7000 + k))
        return out

    extra = {k: [] for k in ("pre_board", "pre_locs", "act_board", "act_locs")}
    inner = Game.execute_actions

    def recording(self, actions):
        extra["pre_board"].append(self.board.copy()), extra["pre_locs"].append(self.agent_locs.copy())
        inner(self, actions)
        extra["act_board"].append(self.board.copy()), extra["act_locs"].append(self.agent_locs.copy())
    Game.execute_actions = recording
    try:
        blob = trace_blob(R, games, actions, dict(time_limit=case["time_limit"], **RAW_VIEW))
    finally:
        Game.execute_actions = inner
    T = len(blob["trace_reward"])
    for k, v in extra.items():
        blob["trace_" + k] = np.array(v[:T])
    if case["locked"]:
        assert (blob["trace_reset_required"][0] > 0).all(), (case["name"], blob["trace_reset_required"][0])
    tr = {k[len("trace_"):]: v for k, v in blob.items() if k.startswith("trace_")}
    tr["points_table"] = tables
    try:
        case["event"](Ctx(case, placement, order, tr, shape, shift))
    except AssertionError:
        print("scripted case %s/%s/%s does not show its event" % (case["name"], placement, order))
        raise
    return blob


# ------------------------------------------------------------------------------------------------ random cases

def random_level(rng, A, H, W, min_performance, default_table, clustered):
    """15 % life, 10 % crates, 5 % walls, coloured goals under a quarter of the cells, two exits; the agents anywhere, or
    (`clustered`) in one 4 x 4 patch together with the exits, and one spawner on the board."""
    kind = rng.random((H, W))
    colors = (rng.integers(1, 8, (H, W)) << 9).astype(np.uint16)
    board = np.zeros((H, W), np.uint16)
    board[kind < 0.15] = 1 | 8
    board[kind < 0.15] |= colors[kind < 0.15]
    board[(kind >= 0.15) & (kind < 0.25)] = CRATE
    board[(kind >= 0.25) & (kind < 0.30)] = WALL
    goals = np.where(rng.random((H, W)) < 0.25, (rng.integers(1, 8, (H, W)) << 9), 0).astype(np.uint16)
    if clustered:
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        patch = [((y0 + i) % H, (x0 + j) % W) for i in range(4) for j in range(4)]
        board[tuple(np.array(patch).T)] = 0
        order = rng.permutation(16)
        cells, exits = [patch[i] for i in order[:A]], [patch[i] for i in order[A:A + 2]]
        while True:
            sp = (int(rng.integers(0, H)), int(rng.integers(0, W)))
            if sp not in patch and sp not in exits:
                break
        board[sp] = SPAWNER | (int(rng.integers(1, 8)) << 9)
    else:
        flat = rng.permutation(H * W)[:A + 2]
        cells = [(int(i) // W, int(i) % W) for i in flat[:A]]
        exits = [(int(i) // W, int(i) % W) for i in flat[A:]]
    for e in exits:
        board[e] = LEVEL_EXIT
    for a, c in enumerate(cells):
        board[c] = agent_cell(a)
    return dict(board=board, goals=goals, agent_locs=np.array(cells, np.int64), spawn_prob=0.3,
                min_performance=min_performance, points_table=agent_tables(default_table, A))


def build_random(R, A, H, W, seed, clustered):
    Game = R.game.SafeLifeGame
    rng = np.random.default_rng(seed)
    n_levels, steps, time_limit = (10, 40, 10) if clustered else (10, 120, 12)
    datas = [random_level(rng, A, H, W, -1.0 if k % 2 == 0 else 0.3, Game.default_points_table, clustered)
             for k in range(n_levels)]
    actions = rng.integers(0, 9, (steps, A))

    def games():
        return [make_golden.seeded(Game.loaddata(dict(d)), 9000 + 17 * seed + k) for k, d in enumerate(datas)]
    return trace_blob(R, games, actions, dict(time_limit=time_limit, **RAW_VIEW))


def event_counts(blob):
    """(kills, exits, time-limit ends, agent-steps with a non-zero action for an agent that is done) of a case."""
    done, success, times_up = blob["trace_done"], blob["trace_success"], blob["trace_times_up"]
    T, A = done.shape
    active = np.ones((T, A), bool)
    for t in range(1, T):
        active[t] = True if t in blob["trace_reset_at"] else active[t - 1] & ~done[t - 1]
    kills = int((done & ~success & ~times_up[:, None] & active).sum())
    exits = int((success & active).sum())
    ends = int((times_up & active.any(axis=1)).sum())
    idle = int(((blob["trace_actions"] != 0) & ~active).sum())
    return kills, exits, ends, idle


# ------------------------------------------------------------------------------------------------ file format

def trace_blob(R, games_fn, actions, env_kw):
    tr = make_golden.run_trace_multi(R, games_fn(), actions, env_kw)
    recs = []
    for g in games_fn():
        rec = make_golden.level_record(g)
        rec["rng"] = make_golden.words(g._rng.bit_generator)
        recs.append(rec)
    blob = {"lv_" + k: np.stack([np.asarray(r[k]) for r in recs]) for k in recs[0]}
    blob["n_levels"] = np.array(len(recs))
    for k, v in tr.items():
        blob["trace_" + k] = v
    blob["trace_obs"] = blob["trace_obs"].astype(np.uint32)
    for k, v in env_kw.items():
        blob["env_" + k] = np.array(-1 if v is None else v)
    return blob


def pack(family, names, blobs, out):
    """Cases of one family, padded to a common shape per key and stacked; <key>__shape holds each case's own."""
    out[family + "/names"] = np.array(names)
    for key in blobs[0]:
        arrs = [np.asarray(b[key]) for b in blobs]
        assert len(set(a.ndim for a in arrs)) == 1 and len(set(a.dtype for a in arrs)) == 1, (family, key)
        full = tuple(max(a.shape[d] for a in arrs) for d in range(arrs[0].ndim))
        stacked = np.zeros((len(arrs),) + full, arrs[0].dtype)
        for i, a in enumerate(arrs):
            stacked[(i,) + tuple(slice(0, s) for s in a.shape)] = a
        out["%s/%s" % (family, key)] = stacked
        out["%s/%s__shape" % (family, key)] = np.array([a.shape for a in arrs], np.int32).reshape(len(arrs), arrs[0].ndim)


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


SEEDS = {(1, 4, 4): 1, (2, 3, 4): 2, (3, 5, 5): 3, (5, 4, 5): 4, (8, 6, 7): 5,
         (8, 16, 16): 11, (8, 16, 17): 12, (8, 32, 32): 13, (8, 25, 41): 14, (3, 32, 33): 15}


def main():
    global make_golden
    import make_golden
    R = make_golden.import_reference()
    out = {}
    names, blobs = [], []
    for case in scripted_cases():
        for placement in ("plain", "colseam", "rowseam"):
            for order in ("fwd", "rev"):
                names.append("%s/%s/%s" % (case["name"], placement, order))
                blobs.append(build_scripted(R, case, placement, order))
    pack("scripted", names, blobs, out)
    print("scripted: %d cases (%d base cases x 3 placements x 2 index orders)" % (len(names), len(names) // 6))
    totals = np.sum([event_counts(b) for b in blobs], axis=0)
    print("  kills=%d exits=%d time-limit ends=%d actions for done agents=%d" % tuple(totals))
    assert totals.min() > 0
    for family, cases, clustered in (("dense", DENSE, False), ("edge", EDGE, True)):
        names, blobs = [], []
        for (A, H, W) in cases:
            blob = build_random(R, A, H, W, SEEDS[(A, H, W)], clustered)
            k, x, e, idle = event_counts(blob)
            print("%s %dx%dx%d: steps=%d episodes=%d kills=%d exits=%d time-limit ends=%d actions for done agents=%d" % (
                family, A, H, W, len(blob["trace_reward"]), len(blob["trace_reset_at"]), k, x, e, idle))
            assert not clustered or len(blob["trace_reward"]) == 40     # (a dense run ends when its ten levels are played)
            if A > 1:               # (a seed that fails this is changed, never the condition)
                assert k > 0 and x > 0 and e > 0 and idle > 0, (family, A, H, W)
            names.append("%dx%dx%d" % (A, H, W))
            blobs.append(blob)
        pack(family, names, blobs, out)
    path = os.path.join(HERE, "multi_step_cases.npz")
    write_npz(path, out)
    print("wrote %s: %d bytes" % (os.path.basename(path), os.path.getsize(path)))
    assert os.path.getsize(path) < 1000 * 1000


if __name__ == "__main__":
    main()
