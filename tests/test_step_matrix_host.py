"""The cases of tests/step_matrix_cases.py do what they claim: every (shape, configuration) of the fused-step matrix run
on the ORACLE alone, asserting the coverage conditions -- so that a pool or a script that has quietly stopped exercising
an edge fails here, not by passing on the device.  No GPU.
"""
import numpy as np
import pytest

import oracle
from safelife_amd.cell_types import CellTypes as CT
from tests import step_matrix_cases as smc
from tests import util


def test_geometry_rule_gives_the_known_workgroup_sizes():
    assert sorted(smc.SHAPES) == sorted(smc.EXPECTED_NB) and len(smc.SHAPES) == 14
    for H in smc.SHAPES:
        g = smc.geometry(H, H)
        assert g["NB"] == smc.EXPECTED_NB[H], H
        assert g["VERT"] == ("rotate" if H == 64 else "shift" if H in (24, 25, 26, 30, 40, 48) else "bpermute"), H
        assert g["cache"] == (H not in (20, 12, 10)), H
        assert g["lean_takes_queue"] == (H >= 40), H


@pytest.mark.parametrize("H", smc.SHAPES)
def test_configurations_reach_every_kernel_slot(H):
    """The twelve configurations of a shape launch all 24 instantiations pick_rollout_t chooses from -- by the rule
    restated in step_matrix_cases.kernel_slots, fed from the pools as built (table count, spawner presence)."""
    slots = set()
    for cfg in smc.CONFIGS:
        case = smc.Case(H, cfg)
        pool = case.pool(util.oracle_counts)
        assert (pool.points_table.shape[0] == 1) == (case.tables == "one")
        assert pool.has_spawner == (case.spawn == "spawn")
        assert np.abs(pool.points_table).max() <= 127 and pool.exit_slots == 8
        lean = case.front == "plain"
        got = smc.kernel_slots(pool.points_table.shape[0], not pool.has_spawner, case.wrapped, lean)
        assert got == case.slots()
        slots |= got
    assert slots == set(range(24)), "%d of 24" % len(slots)
    if smc.geometry(H, H)["lean_takes_queue"]:          # the plain kernels of the wide shapes with a queue: still lean
        assert smc.Case(H, smc.CONFIGS[0], queue=True).slots() == smc.Case(H, smc.CONFIGS[0]).slots()


def _pool_items(H, W=None):
    """Every constructed item a pool promises, read back from its levels."""
    W = H if W is None else W
    WS = (W + 1) // 2
    levels = smc.build_levels(H, W, "many", "spawn")
    assert len(levels) == smc.N_LEVELS
    starts = {tuple(lv.agent_locs[0]) for lv in levels if len(lv.agent_locs)}
    assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= starts
    assert any(x == WS - 1 for _, x in starts) and any(x == WS for _, x in starts)
    assert any(0 < y < H - 1 and x not in (0, WS - 1, WS, W - 1) for y, x in starts)
    assert sum(len(lv.agent_locs) == 0 for lv in levels) == 1
    assert {len(lv.exit_locs) for lv in levels} == {0, 1, 3, 8}
    seam = lambda i: i % W in (0, WS - 1, WS, W - 1)
    assert any(seam(i) for lv in levels for i in lv.exit_locs)
    assert levels[smc.SUCCESS_LEVEL].min_performance == -1
    assert any((lv.goals & CT.alive).any() for lv in levels)
    spawners = [np.argwhere(lv.board & CT.spawning) for lv in levels]
    assert {int(y) for s in spawners for y, _ in s} == {0, H - 1}
    assert {int(x) for s in spawners for _, x in s} == {WS - 1, WS}
    assert {lv.spawn_prob for lv, s in zip(levels, spawners) if len(s)} == {np.float64(0.05), np.float64(0.9)}
    assert sum((lv.board == CT.crate).any() for lv in levels) == 2
    assert len({lv.points_table.tobytes() for lv in levels}) == 3
    still = smc.build_levels(H, W, "one", "still")
    assert not any((lv.board & CT.spawning).any() for lv in still)
    # the life patterns straddle the seams: a blinker over columns W-1 | 0, one over rows H-1 | 0, a block on the four
    # corners of the array, and a glider that is still a glider after crossing row H-1 -> 0 and column W-1 -> 0
    alive = [(lv.board & (CT.alive | CT.frozen)) == CT.alive for lv in still]
    r = H // 2
    assert alive[0][r, W - 1] and alive[0][r, 0] and alive[0][r, 1] and alive[0].sum() == 3
    assert alive[1][H - 1, 2] and alive[1][0, 2] and alive[1][1, 2] and alive[1].sum() == 3
    assert alive[4][0, 0] and alive[4][0, W - 1] and alive[4][H - 1, 0] and alive[4][H - 1, W - 1] and alive[4].sum() == 4
    glider = np.where(alive[smc.EVOLVING_LEVEL], still[smc.EVOLVING_LEVEL].board, 0).astype(np.uint16)
    for n_step, rows, cols in ((0, {H - 3, H - 2, H - 1}, {W - 3, W - 2, W - 1}), (8, {H - 1, 0, 1}, {W - 1, 0, 1})):
        cells = np.argwhere(oracle.advance_board(glider, 0.0, n_step) & CT.alive)
        assert len(cells) == 5 and {int(y) for y, _ in cells} == rows and {int(x) for _, x in cells} == cols, (n_step, cells)


@pytest.mark.parametrize("H", smc.SHAPES)
def test_pools_hold_every_constructed_item(H):
    _pool_items(H)


class Coverage(object):
    """What a run exercised, gathered step by step from the oracle's state."""

    def __init__(self, case, cpu):
        self.case, self.cpu = case, cpu
        self.crossings, self.stood, self.seam_edits, self.pushes = set(), set(), 0, set()
        B = case.B
        self.ends = np.zeros(B, np.int64)
        self.n_success = self.n_times_up = self.max_ends_in_a_step = 0
        self.shaped_differs = self.env_steps = 0
        self.side_effect_seen, self.move_terms = False, set()
        self.goals_changed = False

    def before(self, t):
        case, cpu = self.case, self.cpu
        H, W, WS = case.H, case.W, case.geom["WS"]
        level, steps = cpu.get("level_idx"), cpu.get("num_steps")
        assert np.array_equal(level, case.schedule[t, :, 0]) and np.array_equal(steps, case.schedule[t, :, 1]), \
            "step %d: the oracle is not where the builder's schedule says" % t
        self.board0, self.loc0, self.level0, self.goals0 = cpu.get("board"), cpu.get("agent_loc"), level, cpu.get("goals")
        # the action alone, without the CA step behind it
        acts = np.where(self.loc0[:, 0] >= 0, case.actions[t], 0).astype(np.int64)
        board1 = self.board0.copy()
        locs = np.ascontiguousarray(np.maximum(self.loc0, 0)[:, None, :], dtype=np.int64)
        oracle.execute_actions_batch(board1, locs, acts[:, None])
        self.loc1 = loc1 = locs[:, 0]
        moved = acts != 0
        (y0, x0), (y1, x1) = self.loc0.T, loc1.T
        for name, hit in (("row 0 -> H-1", (y0 == 0) & (y1 == H - 1)), ("row H-1 -> 0", (y0 == H - 1) & (y1 == 0)),
                          ("col 0 -> W-1", (x0 == 0) & (x1 == W - 1)), ("col W-1 -> 0", (x0 == W - 1) & (x1 == 0))):
            if (hit & moved).any():
                self.crossings.add(name)
        self.stood |= {int(x) - (WS - 1) for x in np.unique(x1[moved]) if x in (WS - 1, WS)}
        changed = board1 != self.board0
        edits = changed[:, :, [0, WS - 1, WS, W - 1]].copy()
        for e in np.nonzero((acts >= 5) & np.isin(x0, (0, WS - 1, WS, W - 1)))[0]:
            edits[e, y0[e], (0, WS - 1, WS, W - 1).index(x0[e])] = False      # (the agent's own cell: its orientation)
        self.seam_edits += int(edits[acts >= 5].any(axis=(1, 2)).sum())
        was, now = self.board0 == CT.crate, board1 == CT.crate
        for e in np.nonzero((was != now).any(axis=(1, 2)))[0]:
            src, dst = np.argwhere(was[e] & ~now[e]), np.argwhere(now[e] & ~was[e])
            if len(src) == 1 and len(dst) == 1:
                (ya, xa), (yb, xb) = src[0], dst[0]
                if {int(xa), int(xb)} == {WS - 1, WS}:
                    self.pushes.add("row seam")
                if (ya, yb) == (H - 1, 0):
                    self.pushes.add("row H-1 -> 0")
        if case.wrapped:        # the movement term of the step to come (env_wrappers.py:67-92), from the deque before it
            wa, w = cpu.env.wa, cpu.env.w
            has = self.loc0[:, 0] >= 0
            dist = np.abs(loc1 - wa["prior"][:, 0]).sum(axis=1) + np.maximum(w.move_period - wa["n_prior"], 0)
            self.move_terms |= set(wa["move_table"][dist[has]].tolist())

    def after(self, t, reward, done):
        case, cpu = self.case, self.cpu
        d = done.astype(bool)
        self.ends += d
        self.n_success += int((cpu.get("success")[d] != 0).sum())
        self.n_times_up += int(((cpu.get("times_up")[d] != 0) & (cpu.get("success")[d] == 0)).sum())
        self.max_ends_in_a_step = max(self.max_ends_in_a_step, int(d.sum()))
        self.env_steps += case.B
        if case.wrapped:
            self.shaped_differs += int((cpu.get("shaped_reward") != reward.astype(np.float64)).sum())
            self.side_effect_seen |= bool((cpu.env.wa["last_side_effect"] != 0).any())
        on = (self.level0 == smc.EVOLVING_LEVEL) & ~d
        if on.any() and (cpu.get("goals")[on] != self.goals0[on]).any():
            self.goals_changed = True


def _run(case):
    pool = case.pool(util.oracle_counts)
    cpu = util.OracleBackend(pool, case.B, **case.backend_kw(device=False))
    run = smc.OracleRun(case, cpu, finished=bool(case.queue_capacity))
    cov = Coverage(case, cpu)
    cpu.env.reset()
    still, drew = None, np.zeros(case.B, bool)
    if case.spawn == "spawn":       # the same actions on the pool without its spawners: no draw is ever consumed there
        twin = smc.Case(case.H, (case.tables, "still", case.front), batch=case.batch, queue=bool(case.queue_capacity),
                        W=case.W, family=case.family, big_view=case.big_view)
        still = util.OracleBackend(twin.pool(util.oracle_counts), case.B, **case.backend_kw(device=False))
        still.env.reset()
    for t in range(case.n_steps):
        cov.before(t)
        _, r, d = run.step()
        cov.after(t, r, d)
        if still is not None:
            still.env.step(case.actions[t])
            drew |= (cpu.get("rng") != still.get("rng")).any(axis=1) & ~d.astype(bool)
        if t == case.reset_at:
            cpu.env.reset(case.reset_mask)
            if still is not None:
                still.env.reset(case.reset_mask)
    return cov, drew


@pytest.mark.parametrize("H,cfg", smc.all_cases(), ids=[smc.case_id(H, cfg) for H, cfg in smc.all_cases()])
def test_case_exercises_what_it_claims(H, cfg):
    case = smc.Case(H, cfg)
    assert 5 <= case.time_limit <= 9 and case.B == 2 * smc.EXPECTED_NB[H] + 1 <= 65
    _assert_coverage(case, *_run(case))


def _assert_coverage(case, cov, drew):
    """The coverage conditions of a main-batch case (also those of the size-generic matrix, tests/test_step_generic_host.py)."""
    B, NB = case.B, case.geom["NB"]
    assert cov.crossings == {"row 0 -> H-1", "row H-1 -> 0", "col 0 -> W-1", "col W-1 -> 0"}, cov.crossings
    assert cov.stood == {0, 1}, "the agents stood on columns WS-1 and WS"
    assert cov.seam_edits >= 1
    assert cov.pushes == {"row seam", "row H-1 -> 0"}, cov.pushes
    assert cov.n_success >= 1 and cov.n_times_up >= 1
    assert cov.ends.sum() >= 2 * B
    assert cov.ends[B - 1] >= 1 and cov.ends[NB - 1] >= 1, "the tail env and the last env of the first workgroup"
    assert cov.goals_changed, "the evolving-goal level"
    if case.spawn == "spawn":
        assert drew.sum() * 2 >= B, "draws consumed by %d of %d envs" % (drew.sum(), B)
    if case.wrapped:
        assert cov.shaped_differs * 4 >= cov.env_steps, (cov.shaped_differs, cov.env_steps)
        assert cov.side_effect_seen
        assert len(cov.move_terms) >= 2, cov.move_terms
    if case.queue_capacity:
        assert cov.max_ends_in_a_step > case.queue_capacity, "the queue never overflows"


@pytest.mark.parametrize("H", [H for H in smc.SHAPES if smc.geometry(H, H)["lean_takes_queue"]])
def test_plain_case_with_a_queue_overflows_it(H):
    """The wide shapes' plain kernels also serve a finished-episode queue: the plain cases run once more with one."""
    for cfg in smc.CONFIGS[:4]:
        case = smc.Case(H, cfg, queue=True)
        cov, _ = _run(case)
        assert case.queue_capacity and cov.max_ends_in_a_step > case.queue_capacity


@pytest.mark.parametrize("H", smc.SHAPES)
def test_small_and_sliced_batches_follow_the_schedule(H):
    """The extra batches of the device tests (NB - 1 envs: a last wave that is not full; 129 envs: two slices) play the
    same scripts: the oracle follows the builder's schedule there too and episodes end in every env."""
    for case in (smc.Case(H, ("many", "spawn", "wrap"), batch="small"),
                 smc.Case(H, ("one", "spawn", "plain"), B=129, n_steps=12)):
        cov, _ = _run(case)
        assert cov.ends.min() >= 1
