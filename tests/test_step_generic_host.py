"""The cases of the size-generic matrix (tests/step_generic_cases.py, built by tests/step_matrix_cases.py) do what they
claim: every (shape, configuration) that tests/test_step_generic_gpu.py runs on the device is run here on the ORACLE alone,
under the coverage conditions of tests/test_step_matrix_host.py, unchanged.  Also: the builder still makes the fourteen
row-kernel shapes' cases byte for byte, and the hand-made 3x3 / 3x86 pools exercise what they say.  No GPU.
"""
import hashlib

import numpy as np
import pytest

from safelife_amd.cell_types import CellTypes as CT
from tests import step_generic_cases as sgc
from tests import step_matrix_cases as smc
from tests import test_step_matrix_host as host
from tests import util

ALL = sgc.all_cases()

# blake2b-128 over every case of a row-kernel shape -- the twelve configurations, the small batch and the two-slice batch:
# the levels (board, goals, agent, table, generator words, spawn_prob, min_performance), first_level, schedule, actions,
# reset mask and env keywords -- computed BEFORE the builder learnt rectangular boards and the generic family.
ROW_CASE_DIGESTS = {
    25: "ad787fa6bed0be65fdb992f938153a03",
    26: "77c6cb9629c422df13761fc813b89f0d",
    64: "71c83e720269b36cfac8af341f653981",
    24: "91164c26319710b94b0f1259b4c50519",
    15: "3f87b6470a7d88f182e9d90dba581f75",
    20: "afc8c16351cc35209c4703c7f2514258",
    10: "6a9dca00e44ac70170a260392b78636b",
    8: "a7e2bf0f7a423558b242e676e2b7efc5",
    12: "385d2779f15a07916b9a2b73f053c6a9",
    16: "cd7eaae6021f098385f11ffc66c987f4",
    30: "0731dedfd6cd8949ced97d6007c037a1",
    32: "4a620e04c61773e79df6662a8f9b73d7",
    40: "28e338533846fd861d17424c129f26f1",
    48: "e25d857a68c90c0771d519fd8b30d216",
}


def _row_case_digest(H):
    h = hashlib.blake2b(digest_size=16)
    cases = [smc.Case(H, cfg) for cfg in smc.CONFIGS]
    cases += [smc.Case(H, ("many", "spawn", "wrap"), batch="small"), smc.Case(H, ("one", "spawn", "plain"), B=129, n_steps=12)]
    for c in cases:
        for lv in c.levels:
            for a, dt in ((lv.board, np.uint16), (lv.goals, np.uint16), (lv.agent_locs, np.int64), (lv.points_table, np.int64),
                          (lv.rng_words, np.uint64), (lv.spawn_prob, np.float64), (lv.min_performance, np.float64)):
                h.update(np.ascontiguousarray(a, dtype=dt).tobytes())
        for a, dt in ((c.first_level, np.int32), (c.schedule, np.int32), (c.actions, np.int32), (c.reset_mask, np.uint8)):
            h.update(np.ascontiguousarray(a, dtype=dt).tobytes())
        h.update(repr((c.B, c.time_limit, c.reset_at, c.queue_capacity, c.policy_layout,
                       sorted((k, v) for k, v in c.kw.items() if k != "wrappers"))).encode())
    return h.hexdigest()


@pytest.mark.parametrize("H", smc.SHAPES)
def test_row_shapes_cases_are_unchanged(H):
    assert sorted(ROW_CASE_DIGESTS) == sorted(smc.SHAPES)
    assert _row_case_digest(H) == ROW_CASE_DIGESTS[H]


def test_thread_rule_gives_the_classes_the_shapes_were_chosen_for():
    assert len(sgc.SHAPES) == 12 and len(ALL) == 3 * 12 + 9 * 4
    for (H, W), (threads, passes) in sgc.SHAPES.items():
        g = smc.generic_geometry(H, W)
        assert (g["threads"], g["passes"], g["NB"], g["WS"]) == (threads, passes, 1, (W + 1) // 2), (H, W)
        assert H * W <= 128 * 128 and passes <= 64              # (SL_MAX_CELLS; one bit of a 64-bit mask per pass)
    assert [smc.generic_threads(n) for n in (1, 256, 257, 1024, 1025, 16384)] == [64, 64, 128, 128, 256, 256]
    cells = sorted(H * W for H, W in sgc.SHAPES)
    assert {255, 256, 260, 1023, 1024, 1025, 16383, 16384} <= set(cells)
    assert max(p for _, p in sgc.SHAPES.values()) == 64 and any(32 < p < 64 for _, p in sgc.SHAPES.values())
    assert {W for _, W in sgc.SHAPES} >= {5, 64, 129}           # the row index from a float reciprocal: thin and wide rows
    assert set(sgc.FOUR) <= set(smc.CONFIGS) and {c[2] for c in sgc.FOUR} == {"plain", "obs", "wrap"}
    assert sum(c[2] == "wrap" and c[1] == "spawn" for c in sgc.FOUR) == 1      # the inaction baseline


@pytest.mark.parametrize("H,W", [s for s in sgc.SHAPES if s[0] >= 7])
def test_generic_pools_hold_every_constructed_item(H, W):
    """(Not 4x64 and 5x64: on four or five rows some of the exits land on one another and on the glider.  Those two are
    in the matrix for their 64-cell rows, and meet the coverage conditions like every other shape.)"""
    host._pool_items(H, W)


@pytest.mark.parametrize("H,W,cfg", ALL, ids=[sgc.case_id(*c) for c in ALL])
def test_generic_case_exercises_what_it_claims(H, W, cfg):
    case = sgc.case(H, W, cfg)
    assert 5 <= case.time_limit <= 9 and case.B == sgc.B_MAIN and (case.H, case.W) == (H, W)
    e = np.arange(case.B)
    assert np.array_equal(case.first_level, (e + e // 8) % 8)
    pool = case.pool(util.oracle_counts)
    assert pool.shape == (H, W) and 6 <= pool.exit_slots <= 8 and (pool.exit_slots == 8 or H < 7) and np.abs(pool.points_table).max() <= 127
    assert pool.has_spawner == (cfg[1] == "spawn") and (pool.points_table.shape[0] == 1) == (cfg[0] == "one")
    assert case.inaction == (cfg[1:] == ("spawn", "wrap"))
    if cfg[2] == "obs":
        vh, vw = case.kw["view_shape"]
        if (H, W) in sgc.BIG_VIEW_ON:
            assert vh > H and vw > W and case.kw["output_channels"] is None
        combo_has_queue = (cfg[0] == "many") != (cfg[1] == "spawn")
        assert bool(case.queue_capacity) == combo_has_queue
        assert case.queue_raw == (H * W > smc.GENERIC_QUEUE_MAX_CELLS)
    host._assert_coverage(case, *host._run(case))


def test_extra_batches_follow_the_schedule():
    """B = 1 and B = 129 at 13x20 (one slice; two slices), the compact-record and stream batches: the oracle follows the
    builder's schedule and episodes end in every env."""
    for case in (sgc.case(13, 20, ("one", "spawn", "plain"), B=1, n_steps=12),
                 sgc.case(13, 20, ("one", "spawn", "plain"), B=129, n_steps=12),
                 sgc.case(7, 11, ("many", "spawn", "plain"))):
        cov, drew = host._run(case)
        assert cov.ends.min() >= 1
        assert case.B == 1 or drew.sum() * 2 >= case.B


@pytest.mark.parametrize("kind", sgc.FALLBACKS)
def test_fallback_cases_exercise_what_they_claim(kind):
    """The row-kernel shapes sent to the generic family: the one change is there, it is the only one, and the case still
    meets the coverage conditions."""
    case, plain = sgc.fallback_case(kind), sgc.fallback_case(kind, changed=False)
    pool, pool0 = case.pool(util.oracle_counts), plain.pool(util.oracle_counts)
    assert np.array_equal(case.actions, plain.actions) and np.array_equal(case.schedule, plain.schedule)
    assert pool0.exit_slots == 8 and np.abs(pool0.points_table).max() <= 127
    if kind == "nine-exits":
        assert pool.exit_slots == 9 and case.inaction
    elif kind == "wide-points":
        assert pool.exit_slots == 8 and np.abs(pool.points_table).max() == 300 and np.abs(pool.points_table).min() == 0
        assert case.queue_capacity
    else:
        assert case.policy_layout == "uint8" and plain.policy_layout is None
        assert case.kw["view_shape"] == (40, 40) == plain.kw["view_shape"]
        assert (case.H, case.W) == (64, 64)
    host._assert_coverage(case, *host._run(case))


@pytest.mark.parametrize("H,W", sgc.FLOOR_SHAPES)
def test_floor_pools_exercise_what_they_claim(H, W):
    """3x3 and 3x86 on the oracle: successes, time-limit ends, an env that is done at every step, draws on the spawner
    level, life that changes over the seams, creations that score, and resets of both kinds.  (On 3x3 every cell is a
    neighbour of every other, the agent's included, and nothing is born next to an agent: no draw is consumed there while
    an agent is on the board.)"""
    levels = sgc.floor_levels(H, W)
    assert [len(lv.agent_locs) for lv in levels] == [1, 1, 1, 0] and [len(lv.exit_locs) for lv in levels] == [1, 0, 1, 1]
    assert sum(bool((lv.board & CT.spawning).any()) for lv in levels) == 1
    alive = [(lv.board & (CT.alive | CT.frozen)) == CT.alive for lv in levels]
    assert alive[0][1, W - 1] and alive[0][1, 0] and alive[0][1, 1] and alive[3][:, W // 2].all()
    pool = sgc.floor_pool(H, W, util.oracle_counts)
    kw = sgc.floor_kw()
    cpu = util.OracleBackend(pool, sgc.FLOOR_B, **kw)
    cpu.env.reset()
    assert np.array_equal(cpu.get("level_idx"), kw["first_level"]) and set(kw["first_level"]) == {0, 1, 2, 3}
    n_success = n_times_up = 0
    ends = np.zeros(sgc.FLOOR_B, np.int64)
    rewards, drew, changed, loaded = set(), False, False, set()
    for t in range(sgc.FLOOR_STEPS):
        level, board0, rng0 = cpu.get("level_idx"), cpu.get("board"), cpu.get("rng")
        _, r, d = cpu.env.step(sgc.floor_actions(level, t))
        d = d.astype(bool)
        ends += d
        n_success += int((cpu.get("success")[d] != 0).sum())
        n_times_up += int(((cpu.get("times_up")[d] != 0) & (cpu.get("success")[d] == 0) & (level[d] != 3)).sum())
        assert d[level == sgc.FLOOR_AGENTLESS_LEVEL].all()
        rewards |= set(r.tolist())
        on = (level == sgc.FLOOR_SPAWNER_LEVEL) & ~d
        drew |= bool((cpu.get("rng")[on] != rng0[on]).any())
        changed |= bool((cpu.get("board")[(level == 0) & ~d] != board0[(level == 0) & ~d]).any())
        loaded |= {(int(l), "auto") for l in cpu.get("level_idx")[d]}
        if t == sgc.FLOOR_RESET_AT:
            cpu.env.reset(sgc.FLOOR_RESET_MASK)
            loaded |= {(int(l), "masked") for l in cpu.get("level_idx")[sgc.FLOOR_RESET_MASK != 0]}
    assert n_success >= 2 and n_times_up >= 2 and ends.min() >= 1
    assert drew == (W > 3) and changed and len(rewards) >= 3, rewards
    assert {l for l, how in loaded if how == "auto"} == {0, 1, 2, 3} and len({l for l, how in loaded if how == "masked"}) >= 2
