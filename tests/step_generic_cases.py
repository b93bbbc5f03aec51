"""The matrix of the size-generic single-agent kernels (k_env_rollout_generic, k_env_reset_generic, k_env_obs_generic,
k_inaction_generic of sl_generic.hip): which shapes, which configurations on each, the row-kernel shapes that fall back
to the family, and the hand-made pools of the smallest boards.  tests/test_step_generic_host.py asserts on the oracle
alone that the cases exercise what they claim, tests/test_step_generic_gpu.py runs them on the device.

The shapes are the smallest that sit on each edge of the family (cells; threads per workgroup by
step_matrix_cases.generic_threads; passes = ceil(cells / threads), one eligibility bit of ca_step_block's 64-bit mask each):

    7x11      77   64  smallest the builder supports with margin
    15x17    255   64  one below the class edge
    4x64     256   64  on the class edge: four full passes, 64-cell rows
    13x20    260  128  first class change, ragged last pass
    31x33   1023  128  one below the class edge
    16x64   1024  128  on the class edge
    25x41   1025  256  first above the class edge
    64x5     320  128  tall and thin (the row index from a float reciprocal, W = 5)
    5x64     320  128  long and thin
    100x100 10000 256  40 passes: more than 32 mask bits
    127x129 16383 256  LDS rounding of an odd cell count; W = 129
    128x128 16384 256  SL_MAX_CELLS: all 64 mask bits, 131 200 bytes of LDS
"""
import numpy as np

from safelife_amd.cell_types import CellTypes as CT, DEFAULT_POINTS_TABLE
from safelife_amd.levels import Level, LevelPool
from tests import step_matrix_cases as smc

# (H, W) -> (threads, passes), written out: the rule of smc.generic_threads must give exactly these
SHAPES = {(7, 11): (64, 2), (15, 17): (64, 4), (4, 64): (64, 4), (13, 20): (128, 3), (31, 33): (128, 8), (16, 64): (128, 8),
          (25, 41): (256, 5), (64, 5): (128, 3), (5, 64): (128, 3), (100, 100): (256, 40), (127, 129): (256, 64),
          (128, 128): (256, 64)}
ALL_CONFIGS_ON = ((7, 11), (13, 20), (25, 41))          # one shape per thread class takes all twelve configurations
# the others take four: plain, queue + observation, starting-state wrappers, the inaction baseline
FOUR = (("one", "spawn", "plain"), ("many", "still", "obs"), ("one", "still", "wrap"), ("many", "spawn", "wrap"))
BIG_VIEW_ON = ((127, 129), (128, 128))                  # there the "obs" configuration keeps a view larger than the board
B_MAIN = 17


def all_cases():
    return [(H, W, cfg) for (H, W) in SHAPES for cfg in (smc.CONFIGS if (H, W) in ALL_CONFIGS_ON else FOUR)]


def case_id(H, W, cfg):
    return smc.case_id(H, cfg, W)


def case(H, W, cfg, **kw):
    kw.setdefault("big_view", (H, W) in BIG_VIEW_ON and cfg[2] == "obs")
    return smc.Case(H, cfg, W=W, family="generic", **kw)


# ---------------------------------------------------------------------------------------------- row shapes that fall back

FALLBACKS = ("nine-exits", "wide-points", "wide-policy-view")


def fallback_case(kind, changed=True):
    """A batch of a row-kernel shape that use_rowlane() sends to the size-generic family (changed=False: the same batch
    without the one change, which the row kernels must take):
      nine-exits        25x25, a ninth exit on the eight-exit level (more than 8 exit slots), with the inaction baseline;
      wide-points       25x25, the two levels with tables of their own score -300..300 (entries outside int8), with a queue;
      wide-policy-view  64x64, policy_layout="uint8" on a 40x40 view (more than the fused policy-layout epilogue stages)."""
    assert kind in FALLBACKS
    if kind == "nine-exits":
        c = smc.Case(25, ("one", "spawn", "wrap"))
        if changed:
            lv = c.levels[2]
            assert len(lv.exit_locs) == 8
            board = lv.board.copy()
            y, x = 25 // 2 + 3, c.geom["WS"]                # an empty cell no script of that level reaches
            assert board[y, x] == 0
            board[y, x] = CT.level_exit
            c.levels[2] = Level(board, lv.goals, lv.agent_locs, spawn_prob=lv.spawn_prob, min_performance=lv.min_performance,
                                points_table=lv.points_table, rng_words=lv.rng_words)
            assert len(c.levels[2].exit_locs) == 9
    elif kind == "wide-points":
        c = smc.Case(25, ("many", "still", "obs"))
        if changed:
            for k in (2, 5):
                lv = c.levels[k]
                c.levels[k] = Level(lv.board, lv.goals, lv.agent_locs, spawn_prob=lv.spawn_prob,
                                    min_performance=lv.min_performance, points_table=lv.points_table * 100,
                                    rng_words=lv.rng_words)
    else:
        c = smc.Case(64, ("one", "still", "obs"))
        c.kw.update(view_shape=(40, 40), output_channels=smc.CHANNELS_15)
        c.policy_layout = "uint8" if changed else None
    return c


# ---------------------------------------------------------------------------------------------- the floor: 3x3 and 3x86

FLOOR_SHAPES = ((3, 3), (3, 86))
FLOOR_STEPS, FLOOR_TIME_LIMIT, FLOOR_B, FLOOR_RESET_AT = 20, 7, 9, 11
FLOOR_VIEW = (5, 7)                     # larger than the 3x3 board
# a fixed action for every (level, step of the run); moves 1-4, create / destroy / shove 5-8 (up, right, down, left)
FLOOR_SCRIPTS = ((2, 5, 3, 7, 4, 4, 1, 6, 2, 8, 3, 3, 5, 1, 4, 7, 2, 6, 0, 8),
                 (4, 6, 1, 8, 2, 2, 3, 5, 4, 7, 1, 1, 6, 3, 2, 8, 4, 5, 0, 7),
                 (0, 4, 4, 2, 0, 4, 3, 4, 0, 1, 4, 2, 4, 0, 4, 4, 3, 0, 4, 4),
                 (0,) * 20)
FLOOR_OPEN_EXIT_LEVEL, FLOOR_SPAWNER_LEVEL, FLOOR_AGENTLESS_LEVEL = 2, 1, 3


def floor_levels(H, W):
    """Four levels of the smallest boards, written out cell by cell:
      0: agent on (0, 0); a shut exit on (2, W-1); a row of three live cells over the column seam W-1 | 0 | 1;
      1: agent on (0, W-1); a green spawner on (2, 1) (spawn_prob 0.9) and a goal cell next to it;
      2: agent on (1, 0) facing an exit that is open from the reset and lies across the seam, on (1, W-1);
      3: no agent; a column of live cells over the row seam 2 | 0 | 1; one exit."""
    assert H == 3 and W >= 3
    green, life = CT.color_g, CT.life | CT.color_g
    out = []

    def level(k, board, goals, loc, min_performance, spawn_prob=0.3):
        if loc is not None:
            board[loc] = CT.player | green
        out.append(Level(board, goals, None if loc is None else [loc], spawn_prob=spawn_prob, min_performance=min_performance,
                         points_table=DEFAULT_POINTS_TABLE[None],
                         rng_words=[0xA5A5A5A5DEADBEEF ^ (k * 0x10001), 0x0123456789ABCDEF + 7 * k, 0, 2 * (W * 17 + k) + 1]))

    def blank():
        goals = np.zeros((H, W), np.uint16)
        goals[1, 1] = goals[2, 0] = green
        goals[0, W - 2] = CT.color_b
        return np.zeros((H, W), np.uint16), goals

    b, g = blank()
    b[1, W - 1] = b[1, 0] = b[1, 1] = life
    b[2, W - 1] = CT.level_exit
    level(0, b, g, (0, 0), 0.5)
    b, g = blank()
    b[2, 1] = CT.spawner | green
    level(1, b, g, (0, W - 1), 0.5, spawn_prob=0.9)
    b, g = blank()
    b[1, W - 1] = CT.level_exit
    level(2, b, g, (1, 0), -1.0)
    b, g = blank()
    b[2, W // 2] = b[0, W // 2] = b[1, W // 2] = life
    b[0, 0] = CT.level_exit
    level(3, b, g, None, 0.5)
    return out


def floor_pool(H, W, counts_fn):
    return LevelPool(floor_levels(H, W), counts_fn=counts_fn, min_performance_fraction=1.0)


def floor_kw():
    e = np.arange(FLOOR_B)
    return dict(auto_reset=True, level_stride=1, time_limit=FLOOR_TIME_LIMIT, view_shape=FLOOR_VIEW, output_channels=None,
                first_level=((e + e // 4) % 4).astype(np.int32))


def floor_actions(level_idx, t):
    """The run's actions at step t: every env plays its current level's script."""
    return np.array([FLOOR_SCRIPTS[int(l) % 4][t] for l in level_idx], np.int32)


FLOOR_RESET_MASK = (np.arange(FLOOR_B) % 2 == 0).astype(np.uint8)
