"""Boards that make an EXACT number of random draws in a CA step, and the model of which algorithm deals those draws
(tests/test_draw_deal_host.py asserts both on the oracle alone; tests/test_draw_deal_gpu.py runs the cases on the device).

A spawner board's CA step makes one PCG64 draw per eligible cell, in row-major order (`eligible` below; the oracle's
ca_step, advance_board.c:94-124).  The kernels deal these draws in different ways, chosen by the number of draws the boards
of a wavefront make in the step (`regime` below; resolve_draws_planes, resolve_draws and ca_step in sl_rowlane.hip,
ca_step_block in sl_generic.hip):

    g1:rounds1..8   one board per wave (40, 48, 64 rows), 1..512 draws: round by round, ceil(total / 64) rounds
    g1:block4       one board per wave, 513..1024: blocked deal, 16 draws per lane, two lanes per outcome dword
    g1:block5       one board per wave, 1025..2048: blocked deal, 32 draws per lane
    g1:rows         one board per wave, more than 2048: row by row
    g2:rounds1..4   two boards per wave (24, 25, 26, 32 rows), the larger of the two counts 1..128: round by round on
                    32-lane halves, ceil(max / 32) rounds
    g2:rows         two boards per wave, the larger count above 128: row by row
    rows            three or more boards per wave (8..20 rows): row by row
    word            the word form (30x30: rows that are not kept as bit planes): row by row, resolve_draws
    generic         the size-generic kernels: a prefix count over ballots and a table jump per cell
    none            no board of the wave draws: the resolver is not entered (not a path of its own; kept apart so that the
                    cases with zero draws are not counted for a regime)

Which boards share a wave: a 256-thread workgroup owns NB = 4 G consecutive boards of the batch and wave w of it the G
boards from 4 G blockIdx + G w on (`gb = wave * G + g`, k_advance_rowlane; the one-wave kernels k_advance_small and the
occupancy kernel take boards G blockIdx + g), so board G k + g of a batch is board g of wave k -- every batch of these
tests starts at board 0.

The lattice: spawners on the cells y = 1, x = 1 (mod 3).  Their 3x3 neighbourhoods are disjoint, every spawner adds the
eight cells around it, and a wall on an eligible cell removes exactly that one draw (a wall is frozen, neither alive nor
spawning nor inhibiting: no neighbour's rule changes) -- so any count up to the full lattice's is reached exactly.

Regimes reached per shape and entry point, as tests/test_draw_deal_host.py measures them (it asserts these sets, and for
advance and the fused step already at step 0, where the counts are the cases' own):

    shape             advance n = 1, n = 3, each        occupancy, 12 steps at p = 0       fused step (plain, wrappers)
    64x64             g1:rounds1-8 block4 block5 rows   the same                           the same
    48x48             g1:rounds1-8 block4 block5        the same                           --
    40x40             g1:rounds1-8 block4 block5        the same                           the same
    24, 25, 26, 32    g2:rounds1-4 g2:rows              25, 26, 32: the same               25x25: the same
    30x30             word                              --                                 word
    20x20             rows                              --                                 --
    31x33, 128x128    generic                           --                                 31x33: generic

(48x48 and 40x40 have no g1:rows: their full lattices make 2048 and 1352 draws.)  Occupancy across regime changes
(TRANSITIONS below), 64x64: rows <-> block4, block4 <-> block5, block4 <-> rounds8, rows <-> rounds6, rows -> none -> rows
-> rounds1, block5 -> rounds8; 40x40 and 48x48: block5 -> rounds, rounds8 <-> block4; 25, 26, 32: g2:rounds4 <-> g2:rows.
"""
import numpy as np

from safelife_amd.cell_types import CellTypes as CT
from tests import step_matrix_cases as smc

P_CYCLE = (0.0, 0.5, 1.0, 0.3)          # spawn_prob of board b of a batch: P_CYCLE[(b + rot) % 4]
FULL = None                             # a target: the whole lattice

ROUNDS_1 = 8                            # MAXR of resolve_draws_planes
ROUNDS_2 = 4                            # STRIDE_ROUNDS2


def eligible(board):
    """bool [..., H, W]: the cells that make a draw in the next CA step -- dead, not frozen, no inhibiting cell in the
    3x3, an alive count other than 3, a spawning cell in the 3x3 (the board is a torus)."""
    b = np.asarray(board, np.uint16)
    alive = np.zeros(b.shape, np.int32)
    inhibit = np.zeros(b.shape, bool)
    spawn = np.zeros(b.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            n = np.roll(b, (dy, dx), axis=(-2, -1))
            alive += (n & CT.alive) != 0
            inhibit |= (n & CT.inhibiting) != 0
            spawn |= (n & CT.spawning) != 0
    return ((b & (CT.alive | CT.frozen)) == 0) & ~inhibit & (alive != 3) & spawn


def draws(board):
    """Draws of the next step, per board: int [...]."""
    return eligible(board).sum(axis=(-2, -1))


def lattice(H, W):
    """The lattice sites in row-major order."""
    return [(y, x) for y in range(1, H, 3) for x in range(1, W, 3)]


def _colour(rng):
    return int(rng.integers(0, 8)) << 9


def make_board(H, W, target, rng, agent=None):
    """A board of exactly `target` draws (FULL: the whole lattice): spawners of random colours on the lattice in row-major
    order until the count reaches the target, then walls on the last eligible cells that are too many.  agent: the cell
    of a player, placed first -- it inhibits its 3x3, and the count is taken with it in place."""
    board = np.zeros((H, W), np.uint16)
    if agent is not None:
        board[agent] = CT.player | CT.color_g
    sites = [s for s in lattice(H, W) if s != agent]
    cells = [CT.spawner | _colour(rng) for _ in sites]

    def with_sites(k):
        b = board.copy()
        for (y, x), c in zip(sites[:k], cells[:k]):
            b[y, x] = c
        return b

    if target is FULL:
        return with_sites(len(sites))
    lo, hi = 0, len(sites)              # the count grows with every site: the fewest sites that reach the target
    assert draws(with_sites(hi)) >= target, "%dx%d cannot make %d draws" % (H, W, target)
    while lo < hi:
        mid = (lo + hi) // 2
        if draws(with_sites(mid)) >= target:
            hi = mid
        else:
            lo = mid + 1
    b = with_sites(lo)
    el = np.flatnonzero(eligible(b))
    over = len(el) - target
    if over:
        b.reshape(-1)[el[len(el) - over:]] = CT.wall
    assert draws(b) == target
    return b


def make_full_row_board(n_spawner_rows, rng):
    """64x64 with rows in which ALL 64 cells draw: the plain lattice leaves column 63 out (64 = 3 * 21 + 1), so the first
    `n_spawner_rows` spawner rows also carry a spawner in column 63 -- the rows above and below them are full, 170 draws
    per spawner row in all."""
    b = np.zeros((64, 64), np.uint16)
    for y in range(1, 1 + 3 * n_spawner_rows, 3):
        for x in list(range(1, 64, 3)) + [63]:
            b[y, x] = CT.spawner | _colour(rng)
    return b


def full_rows(board):
    """(row, draws made before it in the step) of every row whose cells all draw."""
    el = eligible(board)
    per_row = el.sum(axis=1)
    before = np.concatenate([[0], np.cumsum(per_row)[:-1]])
    return [(int(y), int(before[y])) for y in np.flatnonzero(per_row == board.shape[1])]


# ---------------------------------------------------------------------------------------------- the regime model

def family(H, W):
    """"row" (a shape with row kernels) or "generic"."""
    return "row" if H == W and H in smc.SHAPES else "generic"


def planes(W):
    """use_planes() of sl_rowlane.hip:980-984, restated: rows of up to 28 cells, of 64, and even rows of 32 to 62."""
    return (W + 1) // 2 + 2 <= 16 or W == 64 or (32 <= W < 64 and W % 2 == 0)


def boards_per_wave(H, W):
    return smc.geometry(H, W)["G"]


def regime(H, W, totals):
    """The label of the path that deals a wave's draws; totals: the draw counts of the boards of ONE wave (its G boards,
    fewer in a batch's last wave).  sl_rowlane.hip: ca_step :991-1004 (planes or words), resolve_draws_planes :739 and
    :761 (rounds, one board), :825-828 (blocked), :875-883 (two boards), :944 (row by row)."""
    totals = [int(t) for t in totals]
    if family(H, W) == "generic":
        return "generic" if max(totals) > 0 else "none"
    if max(totals) == 0:
        return "none"
    if not planes(W):
        return "word"
    G = boards_per_wave(H, W)
    assert 1 <= len(totals) <= G
    if G == 1:
        total = totals[0]
        if total <= 64 * ROUNDS_1:
            return "g1:rounds%d" % ((total + 63) // 64)
        if total <= 32 * 64:
            need = (total + 63) // 64
            return "g1:block%d" % (need - 1).bit_length()           # log2c: 16 or 32 draws per lane
        return "g1:rows"
    if G == 2:
        tmax = max(totals)
        if tmax <= 32 * ROUNDS_2:
            return "g2:rounds%d" % ((tmax + 31) // 32)
        return "g2:rows"
    return "rows"


def wave_regimes(H, W, totals):
    """The labels of the waves of a batch whose boards make `totals` draws."""
    G = boards_per_wave(H, W) if family(H, W) == "row" else 1
    return [regime(H, W, totals[k:k + G]) for k in range(0, len(totals), G)]


def reachable(H, W):
    """Every label a shape can reach ("none" left out)."""
    if family(H, W) == "generic":
        return {"generic"}
    if not planes(W):
        return {"word"}
    G = boards_per_wave(H, W)
    if G == 1:
        out = {"g1:rounds%d" % r for r in range(1, ROUNDS_1 + 1)} | {"g1:block4", "g1:block5"}
        if int(draws(make_board(H, W, FULL, np.random.default_rng(0)))) > 2048:
            out.add("g1:rows")          # (not 48x48: its full lattice makes 2048 draws)
        return out
    if G == 2:
        return {"g2:rounds%d" % r for r in range(1, ROUNDS_2 + 1)} | {"g2:rows"}
    return {"rows"}


# ---------------------------------------------------------------------------------------------- the case list

# one board per wave: draw counts at step 0 (behind the `+`: both sides of every 64 r, so that each shape reaches each
# number of rounds at step 0, whatever the later steps do)
LOWER_ROUNDS = (1, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449)
TARGETS_1 = {
    64: (0, 1, 63, 64, 65, 448, 449, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3000, FULL) + LOWER_ROUNDS[3:13],
    40: (512, 513, 1024, 1025, FULL) + LOWER_ROUNDS,
    48: (512, 513, 1024, 1025, 2047, 2048) + LOWER_ROUNDS,
}
FULL_ROW_BOARDS = (1, 3, 4, 7, 12)      # spawner rows of the 64x64 boards with full-width rows: 170 draws each
# two boards per wave: (board 0, board 1) of a wave, and a last wave that holds one board
PAIRS_2 = ((0, 1), (1, 0), (31, 32), (32, 33), (33, 0), (64, 65), (96, 97), (127, 128), (128, 128), (128, 129), (129, 0),
           (0, 129), (129, 129), (FULL, FULL))
LAST_SINGLE = 97
SHAPES_2 = (25, 26, 24, 32)
TARGETS_WORD = (1, 29, 129, FULL, 97)   # 30x30 (two boards per wave, word form; five boards: a last wave of one)
TARGETS_ROWS = (FULL, 0, 100, FULL)     # 20x20 (three boards per wave; four boards: a last wave of one)
TARGETS_GENERIC = {(31, 33): (300, FULL, 0), (128, 128): (300, FULL, 9000)}

ADVANCE_SHAPES = [(H, H) for H in (64, 40, 48) + SHAPES_2 + (30, 20)] + sorted(TARGETS_GENERIC)
OCCUPANCY_SHAPES = (64, 48, 40, 25, 26, 32)
STEP_SHAPES = ((25, 25), (64, 64), (40, 40), (30, 30), (31, 33))


def targets_of(H, W):
    if (H, W) in TARGETS_GENERIC:
        return TARGETS_GENERIC[(H, W)]
    if H in TARGETS_1:
        return TARGETS_1[H]
    if H in SHAPES_2:
        return tuple(t for pair in PAIRS_2 for t in pair) + (LAST_SINGLE,)
    return {30: TARGETS_WORD, 20: TARGETS_ROWS}[H]


def rng_words(seed, B):
    """uint64 [B, 4]: B PCG64 generators (state, odd increment)."""
    w = np.random.default_rng(seed).integers(0, 2 ** 63, (B, 4), dtype=np.int64).astype(np.uint64)
    w[:, 0] ^= np.uint64(0x9E3779B97F4A7C15)
    w[:, 3] |= np.uint64(1)
    return w


def spawn_probs(B, rot=0):
    """The boards of a wave of two always differ; every board has a fractional probability under rot 0 or rot 1."""
    return np.array([P_CYCLE[(b + rot) % 4] for b in range(B)], np.float32)


_batches = {}


def advance_batch(H, W):
    """(boards uint16 [B, H, W], draw counts at step 0) of a shape's case list, in the order of the list -- the
    consecutive waves of the batch are in different regimes.  64x64: the boards with full-width rows come last."""
    if (H, W) not in _batches:
        rng = np.random.default_rng(1000 * H + W)
        boards = [make_board(H, W, t, rng) for t in targets_of(H, W)]
        if (H, W) == (64, 64):
            boards += [make_full_row_board(k, rng) for k in FULL_ROW_BOARDS]
        boards = np.stack(boards)
        boards.setflags(write=False)
        _batches[(H, W)] = boards, draws(boards)
    return _batches[(H, W)]


def mixed_batch_64():
    """One launch whose consecutive waves are in different regimes: 64x64 at 0, 64, 513, 1025, 2049, 1, 3000, 512, 2048."""
    rng = np.random.default_rng(64064)
    return np.stack([make_board(64, 64, t, rng) for t in (0, 64, 513, 1025, 2049, 1, 3000, 512, 2048)])


def mixed_batch_25():
    """25x25 pairs in different regimes, wave by wave: (0,129) (128,1) (33,64) (129,129) (0,0) (1,20) (90,65) and a single."""
    rng = np.random.default_rng(25025)
    return np.stack([make_board(25, 25, t, rng) for t in (0, 129, 128, 1, 33, 64, 129, 129, 0, 0, 1, 20, 90, 65, 130)])


# The occupancy kernels keep a lane's jump from step to step (JumpCache, sl_rowlane.hip:654-671), keyed on the regime: it
# must be refilled when a board's count crosses a boundary.  Waves of boards whose per-step regimes cross the boundary in BOTH directions within `steps` -- found by a search on the
# oracle over targets, probabilities and seeds; what they cross is asserted by tests/test_draw_deal_host.py.
TRANSITIONS = (
    # H, targets of the wave's boards, their spawn_prob, seed, steps
    (64, (FULL,), (0.8,), 0, 10),               # rows, block4, rows, block4, rows, block4, block5, block4, block5: 2048, 1024
    (64, (FULL,), (0.9,), 0, 8),                # rows, rounds6, rows, block4, rows, block4: 512 and 2048 in one stride
    (64, (1250,), (0.5,), 0, 10),               # block5, rounds8, rounds7, block4, rounds8, block4: 512 between neighbours
    (64, (FULL,), (1.0,), 0, 6),                # rows, none, rows, rounds1: every draw succeeds
    (40, (FULL,), (0.5,), 0, 12),               # block5, rounds8, rounds8, block4, ...: 512
    (48, (1250,), (0.5,), 0, 10),
    (25, (310, 290), (0.5, 0.3), 0, 16),        # the larger count of the two wanders round 128
    (26, (310, 290), (0.5, 0.3), 0, 16),
    (32, (310, 290), (0.5, 0.3), 0, 16),
)
# the boundaries each shape must cross in both directions (the issue's list)
MUST_CROSS = {64: (512, 2048), 40: (512,), 25: (128,)}


def transition_case(H, targets, ps, seed):
    """(boards [G, H, H], spawn_prob [G], generator words [G, 4]) of one wave."""
    rng = np.random.default_rng(seed)
    boards = np.stack([make_board(H, H, t, rng) for t in targets])
    return boards, np.array(ps, np.float32), rng_words(seed, len(targets))


# ---------------------------------------------------------------------------------------------- fused-step pools

def step_levels(H, W):
    """Levels for the fused step: boards of the shape's case list, one level each (64x64 and 25x25: a list of seventeen that
    holds every regime), with a player on an interior cell off the lattice; spawn_prob cycles per level."""
    from safelife_amd.levels import Level
    targets = targets_of(H, W)
    if H == 64:
        targets = (1, 64, 65, 449, 512, 513, 1024, 1025, 2048, 2049, FULL, 511, 129, 193, 257, 321, 385)
    elif H == 25:
        targets = (0, 129, 128, 1, 33, 64, 96, 97, 127, 128, 129, 129, 31, 32, FULL, FULL, 65)
    rng = np.random.default_rng(7000 + 100 * H + W)
    words = rng_words(7000 + H, len(targets))
    levels = []
    for k, t in enumerate(targets):
        agent = (H // 2 + (k % 3), W // 2 + 1 + (k % 2) * 3)
        if agent[0] % 3 == 1 and agent[1] % 3 == 1:
            agent = (agent[0] + 1, agent[1])
        board = make_board(H, W, t, rng, agent=agent)
        levels.append(Level(board, None, [agent], spawn_prob=P_CYCLE[(k + 1) % 4], min_performance=0.5, rng_words=words[k]))
    return levels


STEP_TIME_LIMIT, STEP_SINGLE, STEP_ROLLOUT = 5, 8, 6


def step_case(H, W, wrapped):
    """The fused step on a pool of `step_levels`: env e starts on level e, so the envs of a wave play consecutive levels;
    a short time limit, so that reloads land on these boards too.  -> (levels, B, env keywords, actions [14, B]); the
    first action is 0: step 0 makes exactly the draws of the levels' targets."""
    levels = step_levels(H, W)
    B = len(levels)
    kw = dict(first_level=np.arange(B, dtype=np.int32), auto_reset=True, level_stride=1, time_limit=STEP_TIME_LIMIT,
              view_shape=(5, 7))
    if wrapped:         # the training wrappers with the inaction baseline: a second board advances on these counts
        words = rng_words(9000 + H, B)
        kw["wrappers"] = dict(smc.TRAINING_WRAPPERS, baseline="inaction", inaction_rng=words)
    actions = np.random.default_rng(500 + H + W).integers(0, 9, (STEP_SINGLE + STEP_ROLLOUT, B)).astype(np.int32)
    actions[0] = 0
    return levels, B, kw, actions


def oracle_trace(boards, p, words, n_steps):
    """The oracle, one step at a time: (draw counts int [n_steps, B] made by each step, boards after, words after).
    n_steps: an int, or one count per board."""
    import oracle
    boards = np.array(boards, np.uint16)
    words = np.array(words, np.uint64)
    each = np.broadcast_to(np.asarray(n_steps), (len(boards),))
    counts = np.zeros((int(each.max()) if len(each) else 0, len(boards)), np.int64)
    for s in range(len(counts)):
        on = np.flatnonzero(each > s)
        counts[s, on] = draws(boards[on])
        w = np.ascontiguousarray(words[on])
        boards[on] = oracle.advance_board_batch(boards[on], np.asarray(p, np.float32)[on], 1, w)
        words[on] = w
    return counts, boards, words


def each_steps(B):
    """One step count per board: 0, 1 and 3 mixed within the waves."""
    return np.array([(0, 1, 3, 3, 1)[b % 5] for b in range(B)], np.int32)
