"""Constructed boards for the Life rule (tests/ca_ref.py restates it): every neighbourhood class as a TILE, a SEAM subset
of tiles placed on every edge a kernel layout has, and the rule SOUP (util.random_boards(kind=3)).
tests/test_ca_rule_host.py asserts on the restatement alone what these boards reach; tests/test_ca_rule_gpu.py runs them
on the device.

A tile is a 3x3 neighbourhood -- a centre cell and its eight neighbours, in the order of DIRS -- inside a 5x5 patch whose
ring is empty (ring cells may be born: the restatement covers the whole board).  Tiles are packed 6 cells apart, as many
per board as fit.  Every tile board runs at spawn_prob 0.0 AND at 1.0 (the second half of a tile batch repeats the first):
the outcome of a draw then does not depend on its value, while the generator still advances.

Which rule implementation a shape takes (sl_rowlane.hip: use_planes<H, W>(), struct Geom; sl_abi.hip: the `aligned` test):

    25x25     bit planes, one word per plane (rows of up to 28 cells), two boards per wave
    40x40     bit planes, two words per plane (even rows of 32 to 62 cells), one board per wave
    64x64     bit planes, the split layout (a row is the wave's 64 lanes wide; rows reach each other by rotation)
    30x30     the word form (ca_step: ca_rows and resolve_draws)
    13x20     no row kernel: the size-generic ca_step_block
"""
import collections

import numpy as np

from tests import ca_ref as ref
from tests import step_matrix_cases as smc
from tests import util

DIRS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))      # N NE E SE S SW W NW
R, G, B_ = ref.COLOURS
PLAIN = 9                                  # alive, destructible
TRIPLE = (0, 2, 5)                         # the fixed, asymmetric parents of a three-parent birth: N, E, SW

Tile = collections.namedtuple("Tile", "family cls centre nb")

# centre classes -> the cells that stand for them
CENTRES = collections.OrderedDict([
    ("dead empty", (0,)),
    ("dead residue", (4 | 8, 0x8000, R | G, 0x3000)),
    ("dead frozen", (16, 16 | G)),
    ("dead preserving", (32,)),
    ("dead inhibiting", (64,)),
    ("dead spawning", (128 | R,)),
    ("alive plain", (9 | G,)),
    ("alive non-destructible", (1,)),
    ("alive frozen", (17,)),
    ("alive self-preserving", (33,)),
    ("alive agent", (3 | 8,)),
    ("alive exit", (257, 265)),
    ("level agent", (122,)),
])
_DEAD_FREE = {ref.D_INHIBITED, ref.D_BORN, ref.D_SPAWNED, ref.D_DRAW_MISSED, ref.D_STAYS}
_ALIVE_FREE = {ref.A_PRESERVED, ref.A_SURVIVES, ref.A_DIES}
# ... and the outcomes the rule allows each of them (a frozen cell is kept whatever stands round it, an inhibiting cell
# inhibits itself, a spawning cell never merely stays: it draws)
REACHABLE = {
    "dead empty": _DEAD_FREE, "dead residue": _DEAD_FREE, "dead preserving": _DEAD_FREE,
    "dead frozen": {ref.D_FROZEN}, "level agent": {ref.D_FROZEN}, "dead inhibiting": {ref.D_INHIBITED},
    "dead spawning": _DEAD_FREE - {ref.D_STAYS},
    "alive plain": _ALIVE_FREE, "alive non-destructible": _ALIVE_FREE, "alive agent": _ALIVE_FREE, "alive exit": _ALIVE_FREE,
    "alive frozen": {ref.A_FROZEN}, "alive self-preserving": {ref.A_PRESERVED},
}


def _rot(nb, r):
    return tuple(nb[(k - r) % 8] for k in range(8))


def _with(*pairs):
    nb = [0] * 8
    for pos, cell in pairs:
        nb[pos % 8] = cell
    return tuple(nb)


def tiles():
    """Every tile of the issue's list, in a fixed order."""
    out = []
    colour = lambda k: (k % 8) << 9
    centres = [(cls, c) for cls, cells in CENTRES.items() for c in cells]
    # alive neighbours: 0-8 of them, each count in two rotations of the eight positions
    for cls, c in centres:
        for k in range(9):
            for r in (0, 3):
                out.append(Tile("count", cls, c, _rot(tuple(PLAIN | colour(j + k) for j in range(k)) + (0,) * (8 - k), r)))
    # one flagged neighbour at each position: dead and alive, frozen and not -- alone, and beside three alive parents
    for cls, c in centres:
        for flag in (ref.PRESERVING, ref.INHIBITING, ref.SPAWNING | B_):
            for pos in range(8):
                for alive in (0, 1):
                    for frozen in (0, 16):
                        out.append(Tile("flag", cls, c, _with((pos, flag | alive | frozen))))
                out.append(Tile("flag+3", cls, c, _with((pos, flag), (pos + 1, PLAIN | R), (pos + 3, PLAIN | R | G),
                                                        (pos + 4, PLAIN | G))))
    # three-parent births: all 8^3 colour triples
    for c0 in range(8):
        for c1 in range(8):
            for c2 in range(8):
                out.append(Tile("triple", "dead empty", 0, _with((TRIPLE[0], 1 | c0 << 9), (TRIPLE[1], 1 | c1 << 9),
                                                                 (TRIPLE[2], 1 | c2 << 9))))
    # the destructible-or-exit vote: all 64 combinations of (DESTRUCTIBLE, EXIT) over three parents
    for code in range(64):
        cells = [1 | R | (8 if code >> (2 * k) & 1 else 0) | (256 if code >> (2 * k + 1) & 1 else 0) for k in range(3)]
        out.append(Tile("vote", "dead empty", 0, _with(*zip(TRIPLE, cells))))
    # spawner colours: births and spawned cells beside one and beside two spawners of different colours
    for c1 in range(8):
        for c2 in (None, (c1 + 1) % 8, (c1 + 3) % 8, c1 ^ 7):
            for kind in (152, 144):
                sp = [(3, kind | c1 << 9)] + ([(6, 152 | c2 << 9)] if c2 is not None else [])
                out.append(Tile("spawned", "dead empty", 0, _with(*sp)))
                out.append(Tile("spawner birth", "dead empty", 0, _with((TRIPLE[0], PLAIN | R), (TRIPLE[1], PLAIN | R),
                                                                        (TRIPLE[2], PLAIN | G), *sp)))
    return out


def seam_tiles():
    """Forty tiles that tell all eight directions apart in every plane -- alive, the three colours, destructible, exit,
    preserving, inhibiting, spawning: each holds a plane at one neighbour where the centre's outcome turns on it
    (test_seam_tiles_turn_on_every_direction_and_plane clears the bit and looks)."""
    out = []
    for d in range(8):
        # a birth whose every colour, and the destructible-or-exit vote, has exactly two of three votes
        out.append(Tile("seam birth", "dead empty", 0, _with((d, 1 | R | G | 8), (d + 3, 1 | G | B_ | 256), (d + 5, 1 | R | B_))))
        out.append(Tile("seam preserved", "alive plain", PLAIN | G, _with((d, ref.PRESERVING))))
        out.append(Tile("seam inhibited", "dead empty", 0, _with((d, ref.INHIBITING), (d + 2, PLAIN), (d + 4, PLAIN | R),
                                                                 (d + 6, PLAIN))))
        out.append(Tile("seam spawned", "dead empty", 0, _with((d, 144 | ((d % 7 + 1) << 9)))))
        out.append(Tile("seam count", "alive plain", PLAIN | B_, _with((d, PLAIN), (d + 1, PLAIN | R), (d + 3, PLAIN | G),
                                                                       (d + 6, 1))))
    return out


PLANES = collections.OrderedDict([("alive", 1), ("red", R), ("green", G), ("blue", B_), ("destructible", 8), ("exit", 256),
                                  ("preserving", 32), ("inhibiting", 64), ("spawning", 128)])


def put(board, tile, y, x):
    H, W = board.shape
    board[y, x] = tile.centre
    for (dy, dx), cell in zip(DIRS, tile.nb):
        if cell:
            board[(y + dy) % H, (x + dx) % W] = cell


# ---------------------------------------------------------------------------------------------- shapes and batches

TILE_SHAPES = ((25, 25), (64, 64), (40, 40), (30, 30), (13, 20))
ROW_SHAPES = tuple((H, H) for H in smc.SHAPES)
GENERIC_SHAPES = ((3, 3), (7, 11), (4, 64), (64, 5), (5, 64), (31, 33), (100, 100), (127, 129), (128, 128))
ALL_SHAPES = ROW_SHAPES + GENERIC_SHAPES
FIXTURE_TILE_SHAPE = (25, 25)
FIXTURE_SEAM_SHAPES = ((25, 25), (64, 64), (9, 11))
FIXTURE_SOUP_SHAPES = ((25, 25), (30, 30), (64, 64), (8, 8), (7, 11))
PASS_SHAPES = ((13, 17), (33, 64))          # the side-effect pass's occupancy kernel (seam and soup batches)
SOUP_P = (0.3, 0.0, 1.0, 0.05)


def family(H, W):
    return "row" if (H, W) in ROW_SHAPES else "generic"


def boards_per_wave(H, W):
    return smc.geometry(H, W)["G"] if family(H, W) == "row" else 1


def rng_words(seed, B):
    """uint64 [B, 4]: B PCG64 generators (state, odd increment)."""
    w = np.random.default_rng(seed).integers(0, 2 ** 63, (B, 4), dtype=np.int64).astype(np.uint64)
    w[:, 0] ^= np.uint64(0x9E3779B97F4A7C15)
    w[:, 3] |= np.uint64(1)
    return w


def ragged(boards, H, W):
    """The batch with copies of its first boards behind it until B = 1 (mod 4 G): a last wave that holds ONE board
    of G, whichever kernel takes the batch.  Which launches have workgroups of four waves (NB = 4 G boards): the fused
    step always, and advance_board from 2 * n_cu such workgroups on (k_advance_rowlane; launch_advance_t) -- that is
    `four_wave_batch` below.  A smaller advance batch (k_advance_small) and every occupancy launch run one wave of G
    boards per workgroup, the size-generic kernels one board per workgroup: there a workgroup's first and last board are
    its wave's."""
    NB = 4 * boards_per_wave(H, W)
    extra = (1 - len(boards)) % NB
    return np.concatenate([boards, boards[:extra]]) if extra else boards


Batch = collections.namedtuple("Batch", "boards p words where")      # where: (board, y, x, tile index[, placement])
_cache = {}


def _frozen(b):
    for a in b[:3]:
        a.setflags(write=False)
    return b


def tile_batch(H, W):
    """Every tile on H x W boards, 6 cells apart; the batch is those boards at spawn_prob 0.0, then again at 1.0."""
    key = ("tile", H, W)
    if key not in _cache:
        ts = tiles()
        ny, nx = H // 6, W // 6
        per = ny * nx
        n = -(-len(ts) // per)
        boards = np.zeros((n, H, W), np.uint16)
        where = []
        for k, t in enumerate(ts):
            b, slot = divmod(k, per)
            y, x = 6 * (slot // nx) + 2, 6 * (slot % nx) + 2
            put(boards[b], t, y, x)
            where.append((b, y, x, k))
        boards = np.concatenate([boards, boards])
        p = np.repeat(np.array([0.0, 1.0], np.float32), n)
        _cache[key] = _frozen(Batch(boards, p, rng_words(31 * H + W, 2 * n), np.array(where)))
    return _cache[key]


def seam_placements(H, W):
    """Where a seam tile's centre goes: the four corners, the middle of the four edges, both sides of a row's word split
    (column W / 2 of the two-word layouts: 31 | 32 at 64 wide) in a middle row and in the first and last row, and two
    more cells of the first and last row."""
    raw = [("corner", 0, 0), ("corner", 0, W - 1), ("corner", H - 1, 0), ("corner", H - 1, W - 1),
           ("edge", 0, W // 2), ("edge", H - 1, W // 2), ("edge", H // 2, 0), ("edge", H // 2, W - 1),
           ("split", H // 2, W // 2 - 1), ("split", H // 2, W // 2), ("split", 0, W // 2 - 1), ("split", H - 1, W // 2 - 1),
           ("row", 0, W // 4), ("row", H - 1, (3 * W) // 4)]
    seen, out = set(), []
    for name, y, x in raw:
        if (y, x) not in seen:
            seen.add((y, x))
            out.append((name, y, x))
    return out


def seam_batch(H, W):
    """Every seam tile at every placement, first fit: a tile goes onto the first board on which its 5x5 patch and a
    one-cell gap stay clear of the tiles already there (on the torus).  spawn_prob 1.0 (a spawned cell shows its
    spawner); the `ragged` copies run at 0.0."""
    key = ("seam", H, W)
    if key not in _cache:
        ts = seam_tiles()
        places = seam_placements(H, W)
        boards, centres, where = [], [], []
        tdist = lambda a, b, n: min(abs(a - b), n - abs(a - b))
        for pi, (name, y, x) in enumerate(places):
            for k, t in enumerate(ts):
                for b in range(len(boards)):
                    if all(max(tdist(y, y2, H), tdist(x, x2, W)) >= 6 for y2, x2 in centres[b]):
                        break
                else:
                    b = len(boards)
                    boards.append(np.zeros((H, W), np.uint16))
                    centres.append([])
                put(boards[b], t, y, x)
                centres[b].append((y, x))
                where.append((b, y, x, k, pi))
        n = len(boards)
        boards = ragged(np.stack(boards), H, W)
        p = np.ones(len(boards), np.float32)
        p[n:] = 0.0
        _cache[key] = _frozen(Batch(boards, p, rng_words(37 * H + W, len(boards)), np.array(where)))
    return _cache[key]


def soup_size(H, W):
    """Boards of a soup batch: about 3000 cells' worth and at least five (3x3, where every cell sees the whole board:
    400), then made ragged."""
    B = 400 if H * W == 9 else max(5, -(-3000 // (H * W)))
    NB = 4 * boards_per_wave(H, W)
    return B + (1 - B) % NB


def soup_batch(H, W):
    """util.random_boards(kind=3).  The waves of a batch take turns in the colour bits that vary between their boards'
    cells -- wave w by w % 4: all three; two (one bit cleared on every cell); two beside a bit every cell has (one bit
    set on every cell); all three again, but in every eighth wave one (two bits cleared) -- so that a launch of the
    64-wide occupancy kernels holds boards of the SLOTS = 8 and of the SLOTS = 4 instantiation."""
    key = ("soup", H, W)
    if key not in _cache:
        B = soup_size(H, W)
        rng = np.random.default_rng(5000 + 131 * H + W)
        boards = util.random_boards(rng, B, H, W, kind=3)
        G = boards_per_wave(H, W)
        for k in range(B):
            wave = k // G
            mode, bit = wave % 4, wave // 4 % 3
            if mode == 1:
                boards[k] &= np.uint16(~ref.COLOURS[bit] & 0xFFFF)
            elif mode == 2:
                boards[k] |= np.uint16(ref.COLOURS[(bit + 1) % 3])
            elif mode == 3 and wave % 8 == 7:
                boards[k] &= np.uint16(~(ref.COLOURS[bit] | ref.COLOURS[(bit + 1) % 3]) & 0xFFFF)
        p = np.array([SOUP_P[k % 4] for k in range(B)], np.float32)
        _cache[key] = _frozen(Batch(boards, p, rng_words(41 * H + W, B), None))
    return _cache[key]


# advance_board takes the four-wave k_advance_rowlane only from 2 * n_cu workgroups of NB boards on (launch_advance_t of
# sl_rowlane.hip; 256 CUs on an MI355X); every smaller batch runs k_advance_small, one wave per workgroup.  One shape per
# layout, and each way a lane reaches the rows above and below it (struct Geom: rotate, shift, bpermute):
#   25 planes, one word, shift, G = 2     40 planes, two words, shift, G = 1      64 planes, split, rotate, G = 1
#   30 word form, shift, G = 2            20 planes, one word, bpermute, G = 3    32 planes, two words, bpermute, G = 2
FOUR_WAVE_SHAPES = (25, 40, 64, 30, 20, 32)
FOUR_WAVE_CUS = 256


def advance_kernel(H, W, B, n_cu):
    """"four-wave" (k_advance_rowlane) or "small" (k_advance_small): launch_advance_t's rule, restated."""
    NB = 4 * boards_per_wave(H, W)
    return "four-wave" if -(-B // NB) >= 2 * n_cu else "small"


def four_wave_batch(kind, H):
    """A seam or soup batch repeated to 2 * 256 * NB + 1 boards (boards, p and words alike: copy c of board k makes
    board k's draws), which k_advance_rowlane takes on up to 256 CUs: every board of the batch at many places of the
    four-wave workgroups, a last workgroup of one board.  -> (Batch, idx): board b is board idx[b] of the batch, so what
    is expected of it is row idx[b] of the batch's trajectory."""
    b = BATCHES[kind](H, H)
    NB = 4 * boards_per_wave(H, H)
    B = 2 * FOUR_WAVE_CUS * NB + 1
    idx = np.arange(B) % len(b.boards)
    return Batch(b.boards[idx], b.p[idx], b.words[idx], None), idx


def varying_colour_bits(board):
    """How many colour bits vary between a board's sources (its alive and its spawning cells): what picks the occupancy
    kernel's counters per cell (OccGeom of sl_rowlane.hip: up to two -> SLOTS = 4, three -> SLOTS = 8)."""
    b = np.asarray(board, np.uint16).astype(np.int64)
    src = b[(b & (ref.ALIVE | ref.SPAWNING)) != 0]
    return sum(1 for bit in ref.COLOURS if ((src & bit) != 0).any() and ((src & bit) == 0).any())


BATCHES = collections.OrderedDict([("tile", tile_batch), ("seam", seam_batch), ("soup", soup_batch)])


def shapes_of(kind):
    return TILE_SHAPES if kind == "tile" else ALL_SHAPES


def cases():
    return [(kind, H, W) for kind in BATCHES for H, W in shapes_of(kind)]


def host_cases():
    """... and the batches of the pass shapes, which the CPU tests hold to the same conditions."""
    return cases() + [(kind, H, W) for kind in ("seam", "soup") for H, W in PASS_SHAPES]


def case_id(case):
    return "%s-%dx%d" % case


def each_steps(B):
    """One step count per board, 0-3 mixed within the waves."""
    return np.array([(0, 1, 3, 2, 3, 1, 2)[b % 7] for b in range(B)], np.int32)


N_LONG = 20             # past the 15-step flush of the occupancy kernels' register counters
_runs = {}


def ref_steps(H, W):
    """How many steps the restatement follows a batch: N_LONG, or 7 on boards of more than 4096 cells (whole-array numpy
    on 161 boards of 128x128 takes half a second per step; the oracle, which the host tests hold to the restatement on
    these very boards for the first 7 steps, stands in for it at N_LONG)."""
    return N_LONG if H * W <= 4096 else 7


def run(kind, H, W):
    """The restatement's trajectory of a batch (computed once, shared): ca_ref.trajectory over ref_steps(H, W) steps."""
    key = (kind, H, W)
    if key not in _runs:
        b = BATCHES[kind](H, W)
        _runs[key] = ref.trajectory(b.boards, b.p, b.words, ref_steps(H, W), count_steps=(1, 2, 7, N_LONG))
    return _runs[key]


def expected_occupancy(kind, H, W, n):
    """(counts, words after) of life_occupancy over n steps: the restatement's, or past ref_steps the oracle's."""
    if n <= ref_steps(H, W) and n in (1, 2, 7, N_LONG):
        r = run(kind, H, W)
        return r["counts"][n], r["words"][n]
    import oracle
    b = BATCHES[kind](H, W)
    w = b.words.copy()
    return oracle.life_occupancy_batch(b.boards, b.p, n, w, n_threads=8), w


def each_from(run_, each):
    """Boards and words after each[b] steps of board b, out of a trajectory."""
    boards = np.stack([run_["boards"][int(s)][b] for b, s in enumerate(each)])
    words = np.stack([run_["words"][int(s)][b] for b, s in enumerate(each)])
    return boards, words


# ---------------------------------------------------------------------------------------------- levels of the fused step

STEP_KINDS = ("tile", "soup")
STEP_TIME_LIMIT, STEP_SINGLE, STEP_ROLLOUT = 4, 3, 4
MAX_EXITS = 8           # exit slots the row kernels' fused step takes (sl_abi.hip: more run the size-generic kernels)


def step_board(board):
    """A tile or soup board as a level: the real agent (CellTypes.player) stands at (H - 2, W - 2) inside a 3x3 block of
    frozen walls -- it cannot move, and neither it nor the walls reach a cell outside the block (a wall is frozen, not
    alive, carries no flag; the agent's flags stop at the walls) -- and of the cells the env takes for exits (EXIT without
    AGENT) all but the first eight get the AGENT bit too: the rule never reads that bit, an alive parent's EXIT still
    votes, and the pool keeps the eight exit slots of the row kernels."""
    b = np.array(board, np.uint16)
    H, W = b.shape
    b[H - 3:, W - 3:] = 16
    b[H - 2, W - 2] = 122
    flat = b.reshape(-1)
    exits = np.flatnonzero((flat & (ref.EXIT | ref.AGENT)) == ref.EXIT)
    flat[exits[MAX_EXITS:]] |= np.uint16(ref.AGENT)
    return b, (H - 2, W - 2)


def step_case(kind, H, W, wrapped):
    """The fused step on a pool of one level per board of the batch, built the way draw_deal_cases.step_case does it: env e
    starts on level e, a short time limit so that reloads land on these boards too; three single no-op steps, then a
    T-step launch of random actions (the agent is walled in: an action turns it, nothing else).
    -> (levels, B, env keywords, actions [STEP_SINGLE + STEP_ROLLOUT, B])."""
    from safelife_amd.levels import Level
    b = BATCHES[kind](H, W)
    levels = []
    for k in range(len(b.boards)):
        board, agent = step_board(b.boards[k])
        levels.append(Level(board, None, [agent], spawn_prob=float(b.p[k]), min_performance=0.5, rng_words=b.words[k].copy()))
    B = len(levels)
    kw = dict(first_level=np.arange(B, dtype=np.int32), auto_reset=True, level_stride=1, time_limit=STEP_TIME_LIMIT,
              view_shape=(5, 7))
    if wrapped:         # the training wrappers with the inaction baseline: a second board advances by the same rule
        kw["wrappers"] = dict(smc.TRAINING_WRAPPERS, baseline="inaction", inaction_rng=rng_words(9000 + H, B))
    actions = np.random.default_rng(600 + H + W).integers(0, 9, (STEP_SINGLE + STEP_ROLLOUT, B)).astype(np.int32)
    actions[:STEP_SINGLE] = 0
    return levels, B, kw, actions


# ---------------------------------------------------------------------------------------------- what the soup holds

def soup_events(run_, steps=3):
    """Over the first `steps` steps of a trajectory: births whose DESTRUCTIBLE bit depends on an alive parent's EXIT bit;
    deaths of alive AGENT or EXIT cells that are not frozen; cells whose exclusion from the occupancy count (alive and
    AGENT, EXIT or FROZEN) differs from one step to the next."""
    exit_births = deaths = changes = 0
    for s in range(steps):
        before, after, outcome = run_["boards"][s], run_["boards"][s + 1], run_["outcomes"][s]
        b = before.astype(np.int64)
        votes_d = np.zeros(b.shape, np.int64)
        for dy, dx in [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]:
            n = np.roll(b, (dy, dx), axis=(-2, -1))
            votes_d += ((n & 1) != 0) & ((n & 8) != 0)
        exit_births += int(((outcome == ref.D_BORN) & ((after & 8) != 0) & (votes_d < 2)).sum())
        deaths += int(((outcome == ref.A_DIES) & ((b & (ref.AGENT | ref.EXIT)) != 0)).sum())
        excl = lambda a: ((a & 1) != 0) & ((a & (ref.AGENT | ref.EXIT | ref.FROZEN)) != 0)
        changes += int((excl(before) != excl(after)).sum())
    return dict(exit_births=exit_births, deaths=deaths, changes=changes)
