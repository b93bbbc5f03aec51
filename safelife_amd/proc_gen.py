"""
Procedural levels: the project's own generator for the reference's level-spec schema (its ``levels/random/*.yaml``), with
every pattern -- the expensive part, ``speedups.gen_pattern`` -- generated in batches on the device.

A spec is a dict with the reference's keys: ``board_shape``, ``min_performance``, ``partitioning`` (``min_regions``,
``max_regions``), ``starting_region`` / ``later_regions`` / ``buffer_region`` (names into ``named_regions``), ``named_regions``
(name -> list of layers; layer keys ``color, fences, spawners, tree_lattice, pattern, movable_walls, movable_trees,
hardened_life, buffer_zone, target, fountains``), ``agents`` and ``agent_types``.  Any value may be randomised with
``{"choices": [...]}`` (optionally ``weights``, or a dict value -> weight) or ``{"uniform": [low, high]}``.
``load_params(path, defaults=...)`` reads a spec file over a defaults file the way the reference's level iterator does.

How it runs.  The glue around the sampler is cheap numpy; one Metropolis chain is sequential; thousands of chains are not.
So a level is a GENERATOR FUNCTION: where it needs a pattern it yields a ``PatternRequest`` (board, mask, seeds, arguments
and its own generator's six words) and is resumed with the answer; the retry ladder (min_fill x 0.94 on max-iter, max_fill x
1.07 on an overfull pattern, ten retries) is simply more yields.  ``gen_games(params, seeds)`` drives N such coroutines and
hands each round's pending requests to the backend in ONE call; the default backend groups them by (H, W, period) and runs
``speedups.gen_pattern_batch``, one wavefront per chain.  The region partition -- a scalar loop of a few hundred turns, most
of the glue's time -- goes the same way: a level yields a ``PartitionRequest`` (its generator's six words, the shape, the
bounds), a round's partition requests go to the ``partition_backend`` in one call, and the default one runs
``speedups.partition_batch``, one wavefront per partition, bit-equal to ``partition`` below, which stays the reference.

Two properties are the contract:

* level k depends on ``seeds[k]`` and ``params`` only -- every draw of a level comes from ``np.random.default_rng(seed)``,
  whose state travels through the pattern calls -- not on the batch, its order or its size;
* under any exact backend (the device, a compiled ``gen_pattern`` drop-in via ``function_backend``, a restatement) the same
  seed gives the same level, byte for byte.

NOT a goal: levels equal to the reference's ``gen_game`` for the same seed.  The partition here is a seeded region growth of
its own (the reference's depends on CPython's set order and scipy's filters), a fence is the open area's whole rim before
the coin flips (the reference thins it), the tree lattice is a rotated square lattice chosen by ``spacing``, the layers of an
oscillating pattern are followed at spawn probability 0, and the order of the draws is this module's.  What a spec MEANS is
kept: region types, layer semantics, masks, the retry ladder, goals and colours, agents and the exit in the buffer region.
"""
import copy

import numpy as np

from . import speedups
from .cell_types import CellTypes, DEFAULT_POINTS_TABLE
from .levels import Level

NEW_CELL, CAN_OSCILLATE, INCLUDE_VIOLATIONS = (speedups.NEW_CELL_MASK, speedups.CAN_OSCILLATE_MASK,
                                               speedups.INCLUDE_VIOLATIONS_MASK)
NUM_RETRIES = 10
MIN_FILL_STEP, MAX_FILL_STEP = 0.94, 1.07

COLORS = {"black": 0, "red": int(CellTypes.color_r), "green": int(CellTypes.color_g), "blue": int(CellTypes.color_b),
          "yellow": int(CellTypes.color_r | CellTypes.color_g), "magenta": int(CellTypes.color_r | CellTypes.color_b),
          "cyan": int(CellTypes.color_g | CellTypes.color_b), "white": int(CellTypes.rainbow_color)}
AGENT_FLAGS = {k: int(getattr(CellTypes, k)) for k in ("alive", "pushable", "pullable", "destructible", "frozen",
                                                       "preserving", "inhibiting", "spawning")}
DEFAULT_AGENT = {"color": "black", "flags": ["preserving", "inhibiting"], "points_table": DEFAULT_POINTS_TABLE.tolist()}
PATTERN_KEYS = ("max_iter", "min_fill", "temperature", "osc_bonus", "alive", "wall", "tree")
_RAINBOW = int(CellTypes.rainbow_color)
_WALL, _TREE, _LIFE = int(CellTypes.wall), int(CellTypes.tree), int(CellTypes.life)


# --------------------------------------------------------------------------- specs

def load_params(path, defaults=None):
    """A spec file (YAML) as a dict; with `defaults` (a path or a dict) merged under it the way the reference's level
    iterator does: top-level keys of the spec win, and ``named_regions`` / ``agent_types`` are merged name by name."""
    import yaml
    with open(path) as f:
        data = yaml.safe_load(f) or {}
    if defaults is None:
        return data
    base = load_params(defaults) if isinstance(defaults, str) else copy.deepcopy(defaults)
    out = dict(base)
    out.update(data)
    for key in ("named_regions", "agent_types"):
        out[key] = dict(base.get(key) or {})
        out[key].update(data.get(key) or {})
    return out


def _resolve(val, rng):
    """Replace every ``choices`` / ``uniform`` node below `val` by a draw, in the order the spec lists its keys."""
    if isinstance(val, list):
        return [_resolve(v, rng) for v in val]
    if not isinstance(val, dict):
        return val
    if "choices" in val:
        choices = val["choices"]
        if isinstance(choices, dict):
            keys, weights = list(choices.keys()), [float(w) for w in choices.values()]
        elif isinstance(choices, list):
            keys = choices
            weights = [float(w) for w in (val.get("weights") or [1.0] * len(choices))]
        else:
            raise ValueError("The 'choices' object must be a list of options or a dictionary option -> probability.")
        w = np.array(weights, np.float64)
        if len(w) != len(keys) or (w < 0).any() or not w.sum() > 0:
            raise ValueError("The weights of 'choices' must be non-negative, one per option, and their sum positive.")
        pick = int(np.searchsorted(np.cumsum(w / w.sum()), rng.random(), side="right"))
        return _resolve(keys[min(pick, len(keys) - 1)], rng)
    if "uniform" in val:
        low, high = (float(x) for x in val["uniform"])
        return low + (high - low) * float(rng.random())
    return {k: _resolve(v, rng) for k, v in val.items()}


# --------------------------------------------------------------------------- small torus helpers

def _grow(a, reach=1):
    """Cells within `reach` (Chebyshev, wrapped) of a True cell."""
    a = np.asarray(a, bool)
    out = a.copy()
    for dy in range(-reach, reach + 1):
        for dx in range(-reach, reach + 1):
            if dy or dx:
                out |= np.roll(a, (dy, dx), (0, 1))
    return out


def _shrink(a):
    return ~_grow(~np.asarray(a, bool))


def _coins(rng, p, shape):
    return rng.random(shape) < float(p)


def _life_step(board):
    """One step of the Life rule without spawning: what is EMPTY and what is not through an oscillator's cycle is all
    the caller looks at, so newborn cells are plain life."""
    b = board.astype(np.int32)
    alive = (b & 1) != 0
    n = sum(np.roll(alive.astype(np.int32), (dy, dx), (0, 1)) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    frozen = (b & int(CellTypes.frozen)) != 0
    pres = _grow((b & int(CellTypes.preserving)) != 0)
    inh = _grow((b & int(CellTypes.inhibiting)) != 0)
    keep = frozen | (alive & (pres | (n == 3) | (n == 4))) | (~alive & inh)
    out = np.where(keep, b, 0)
    out = np.where(~alive & ~frozen & ~inh & (n == 3), _LIFE, out)
    return out.astype(np.uint16)


# --------------------------------------------------------------------------- the partition

def partition(rng, shape, min_regions=2, max_regions=5, **_):
    """int16 [H, W]: 0 = buffer, 1.. = regions.  Every region is connected (4-neighbour), and cells of two different regions
    are never within two cells of each other (wrapped): at least two buffer cells lie between them (a lone region stops at four fifths of the board).  Regions grow from seed
    cells, one cell per turn; a turn goes to a region with probability proportional to the size of its frontier."""
    H, W = int(shape[0]), int(shape[1])
    lo = max(1, int(min_regions))
    n_regions = lo + int(rng.integers(0, max(int(max_regions), lo) - lo + 1))
    label = [0] * (H * W)               # a flat Python list: the loop below is all scalar look-ups
    near = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3)]

    def foreign_near(r, c, k):
        for dy, dx in near:
            v = label[((r + dy) % H) * W + (c + dx) % W]
            if v and v != k:
                return True
        return False

    frontiers, queued = [], []
    for k in range(1, n_regions + 1):
        free = [i for i in range(H * W) if not label[i] and not foreign_near(i // W, i % W, k)]
        if not free:
            break
        cell = free[int(rng.integers(0, len(free)))]
        label[cell] = k
        frontiers.append([])
        queued.append({cell})
        for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):
            nxt = ((cell // W + dy) % H) * W + (cell % W + dx) % W
            if nxt not in queued[-1]:
                queued[-1].add(nxt)
                frontiers[-1].append(nxt)
    taken, room = len(frontiers), (4 * H * W) // 5      # a lone region has no neighbour to stop it: it leaves a fifth as buffer
    while True:
        sizes = [len(f) for f in frontiers]
        total = sum(sizes)
        if not total:
            break
        at, k = rng.random() * total, 0             # a turn goes to region k with probability frontier_k / total
        while k < len(sizes) - 1 and (at >= sizes[k] or not sizes[k]):
            at -= sizes[k]
            k += 1
        while not frontiers[k]:
            k = (k + 1) % len(frontiers)
        f = frontiers[k]
        j = int(rng.integers(0, len(f)))
        f[j], f[-1] = f[-1], f[j]
        cell = f.pop()
        r, c = divmod(cell, W)
        if label[cell] or foreign_near(r, c, k + 1):
            continue
        if len(frontiers) == 1 and taken >= room:
            break
        label[cell] = k + 1
        taken += 1
        for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):
            nxt = ((r + dy) % H) * W + (c + dx) % W
            if nxt not in queued[k] and not label[nxt]:
                queued[k].add(nxt)
                f.append(nxt)
    return np.array(label, np.int16).reshape(H, W)


# --------------------------------------------------------------------------- requests

class PartitionRequest(object):
    """The partition a level is waiting for: the level generator's six words, the board shape and the bounds as the spec
    gives them (``partition`` clamps them).  The answer is ``(labels, words)``: int16 [H, W] and the words after."""

    def __init__(self, words, shape, min_regions=2, max_regions=5):
        self.words, self.shape, self.min_regions, self.max_regions = words, tuple(shape), min_regions, max_regions


class PatternRequest(object):
    """One call of gen_pattern a level is waiting for: board uint16 [H, W], mask int32 [H, W], seeds int32 [H, W] or None,
    period, kwargs (the keywords of ``speedups.gen_pattern``) and the level generator's six words.  The answer is
    ``(board, status, words)``: the new board (the input where status is not 0), 0 or -1 (max-iter), the words after."""

    def __init__(self, board, mask, seeds, period, kwargs, words):
        self.board, self.mask, self.seeds, self.period, self.kwargs, self.words = board, mask, seeds, int(period), kwargs, words


def _lattice(shape, spacing, stagger):
    rows, cols = np.arange(shape[0])[:, None], np.arange(shape[1])[None, :]
    if not stagger:
        s = max(1, int(spacing))
        return (rows % s == 0) & (cols % s == 0)
    if spacing <= 3:
        return (rows % 3 == 0) & ((cols + rows // 3) % 3 == 0)
    a, b = {4: (1, 3), 5: (2, 3)}.get(int(spacing), (1, 4))     # the square lattice spanned by (a, b) and (-b, a)
    return (a * cols - b * rows) % (a * a + b * b) == 0


def _pattern(rng, board, mask, seeds, period, args):
    """The retry ladder around one pattern; a generator: yields PatternRequests, returns the board."""
    kw = {k: args[k] for k in PATTERN_KEYS if k in args}
    for k in ("alive", "wall", "tree"):
        if k in kw:
            kw[k] = (float(kw[k][0]), float(kw[k][1]))
    min_fill = float(kw.get("min_fill", 0.2))
    max_fill = float(args.get("max_fill", 2 * min_fill))
    retries = int(args.get("num_retries", NUM_RETRIES))
    area = (mask & NEW_CELL) != 0
    while True:
        kw["min_fill"] = min_fill
        words = speedups.pcg64_words6(rng.bit_generator)
        new_board, status, words = yield PatternRequest(board, mask, seeds, period, dict(kw), words)
        speedups.pcg64_set_words6(rng.bit_generator, words)
        if status == 0:
            if not area.any() or ((new_board != 0) & area).sum() / area.sum() <= max_fill:
                return np.array(new_board, np.uint16)
            max_fill *= MAX_FILL_STEP
        elif status == -1:
            min_fill *= MIN_FILL_STEP
        else:
            return board
        if retries <= 0:
            return board
        retries -= 1


def _populate(rng, region, layers):
    """Fill one region (bool [H, W]) layer by layer; a generator: yields PatternRequests, returns (board, goals)."""
    region = np.asarray(region, bool)
    rim = _grow(region) & ~region
    gen_mask = (region * (NEW_CELL | CAN_OSCILLATE | INCLUDE_VIOLATIONS) + rim * INCLUDE_VIOLATIONS).astype(np.int32)
    board = np.zeros(region.shape, np.uint16)
    foreground, background, background_color = (np.zeros(region.shape, bool) for _ in range(3))
    seeds, max_period = None, 1
    for layer in layers:
        if not isinstance(layer, dict):
            raise ValueError("a region is a list of layer dictionaries")
        layer = _resolve(layer, rng)
        old_board = board.copy()
        was_open = (gen_mask & NEW_CELL) != 0
        interior = _shrink(was_open)
        color = np.uint16(COLORS.get(layer.get("color"), 0))

        fence_frac = float(layer.get("fences", 0) or 0)
        if fence_frac > 0:          # the open area's rim: no open cell behind it touches a cell outside
            fence = was_open & ~interior & _coins(rng, fence_frac, board.shape)
            gen_mask[fence] &= ~(NEW_CELL | CAN_OSCILLATE)
            board[fence] = CellTypes.wall

        spawners = float(layer.get("spawners", 0) or 0)
        if spawners > 0:
            free = was_open & interior
            cells = free & _coins(rng, spawners, board.shape)
            if free.any() and not cells.any():          # at least one
                idx = np.flatnonzero(free)
                cells.reshape(-1)[idx[int(rng.integers(0, len(idx)))]] = True
            gen_mask[cells] &= ~NEW_CELL
            board[cells] = CellTypes.spawner | color

        lattice = layer.get("tree_lattice")
        if lattice is not None and lattice is not False:
            opts = lattice if isinstance(lattice, dict) else {}
            cells = _lattice(board.shape, float(opts.get("spacing", 5)), bool(opts.get("stagger", True)))
            cells &= (gen_mask & NEW_CELL) != 0
            board[cells] = CellTypes.tree | color

        period = 1
        if "pattern" in layer:
            args = dict(layer["pattern"] or {})
            period = int(args.get("period", 1))
            if period == 1:             # a still life on top of whatever oscillates already
                mask2, args["osc_bonus"] = gen_mask & ~CAN_OSCILLATE, 0
            elif period == 0:           # anything goes: violations are not looked at
                mask2, args["osc_bonus"] = gen_mask & ~INCLUDE_VIOLATIONS, 0
            elif period < max_period:
                raise ValueError("Periods of a region's layers must be 0, 1, or at least the largest period so far.")
            else:
                mask2, max_period = gen_mask, period
            board = yield from _pattern(rng, board, mask2.astype(np.int32), seeds, max_period, args)
            # later layers must not touch this one: its cells, and around the cells that blink
            cycle = [board]
            for _ in range(1, max_period):
                cycle.append(_life_step(cycle[-1]))
            filled = np.stack(cycle) != 0
            still = filled.all(axis=0)
            blinking = filled.any(axis=0) & ~still
            gen_mask[blinking] &= ~(NEW_CELL | INCLUDE_VIOLATIONS)
            gen_mask[still | _grow(blinking)] &= ~(NEW_CELL | CAN_OSCILLATE)
            new_life = (board != old_board) & ((board & CellTypes.alive) != 0)
            board[new_life] |= color
            seeds = (((board & CellTypes.alive) != 0) & region).astype(np.int32)

        new = board != old_board
        kind = board & ~np.uint16(_RAINBOW)
        for key, what, bits, add in (("movable_walls", _WALL, CellTypes.movable, True),
                                     ("movable_trees", _TREE, CellTypes.movable, True),
                                     ("hardened_life", _LIFE, CellTypes.destructible, False)):
            frac = float(layer.get(key, 0) or 0)
            if frac > 0:
                cells = _coins(rng, frac, board.shape) & new & (kind == what)
                if add:
                    board[cells] |= bits
                else:
                    board[cells] &= ~bits

        reach = int(layer.get("buffer_zone", 0) or 0)
        gen_mask[_grow((board & CellTypes.alive) != 0, reach)] &= ~NEW_CELL

        target = layer.get("target", "board")
        if target == "board" or target == "both":
            foreground[new] = True
            if period > 0:
                background[new] = True
                if target == "both":
                    background_color[new] = True
        elif target == "goals":
            background[new] = True
            background_color[new] = True
            foreground[new & ((board & CellTypes.alive) == 0)] = True      # walls and the like stay on the board
        else:
            raise ValueError("Unexpected value for 'target': %s" % (target,))

        fountains = float(layer.get("fountains", 0) or 0)
        if fountains > 0:
            is_open = (gen_mask & NEW_CELL) != 0
            cells = _coins(rng, fountains, board.shape) & is_open
            around = _grow(cells) & is_open
            gen_mask[around] = INCLUDE_VIOLATIONS
            if reach > 0:
                gen_mask[_grow(around, reach)] &= ~NEW_CELL
            board[around] = CellTypes.wall | color
            board[cells] = CellTypes.fountain | color
            foreground[cells] = True
            background[around] = True
            background_color[around] = True

    goals = board * background
    goals &= ~CellTypes.spawning
    goals[~background_color] &= ~np.uint16(_RAINBOW)
    return board * foreground, goals


def _place_agents(rng, board, regions, agents, agent_types):
    """Agents onto random buffer cells, the exit onto the buffer cell farthest from them; the 3x3 around each leaves the
    regions (-1).  -> (agent_locs [A, 2], points tables, names)"""
    types = {"default": DEFAULT_AGENT}
    types.update(agent_types or {})
    values, tables, names = [], [], []
    for name in _resolve(agents, rng) or []:
        name = _resolve(name, rng)
        if name not in types:
            continue
        agent = dict(DEFAULT_AGENT)
        agent.update(types[name] or {})
        value = int(CellTypes.agent | CellTypes.frozen) | COLORS.get(agent["color"], 0)
        for flag in agent["flags"] or []:
            value |= AGENT_FLAGS.get(flag, 0)
        values.append(value)
        tables.append(np.array(agent["points_table"], np.int64).reshape(8, 9))
        names.append(str(name))
    H, W = board.shape
    buffer_cells = np.flatnonzero(regions.reshape(-1) == 0)
    values = values[:len(buffer_cells)]
    if not values:
        return np.zeros((0, 2), np.int64), np.zeros((0, 8, 9), np.int64), []
    picks = []
    pool = [int(x) for x in buffer_cells]
    for _ in values:                        # without replacement, one draw each
        picks.append(pool.pop(int(rng.integers(0, len(pool)))))
    locs = np.array([divmod(p, W) for p in picks], np.int64)
    board[locs[:, 0], locs[:, 1]] = values
    dr = np.abs(np.arange(H)[:, None] - locs[None, :, 0])
    dc = np.abs(np.arange(W)[:, None] - locs[None, :, 1])
    dist = np.minimum(dr, H - dr).sum(1)[:, None] + np.minimum(dc, W - dc).sum(1)[None, :]
    dist = np.where((regions == 0) & (board == 0), dist + 1, 0)
    exit_loc = divmod(int(np.argmax(dist)), W)
    if dist[exit_loc] > 0:
        board[exit_loc] = CellTypes.level_exit | CellTypes.color_r
        spots = np.vstack([locs, [exit_loc]])
    else:
        spots = locs
    for r, c in spots:
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                regions[(r + dy) % H, (c + dx) % W] = -1
    return locs, np.stack(tables[:len(values)]), names[:len(values)]


def level_coroutine(params, seed, name=None):
    """One level as a generator: yields one PartitionRequest, then PatternRequests (send the answers back), returns the
    ``levels.Level``.  Every draw comes from ``np.random.default_rng(seed)``."""
    rng = np.random.default_rng(seed)
    shape = tuple(int(x) for x in _resolve(params.get("board_shape", (25, 25)), rng))
    min_performance = float(_resolve(params.get("min_performance", -1), rng))
    bounds = _resolve(params.get("partitioning") or {}, rng)
    regions, words = yield PartitionRequest(speedups.pcg64_words6(rng.bit_generator), shape, bounds.get("min_regions", 2),
                                            bounds.get("max_regions", 5))
    speedups.pcg64_set_words6(rng.bit_generator, words)
    regions = np.array(regions, np.int16).reshape(shape)
    partition_map = regions.copy()
    board = np.zeros(shape, np.uint16)
    goals = np.zeros(shape, np.uint16)
    named = params.get("named_regions") or {}
    locs, tables, names = _place_agents(rng, board, regions, params.get("agents", ["default"]), params.get("agent_types"))
    first = params.get("starting_region")
    for k in range(1, int(regions.max()) + 1):
        region = regions == k
        if not region.any():
            continue
        region_name = _resolve(first if first is not None else params.get("later_regions"), rng)
        first = None
        if region_name not in named:
            continue
        rboard, rgoals = yield from _populate(rng, region, named[region_name])
        board += rboard
        goals += rgoals
    buffer_name = _resolve(params.get("buffer_region"), rng)
    if buffer_name is not None and buffer_name in named:
        rboard, rgoals = yield from _populate(rng, regions == 0, named[buffer_name])
        board += rboard * (board == 0)
        goals += rgoals * (goals == 0)
    goals[(regions <= 0) & ((goals & CellTypes.rainbow_color) == 0)] |= CellTypes.rainbow_color    # the buffer shows white
    level = Level(board, goals, locs, min_performance=min_performance, points_table=tables if len(tables) else None,
                  orientation=1, name=name, rng_words=speedups.pcg64_words(rng.bit_generator))
    level.seed = seed
    level.agent_names = names
    level.regions = partition_map
    return level


# --------------------------------------------------------------------------- backends and the driver

def device_backend(requests):
    """All pending requests in as few launches as there are (H, W, period) groups: ``speedups.gen_pattern_batch``."""
    answers = [None] * len(requests)
    groups = {}
    for i, rq in enumerate(requests):
        groups.setdefault(rq.board.shape + (rq.period,), []).append(i)
    for (H, W, period), idx in groups.items():
        boards = np.stack([requests[i].board for i in idx]).astype(np.uint16)
        masks = np.stack([requests[i].mask for i in idx]).astype(np.int32)
        seeds = np.stack([requests[i].mask if requests[i].seeds is None else requests[i].seeds for i in idx]).astype(np.int32)
        params = np.stack([speedups.gen_pattern_params(**requests[i].kwargs) for i in idx])
        rng = np.stack([requests[i].words for i in idx]).astype(np.uint64)
        out, status, _ = speedups.gen_pattern_batch(boards, masks, period, seeds, params, rng)
        for j, i in enumerate(idx):
            answers[i] = (out[j], int(status[j]), rng[j].copy())
    return answers


def host_partition_backend(requests):
    """``partition`` per request, on a generator set to the request's words."""
    bitgen = np.random.PCG64(0)
    answers = []
    for rq in requests:
        speedups.pcg64_set_words6(bitgen, rq.words)
        labels = partition(np.random.Generator(bitgen), rq.shape, min_regions=rq.min_regions, max_regions=rq.max_regions)
        answers.append((labels, speedups.pcg64_words6(bitgen)))
    return answers


def device_partition_backend(requests):
    """All pending partitions in as few launches as there are board shapes: ``speedups.partition_batch``.  A problem the
    device refuses (a shape or a number of regions outside its range) or caps is run on the host from the request's words."""
    answers = [None] * len(requests)
    groups = {}
    for i, rq in enumerate(requests):
        groups.setdefault(rq.shape, []).append(i)
    for shape, idx in groups.items():
        words = np.stack([requests[i].words for i in idx]).astype(np.uint64)
        lo = np.array([int(requests[i].min_regions) for i in idx], np.int64)
        hi = np.array([int(requests[i].max_regions) for i in idx], np.int64)
        labels, after, status = speedups.partition_batch(words, shape, lo, hi)
        for j, i in enumerate(idx):
            if int(status[j]) == 0:
                answers[i] = (labels[j], after[j].copy())
            else:
                answers[i] = host_partition_backend([requests[i]])[0]
    return answers


def function_backend(module):
    """A backend over any drop-in of the reference's native module (``gen_pattern``, ``set_bit_generator``,
    ``MaxIterException``, ``BoardGenException``): one call per request, on a generator set to the request's words."""
    bitgen = np.random.PCG64(0)

    def backend(requests):
        module.set_bit_generator(bitgen)
        answers = []
        for rq in requests:
            speedups.pcg64_set_words6(bitgen, rq.words)
            try:
                out = module.gen_pattern(rq.board.copy(), rq.mask.copy(), rq.period,
                                         seeds=None if rq.seeds is None else rq.seeds.copy(), **rq.kwargs)
                status = 0
            except module.MaxIterException:
                out, status = rq.board, -1
            except module.BoardGenException:
                out, status = rq.board, -2
            answers.append((np.array(out, np.uint16), status, speedups.pcg64_words6(bitgen)))
        return answers
    return backend


def gen_games(params, seeds, backend=None, name="procgen", partition_backend=None):
    """N levels of the spec `params`, level k from ``seeds[k]`` alone.  Each round, the levels that wait for a pattern hand
    their requests to `backend` in one call (default: ``device_backend``), and the levels that wait for their partition hand
    theirs to `partition_backend` in one call (default: ``device_partition_backend`` where the patterns run on the device
    too, ``host_partition_backend`` under an explicit `backend`).  -> list of ``levels.Level`` with board, goals, agent_locs,
    points_table, min_performance and name."""
    if partition_backend is None:
        partition_backend = device_partition_backend if backend is None else host_partition_backend
    backend = backend or device_backend
    seeds = list(seeds)
    coros = [level_coroutine(params, s, name="%s-%s" % (name, s)) for s in seeds]
    done = [None] * len(coros)
    waiting = {}
    for k, co in enumerate(coros):
        try:
            waiting[k] = next(co)
        except StopIteration as stop:
            done[k] = stop.value
    while waiting:
        order = sorted(waiting)
        answers = {}
        for kind, serve in ((PartitionRequest, partition_backend), (PatternRequest, backend)):
            mine = [k for k in order if isinstance(waiting[k], kind)]
            if mine:
                answers.update(zip(mine, serve([waiting[k] for k in mine])))
        for k in order:
            answer = answers[k]
            try:
                waiting[k] = coros[k].send(answer)
            except StopIteration as stop:
                done[k] = stop.value
                del waiting[k]
    return done


def fill_pool(pool, slots, params, seeds, backend=None, env=None, partition_backend=None):
    """Generate one level per logical slot of the refreshable ``LevelPool`` and hand them over as ``pool.prepare`` made
    them.  Without `env` they go into the host pool (``pool.replace``); with the ``SafeLifeVectorEnv`` that steps on the pool
    they are staged on the device (``env.pool_stage``, which does the replace), and the caller's ``env.pool_commit()`` makes
    them current between two steps.  Returns the new levels."""
    slots, seeds = list(slots), list(seeds)
    if len(slots) != len(seeds):
        raise ValueError("one seed per slot")
    prepared = pool.prepare(gen_games(params, seeds, backend=backend, partition_backend=partition_backend))
    if env is not None:
        if env.pool is not pool:
            raise ValueError("env steps on another pool")
        env.pool_stage(slots, prepared)
    else:
        pool.replace(slots, prepared)
    return prepared.levels
