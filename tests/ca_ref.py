"""One step of the cellular automaton and the occupancy count, restated by COUNTING -- whole-array numpy that shares
nothing with the oracle (oracle/sl_oracle.c), the kernels or safelife_amd.plane_sim, and does not follow the reference's
two-pass bit trick either (tests/test_ca_rule_host.py holds it to the reference's recorded output, bit for bit).

For each cell, over its nine cells on the torus (itself included):

    n_alive         the number of ALIVE cells
    pres, inh, spawn  whether any of the nine carries PRESERVING, INHIBITING, SPAWNING
    twice(bit)      whether at least two ALIVE cells of the nine carry the bit: the colour bits 9-11, and
                    "destructible or exit" (cell & 8 or cell & 256)
    spawn_colours   the OR of the colour bits of those of the nine that carry SPAWNING

    alive cell      kept if FROZEN (its own bit), or pres, or n_alive in {3, 4}; else it becomes 0
    dead cell       kept if FROZEN or inh;
                    else n_alive == 3: ALIVE | twice(colours) | spawn_colours | (DESTRUCTIBLE if twice(destructible-or-exit))
                    else spawn: one draw is consumed, whatever spawn_prob is; draw < float64(float32(p)):
                         ALIVE | DESTRUCTIBLE | twice(colours) | spawn_colours, otherwise kept
                    else kept

Draws are taken in row-major order of the cells that reach that branch, from np.random.Generator(bitgen).random().
Occupancy: after each step, counts[y, x, colour] += 1 for the cells that are ALIVE and carry none of AGENT, EXIT, FROZEN.

`step` takes optional `readings`: names of deliberately WRONG readings of the rule (WRONG_READINGS), which the host
tests show the fixture to tell apart from the rule.
"""
import numpy as np

ALIVE, AGENT, DESTRUCTIBLE, FROZEN, PRESERVING, INHIBITING, SPAWNING, EXIT = 1, 2, 8, 16, 32, 64, 128, 256
COLOURS = (0x200, 0x400, 0x800)
COLOUR_MASK = 0xE00

# what became of a cell in a step
A_FROZEN, A_PRESERVED, A_SURVIVES, A_DIES, D_FROZEN, D_INHIBITED, D_BORN, D_SPAWNED, D_DRAW_MISSED, D_STAYS = range(10)
OUTCOMES = ("alive: frozen", "alive: preserved", "alive: 3 or 4", "alive: dies", "dead: frozen", "dead: inhibited",
            "dead: born", "dead: spawned", "dead: draw missed", "dead: stays")

WRONG_READINGS = ("exit_not_in_vote", "strict_majority_no_spawn_colours", "centre_flags_not_counted",
                  "killed_keeps_bits", "newborn_keeps_residue", "frozen_from_neighbourhood", "no_draw_at_p0",
                  "occupancy_counts_agent_exit", "occupancy_mask_from_initial_board")

_OFFSETS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def _nine(a):
    """The nine torus shifts of [..., H, W]: element k holds, for every cell, its neighbour at _OFFSETS[k]."""
    return [np.roll(a, (-dy, -dx), axis=(-2, -1)) for dy, dx in _OFFSETS]


def gen_from_words(words):
    """np.random.Generator over a PCG64 at the state of four uint64 words (state hi, lo, increment hi, lo)."""
    w = [int(x) for x in words]
    bg = np.random.PCG64(0)
    st = bg.state
    st["state"]["state"] = (w[0] << 64) | w[1]
    st["state"]["inc"] = (w[2] << 64) | w[3]
    st["has_uint32"], st["uinteger"] = 0, 0
    bg.state = st
    return np.random.Generator(bg)


def words_of(gen):
    st = gen.bit_generator.state["state"]
    m = (1 << 64) - 1
    return np.array([st["state"] >> 64, st["state"] & m, st["inc"] >> 64, st["inc"] & m], np.uint64)


def step(boards, p, gens, readings=()):
    """One step of boards uint16 [B, H, W] at spawn_prob p [B], board b drawing from gens[b].
    -> (the new boards, the outcome of every cell: uint8 [B, H, W] of the codes above)."""
    b = np.asarray(boards, np.uint16).astype(np.int32)
    B = len(b)
    p = np.broadcast_to(np.asarray(p, np.float32), (B,)).astype(np.float64)       # float64(float32(p))
    own_flags = "centre_flags_not_counted" not in readings
    nine = _nine(b)
    n_alive = np.zeros(b.shape, np.int32)
    pres, inh, spawn = (np.zeros(b.shape, bool) for _ in range(3))
    votes = {bit: np.zeros(b.shape, np.int32) for bit in COLOURS}
    votes_dx = np.zeros(b.shape, np.int32)
    spawn_colours = np.zeros(b.shape, np.int32)
    frozen = (b & FROZEN) != 0
    for k, n in enumerate(nine):
        alive = (n & ALIVE) != 0
        n_alive += alive
        if own_flags or _OFFSETS[k] != (0, 0):
            pres |= (n & PRESERVING) != 0
            inh |= (n & INHIBITING) != 0
            spawn |= (n & SPAWNING) != 0
            spawn_colours |= np.where((n & SPAWNING) != 0, n & COLOUR_MASK, 0)
        for bit in COLOURS:
            votes[bit] += alive & ((n & bit) != 0)
        dx = (n & DESTRUCTIBLE) != 0
        if "exit_not_in_vote" not in readings:
            dx = dx | ((n & EXIT) != 0)
        votes_dx += alive & dx
        if "frozen_from_neighbourhood" in readings:
            frozen = frozen | ((n & FROZEN) != 0)
    if "strict_majority_no_spawn_colours" in readings:
        spawn_colours[:] = 0
    child = np.zeros(b.shape, np.int32)
    for bit in COLOURS:
        child |= np.where(votes[bit] >= 2, bit, 0)
    child |= spawn_colours
    born = ALIVE | child | np.where(votes_dx >= 2, DESTRUCTIBLE, 0)
    spawned = ALIVE | DESTRUCTIBLE | child
    if "newborn_keeps_residue" in readings:
        born, spawned = born | b, spawned | b

    is_alive = (b & ALIVE) != 0
    outcome = np.full(b.shape, D_STAYS, np.uint8)
    a_keep_count = (n_alive == 3) | (n_alive == 4)
    outcome[is_alive] = A_DIES
    outcome[is_alive & a_keep_count] = A_SURVIVES
    outcome[is_alive & pres] = A_PRESERVED
    outcome[is_alive & frozen] = A_FROZEN
    draws = ~is_alive & ~frozen & ~inh & (n_alive != 3) & spawn
    outcome[draws] = D_DRAW_MISSED
    outcome[~is_alive & ~frozen & ~inh & (n_alive == 3)] = D_BORN
    outcome[~is_alive & inh] = D_INHIBITED
    outcome[~is_alive & frozen] = D_FROZEN
    for k in range(B):
        if "no_draw_at_p0" in readings and p[k] == 0.0:
            continue
        cells = np.flatnonzero(draws[k])            # row-major
        if len(cells):
            hit = gens[k].random(len(cells)) < p[k]
            outcome[k].reshape(-1)[cells[hit]] = D_SPAWNED

    new = b.copy()
    new[outcome == A_DIES] = 0
    if "killed_keeps_bits" in readings:
        new = np.where(outcome == A_DIES, b & ~ALIVE, new)
    new = np.where(outcome == D_BORN, born, new)
    new = np.where(outcome == D_SPAWNED, spawned, new)
    return new.astype(np.uint16), outcome


def countable(boards, readings=()):
    """bool: the cells the occupancy count takes."""
    b = np.asarray(boards, np.uint16).astype(np.int32)
    if "occupancy_counts_agent_exit" in readings:
        return ((b & ALIVE) != 0) & ((b & FROZEN) == 0)
    return ((b & ALIVE) != 0) & ((b & (AGENT | EXIT | FROZEN)) == 0)


def trajectory(boards, p, words, n_steps, count_steps=(), keep=3, readings=(), count_dtype=np.uint8):
    """THE stepping and counting loop.  One run of n_steps steps answers every call on (boards, p, words) at once:
    advance_board and life_occupancy make the same draws step by step.  -> boards[s], words[s] after s = 0..n_steps steps
    (lists), counts[s] for the s of count_steps (uint8 by default: n_steps < 256), outcomes[s] of step s + 1; boards
    and outcomes only up to s = keep."""
    assert n_steps <= np.iinfo(count_dtype).max
    boards = np.array(boards, np.uint16)
    B, H, W = boards.shape
    gens = [gen_from_words(w) for w in words]
    out = dict(boards=[boards], words=[np.array(words, np.uint64).reshape(B, 4)], counts={}, outcomes=[])
    counts = np.zeros((B, H, W, 8), count_dtype)
    colour_of = np.arange(8)
    excluded0 = ((boards & ALIVE) != 0) & ~countable(boards)      # (only the wrong reading below looks at it)
    for s in range(1, n_steps + 1):
        boards, outcome = step(boards, p, gens, readings)
        if s <= keep:
            out["boards"].append(boards)
            out["outcomes"].append(outcome)
        out["words"].append(np.stack([words_of(g) for g in gens]))
        take = countable(boards, readings)
        if "occupancy_mask_from_initial_board" in readings:
            take = ((boards & ALIVE) != 0) & ~excluded0
        colour = (boards >> np.uint16(9)) & np.uint16(7)
        counts += take[..., None] & (colour[..., None] == colour_of)
        if s in count_steps:
            out["counts"][s] = counts.copy()
    return out


def advance(boards, p, n_steps, words, readings=()):
    """advance_board: n_steps steps (an int, or one count per board) -> (boards after, generator words after [B, 4])."""
    each = np.broadcast_to(np.asarray(n_steps), (len(boards),))
    top = int(each.max()) if len(each) else 0
    run = trajectory(boards, p, words, top, keep=top, readings=readings)
    return (np.stack([run["boards"][int(s)][b] for b, s in enumerate(each)]),
            np.stack([run["words"][int(s)][b] for b, s in enumerate(each)]))


def occupancy(boards, p, n_steps, words, readings=()):
    """life_occupancy: int32 [B, H, W, 8] counts of n_steps steps, and the generator words after."""
    run = trajectory(boards, p, words, n_steps, count_steps=(n_steps,), keep=0, readings=readings, count_dtype=np.int32)
    return run["counts"][n_steps], run["words"][n_steps]
