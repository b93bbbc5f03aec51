"""
Writes tests/golden/obs_cases.npz: levels with several exits and the observation the REFERENCE returns for them, for
tests/test_obs_reference.py.

Runs only in the build container (``python tests/golden/make_golden_obs.py``): it imports the reference through
``make_golden.import_reference`` (the compiled extension of ``make -C oracle ref`` and the reference's own Python).  Every
output is ``SafeLifeEnv.get_obs`` of the reference (safelife_env.py:105-146) on a ``SafeLifeGame`` loaded from the case's
board, goals and agent; ``helper_utils.recenter_view`` on the same words is asserted to agree.  Inputs and the reference's
outputs only are stored.

``cases`` lists the names; ``channel_lists`` / ``channel_list_<name>`` the channel lists (``raw`` = None).  A case ``c`` has
    c_board, c_goals  uint16 [H,W]      c_agent  int32 [2] (y, x); (-1, -1): no agent
    c_exits  int32 [E] flat cells in the reference's order (row-major), -1 = unused slot (E = 8, or 9)
    c_view   int32 [2]                  c_channels  name of its channel list      c_rwg  remove_white_goals
    c_out    uint8 [vh,vw,C], or uint32 [vh,vw] for the raw view

Exit cells carry distinct colours and lie on random goals, so WHICH exit was painted on a perimeter cell shows.  The
generator asserts that everything the tests rely on actually occurs (``require`` below).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference    # noqa: E402

PLAYER, EXIT, WHITE = 122, 272, 0x0E00
#: board cells: empty mostly, walls, crates, life and trees in colours, a spawner, ice, a fountain (no agent, no exit)
PALETTE = np.array([0] * 10 + [16, 16, 16 | 4, 16 | 0x8000, 9, 9 | 0x200, 9 | 0x400, 9 | 0x800, 9 | 0xE00, 17 | 0x400, 152,
                    16 | 96 | 4, 48 | 0x600, 53, 85], np.uint16)

STD15 = tuple(range(12)) + (25, 26, 27)
STD19 = tuple(range(16)) + (25, 26, 27)
CHANNEL_LISTS = {
    "raw": None,
    "std15": STD15,
    "std19": STD19,
    "perm15": (25, 26, 27) + tuple(range(11, -1, -1)),                      # 15 entries, not the standard list
    "split19": (0, 2, 4, 6, 1, 3, 5, 7) + tuple(range(8, 16)) + (25, 26, 27),   # 19 entries, two non-consecutive fours
    "one": (8,),
    "three": (26, 1, 9),
    "twenty": tuple(range(16)) + (25, 26, 27, 28),
}

SHAPES = ((25, 25), (26, 26), (64, 64), (8, 8), (7, 11))
VIEWS = ((9, 9), (8, 6), (5, 8), (1, 1), (15, 9))
EXTRA_VIEWS = {(25, 25): ((33, 33), (25, 25)), (8, 8): ((9, 9), (8, 8))}    # larger than the board, and equal to it


def offsets(H, W, vh, vw, rng):
    """Exit positions relative to the view's centre, by what they exercise."""
    up, down, left, right = -(vh // 2), vh - 1 - vh // 2, -(vw // 2), vw - 1 - vw // 2      # the view's edge rows / columns
    return {
        "sides": [(up - 2, 0), (down + 2, 1), (0, left - 2), (-1, right + 2)],
        "corners": [(up - 1, left - 2), (up - 2, right + 1), (down + 1, left - 1), (down + 2, right + 2)],
        "pile_top": [(up - 1, 1), (up - 3, 1), (up - 2, 1)],                # three exits clipped to one cell
        "pile_corner": [(down + 1, right + 1), (down + 2, right + 3)],      # two on the corner cell
        "tie": [(H // 2, W // 2), (H // 2, 0), (0, W // 2)],                 # on even boards: exactly half a board away
        "inside": [(1, -1) if vh > 2 and vw > 2 else (0, 0)],
        "edge": [(up, 0), (down, -1 if vw > 1 else 0), (0, left), (1 if vh > 1 else 0, right)],
        "random": [tuple(int(v) for v in rng.integers(-32, 33, 2)) for _ in range(12)],
    }


def classify(case):
    """What a case exercises: a set of tags (see ``require`` in main)."""
    H, W = case["board"].shape
    vh, vw = (int(v) for v in case["view"])
    y0, x0 = (int(v) for v in case["agent"]) if case["agent"][0] >= 0 else (0, 0)
    e = case["exits"][case["exits"] >= 0].astype(np.int64)
    tags = {"shape_%dx%d" % (H, W), "view_%dx%d" % (vh, vw), "exits_%d" % len(e), "chan_" + str(case["channels"]),
            "rwg_%d" % int(case["rwg"])}
    if case["agent"][0] < 0:
        tags.add("no_agent")
    elif (y0, x0) == (0, 0):
        tags.add("agent_origin")
    elif (y0, x0) == (H - 1, W - 1):
        tags.add("agent_last_cell")
    if vh * vw % 4:
        tags.add("cells_not_multiple_of_4")
    if vh * vw % 16:
        tags.add("cells_not_multiple_of_16")
    if vh > H and vw > W:
        tags.add("view_larger_than_board")
    if (vh, vw) == (H, W):
        tags.add("view_equals_board")
    iy, ix = np.divmod(e, W)
    dy, dx = (iy - y0 + H // 2) % H - H // 2, (ix - x0 + W // 2) % W - W // 2
    uy, ux = dy + vh // 2, dx + vw // 2                 # before clipping
    above, below, lft, rgt = uy < 0, uy >= vh, ux < 0, ux >= vw
    rows_in, cols_in = ~above & ~below, ~lft & ~rgt
    for name, m in (("out_top", above & cols_in), ("out_bottom", below & cols_in), ("out_left", lft & rows_in),
                    ("out_right", rgt & rows_in), ("corner_tl", above & lft), ("corner_tr", above & rgt),
                    ("corner_bl", below & lft), ("corner_br", below & rgt)):
        if m.any():
            tags.add(name)
    seen = rows_in & cols_in
    if (seen & (uy > 0) & (uy < vh - 1) & (ux > 0) & (ux < vw - 1)).any():
        tags.add("exit_inside")
    if (seen & ((uy == 0) | (uy == vh - 1) | (ux == 0) | (ux == vw - 1))).any() and min(vh, vw) > 1:
        tags.add("exit_on_edge_unclipped")
    if H % 2 == 0 and W % 2 == 0 and ((dy == -(H // 2)) & (dx == -(W // 2))).any():
        tags.add("tie_both_axes")
    clipped = ~seen
    cells = list(zip(np.clip(uy, 0, vh - 1).tolist(), np.clip(ux, 0, vw - 1).tolist()))
    piles = {}
    for k, c in enumerate(cells):
        if clipped[k]:
            piles[c] = piles.get(c, 0) + 1
    if min(vh, vw) > 1 and any(n >= 2 for n in piles.values()):
        tags.add("two_on_one_cell")
    if min(vh, vw) > 1 and any(n >= 3 for n in piles.values()):
        tags.add("three_on_one_cell")
    if (clipped & ((case["goals"][iy, ix] & WHITE) == WHITE)).any():
        tags.add("white_goal_under_painted_exit_rwg_%d" % int(case["rwg"]))
    if ((case["goals"] & WHITE) == WHITE).any():
        tags.add("white_goals_rwg_%d" % int(case["rwg"]))
    return tags


def main():
    R = import_reference()
    from safelife.helper_utils import recenter_view
    Game, Env = R.game.SafeLifeGame, R.env.SafeLifeEnv
    rng = np.random.default_rng(20261018)
    cases, tags_of = {}, {}

    def add(name, H, W, view, agent, kinds, n_exits, channels, rwg):
        board = PALETTE[rng.integers(0, len(PALETTE), (H, W))]
        goals = (rng.integers(0, 8, (H, W)) * (rng.random((H, W)) < 0.6)).astype(np.uint16) << 9
        y0, x0 = agent if agent is not None else (0, 0)
        table = offsets(H, W, view[0], view[1], rng)
        want = [o for kind in kinds for o in table[kind]] + table["random"]
        cells = []
        for dy, dx in want:
            cell = ((y0 + dy) % H, (x0 + dx) % W)
            if cell not in cells and cell != agent and len(cells) < n_exits:
                cells.append(cell)
        while len(cells) < n_exits:                     # (small boards: the offsets collide)
            cell = (int(rng.integers(0, H)), int(rng.integers(0, W)))
            if cell not in cells and cell != agent:
                cells.append(cell)
        for k, (r, c) in enumerate(cells):
            board[r, c] = EXIT | ((1 + k % 7) << 9)     # distinct colours: which exit was painted shows
            if k % 3 == 0:
                goals[r, c] = WHITE                     # a white goal under an exit
        if agent is not None:
            board[agent] = PLAYER
        data = dict(board=board.copy(), goals=goals.copy(),
                    agent_locs=np.array([agent] if agent is not None else [], np.int64).reshape(-1, 2))
        game = Game.loaddata(data)
        # (loading repaints every exit in one colour and marks the agent as free to leave: the case's own cells go back
        #  in -- get_obs reads the game's board, goals, agent_locs and exit_locs, nothing else)
        game.board = board.copy()
        game.update_exit_locs()
        env = Env(iter(()), view_shape=tuple(view), output_channels=CHANNEL_LISTS[channels], remove_white_goals=bool(rwg),
                  should_calculate_side_effects=False)
        env.game = game
        out = env.get_obs()
        flat = np.ravel_multi_index(game.exit_locs, (H, W)).astype(np.int32)
        assert sorted(flat.tolist()) == sorted(r * W + c for r, c in cells) and np.all(np.diff(flat) > 0)
        # the same through helper_utils.recenter_view on the same words
        tint = goals.astype(np.uint32) & WHITE
        if rwg:
            tint = tint * (tint != WHITE)
        words = (board.astype(np.uint32) + (tint << 16)).astype(np.uint32)
        direct = recenter_view(words, tuple(view), (y0, x0), game.exit_locs)
        if CHANNEL_LISTS[channels]:
            shift = np.array(CHANNEL_LISTS[channels], np.uint32)
            direct = ((direct[..., None] & (1 << shift)) >> shift).astype(np.uint8)
        assert out.dtype == (np.uint8 if CHANNEL_LISTS[channels] else np.uint32), (name, out.dtype)
        assert direct.shape == out.shape and np.array_equal(direct, out), name
        assert np.array_equal(game.board, board) and np.array_equal(game.goals, goals)      # get_obs changed nothing
        E = max(8, len(flat))
        c = {"board": board, "goals": goals, "agent": np.array(agent if agent is not None else (-1, -1), np.int32),
             "exits": np.concatenate([flat, np.full(E - len(flat), -1, np.int32)]).astype(np.int32),
             "view": np.array(view, np.int32), "channels": np.array(channels), "rwg": np.array(bool(rwg)),
             "out": np.ascontiguousarray(out)}
        assert name not in cases
        cases[name], tags_of[name] = c, classify(c)

    chan_names = list(CHANNEL_LISTS)
    counts = (0, 1, 2, 3, 8)
    layouts = (("sides", "inside"), ("corners", "edge"), ("pile_top", "pile_corner", "tie"), ("tie", "edge", "sides"),
               ("pile_corner", "corners", "inside"))
    n = 0
    for H, W in SHAPES:
        agents = [(0, 0), (H - 1, W - 1), None, (H // 2, W // 3), (1, W - 2)]
        views = VIEWS + EXTRA_VIEWS.get((H, W), ())
        if (H, W) == (64, 64):
            views = VIEWS[:3] + ((15, 9),)              # (the big boards: fewer cases, the file stays small)
        for vi, view in enumerate(views):
            for rep in range(2 if (H, W) != (64, 64) else 1):
                agent = agents[(vi + 2 * rep + n) % len(agents)]
                ne = counts[(n + rep) % len(counts)]
                add("c%03d_%dx%d_v%dx%d_e%d" % (n, H, W, view[0], view[1], ne), H, W, view, agent,
                    layouts[(vi + rep) % len(layouts)], ne, chan_names[n % len(chan_names)], (n // 3 + rep) % 2 == 0)
                n += 1
    # what the rotation above does not reach by itself
    for H, W, view, agent, kinds, ne, chans, rwg in (
            (25, 25, (9, 9), (12, 12), ("pile_top", "pile_corner", "sides", "corners"), 9, "std15", True),   # E > 8
            (25, 25, (8, 6), (0, 0), ("pile_top", "corners", "sides"), 8, "std19", False),
            (26, 26, (8, 6), (25, 25), ("tie", "pile_top", "pile_corner"), 8, "std15", True),
            (26, 26, (9, 9), None, ("tie", "sides", "corners"), 8, "raw", False),
            (64, 64, (8, 6), (63, 63), ("tie", "pile_top", "corners", "sides"), 8, "std19", True),
            (8, 8, (5, 8), (7, 7), ("tie", "pile_top"), 3, "perm15", False),
            (7, 11, (5, 8), (6, 10), ("pile_top", "sides", "corners"), 8, "split19", True),
            (7, 11, (1, 1), None, ("sides",), 2, "twenty", False),
            (25, 25, (15, 9), (24, 24), ("pile_top", "sides", "edge"), 3, "one", False),
            (26, 26, (5, 8), (0, 0), ("corners", "pile_corner", "inside"), 8, "three", True)):
        add("c%03d_%dx%d_v%dx%d_e%d" % (n, H, W, view[0], view[1], ne), H, W, view, agent, kinds, ne, chans, rwg)
        n += 1

    have = set().union(*tags_of.values())
    require = (["shape_%dx%d" % s for s in SHAPES] + ["view_%dx%d" % v for v in VIEWS + ((33, 33),)]
               + ["exits_%d" % k for k in (0, 1, 2, 3, 8, 9)] + ["chan_" + k for k in CHANNEL_LISTS]
               + ["out_top", "out_bottom", "out_left", "out_right", "corner_tl", "corner_tr", "corner_bl", "corner_br",
                  "two_on_one_cell", "three_on_one_cell", "tie_both_axes", "exit_inside", "exit_on_edge_unclipped",
                  "agent_origin", "agent_last_cell", "no_agent", "cells_not_multiple_of_4", "cells_not_multiple_of_16",
                  "view_larger_than_board", "view_equals_board", "white_goals_rwg_0", "white_goals_rwg_1",
                  "white_goal_under_painted_exit_rwg_0", "white_goal_under_painted_exit_rwg_1"])
    missing = [t for t in require if t not in have]
    assert not missing, "the case set lacks: %s" % missing

    def both(*tags):
        return any(all(t in tg for t in tags) for tg in tags_of.values())
    assert both("shape_25x25", "view_33x33") and both("shape_8x8", "view_9x9") and both("shape_25x25", "exits_9")
    for shape in ("shape_26x26", "shape_64x64"):
        assert both(shape, "tie_both_axes"), shape
    for tag in sorted(have):
        print("%-40s %d cases" % (tag, sum(tag in tg for tg in tags_of.values())))

    arrays = {"cases": np.array(list(cases)), "channel_lists": np.array(list(CHANNEL_LISTS))}
    for k, v in CHANNEL_LISTS.items():
        arrays["channel_list_" + k] = np.array(v if v is not None else (), np.int32)
    for name, c in cases.items():
        for k, v in c.items():
            arrays["%s_%s" % (name, k)] = v
    path = os.path.join(HERE, "obs_cases.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d cases, %d bytes" % (os.path.basename(path), len(cases), os.path.getsize(path)))
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
