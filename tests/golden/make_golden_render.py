"""
Writes tests/golden/render_cases.npz and tests/golden/render_table.npz: boards with the frames the REFERENCE draws for
them, for tests/test_render_host.py and tests/test_render_gpu.py.

Runs only in the build container (``python tests/golden/make_golden_render.py``): it imports the compiled reference
extension through ``oracle.load_ref()`` and the reference's own ``render_graphics`` / ``helper_utils`` Python for the view
cases.  ``render_graphics`` imports imageio, which is not installed: a placeholder module hands it the sheet as PIL loads
it (mode LA -> RGBA).  Inputs and the reference's outputs only are stored.

Every case ``c`` of ``cases`` has
    c_board  uint16 [S,H,W]       c_goals uint16 [S,H,W] or [H,W] (one goal array under every frame)
    c_sheet  "real" | "synth"     which sheet it was drawn with (``real_sheet`` float32, ``synth_sheet`` uint8: / float32(255))
    c_out    uint8 [N,vh*14,vw*14,3]   what the reference drew
    optional: c_orientation int32 [N]; c_index int32 [N] (frames gathered from the S source frames);
              c_view int32 [2] with c_centers int32 [N,2] ((-1,-1): no agent) and c_exits int32 [N,E] (flat, -1 unused)

    table_*   the 20 tile cases x 8 foreground colours as a 20x8 board, x 8 goal colours as 8 frames; with the synthetic
              sheet of fractional values (render_table.npz: the case that pins the arithmetic) and with the shipped one
    real_*    whole boards of committed levels
    shape_*   seeded random cells of the 20 cases and random colours, shapes chosen for the kernel's paths
    view_*    the reference's render_game on a 7x9 board with three exits
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference    # noqa: E402

NAMED = [9, 1, 53, 32789, 17, 32884, 48, 16, 32788, 85, 152, 272, 144]
PLAYER = 122
#: the 20 tile cases: 13 named types, empty, an empty cell that carries other bits, the agent's four orientations, unknown
TILE_CASES = NAMED + [0, 1 << 12] + [PLAYER | (o << 12) for o in range(4)] + [64]
GREYS = np.array([0, 37, 85, 128, 200, 255], np.uint8)


def load_real_sheet(reference_root):
    from PIL import Image
    with Image.open(os.path.join(reference_root, "safelife", "sprites.png")) as im:
        return np.asarray(im.convert("RGBA"))


def fused_blend(board, goals, sheet):
    """The same frames with the blend's last multiply-add fused (one rounding): what the fixture must tell apart."""
    from safelife_amd import render
    s = 14
    tiles = sheet.astype(np.float32).reshape(5, s, 5, s, 4).transpose(0, 2, 1, 3, 4).reshape(25, 1, 1, s, s, 4)
    mask, rgb = tiles[..., 3:4], tiles[..., 0:3]
    fg = render.foreground_colors.astype(np.float32).reshape(1, 8, 1, 1, 1, 3)
    bg = render.background_colors.astype(np.float32).reshape(1, 1, 8, 1, 1, 3)
    left = (bg * (np.float32(1) - mask)).astype(np.float64)
    prod = (mask * rgb).astype(np.float64) * fg.astype(np.float64)       # exact in float64
    value = np.float32(255) * (left + prod).astype(np.float32)
    table = value.astype(np.uint8)
    img = table[render._tile_index(board), (board & 0xE00) >> 9, (goals & 0xE00) >> 9]
    H, W = board.shape[-2:]
    return np.ascontiguousarray(np.moveaxis(img, -3, -4)).reshape(board.shape[:-2] + (H * s, W * s, 3))


def main():
    R = import_reference()
    real_bytes = load_real_sheet("/root/reference")
    imageio = types.ModuleType("imageio")
    imageio.imread = lambda path: real_bytes
    sys.modules["imageio"] = imageio
    from safelife import render_graphics as rg
    ref_render = R.speedups._render_board

    rng = np.random.default_rng(20261017)
    synth_bytes = GREYS[rng.integers(0, len(GREYS), (70, 70, 4))]
    real_sheet = (real_bytes / np.float32(255)).astype(np.float32)
    synth_sheet = (synth_bytes / np.float32(255)).astype(np.float32)
    assert np.array_equal(real_sheet, rg.sprite_sheet)
    sheets = {"real": real_sheet, "synth": synth_sheet}

    cases = {}

    def add(name, board, goals, sheet, out, **extra):
        c = {"board": np.ascontiguousarray(board, np.uint16), "goals": np.ascontiguousarray(goals, np.uint16),
             "sheet": np.array(sheet), "out": np.ascontiguousarray(out, np.uint8)}
        for k, v in extra.items():
            c[k] = np.ascontiguousarray(v, np.int32)
        cases[name] = c
        print("%-28s board %-14s out %s" % (name, c["board"].shape, c["out"].shape))

    # ---- table
    colours = (np.arange(8, dtype=np.uint16) << 9)
    tboard = (np.array(TILE_CASES, np.uint16)[:, None] | colours[None, :])
    tboards = np.broadcast_to(tboard, (8, 20, 8)).copy()
    tgoals = np.broadcast_to(colours[:, None, None], (8, 20, 8)).copy()
    for sheet in ("synth", "real"):
        add("table_" + sheet, tboards, tgoals, sheet, ref_render(tboards, tgoals, sheets[sheet]))
    differ = int(np.sum(fused_blend(tboards, tgoals, synth_sheet) != cases["table_synth"]["out"]))
    print("a fused blend differs from the reference in %d bytes of table_synth" % differ)
    assert differ >= 1, "the synthetic sheet does not tell a fused blend from the reference's: it pins nothing"

    # ---- whole boards of committed levels
    def level_board(path, key_board, key_goals, pick=None):
        with np.load(os.path.join(HERE, path), allow_pickle=True) as d:
            b, g = d[key_board], d[key_goals]
        return (b, g) if pick is None else (b[pick], g[pick])
    for name, (b, g) in (("real_v10_prune_still", level_board("pool_prune_still_25.npz", "board", "goals", 3)),
                         ("real_ex_color_test", level_board("trace_ex_color_test.npz", "level0_board", "level0_goals")),
                         ("real_multi_asym1", level_board("trace_multi_asym1.npz", "level0_board", "level0_goals"))):
        add(name, b[None], g[None], "real", ref_render(b[None], g[None], real_sheet))

    # ---- shapes
    def random_cells(shape):
        cells = np.array(TILE_CASES, np.uint16)[rng.integers(0, 20, shape)]
        return cells | (rng.integers(0, 8, shape).astype(np.uint16) << 9)
    for N, H, W in ((1, 3, 3), (3, 5, 7), (2, 4, 6), (5, 1, 9)):
        b, g = random_cells((N, H, W)), rng.integers(0, 8, (N, H, W)).astype(np.uint16) << 9
        add("shape_%dx%dx%d" % (N, H, W), b, g, "synth", ref_render(b, g, synth_sheet))
    b, g = random_cells((4, 5, 6)), rng.integers(0, 8, (5, 6)).astype(np.uint16) << 9
    add("shape_goals_broadcast", b, g, "synth", ref_render(b, np.broadcast_to(g, b.shape).copy(), synth_sheet))
    b, g = random_cells((4, 4, 5)), rng.integers(0, 8, (4, 4, 5)).astype(np.uint16) << 9
    orientation = np.array([3, 0, 2, 1])
    rg.sprite_sheet = synth_sheet
    add("shape_orientation", b, g, "synth", rg.render_board(b.copy(), g, orientation), orientation=orientation)
    rg.sprite_sheet = real_sheet
    b, g = random_cells((6, 3, 5)), rng.integers(0, 8, (6, 3, 5)).astype(np.uint16) << 9
    index = np.array([4, 1, 5, 1, 0])
    add("shape_gather", b, g, "synth", ref_render(b[index], g[index], synth_sheet), index=index)

    # ---- views: the reference's render_game on a 7x9 board with three exits
    H, W = 7, 9
    exit_cell = 272
    vb = random_cells((H, W))
    vg = rng.integers(0, 8, (H, W)).astype(np.uint16) << 9
    # placements of the three exits (row, col), chosen against the agent positions below so that, over the cases, exits
    # fall outside the view on every side and past a corner, and two of them clip to the SAME perimeter cell
    layouts = {"a": [(0, 0), (6, 8), (3, 8)], "b": [(6, 0), (6, 1), (0, 4)], "c": [(3, 0), (0, 8), (1, 8)]}
    agents = {"corner": (0, 0), "centre": (3, 4), "none": None}
    for (vh, vw) in ((5, 5), (4, 6), (5, 9), (9, 11), (1, 1)):
        for aname, loc in agents.items():
            for lname, exits in layouts.items():
                if (vh, vw) != (5, 5) and lname != {"corner": "a", "centre": "b", "none": "c"}[aname]:
                    continue                                   # every layout x agent at 5x5, one pairing elsewhere
                board = vb.copy()
                ex = list(exits)
                if lname == "c":
                    ex = ex[:2]                                # (the third slot of this table is padding)
                for k, (r, c) in enumerate(ex):
                    board[r, c] = exit_cell | ((k + 1) << 9)   # distinct colours: which exit was painted shows
                if loc is not None:
                    board[loc] = PLAYER
                game = types.SimpleNamespace(
                    board=board, goals=vg, edit_color=0, edit_loc=(0, 0),
                    agent_locs=np.array([loc] if loc is not None else [], np.int64).reshape(-1, 2),
                    exit_locs=(np.array([r for r, _ in ex]), np.array([c for _, c in ex])))
                out = rg.render_game(game, (vh, vw))
                flat = [r * W + c for r, c in ex] + [-1] * (3 - len(ex))
                add("view_%dx%d_%s_%s" % (vh, vw, aname, lname), board[None], vg[None], "real", out[None],
                    view=[vh, vw], centers=[loc if loc is not None else (-1, -1)], exits=[flat])
    # two exits on one perimeter cell must actually occur
    hits = 0
    for name, c in cases.items():
        if "view" in c:
            vh, vw = c["view"]
            y0, x0 = c["centers"][0] if c["centers"][0][0] >= 0 else (0, 0)
            e = c["exits"][0]
            e = e[e >= 0]
            jy = np.clip((e // W - y0 + H // 2) % H - H // 2 + vh // 2, 0, vh - 1)
            jx = np.clip((e % W - x0 + W // 2) % W - W // 2 + vw // 2, 0, vw - 1)
            hits += len(set(zip(jy, jx))) < len(e) and min(vh, vw) > 1
    assert hits >= 1, "no view case clips two exits to one perimeter cell"
    print("%d view cases clip two exits to one cell" % hits)

    def save(path, names):
        arrays = {"cases": np.array(names), "real_sheet": real_sheet, "synth_sheet": synth_bytes}
        for n in names:
            for k, v in cases[n].items():
                arrays["%s_%s" % (n, k)] = v
        np.savez_compressed(path, **arrays)
        print("%s: %d cases, %d bytes" % (os.path.basename(path), len(names), os.path.getsize(path)))
        assert os.path.getsize(path) < (1 << 20)
    save(os.path.join(HERE, "render_table.npz"), ["table_synth"])
    save(os.path.join(HERE, "render_cases.npz"), [n for n in cases if n != "table_synth"])


if __name__ == "__main__":
    main()
