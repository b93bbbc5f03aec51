"""
Rendering on the host: the numpy path of safelife_amd.render against the frames the reference drew
(tests/golden/render_cases.npz, render_table.npz; written by tests/golden/make_golden_render.py), the sprite sheet
loader, the shape rules of speedups._render_board and the exported symbols.  No GPU.
"""
import ctypes
import os
import types

import numpy as np
import pytest

from safelife_amd import render, speedups, _hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_cases():
    cases = {}
    sheets = {}
    for fname in ("render_table.npz", "render_cases.npz"):
        with np.load(os.path.join(GOLDEN, fname)) as d:
            sheets["real"] = d["real_sheet"]
            sheets["synth"] = d["synth_sheet"] / np.float32(255)
            for name in d["cases"]:
                name = str(name)
                prefix = name + "_"
                cases[name] = {k[len(prefix):]: d[k] for k in d.files
                               if k.startswith(prefix) and k[len(prefix):] in
                               ("board", "goals", "sheet", "out", "orientation", "index", "view", "centers", "exits")}
    return cases, sheets


CASES, SHEETS = load_cases()


def host_render(case):
    """A fixture case through the host path."""
    sheet = SHEETS[str(case["sheet"])]
    board, goals = case["board"], case["goals"]
    if "index" in case:
        board = board[case["index"]]
        goals = goals if goals.ndim == 2 else goals[case["index"]]
    if "view" in case:
        frames = []
        for n in range(len(board)):
            H, W = board[n].shape
            cy, cx = case["centers"][n]
            e = case["exits"][n]
            e = e[e >= 0]
            game = types.SimpleNamespace(board=board[n], goals=goals[n],
                                         agent_locs=np.array([[cy, cx]] if cy >= 0 else []).reshape(-1, 2),
                                         exit_locs=(e // W, e % W))
            frames.append(render.render_game_host(game, tuple(case["view"]), sheet))
        return np.stack(frames)
    return render.render_board_host(board, goals, case.get("orientation"), sheet)


def test_fixture_has_the_cases():
    names = set(CASES)
    assert {"table_synth", "table_real", "shape_1x3x3", "shape_3x5x7", "shape_2x4x6", "shape_5x1x9",
            "shape_goals_broadcast", "shape_orientation", "shape_gather"} <= names
    assert sum(n.startswith("real_") for n in names) == 3
    assert sum(n.startswith("view_") for n in names) >= 15
    assert CASES["table_synth"]["out"].shape == (8, 20 * 14, 8 * 14, 3)
    assert any((c["exits"] < 0).any() for c in CASES.values() if "exits" in c)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_path_reproduces_reference(name):
    case = CASES[name]
    got = host_render(case)
    assert got.dtype == np.uint8 and got.shape == case["out"].shape
    assert np.array_equal(got, case["out"]), "%d bytes differ" % int(np.sum(got != case["out"]))


def test_table_tells_the_arithmetic_apart():
    """The synthetic sheet makes rounding visible: evaluating the blend in float64 changes bytes of the table, so the
    case above does pin the float32, unfused, left-to-right evaluation."""
    case = CASES["table_synth"]
    sheet = SHEETS["synth"].astype(np.float64)
    s = 14
    tiles = sheet.reshape(5, s, 5, s, 4).transpose(0, 2, 1, 3, 4).reshape(25, 1, 1, s, s, 4)
    mask, rgb = tiles[..., 3:4], tiles[..., 0:3]
    fg = render.foreground_colors.astype(np.float32).astype(np.float64).reshape(1, 8, 1, 1, 1, 3)
    bg = render.background_colors.astype(np.float32).astype(np.float64).reshape(1, 1, 8, 1, 1, 3)
    table = (255.0 * (bg * (1.0 - mask) + mask * rgb * fg)).astype(np.uint8)
    b, g = case["board"], case["goals"]
    img = table[render._tile_index(b), (b & 0xE00) >> 9, (g & 0xE00) >> 9]
    img = np.ascontiguousarray(np.moveaxis(img, -3, -4)).reshape(case["out"].shape)
    assert np.sum(img != case["out"]) > 0


def test_load_sprite_sheet():
    sheet = render.load_sprite_sheet()
    assert sheet.dtype == np.float32 and sheet.shape == (70, 70, 4)
    assert np.array_equal(sheet, SHEETS["real"])
    assert np.array_equal(render.load_sprite_sheet(render.DEFAULT_SPRITE_PATH), sheet)
    assert render.SPRITE_SIZE == 14
    assert render.foreground_colors.shape == (8, 3) and render.background_colors.shape == (8, 3)


def test_render_board_shapes_without_a_device(monkeypatch):
    monkeypatch.setattr(render, "_have_device", lambda: False)
    case = CASES["shape_3x5x7"]
    sheet = SHEETS["synth"]
    out = render.render_board(case["board"], case["goals"], sprite_sheet=sheet)
    assert np.array_equal(out, case["out"])
    one = render.render_board(case["board"][1], case["goals"][1], sprite_sheet=sheet)          # [H,W] -> [H*14,W*14,3]
    assert np.array_equal(one, case["out"][1])
    stacked = render.render_board(case["board"].reshape(3, 1, 5, 7), case["goals"].reshape(3, 1, 5, 7), sprite_sheet=sheet)
    assert stacked.shape == (3, 1, 70, 98, 3) and np.array_equal(stacked[:, 0], case["out"])
    buf = np.zeros_like(case["out"])
    assert render.render_board(case["board"], case["goals"], sprite_sheet=sheet, out=buf) is buf
    assert np.array_equal(buf, case["out"])


def test_speedups_render_board_rules(monkeypatch):
    monkeypatch.setattr(render, "_have_device", lambda: False)
    case = CASES["shape_2x4x6"]
    sheet = SHEETS["synth"]
    out = speedups._render_board(case["board"], case["goals"], sheet)
    assert out.dtype == np.uint8 and np.array_equal(out, case["out"])
    # sizes are compared, not shapes (module.c:469); the sheet may come flat
    assert np.array_equal(speedups._render_board(case["board"], case["goals"].reshape(-1), sheet.reshape(-1)), case["out"])
    with pytest.raises(ValueError, match="same size"):
        speedups._render_board(case["board"], case["goals"][:1], sheet)
    with pytest.raises(ValueError, match=r"\(70, 70, 4\)"):
        speedups._render_board(case["board"], case["goals"], sheet[:, :, :3])
    with pytest.raises(ValueError, match="two dimensions"):
        speedups._render_board(case["board"].reshape(-1), case["goals"].reshape(-1), sheet)


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("view_")))
def test_render_game_views(name, monkeypatch):
    monkeypatch.setattr(render, "_have_device", lambda: False)
    case = CASES[name]
    W = case["board"].shape[-1]
    cy, cx = case["centers"][0]
    e = case["exits"][0]
    e = e[e >= 0]
    game = types.SimpleNamespace(board=case["board"][0], goals=case["goals"][0],
                                 agent_locs=np.array([[cy, cx]] if cy >= 0 else [], np.int64).reshape(-1, 2),
                                 exit_locs=np.unravel_index(e, case["board"].shape[-2:]))
    assert np.array_equal(render.render_game(game, tuple(case["view"])), case["out"][0])
    whole = render.render_game(game)
    assert np.array_equal(whole, render.render_board_host(case["board"][0], case["goals"][0]))


def test_symbols_exported():
    assert "slhip_render_boards" in _hip.EXPORTS and "slhip_env_render" in _hip.EXPORTS
    lib = _hip.lib()                 # (loads the cross-compiled library; no device is touched)
    assert isinstance(lib, ctypes.CDLL)
    for name in ("slhip_render_boards", "slhip_env_render"):
        assert hasattr(lib, name), name
