"""
The observation of one environment, written a second time in plain numpy: what ``SafeLifeEnv.get_obs`` of the reference
computes (safelife_env.py:105-146 with helper_utils.py:42-75) from the state arrays the device holds.  numpy only: nothing
here comes from ``safelife_amd`` or ``oracle``, and nothing is shaped like the kernels -- whole-array word building, a
``np.take(mode="wrap")`` crop, ONE fancy assignment for the exits (so "the last exit wins" is numpy's rule, not a loop's),
a broadcast shift for the channels and a transpose for the policy layout.

``MUTANTS`` names deliberate mistakes a kernel could make; ``get_obs(..., mutant=name)`` makes that mistake.  The fixture
of tests/golden/make_golden_obs.py must tell every one of them from the reference's output (tests/test_obs_reference.py).
"""
import numpy as np

COLOURS = 0x0E00            # the three colour bits of a cell; all set = white

#: the two channel lists the kernels know at compile time (training: bits 0-11 + goal colour; default: 0-15 + goal colour)
STD15 = tuple(range(12)) + (25, 26, 27)
STD19 = tuple(range(16)) + (25, 26, 27)

MUTANTS = ("first_exit_wins", "no_clipping", "tie_to_plus_half", "view_half_rounded_down", "exit_shows_cell_under_it",
           "white_goal_kept_under_exit", "policy_xy_swapped", "empty_slot_is_last_cell")


def view_words(board, goals, remove_white_goals=True):
    """uint32 [H,W]: the cell in the low half, the goal's colour bits in the high half; white goals dropped on request."""
    tint = np.asarray(goals).astype(np.uint32) & np.uint32(COLOURS)
    if remove_white_goals:
        tint = tint * (tint != COLOURS)
    return np.asarray(board).astype(np.uint32) | (tint << np.uint32(16))


def get_view(board, goals, agent_loc, exit_locs, view_shape, remove_white_goals=True, mutant=None):
    """uint32 [vh,vw]: the board seen from `agent_loc` ((y, x); None or negative = no agent: seen from (0, 0)), exits that
    fall outside painted on the perimeter.  `exit_locs`: flat cell indices in painting order, negative = unused slot."""
    assert mutant is None or mutant in MUTANTS, mutant
    H, W = np.shape(board)
    vh, vw = (int(v) for v in view_shape)
    y0, x0 = (0, 0) if agent_loc is None or int(agent_loc[0]) < 0 else (int(agent_loc[0]), int(agent_loc[1]))
    hh, hw = (vh // 2, vw // 2) if mutant != "view_half_rounded_down" else ((vh - 1) // 2, (vw - 1) // 2)
    words = view_words(board, goals, remove_white_goals)
    rows, cols = y0 - hh + np.arange(vh), x0 - hw + np.arange(vw)
    view = np.take(np.take(words, rows, axis=0, mode="wrap"), cols, axis=1, mode="wrap")

    flat = np.asarray(exit_locs, np.int64).ravel()
    if mutant == "empty_slot_is_last_cell":
        flat = np.where(flat < 0, H * W - 1, flat)
    flat = flat[flat >= 0]
    if mutant == "first_exit_wins":
        flat = flat[::-1]
    iy, ix = np.divmod(flat, W)
    if mutant == "tie_to_plus_half":        # offsets in (-H/2, H/2] instead of [-H/2, H/2)
        dy, dx = (iy - y0) % H, (ix - x0) % W
        dy, dx = np.where(2 * dy > H, dy - H, dy), np.where(2 * dx > W, dx - W, dx)
    else:
        dy, dx = (iy - y0 + H // 2) % H - H // 2, (ix - x0 + W // 2) % W - W // 2
    jy, jx = dy + hh, dx + hw
    if mutant == "no_clipping":
        seen = (jy >= 0) & (jy < vh) & (jx >= 0) & (jx < vw)
        jy, jx, iy, ix = jy[seen], jx[seen], iy[seen], ix[seen]
    jy, jx = np.clip(jy, 0, vh - 1), np.clip(jx, 0, vw - 1)
    paint = words if mutant != "white_goal_kept_under_exit" else view_words(board, goals, False)
    if mutant == "exit_shows_cell_under_it":
        iy, ix = rows[jy] % H, cols[jx] % W
    view[jy, jx] = paint[iy, ix]
    return view


def channel_bits(view, channels):
    """uint8 [..., C]: bit channels[c] of every word; the words themselves for ``channels=None``."""
    if channels is None or len(channels) == 0:
        return view
    shifts = np.asarray(channels, np.uint32)
    return ((view[..., None] >> shifts) & np.uint32(1)).astype(np.uint8)


def get_obs(board, goals, agent_loc, exit_locs, view_shape, channels, remove_white_goals=True, mutant=None):
    """``SafeLifeEnv.get_obs`` of a single agent: uint8 [vh,vw,C], or the uint32 view for ``channels=None``."""
    return channel_bits(get_view(board, goals, agent_loc, exit_locs, view_shape, remove_white_goals, mutant), channels)


def policy_layout(obs, dtype=np.uint8, mutant=None):
    """The observation as the policy network takes it (training/models.py:100-103: ``obs.transpose(-1, -3)``):
    [C, vw, vh] of `dtype`."""
    order = (2, 1, 0) if mutant != "policy_xy_swapped" else (2, 0, 1)
    return np.ascontiguousarray(np.transpose(obs, order)).astype(dtype)


def first_difference(got, want):
    """None when equal; otherwise a short text naming the first differing element (index and both values)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape %s != %s" % (got.shape, want.shape)
    bad = np.argwhere(got != want)
    if not len(bad):
        return None
    at = tuple(int(i) for i in bad[0])
    return "%d elements differ, first at %s: got %s, want %s" % (len(bad), at, got[at], want[at])
