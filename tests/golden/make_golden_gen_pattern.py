"""
Writes tests/golden/gen_pattern_cases.npz: what the REFERENCE's compiled speedups.gen_pattern makes of the constructed
problems below, for tests/test_gen_pattern_host.py (the restatement tests/gen_pattern_ref.py must reproduce every case) and
tests/test_gen_pattern_gpu.py.

Run once on a CPU with the reference extension built (``make -C oracle ref``, then
``python tests/golden/make_golden_gen_pattern.py``) and commit the output.  Every case is one call of its own on a numpy
PCG64 set to the case's six words (state hi, lo, increment hi, lo, has_uint32, uinteger); the words after the call are
recorded, also where the call ended in MaxIterException (status -1: the board is then the input board).

    cases                   the names, "p<period>-<H>x<W>-<what>"
    <case>_board            uint16 [H, W]       <case>_mask   int32 [H, W]      <case>_seeds  int32 [H, W] (absent: None)
    <case>_period           int
    <case>_args             float64 [10]: max_iter, min_fill, temperature, osc_bonus, alive (2), wall (2), tree (2)
    <case>_w0, <case>_w1    uint64 [6] before and after
    <case>_status           0 or -1             <case>_out    uint16 [H, W]
    <case>_iters, <case>_margin    from the restatement, which reproduced the case when this file was written: the
                            iterations run, and the smallest |cum_probs[k] - target| / total of the run

exp() is not bit-defined across libraries, so a case is kept only if its margin is at least MIN_MARGIN; one that is not moves
to the next generator seed.  Period 2-4 cases have max_iter cut so that no case runs more than ITER_CAP iterations.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle                                   # noqa: E402
from tests import gen_pattern_ref as gpr        # noqa: E402

MIN_MARGIN = 1e-12
ITER_CAP = 240
FULL = gpr.NEW_CELL | gpr.CAN_OSCILLATE | gpr.INCLUDE_VIOLATIONS
WALL, TREE, LIFE = 16, 17, 9
SPAWNER = 16 | 128 | 0x400          # frozen, spawning, one colour bit
GREEN_LIFE = 1 | 8 | 0x400
ARG_NAMES = ("max_iter", "min_fill", "temperature", "osc_bonus")


def mask_full(H, W):
    return np.full((H, W), FULL, np.int32)


def mask_region(H, W):
    """An interior region that takes new cells, a one-cell border that only reports violations, nothing outside."""
    m = np.zeros((H, W), np.int32)
    m[1:H - 1, 1:W - 2] = gpr.INCLUDE_VIOLATIONS
    m[2:H - 2, 2:W - 3] = FULL
    return m


def mask_no_osc(H, W):
    return np.full((H, W), gpr.NEW_CELL | gpr.INCLUDE_VIOLATIONS, np.int32)


def mask_zero(H, W):
    return np.zeros((H, W), np.int32)


def start_board(H, W):
    """Frozen cells, a spawner with dead cells around it (the layer pass draws for them), a blinker and a coloured cell."""
    b = np.zeros((H, W), np.uint16)
    b[0, :] = WALL
    b[H - 1, 0] = TREE
    b[H // 2, W // 2] = SPAWNER
    if H >= 8:
        b[2, 1:4] = LIFE
        b[H - 3, W - 3] = GREEN_LIFE
    return b


def mask_for(board, base):
    """`base` with NEW_CELL taken off the frozen cells (the coloured life cell keeps it)."""
    m = base.copy()
    m[(board & 16) != 0] &= ~gpr.NEW_CELL
    return m


def few_seeds(H, W):
    s = np.zeros((H, W), np.int32)
    s[H // 2, W // 2] = 1
    s[1, W - 2] = 5
    s[H - 2, 1] = -1
    return s


def problems():
    """(name, period, board, mask, seeds, kwargs, first generator seed, start with a buffered half)"""
    out = []

    def add(what, period, H, W, mask=None, board=None, seeds=None, seed=1, buffered=False, **kw):
        board = np.zeros((H, W), np.uint16) if board is None else board
        mask = mask_full(H, W) if mask is None else mask
        out.append(("p%d-%dx%d-%s" % (period, H, W, what), period, board, mask, seeds, kw, seed, buffered))

    # period 1: still lifes
    for s in (1, 2, 3):
        add("full-s%d" % s, 1, 3, 3, seed=s)
    for s in (1, 2):
        add("full-s%d" % s, 1, 4, 5, seed=10 + s)
    add("full", 1, 8, 8, seed=20)
    add("region", 1, 8, 8, mask=mask_region(8, 8), seed=21)
    add("no-osc", 1, 8, 8, mask=mask_no_osc(8, 8), seed=22)
    add("zero-mask", 1, 8, 8, mask=mask_zero(8, 8), seed=23)
    add("zero-mask-buffered", 1, 8, 8, mask=mask_zero(8, 8), seed=24, buffered=True)
    for s in (1, 2, 3):
        add("full-s%d" % s, 1, 10, 10, seed=30 + s)
    add("region", 1, 10, 10, mask=mask_region(10, 10), seed=34)
    add("region-seeds-few", 1, 10, 10, mask=mask_region(10, 10), seeds=few_seeds(10, 10), seed=35)
    add("seeds-few", 1, 10, 10, seeds=few_seeds(10, 10), seed=36)
    add("seeds-empty", 1, 10, 10, seeds=np.zeros((10, 10), np.int32), seed=37)
    sb = start_board(10, 10)
    add("start-board", 1, 10, 10, board=sb, mask=mask_for(sb, mask_full(10, 10)), seed=38)
    add("start-board-all-new", 1, 10, 10, board=sb, seed=39)
    add("min-fill-0", 1, 10, 10, seed=40, min_fill=0.0)
    add("min-fill-0-start-board", 1, 10, 10, board=sb, mask=mask_for(sb, mask_full(10, 10)), seed=41, min_fill=0.0)
    add("temp-0.1", 1, 10, 10, seed=42, temperature=0.1, max_iter=3)
    add("temp-1.5", 1, 10, 10, seed=43, temperature=1.5)
    add("buffered", 1, 10, 10, seed=44, buffered=True)
    add("walls-trees", 1, 10, 10, seed=45, wall=(1, 20), tree=(1, 20), min_fill=0.3)
    add("walls-cheap", 1, 10, 10, seed=46, wall=(0.5, 4), tree=(100, 100), alive=(0.25, 3), min_fill=0.4)
    add("trees-cheap", 1, 10, 10, seed=47, wall=(100, 100), tree=(0, 6), alive=(1, 0), min_fill=0.4, max_iter=4)
    add("max-iter-short", 1, 10, 10, seed=48, max_iter=0.05)
    add("fill-high", 1, 10, 10, seed=49, min_fill=0.45, max_iter=4)
    add("odd-shape", 1, 7, 11, seed=50)
    add("walls-trees", 1, 26, 26, seed=51, wall=(1, 20), tree=(1, 20), min_fill=0.1)

    # periods 2-4: oscillators, max_iter cut to ITER_CAP iterations
    def capped(what, period, H, W, iters=ITER_CAP, mask=None, **kw):
        mask = mask_full(H, W) if mask is None else mask
        area = int(((mask & gpr.NEW_CELL) != 0).sum())
        kw.setdefault("max_iter", iters / float(max(area, 1) * period) + 1e-9)
        add(what, period, H, W, mask=mask, **kw)

    for s in (1, 2, 3):
        capped("full-s%d" % s, 2, 3, 3, iters=60, seed=60 + s)
    capped("no-osc", 2, 3, 3, iters=60, mask=mask_no_osc(3, 3), seed=64)
    for s in (1, 2):
        capped("full-s%d" % s, 2, 5, 5, iters=120, seed=70 + s)
    capped("no-osc", 2, 5, 5, iters=120, mask=mask_no_osc(5, 5), seed=73)
    capped("seeds-few", 2, 5, 5, iters=120, seeds=few_seeds(5, 5), seed=74)
    capped("min-fill-0", 2, 5, 5, iters=120, seed=75, min_fill=0.0, seeds=few_seeds(5, 5))
    for s in (1, 2):
        capped("full-s%d" % s, 2, 10, 10, seed=80 + s)
    capped("region", 2, 10, 10, mask=mask_region(10, 10), seed=83)
    capped("no-osc", 2, 10, 10, mask=mask_no_osc(10, 10), seed=84)
    capped("start-board", 2, 10, 10, board=sb, mask=mask_for(sb, mask_full(10, 10)), seed=85)
    capped("start-board-buffered", 2, 10, 10, board=sb, mask=mask_for(sb, mask_full(10, 10)), seed=86, buffered=True)
    capped("temp-1.5", 2, 10, 10, seed=87, temperature=1.5)
    capped("temp-0.1", 2, 10, 10, seed=88, temperature=0.1, iters=120)
    capped("seeds-empty", 2, 10, 10, seed=89, seeds=np.zeros((10, 10), np.int32))
    capped("osc-bonus-1", 2, 10, 10, seed=90, osc_bonus=1.0, min_fill=0.05)
    capped("zero-mask-start-board", 2, 10, 10, board=sb, mask=mask_zero(10, 10), seed=91)
    sb45 = start_board(4, 5)
    for s in (1, 2):
        capped("full-s%d" % s, 3, 4, 5, iters=60, seed=100 + s)
    capped("no-osc", 3, 4, 5, iters=60, mask=mask_no_osc(4, 5), seed=103)
    capped("start-board", 3, 4, 5, iters=60, board=sb45, mask=mask_for(sb45, mask_full(4, 5)), seed=104)
    capped("full", 3, 8, 8, iters=60, seed=105)
    capped("full", 4, 5, 5, iters=30, seed=110)
    capped("start-board", 4, 8, 8, iters=30, board=start_board(8, 8), mask=mask_for(start_board(8, 8), mask_full(8, 8)),
           seed=111)
    return out


def start_words(seed, buffered):
    bg = np.random.PCG64(seed)
    if buffered:
        np.random.Generator(bg).integers(0, 1 << 32, dtype=np.uint32)       # one 32-bit draw: the other half stays buffered
        assert bg.state["has_uint32"] == 1
    return gpr.words6(bg)


def kwargs_of(args):
    kw = dict(zip(ARG_NAMES, (float(x) for x in args[:4])))
    kw.update(alive=tuple(args[4:6]), wall=tuple(args[6:8]), tree=tuple(args[8:10]))
    return kw


def main():
    oracle.build()
    sp = oracle.load_ref()
    assert sp is not None, "run `make -C oracle ref` first"
    bg = np.random.PCG64(0)
    sp.set_bit_generator(bg)
    out, names = {}, []
    for name, period, board, mask, seeds, kw, seed, buffered in problems():
        args = np.array([kw.get("max_iter", 40), kw.get("min_fill", 0.2), kw.get("temperature", 0.5), kw.get("osc_bonus", 0.3)]
                        + list(kw.get("alive", (0, 0))) + list(kw.get("wall", (100, 100))) + list(kw.get("tree", (100, 100))),
                        np.float64)
        while True:
            w0 = start_words(seed, buffered)
            gpr.set_words6(bg, w0)
            try:
                got = sp.gen_pattern(board.copy(), mask.copy(), period, seeds=None if seeds is None else seeds.copy(),
                                     **kwargs_of(args))
                status = 0
            except sp.MaxIterException:
                got, status = board, -1
            w1 = gpr.words6(bg)
            mine = gpr.gen_pattern(board, mask, period, seeds=seeds, words=w0, **kwargs_of(args))
            if mine["margin"] < MIN_MARGIN:
                print(name, "margin", mine["margin"], "-> next seed")
                seed += 1000
                continue
            assert mine["status"] == status and (mine["board"] == got).all() and (mine["words"] == w1).all(), name
            break
        names.append(name)
        out[name + "_board"], out[name + "_mask"], out[name + "_period"] = board, mask, np.int32(period)
        if seeds is not None:
            out[name + "_seeds"] = seeds
        out[name + "_args"], out[name + "_w0"], out[name + "_w1"] = args, w0, w1
        out[name + "_status"], out[name + "_out"] = np.int32(status), np.array(got, np.uint16)
        out[name + "_iters"], out[name + "_margin"] = np.int32(mine["iterations"]), np.float64(mine["margin"])
        print("%-36s status %2d  iterations %4d  changed %3d  buffered after %d  margin %.2e"
              % (name, status, mine["iterations"], int((got != board).sum()), int(w1[4]), mine["margin"]))
    out["cases"] = np.array(names)
    path = os.path.join(HERE, "gen_pattern_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
