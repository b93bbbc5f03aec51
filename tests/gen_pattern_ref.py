"""The pattern sampler (the reference's speedups.gen_pattern) and numpy's two PCG64 draw paths, restated in plain Python
over lists -- shares nothing with safelife_amd/csrc/sl_gen_pattern_core.h or the kernel.  tests/test_gen_pattern_host.py
holds it to the compiled reference's recorded output (tests/golden/gen_pattern_cases.npz): board, status, iteration count
and the generator's six words.

The chain, per iteration:

    stop        when no cell is in the BAD set and the populated part of the NEW_CELL area has reached min_fill
    sample      a cell from BAD if it has members, else from SEEDS, else from UNMASKED; an EMPTY set hands out any of the
                layer's indices from its backing array.  The sampled cell leaves SEEDS, wherever it came from.
    price       empty: 2 below 90% of min_fill, 20 (1 - t) up to it, 0 above; wall / alive / tree: intercept + density * slope
    candidates  every NEW_CELL cell of the (2 depth + 1)^2 window, each of its three other cell types: swap it in, carry
                the change through the later layers by the SIMPLIFIED rule, count the change in violations and oscillating
                cells, swap back -- the swaps leave the stored violations of the cells they touched up to date
    pick        cumulative exp(log_prob - max), one uniform draw, the first candidate above it; that swap stays, and the
                cells it touched enter or leave BAD

Draws: `random_int` takes 32-bit values -- the LOW half of a 64-bit output first, the high half buffered for the next call
(has_uint32 / uinteger) -- masks them with the smallest all-ones mask >= high and rejects values >= high; the uniform draw
takes the top 53 bits of a fresh 64-bit output and leaves the buffer alone.

Each run also reports its MARGIN: the smallest |cum_probs[k] - target| / total over all iterations and candidates.  exp() is
the one operation that is not bit-defined across libraries; a pick can differ from another library's only when the margin is
within a few ulps times the number of candidates.

`readings`: names of deliberately WRONG readings (WRONG_READINGS) which the host tests show the fixture to tell apart.
"""
import math

import numpy as np

from tests import ca_ref

ALIVE, DESTRUCTIBLE, FROZEN = 1, 8, 16
NEW_CELL, CAN_OSCILLATE, INCLUDE_VIOLATIONS = 1, 2, 4
MAX_ITER = -1
CELL_OF_TYPE = (0, FROZEN, ALIVE | DESTRUCTIBLE, FROZEN | ALIVE)        # empty, wall, alive, tree
IS_OSC = 3

WRONG_READINGS = ("no_uint32_buffer", "seeds_not_discarded", "empty_set_size0", "penalties_in_keyword_order",
                  "penalties_not_converted", "layers_from_simplified_rule", "no_draw_at_p0")

_M64 = (1 << 64) - 1
_M128 = (1 << 128) - 1
_MULT = 0x2360ED051FC65DA44385DF649FCCF645


class Pcg64:
    """numpy's PCG64 from six words: state hi, lo, increment hi, lo, has_uint32, uinteger."""

    def __init__(self, words, buffered=True):
        w = [int(x) for x in words]
        self.state, self.inc = (w[0] << 64) | w[1], (w[2] << 64) | w[3]
        self.has_uint32, self.uinteger = w[4], w[5]
        self.buffered = buffered

    def words(self):
        return np.array([self.state >> 64, self.state & _M64, self.inc >> 64, self.inc & _M64,
                         self.has_uint32, self.uinteger], np.uint64)

    def next64(self):
        self.state = (self.state * _MULT + self.inc) & _M128
        hi, lo = self.state >> 64, self.state & _M64
        x, rot = hi ^ lo, hi >> 58
        return ((x >> rot) | (x << (64 - rot))) & _M64

    def next32(self):
        if self.has_uint32 and self.buffered:
            self.has_uint32 = 0
            return self.uinteger
        n = self.next64()
        if self.buffered:
            self.has_uint32, self.uinteger = 1, n >> 32
        return n & 0xFFFFFFFF

    def next_double(self):
        return (self.next64() >> 11) * (1.0 / 9007199254740992.0)

    def random_int(self, high):
        if high == 0:
            return 0
        mask = (1 << int(high).bit_length()) - 1            # smallest all-ones mask >= high
        while True:
            v = self.next32() & mask
            if v < high:
                return v


def words6(bitgen):
    """The six words of a numpy PCG64 BitGenerator."""
    st = bitgen.state
    s, i = st["state"]["state"], st["state"]["inc"]
    return np.array([s >> 64, s & _M64, i >> 64, i & _M64, st["has_uint32"], st["uinteger"]], np.uint64)


def set_words6(bitgen, words):
    w = [int(x) for x in words]
    st = bitgen.state
    st["state"]["state"], st["state"]["inc"] = (w[0] << 64) | w[1], (w[2] << 64) | w[3]
    st["has_uint32"], st["uinteger"] = w[4], w[5]
    bitgen.state = st


def penalties(alive=(0, 0), wall=(100, 100), tree=(100, 100), readings=()):
    """The keywords' (value at density 0, value at density 1) -> eight doubles, (intercept, slope) per cell type in the order
    empty, wall, alive, tree."""
    order = (alive, wall, tree) if "penalties_in_keyword_order" in readings else (wall, alive, tree)
    cp = [0.0, 0.0]
    for at0, at1 in order:
        at0, at1 = float(at0), float(at1)
        cp += [at0, at1 if "penalties_not_converted" in readings else at1 - at0]
    return np.array(cp, np.float64)


def layers_of(board, period, words, readings=()):
    """Layers 1 .. period-1: one step each of the FULL rule at spawn probability 0, drawing (and throwing away) what the
    spawners cost.  -> (int lists per layer, the six words after)."""
    layers = [np.array(board, np.uint16)]
    words = np.array(words, np.uint64)
    for _ in range(1, period):
        if "layers_from_simplified_rule" in readings:
            b = layers[-1].astype(np.int32)
            n = sum(np.roll(b & ALIVE, (dy, dx), (0, 1)) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
            alive, frozen = (b & ALIVE) != 0, (b & FROZEN) != 0
            new = np.where(frozen, b, np.where(alive, np.where((n == 3) | (n == 4), b, 0), np.where(n == 3, ALIVE, b)))
            layers.append(new.astype(np.uint16))
            continue
        sub = tuple(r for r in readings if r == "no_draw_at_p0")
        new, w4 = ca_ref.advance(layers[-1][None], np.float32(0.0), 1, words[None, :4], readings=sub)
        words = np.concatenate([w4[0], words[4:]])
        layers.append(new[0])
    return layers, words


class _ISet:
    def __init__(self, n):
        self.set, self.ptr, self.size, self.n = list(range(n)), list(range(n)), 0, n

    def _swap(self, k, val, top):
        y = self.set[top]
        self.set[top], self.ptr[val] = val, top
        self.set[k], self.ptr[y] = y, k

    def add(self, val):
        k = self.ptr[val]
        if k >= self.size:
            self._swap(k, val, self.size)
            self.size += 1

    def discard(self, val):
        k = self.ptr[val]
        if k < self.size:
            self.size -= 1
            self._swap(k, val, self.size)


def _violation(src, dst, n):
    if src & FROZEN:
        return int(src != dst)
    if src & ALIVE:
        return int((n == 3 or n == 4) != bool(dst & ALIVE))
    return int((n == 3) != bool(dst & ALIVE))


def _type(cell):
    return ((cell & ALIVE) << 1) | ((cell & FROZEN) >> 4)


def gen_pattern(board, mask, period, seeds=None, max_iter=40, min_fill=0.2, temperature=0.5, osc_bonus=0.3,
                alive=(0, 0), wall=(100, 100), tree=(100, 100), words=None, readings=()):
    """-> dict(board uint16 [H, W], status, iterations, words uint64 [6], margin).  `words`: the generator's six words."""
    board = np.array(board, np.uint16)
    H, W = board.shape
    L, D = H * W, int(period)
    msk = [int(x) for x in np.asarray(mask, np.int32).reshape(-1)]
    sds = msk if seeds is None else [int(x) for x in np.asarray(seeds, np.int32).reshape(-1)]
    cp = [float(x) for x in penalties(alive, wall, tree, readings)]
    layers, words = layers_of(board, D, words, readings)
    rng = Pcg64(words, buffered="no_uint32_buffer" not in readings)
    b = [int(x) for lay in layers for x in lay.reshape(-1)]

    def idx(layer, r, c):
        return (c % W) + ((r % H) + layer * H) * W

    nbr = [0] * (D * L)
    for layer in range(D):
        for r in range(H):
            for c in range(W):
                nbr[idx(layer, r, c)] = sum(b[idx(layer, r + dr, c + dc)] & ALIVE for dr in (-1, 0, 1) for dc in (-1, 0, 1))
    osc = [0] * L
    for layer in range(D):
        for k in range(L):
            osc[k] |= (b[k + layer * L] & ALIVE) + ALIVE
    last = (D - 1) * L
    viol = [0] * L
    bad, unmasked, seedset = _ISet(L), _ISet(L), _ISet(L)
    totals, area = [0, 0, 0, 0], 0
    for i in range(L):
        viol[i] = _violation(b[i + last], b[i], nbr[i + last])
        if sds[i]:
            seedset.add(i)
        if viol[i] and msk[i] & INCLUDE_VIOLATIONS:
            bad.add(i)
        if msk[i] & NEW_CELL:
            unmasked.add(i)
            area += 1
            totals[_type(b[i])] += 1

    def swap_single(layer, r, c, new):
        i0 = idx(layer, r, c)
        old = b[i0]
        if old == new:
            return 0
        b[i0] = new
        da = (new & ALIVE) - (old & ALIVE)
        if not da:
            return 1
        for rr in (r - 1, r, r + 1):
            for cc in (c - 1, c, c + 1):
                nbr[idx(layer, rr, cc)] += da
        return 2

    def swap_cells(r0, c0, new, track):
        x1 = x2 = c0
        y1 = y2 = r0
        did = swap_single(0, r0, c0, new)
        if did == 0:
            return 0, 0
        if did == 2:
            x1, y1, x2, y2 = x1 - 1, y1 - 1, x2 + 1, y2 + 1
        for layer in range(1, D):
            any_swap = 0
            r = y1
            while r <= y2:                      # the area grows while it is walked
                c = x1
                while c <= x2:
                    i1 = idx(layer - 1, r, c)
                    b1, n1 = b[i1], nbr[i1]
                    if b1 & FROZEN:
                        b2 = b1
                    elif b1 & ALIVE:
                        b2 = b1 if n1 in (3, 4) else 0
                    else:
                        b2 = ALIVE if n1 == 3 else b1
                    did = swap_single(layer, r, c, b2)
                    any_swap |= did
                    if did:
                        if c == x1:
                            x1 -= 1
                        if c == x2:
                            x2 += 1
                        if r == y1:
                            y1 -= 1
                        if r == y2:
                            y2 += 1
                    c += 1
                r += 1
            if not any_swap:
                break
        d_viol = d_osc = 0
        for r in range(y1, y2 + 1):
            for c in range(x1, x2 + 1):
                i1 = idx(0, r, c)
                b1 = b[i1]
                if b1 & FROZEN:
                    o = v = 0
                else:
                    o, b2, i2 = (b1 & ALIVE) + ALIVE, b1, i1
                    for _ in range(1, D):
                        i2 += L
                        b2 = b[i2]
                        o |= (b2 & ALIVE) + ALIVE
                    v = _violation(b2, b1, nbr[i2])
                if o == IS_OSC and not msk[i1] & CAN_OSCILLATE:
                    v += 1
                d_viol += v - viol[i1]
                d_osc += int(o == IS_OSC) - int(osc[i1] == IS_OSC)
                viol[i1], osc[i1] = v, o
                if track:
                    if v and msk[i1] & INCLUDE_VIOLATIONS:
                        bad.add(i1)
                    else:
                        bad.discard(i1)
        return d_viol, d_osc

    limit = int(np.float64(max_iter) * area * D)                # C truncation towards zero
    fill = float(np.float64(min_fill) * area)
    beta = float(np.float64(1.0) / np.float64(temperature)) if temperature != 0 else math.inf
    osc_bonus = float(osc_bonus)
    margin = math.inf
    it = 0
    while it < limit:
        not_empty = area - totals[0]
        if bad.size == 0 and not_empty >= fill:
            break
        s = bad if bad.size > 0 else seedset if seedset.size > 0 else unmasked
        n = s.size if (s.size or "empty_set_size0" in readings) else s.n
        k0 = s.set[rng.random_int(n)]
        if "seeds_not_discarded" not in readings:
            seedset.discard(k0)
        r0, c0 = divmod(k0, W)
        with np.errstate(all="ignore"):
            t = float(np.float64(not_empty) / np.float64(fill))
        pen = [2.0 if t < 0.9 else 20 * (1 - t) if t < 1 else 0.0]
        for j in (1, 2, 3):
            t = totals[j] / (not_empty + 1.0)
            pen.append(cp[2 * j] + t * cp[2 * j + 1])
        lps, types, cells = [], [], []
        for r in range(r0 - D, r0 + D + 1):
            for c in range(c0 - D, c0 + D + 1):
                i1 = idx(0, r, c)
                if not msk[i1] & NEW_CELL:
                    continue
                current = b[i1]
                start = _type(current) + 1
                dv = do = 0
                for j in range(start, start + 3):
                    target = CELL_OF_TYPE[j & 3]
                    a, o = swap_cells(r, c, target, False)
                    dv, do = dv + a, do + o
                    lp = float(dv)
                    lp -= osc_bonus * do
                    lp += pen[j & 3]
                    lp *= -beta
                    lps.append(lp)
                    types.append(target)
                    cells.append(i1)
                swap_cells(r, c, current, False)
        top = -1e100
        for lp in lps:
            if top < lp:
                top = lp
        total, cum = 0.0, []
        for lp in lps:
            total += math.exp(lp - top)
            cum.append(total)
        target = rng.next_double() * total
        if total > 0:
            for x in cum:
                margin = min(margin, abs(x - target) / total)
        for k, x in enumerate(cum):
            if x > target:
                cell = cells[k]
                old, new = b[cell], types[k]
                swap_cells(cell // W, cell % W, new, True)
                totals[_type(old)] -= 1
                totals[_type(new)] += 1
                break
        it += 1
    status = MAX_ITER if it == limit else 0
    out = np.array(b[:L], np.uint16).reshape(H, W) if status == 0 else board
    return dict(board=out, status=status, iterations=it, words=rng.words(), margin=margin)


# ---- the fixture -------------------------------------------------------------------------------------------------------------

ARG_NAMES = ("max_iter", "min_fill", "temperature", "osc_bonus")


def kwargs_of(args):
    """<case>_args float64 [10] -> the keywords of gen_pattern."""
    kw = dict(zip(ARG_NAMES, (float(x) for x in args[:4])))
    kw.update(alive=tuple(float(x) for x in args[4:6]), wall=tuple(float(x) for x in args[6:8]),
              tree=tuple(float(x) for x in args[8:10]))
    return kw


def load_cases(path):
    """tests/golden/gen_pattern_cases.npz -> a list of dicts: name, board, mask, seeds (or None), period, args, kwargs, w0, w1,
    status, out, iters, margin."""
    z = np.load(path)
    cases = []
    for name in z["cases"]:
        name = str(name)
        c = {k: z[name + "_" + k] for k in ("board", "mask", "args", "w0", "w1", "out")}
        c.update(name=name, period=int(z[name + "_period"]), status=int(z[name + "_status"]), iters=int(z[name + "_iters"]),
                 margin=float(z[name + "_margin"]), seeds=z[name + "_seeds"] if name + "_seeds" in z.files else None)
        c["kwargs"] = kwargs_of(c["args"])
        cases.append(c)
    return cases


def run_case(case, readings=()):
    return gen_pattern(case["board"], case["mask"], case["period"], seeds=case["seeds"], words=case["w0"], readings=readings,
                       **case["kwargs"])


def same_as_recorded(case, got):
    return (got["status"] == case["status"] and np.array_equal(got["board"], case["out"])
            and np.array_equal(got["words"], case["w1"]))
