"""
Writes tests/golden/emd_cases.npz: transport problems with the host LP's answer, for tests/test_emd.py.

Run once on a CPU (``python tests/golden/make_golden_emd.py``; the 64x64 case alone is minutes of HiGHS) and commit
the output.  A case is two integer boards ``a``, ``b`` over one denominator (the distributions are a / den, b / den:
occupancy counts over num_samples, or 0/1 masks over 1) and what ``side_effects.earth_mover_distance`` -- the FULL
n x n transportation LP over the participating cells, nothing cancelled -- returns for them.

    names [N]          case names
    shapes [N,2], den [N], offsets [N+1]    board a of case i = a_flat[offsets[i]:offsets[i+1]].reshape(shapes[i])
    a_flat, b_flat     int32
    value [N]          the LP of earth_mover_distance(a / den, b / den) (same cells, same matrix, method="highs"), solved
                       with HiGHS's feasibility tolerances at 1e-10 -- see REFERENCE_OPTIONS
    mass [N]           np.sum(a / den)
    n_cells [N]        participating cells
    spread [N]         n_cells <= 150: |highs-ds - highs-ipm| of the same LP; NaN above
    lp_spread          max of spread: how far two exact-in-principle LP solves of these problems differ

Cases: every (cell type) problem of the three committed side-effect fixtures; seeded random problems on 8x8 .. 25x25
boards; single-cell moves across each seam in both directions; equal boards; one-sided boards; 0/1 masks; non-square
shapes.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from safelife_amd import side_effects as se     # noqa: E402

SPREAD_MAX_N = 150
# tests/test_emd.py holds a device value to 1e-9 relative of the recorded one.  HiGHS stops at primal / dual
# feasibility tolerances of 1e-7 by default, which is coarser than that check: a reference that is to be compared at
# 1e-9 has to be solved below 1e-9.  On problems of a few hundred cells the defaults happen to land within 1e-14 of
# the optimum (lp_spread); on the 64x64 problem (1735 cells, 3 million variables) they stop at 9.846412666445385,
# 1.26e-8 above the 9.84641265387246 the same LP gives with the tolerances below.  Every case is recorded this way;
# test_fixture_values_are_the_host_lp checks that the package's own call agrees on the cases it can afford.
REFERENCE_OPTIONS = dict(primal_feasibility_tolerance=1e-10, dual_feasibility_tolerance=1e-10)


def participating(a, b):
    gap = np.abs(a - b)
    return np.nonzero(gap > 1e-3 * gap.max())


def lp(a, b, method, options=None):
    """earth_mover_distance's LP with the reference's defaults, by another HiGHS method / other solver options."""
    if np.abs(a - b).max() == 0:
        return 0.0
    rows, cols = participating(a, b)
    dist = se._ground_distance(rows, cols, a.shape, "manhattan", True, True, 5.0)
    return se._emd_hat(a[rows, cols], b[rows, cols], dist, 1.0, method=method, options=options)


def fixture_cases():
    def problems(tag, b0, b2, occ0, occ1, den):
        inaction, _ = se.distributions_from_counts(b0, b2, np.stack([occ0, occ1]), den)
        for key in inaction:
            key = int(key)
            if key & 0x1FF == int(se.CellTypes.life) and not key & int(se.CellTypes.frozen):
                i = (key >> int(se.CellTypes.color_bit)) & 7
                yield "%s/%s" % (tag, se.cell_name(key)), occ0[..., i], occ1[..., i], den
            else:
                yield "%s/%s" % (tag, se.cell_name(key)), (b0 == key).astype(np.int32), (b2 == key).astype(np.int32), 1
    for name in ("side_effect_inputs", "side_effect_inputs_64"):
        with np.load(os.path.join(HERE, name + ".npz")) as d:
            yield from problems(name, d["b0"], d["b2"], d["occ0"], d["occ1"], 1000)
    with np.load(os.path.join(HERE, "side_effect_inputs_multi.npz")) as d:
        for g in range(int(d["n_games"])):
            yield from problems("side_effect_inputs_multi/g%d" % g, d["g%d_b0" % g], d["g%d_b2" % g],
                                d["g%d_occ0" % g], d["g%d_occ1" % g], int(d["num_samples"]))


def random_cases():
    rng = np.random.default_rng(20261016)
    shapes = [(8, 8), (9, 13), (12, 12), (16, 16), (20, 20), (25, 25), (25, 25), (13, 9)]
    targets = [1, 2, 3, 5, 8, 12, 20, 30, 45, 60, 80, 100, 120, 150]
    for c in range(48):
        H, W = shapes[c % len(shapes)]
        n = min(targets[c % len(targets)], H * W)
        den = (1000, 200, 1000, 50)[c % 4]
        a, b = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
        cells = rng.choice(H * W, n, replace=False)
        style = c % 6
        for cell in cells:
            r, q = divmod(int(cell), W)
            if style == 0:          # occupancy-like: both sides present, small differences
                a[r, q] = rng.integers(0, den + 1)
                b[r, q] = np.clip(a[r, q] + rng.integers(-den // 4, den // 4 + 1), 0, den)
            elif style == 1:        # disjoint supports
                (a if rng.random() < 0.5 else b)[r, q] = rng.integers(1, den + 1)
            elif style == 2:        # much more mass in a
                a[r, q] = rng.integers(den // 2, den + 1)
                b[r, q] = rng.integers(0, den // 4 + 1)
            elif style == 3:        # much more mass in b
                b[r, q] = rng.integers(den // 2, den + 1)
                a[r, q] = rng.integers(0, den // 4 + 1)
            elif style == 4:        # differences of one count next to full ones: the 1e-3 threshold cuts
                a[r, q] = rng.integers(0, den + 1)
                b[r, q] = a[r, q] + (1 if rng.random() < 0.5 and a[r, q] < den else -int(a[r, q]))
                b[r, q] = max(int(b[r, q]), 0)
            else:                   # cells along the seams
                r2, q2 = (0 if rng.random() < 0.5 else H - 1), (0 if rng.random() < 0.5 else W - 1)
                if rng.random() < 0.5:
                    r2 = r
                else:
                    q2 = q
                (a if rng.random() < 0.5 else b)[r2, q2] += rng.integers(1, den // 2 + 1)
        yield "random%02d/style%d/%dx%d" % (c, style, H, W), a, b, den
    for c in range(6):              # 0/1 masks: things pushed about
        H, W = ((10, 10), (25, 25), (11, 17))[c % 3]
        a = (rng.random((H, W)) < 0.08).astype(np.int32)
        b = a.copy()
        for cell in np.flatnonzero(a)[: 3 + 4 * c]:
            r, q = divmod(int(cell), W)
            b[r, q] = 0
            if c != 4 or rng.random() < 0.5:        # (case 4: some are destroyed, not moved)
                b[(r + rng.integers(-2, 3)) % H, (q + rng.integers(-2, 3)) % W] = 1
        yield "mask%d/%dx%d" % (c, H, W), a, b, 1


def closed_form_cases():
    H, W = 6, 7
    def one(src, dst, units=7):
        a, b = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
        a[src], b[dst] = units, units
        return a, b
    # the seam cases of test_emd_restatement_known_answers and their row twins; den = 10: 0.7 of mass
    yield ("seam/col+2",) + one((1, 1), (1, 3)) + (10,)
    yield ("seam/col-2",) + one((1, 3), (1, 1)) + (10,)
    yield ("seam/col_1_to_6",) + one((1, 1), (1, 6)) + (10,)      # c_i < c_j: the long way, 5 columns
    yield ("seam/col_6_to_1",) + one((1, 6), (1, 1)) + (10,)      # c_i > c_j: min(5, 7 - 5) = 2
    yield ("seam/row_0_to_5",) + one((0, 2), (5, 2)) + (10,)      # 5 rows
    yield ("seam/row_5_to_0",) + one((5, 2), (0, 2)) + (10,)      # min(5, 6 - 5) = 1
    yield ("seam/both_0_0_to_5_6",) + one((0, 0), (5, 6)) + (10,)
    yield ("seam/both_5_6_to_0_0",) + one((5, 6), (0, 0)) + (10,)
    a, b = one((1, 6), (1, 1))
    b[4, 4] = 3                                                     # extra mass in b: + 1.0 * 0.3 (wait: den 10 -> 0.3)
    yield "seam/col_6_to_1_plus_extra", a, b, 10
    z = np.zeros((H, W), np.int32)
    yield "equal/zeros", z, z.copy(), 1000
    e = np.arange(H * W, dtype=np.int32).reshape(H, W) * 3
    yield "equal/ramp", e, e.copy(), 1000
    yield "onesided/b_zero", e, z.copy(), 1000
    yield "onesided/a_zero", z.copy(), e, 1000
    m = (e % 2).astype(np.int32)
    yield "onesided/mask_gone", m, z.copy(), 1


def main():
    cases = list(fixture_cases()) + list(random_cases()) + list(closed_form_cases())
    names, shapes, dens, a_flat, b_flat, value, mass, n_cells, spread = [], [], [], [], [], [], [], [], []
    for name, a, b, den in cases:
        a, b = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)
        fa, fb = a / den, b / den
        rows, _ = participating(fa, fb)
        n = int(rows.size)
        t0 = time.time()
        v = lp(fa, fb, "highs", REFERENCE_OPTIONS)
        s = np.nan
        if 0 < n <= SPREAD_MAX_N:
            s = abs(lp(fa, fb, "highs-ds") - lp(fa, fb, "highs-ipm"))
        elif n == 0:
            s = 0.0
        print("%-48s n=%4d value=%.12g spread=%.3g  (%.1f s)" % (name, n, v, s, time.time() - t0), flush=True)
        names.append(name), shapes.append(a.shape), dens.append(den), a_flat.append(a.ravel()), b_flat.append(b.ravel())
        value.append(v), mass.append(float(np.sum(fa))), n_cells.append(n), spread.append(s)
    offsets = np.concatenate([[0], np.cumsum([x.size for x in a_flat])]).astype(np.int64)
    out = os.path.join(HERE, "emd_cases.npz")
    np.savez_compressed(out, names=np.array(names), shapes=np.array(shapes, np.int32), den=np.array(dens, np.int32),
                        offsets=offsets, a_flat=np.concatenate(a_flat), b_flat=np.concatenate(b_flat),
                        value=np.array(value), mass=np.array(mass), n_cells=np.array(n_cells, np.int32),
                        spread=np.array(spread), lp_spread=np.array(np.nanmax(spread)))
    print("emd_cases: %d cases, lp_spread %.3g, %d bytes" % (len(names), np.nanmax(spread), os.path.getsize(out)))


if __name__ == "__main__":
    main()
