"""
An exact reference for the earth-mover distance of side_effect_score, independent of both solvers of the package
(the host LP of side_effects.earth_mover_distance and the device solver csrc/sl_emd.hip): unit expansion + the
Hungarian method (scipy.optimize.linear_sum_assignment).

a, b are integer boards over one denominator.  Every unit of `a` at a participating cell becomes a row and every unit
of `b` a column of a rectangular assignment problem; the cost of a (row, column) pair is the ground distance between
their cells.  Nothing is cancelled (a cell with a = 5, b = 3 has five rows and three columns, at zero cost to each
other) and there is no dummy node (the rectangular assignment matches all of the smaller side: min(sum a, sum b)
units move).  The optimum is combinatorial, exact up to the one final float sum (math.fsum: correctly rounded).

The ground distance is the reference's formula (side_effects.py:38-56) written out on the pairs, NOT read out of
side_effects.ground_table: per axis the signed gap c_i - c_j, min(g, size - g) when the axis wraps and g > 0, then
manhattan or hypot, then tanh(d / scale).

Cost: O(units^3) worst case; keep a problem below about 2500 units per side.
"""
import math

import numpy as np

THRESHOLD = 1e-3


def participating(a, b, den):
    """Boolean [H,W]: the cells that take part, by the host formula (side_effects.py:30-33)."""
    gap = np.abs(np.asarray(a) / den - np.asarray(b) / den)
    return gap > THRESHOLD * gap.max()


def pair_costs(rows, cols, shape, metric="manhattan", wrap_x=True, wrap_y=True, tanh_scale=5.0):
    """Ground distance [n,n] from cell i to cell j of the cells (rows[k], cols[k]) of a board of `shape`."""
    H, W = shape
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    gy = rows[:, None] - rows[None, :]
    gx = cols[:, None] - cols[None, :]
    if wrap_y:
        gy = np.where(gy > 0, np.minimum(gy, H - gy), gy)
    if wrap_x:
        gx = np.where(gx > 0, np.minimum(gx, W - gx), gx)
    if metric == "manhattan":
        d = np.abs(gx).astype(np.float64) + np.abs(gy)
    elif metric == "euclidean":
        d = np.hypot(gx, gy)
    else:
        raise ValueError(metric)
    return np.tanh(d / tanh_scale)


def emd_reference(a, b, den, metric="manhattan", wrap_x=True, wrap_y=True, tanh_scale=5.0, penalty=1.0,
                  with_assignment=False):
    """dict(value, mass, n_cells, units) of the integer boards a, b over `den`; with_assignment adds `costs`, the
    cost of every matched (unit of a, unit of b) pair of one optimal assignment."""
    from scipy.optimize import linear_sum_assignment
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    assert a.shape == b.shape and a.ndim == 2 and a.min() >= 0 and b.min() >= 0
    out = dict(value=0.0, mass=float(a.sum()) / den, n_cells=0, units=0)
    if with_assignment:
        out["costs"] = np.zeros(0)
    rows, cols = np.nonzero(participating(a, b, den))
    if rows.size == 0:
        return out
    ua, ub = a[rows, cols], b[rows, cols]
    cell_cost = pair_costs(rows, cols, a.shape, metric, wrap_x, wrap_y, tanh_scale)
    src = np.repeat(np.arange(rows.size), ua)
    dst = np.repeat(np.arange(rows.size), ub)
    costs = np.zeros(0)
    if src.size and dst.size:
        matrix = cell_cost[np.ix_(src, dst)]
        ri, ci = linear_sum_assignment(matrix)
        assert ri.size == min(src.size, dst.size)
        costs = matrix[ri, ci]
    sa, sb = int(ua.sum()), int(ub.sum())
    out.update(value=math.fsum(costs) / den + penalty * abs(sa - sb) / den, n_cells=int(rows.size), units=max(sa, sb))
    if with_assignment:
        out["costs"] = costs
    return out


def device_tolerance(units, value):
    """How far an exact device value may be from the reference's: both are optima and differ by float64 rounding only
    -- of the f * cost terms, at most one per unit of flow, and of the 1-ulp tanh slack per unit."""
    return 4 * units * 2.0 ** -53 * max(1.0, abs(value))


def option_grid():
    """{manhattan, euclidean} x the four wrap combinations x tanh scale {2, 5} x penalty {0, 0.25, 1, 3}: the 16
    (metric, wrap_x, wrap_y) x scale tables, penalties cycled over them -- 32 option sets, each penalty with each metric,
    each wrap combination and each scale."""
    out = []
    for m, metric in enumerate(("manhattan", "euclidean")):
        for wrap_x in (True, False):
            for wrap_y in (True, False):
                for s, scale in enumerate((2.0, 5.0)):
                    # (the parity of the four choices picks the pair, so no single choice fixes it)
                    for penalty in ((0.0, 1.0), (0.25, 3.0))[(m + wrap_x + wrap_y + s) % 2]:
                        out.append(dict(metric=metric, wrap_x=wrap_x, wrap_y=wrap_y, tanh_scale=scale, penalty=penalty))
    return out


def random_problem(rng, shape, den, n, style=None):
    """Integer boards a, b in 0..den with about `n` differing cells (masks when den == 1)."""
    H, W = shape
    n = min(n, H * W)
    cells = rng.choice(H * W, size=n, replace=False)
    a = np.zeros(H * W, np.int64)
    b = np.zeros(H * W, np.int64)
    style = int(rng.integers(0, 4)) if style is None else style
    if den == 1:
        side = rng.random(n) < (0.5 if style < 2 else 0.3 + 0.1 * style)
        a[cells[side]] = 1
        b[cells[~side]] = 1
        same = rng.choice(H * W, size=min(H * W, 5), replace=False)      # cells present in both: no part of the problem
        same = np.setdiff1d(same, cells)
        a[same] = b[same] = 1
    elif style == 0:      # independent draws: most cells both supply and consume before cancelling
        a[cells] = rng.integers(0, den + 1, n)
        b[cells] = rng.integers(0, den + 1, n)
    elif style == 1:      # pure suppliers and pure consumers, unequal masses
        side = rng.random(n) < 0.5
        a[cells[side]] = rng.integers(1, den + 1, int(side.sum()))
        b[cells[~side]] = rng.integers(1, den + 1, int((~side).sum()))
    elif style == 2:      # small gaps on a large common background (some fall under the threshold when den is large)
        base = rng.integers(0, den, n)
        a[cells] = base
        b[cells] = np.clip(base + rng.integers(-2, 3, n), 0, den)
        k = cells[0]
        a[k], b[k] = den, 0
    else:                 # b a shifted copy of a: equal masses, structured optimum
        a[cells] = rng.integers(1, den + 1, n)
        b = np.roll(a.reshape(H, W), (int(rng.integers(-2, 3)), int(rng.integers(-2, 3))), (0, 1)).reshape(-1).copy()
    return a.reshape(H, W), b.reshape(H, W)
