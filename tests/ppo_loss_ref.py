"""The PPO update restated in numpy: the loss of the reference's PPO.calculate_loss (training/ppo.py:145-166) with its
gradients WRITTEN OUT BY HAND -- no autograd, so the restatement shares nothing with torch's backward -- in float64 or in
float32, and the host model of the minibatch deal (keys, stable argsort, the reference's split points).  What the fixture
tests/golden/ppo_loss_cases.npz (the reference's own results) holds both this and the kernels of sl_ppo.hip to.

The conventions of torch's autograd the gradients follow: a clamp passes the gradient where its input EQUALS a bound, the
elementwise maximum gives each side half on a tie, sign(0) = 0, and a mean's backward divides by the number of rows.

WRONG_VARIANTS names deliberately wrong readings of the rule; ``loss_and_grads(..., **{variant: True})`` computes one."""
import os

import numpy as np

from tests import util

WRONG_VARIANTS = ("two_sided_policy_clamp", "min_of_value_errors", "entropy_clip_per_row", "clamp_blocks_at_equality")
HYPER = ("eps_policy", "eps_value", "vf_coef", "entropy_reg", "entropy_clip")
INPUTS = ("values", "policy", "actions", "action_prob", "old_values", "returns", "advantages")


def load_cases(path=None):
    z = np.load(path or os.path.join(util.GOLDEN, "ppo_loss_cases.npz"))
    ro, po = z["row_offsets"], z["pol_offsets"]
    cases = []
    for i, name in enumerate(z["name"]):
        n, A = int(z["n"][i]), int(z["n_actions"][i])
        c = dict(id=str(name), n=n, n_actions=A, hyper=tuple(float(x) for x in z["hyper"][i]), kink=bool(z["kink"][i]))
        for k in ("values", "actions", "action_prob", "old_values", "returns", "advantages", "entropy32", "entropy64",
                  "dvalues32", "dvalues64"):
            c[k] = z[k][ro[i]:ro[i + 1]]
        for k in ("policy", "dpolicy32", "dpolicy64"):
            c[k] = z[k][po[i]:po[i + 1]].reshape(n, A)
        for k in ("branch32", "branch64"):
            c[k] = z[k][3 * ro[i]:3 * ro[i + 1]].reshape(n, 3)
        for k in ("loss32", "loss64", "flag32", "flag64"):
            c[k] = z[k][i]
        c["means32"], c["means64"] = z["means32"][i], z["means64"][i]
        cases.append(c)
    return cases


def load_splits(path=None):
    z = np.load(path or os.path.join(util.GOLDEN, "ppo_loss_cases.npz"))
    o = z["split_offsets"]
    return [(int(N), int(m), z["split_points"][o[i]:o[i + 1]].tolist())
            for i, (N, m) in enumerate(zip(z["split_N"], z["split_m"]))]


def inputs(case, dtype):
    return {k: (case[k] if k == "actions" else case[k].astype(dtype)) for k in INPUTS}


def loss_and_grads(hyper, values, policy, actions, action_prob, old_values, returns, advantages, grad_loss=1.0,
                   grad_entropy=None, two_sided_policy_clamp=False, min_of_value_errors=False, entropy_clip_per_row=False,
                   clamp_blocks_at_equality=False):
    """-> dict(entropy [n], loss, means [3], flag, branch uint8 [n, 3], dvalues [n], dpolicy [n, A]) in the dtype of
    `values` (every scalar is rounded to it first, as a Python float meeting a torch tensor is)."""
    dt = values.dtype.type
    eps_p, eps_v, vf, reg, clip = (dt(x) for x in hyper)
    one, two, half = dt(1), dt(2), dt(0.5)
    n, A = policy.shape
    idx = np.arange(n)
    nf = dt(n)

    # ---- forward
    pa = policy[idx, actions]
    sg = np.sign(advantages)
    pd = sg * (one - pa / action_prob)
    if two_sided_policy_clamp:
        clamped = np.clip(pd, -eps_p, eps_p)
        pol_pass = (pd >= -eps_p) & (pd <= eps_p)
    else:
        clamped = np.maximum(pd, -eps_p)
        pol_pass = pd > -eps_p if clamp_blocks_at_equality else pd >= -eps_p
    pol = np.abs(advantages) * clamped

    dv = values - old_values
    vc = old_values + np.clip(dv, -eps_v, eps_v)
    ea, eb = vc - returns, values - returns
    sa, sb = ea * ea, eb * eb
    val = np.minimum(sa, sb) if min_of_value_errors else np.maximum(sa, sb)
    if clamp_blocks_at_equality:
        inside = (dv > -eps_v) & (dv < eps_v)
    else:
        inside = (dv >= -eps_v) & (dv <= eps_v)

    x = policy + dt(1e-12)
    L = np.log(x)
    terms = (-policy) * L
    ent = terms[:, 0].copy()
    for k in range(1, A):
        ent = ent + terms[:, k]

    pm, vm, em = pol.sum(dtype=np.float64) / n, val.sum(dtype=np.float64) / n, ent.sum(dtype=np.float64) / n
    if dt is np.float32:        # the reference's means are float32 numbers; the sums above are the better ones of the kernel
        pm, vm, em = dt(pm), dt(vm), dt(em)
    if entropy_clip_per_row:
        row_open = ent <= clip
        term = -reg * dt(np.where(row_open, ent, clip).sum(dtype=np.float64) / n)
        flag = bool(row_open.any())
    else:
        flag = bool(em <= clip)
        row_open = np.full(n, flag)
        term = -reg * (em if flag else clip)
    loss = dt(pm + vf * vm + term)

    branch = np.zeros((n, 3), np.uint8)
    branch[:, 0] = np.where(pd < -eps_p, 1, np.where(pd == -eps_p, 2, 0))
    branch[:, 1] = np.where(dv < -eps_v, 1, np.where(dv > eps_v, 2, np.where(dv == -eps_v, 3, np.where(dv == eps_v, 4, 0))))
    active = (branch[:, 1] == 1) | (branch[:, 1] == 2)
    branch[:, 2] = np.where(active, np.where(sa > sb, 0, np.where(sb > sa, 1, 2)), 3)

    # ---- backward, by hand
    g = dt(grad_loss)
    gp = g / nf
    gv = (g * vf) / nf
    ge = np.where(row_open, (g * -reg) / nf, dt(0)).astype(values.dtype)
    if grad_entropy is not None:
        ge = ge + grad_entropy.astype(values.dtype)

    t = np.where(pol_pass, gp * np.abs(advantages), dt(0))
    dpa = (-(t * sg)) / action_prob

    if min_of_value_errors:
        ga = np.where(sa < sb, gv, np.where(sa == sb, gv * half, dt(0)))
        gb = np.where(sb < sa, gv, np.where(sa == sb, gv * half, dt(0)))
    else:
        ga = np.where(sa > sb, gv, np.where(sa == sb, gv * half, dt(0)))
        gb = np.where(sb > sa, gv, np.where(sa == sb, gv * half, dt(0)))
    dvalues = np.where(inside, ga * (two * ea), dt(0)) + gb * (two * eb)

    gek = ge[:, None]
    dpolicy = (-(gek * L)) + (gek * (-policy)) / x
    dpolicy[idx, actions] += dpa
    return dict(entropy=ent, loss=loss, means=np.array([pm, vm, em], np.float64), flag=int(flag), branch=branch,
                dvalues=dvalues.astype(values.dtype), dpolicy=dpolicy.astype(values.dtype))


# ---------------------------------------------------------------------------------------------------------------- the deal

G64, MIX, M64 = 0x9E3779B97F4A7C15, 0x100000001B3, (1 << 64) - 1


def key(seed, epoch, i):
    """Key i of an epoch in Python integers: splitmix64's finalizer of seed + G * (epoch * MIX + i + 1) mod 2^64."""
    z = (seed + G64 * ((epoch * MIX + i + 1) & M64)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def keys(num_rows, seed, epoch):
    i = np.arange(num_rows, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) + np.uint64(G64) * (np.uint64((epoch * MIX) & M64) + i + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def split_points(num_rows, num_minibatches, pieces_equal_minibatches=False):
    """Where train_batch cuts: np.linspace(0, N, m + 2, dtype=int)[1:-1] -- m + 1 pieces.  In integers: linspace computes
    k * (N / (m + 1)) in float64 and truncates; an exact multiple comes out exact and nothing else can round up across an
    integer for N below 2^52, so the points are k * N // (m + 1)."""
    pieces = num_minibatches if pieces_equal_minibatches else num_minibatches + 1
    return [k * num_rows // pieces for k in range(1, pieces)]


def permutation(num_rows, seed, epoch):
    """The stable argsort of the keys, compared as two's-complement int64 (how torch.sort reads them)."""
    return np.argsort(keys(num_rows, seed, epoch).view(np.int64), kind="stable").astype(np.int64)


def deal(num_rows, num_minibatches, seed, epoch):
    """The pieces of an epoch, zero-row pieces left out."""
    perm = permutation(num_rows, seed, epoch)
    bounds = [0] + split_points(num_rows, num_minibatches) + [num_rows]
    return [perm[lo:hi] for lo, hi in zip(bounds[:-1], bounds[1:]) if hi > lo]
