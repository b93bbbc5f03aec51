#!/usr/bin/env python3
"""
Writes tests/golden/ppo_loss_cases.npz by RUNNING THE REFERENCE's PPO.calculate_loss (training/ppo.py:145-166) and the split
rule of PPO.train_batch (:168-182) on the CPU: what slhip_ppo_loss_forward / _backward, safelife_amd.ppo.MinibatchDeal and
tests/ppo_loss_ref.py are held to.

    python tests/golden/make_golden_ppo_loss.py

Runs where make_golden.py runs (it needs the reference's Python, loaded through make_golden.import_reference()).

calculate_loss is called on a stub `self` whose `model` returns preset leaf tensors (values, policy), then loss.backward()
gives d loss / d values and d loss / d policy.  Every case runs twice on the same numbers: with float32 tensors -- what the
reference trains with -- and with the same float32 numbers widened to float64.  Per case (flat arrays; rows of case i at
[row_offsets[i], row_offsets[i+1]), its policy elements at [pol_offsets[i], pol_offsets[i+1])):
    n, n_actions, hyper [5] (eps_policy, eps_value, vf_coef, entropy_reg, entropy_clip), kink (1: a kink case), name
    values, policy, actions, action_prob, old_values, returns, advantages        the inputs (float32; actions int64)
    entropy32/64 [n], loss32/64, dvalues32/64 [n], dpolicy32/64 [n, A]           what the reference returned / autograd gave
    means32/64 [3]    mean policy loss, mean value loss, mean entropy: the reference's own sub-expressions, evaluated here
                      again (calculate_loss does not return them) and checked to recombine into its loss bit for bit
    branch32/64 uint8 [n, 3], flag32/64     which side of every kink the run took (see branches())

Random cases: rows 1, 63, 64, 65, 257 (four cases each: two with the mean entropy below entropy_clip, two above) and 4099
(one, above: its entropy gradient is zero, which keeps the fixture under the size limit -- 257 rows already span two
workgroups with the bonus on), 9 actions; 2 and 32 actions at 65 rows.  They are drawn so that the reference ALONE is well
conditioned: a row is drawn again while (in float64) sign(A)(1 - pi/pi_old) lies within 1e-3 of -eps_policy, |v - v_old|
within 1e-3 of eps_value, the value clamp is active and the two squared errors lie within a relative 1e-3 of each other, or
0 < |A| < 1e-3 (about one row in a hundred meets one of these, so a case of 4099 rows would never pass as a whole: the ROWS
are redrawn, then the whole case is checked); the whole case is drawn again while its mean entropy lies within 1e-3 of
entropy_clip.  The two runs must then take the same branch in every row (asserted).

Kink cases: 16 rows of dyadic numbers (eps_policy = eps_value = 0.25; probabilities, values and returns multiples of 2^-6),
on which float32 and float64 agree exactly about the side: advantage exactly 0, the policy clamp exactly at its edge (both
signs) and beyond it, v - v_old exactly +-eps_value and beyond, a clamped row whose two squared errors tie, rows with zero
probabilities (the 1e-12 guard), once with the mean entropy above the clip (bonus off) and once below; and a case of one-hot
policies with entropy_clip = 0, whose float32 mean entropy is exactly 0: AT the clip, where the clamp passes the gradient.

Split points: for a few (N, num_minibatches) the reference's train_batch is run for one epoch on a stub that records the
size of every minibatch it is asked about.
"""
import collections
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

DEFAULTS = (0.2, 0.2, 0.5, 0.01, 1.0)
SPLIT_PAIRS = ((1, 4), (3, 4), (4, 4), (5, 4), (80, 4), (260, 4), (1300, 4), (4099, 4), (65536, 4), (7, 1), (100, 8),
               (199, 7), (163840, 4))


def branches(np_, hyper, values, policy, actions, action_prob, old_values, returns, advantages):
    """uint8 [n, 3] and the flag, in the arrays' own precision:
    [:, 0] policy clamp: 0 not active (pd > -eps), 1 active (pd < -eps), 2 exactly at the edge
    [:, 1] value clamp: 0 strictly inside, 1 below -eps, 2 above +eps, 3 exactly -eps, 4 exactly +eps
    [:, 2] the maximum, where the clamp is active (1, 2): 0 the clipped error is larger, 1 the plain one, 2 a tie; else 3
    flag   1: mean entropy <= entropy_clip"""
    dt = values.dtype.type
    eps_p, eps_v, clip = dt(hyper[0]), dt(hyper[1]), dt(hyper[4])
    pa = policy[np.arange(len(actions)), actions]
    pd = np.sign(advantages) * (dt(1) - pa / action_prob)
    b = np.zeros((len(values), 3), np.uint8)
    b[:, 0] = np.where(pd < -eps_p, 1, np.where(pd == -eps_p, 2, 0))
    dv = values - old_values
    b[:, 1] = np.where(dv < -eps_v, 1, np.where(dv > eps_v, 2, np.where(dv == -eps_v, 3, np.where(dv == eps_v, 4, 0))))
    vc = old_values + np.clip(dv, -eps_v, eps_v)
    sa, sb = (vc - returns) ** 2, (values - returns) ** 2
    b[:, 2] = np.where((b[:, 1] == 1) | (b[:, 1] == 2), np.where(sa > sb, 0, np.where(sb > sa, 1, 2)), 3)
    return b, pd, dv, sa, sb


def run_reference(PPO, torch, hyper, arrays, dtype):
    """The reference's calculate_loss and backward on the arrays in `dtype` -> entropy, loss, d_values, d_policy, means."""
    t = {k: torch.tensor(v if k == "actions" else v.astype(dtype)) for k, v in arrays.items()}
    values, policy = t["values"].requires_grad_(), t["policy"].requires_grad_()
    stub = types.SimpleNamespace(model=lambda obs: (values, policy), eps_policy=hyper[0], eps_value=hyper[1], vf_coef=hyper[2],
                                 entropy_reg=hyper[3], entropy_clip=hyper[4])
    entropy, loss = PPO.calculate_loss(stub, None, t["actions"], t["action_prob"], t["old_values"], t["returns"],
                                       t["advantages"])
    loss.backward()
    with torch.no_grad():       # the reference's sub-expressions again, for the component means
        a_policy = torch.gather(policy, -1, t["actions"][..., np.newaxis])[..., 0]
        prob_diff = t["advantages"].sign() * (1 - a_policy / t["action_prob"])
        pm = (t["advantages"].abs() * torch.clamp(prob_diff, min=-hyper[0])).mean()
        v_clip = t["old_values"] + torch.clamp(values - t["old_values"], min=-hyper[1], max=+hyper[1])
        vm = torch.max((v_clip - t["returns"]) ** 2, (values - t["returns"]) ** 2).mean()
        em = entropy.mean()
        el = torch.clamp(em, max=hyper[4])
        el *= -hyper[3]
        again = pm + vm * hyper[2] + el
        assert again.dtype == loss.dtype and again.item() == loss.item(), (again.item(), loss.item())
    return dict(entropy=entropy.detach().numpy(), loss=loss.detach().numpy(), dvalues=values.grad.numpy(),
                dpolicy=policy.grad.numpy(), means=np.array([pm.item(), vm.item(), em.item()], np.float64))


def draw_rows(rng, n, A, scale, hyper):
    logits = rng.normal(0.0, scale, (n, A))
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    policy = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    actions = rng.integers(0, A, n).astype(np.int64)
    pa = policy[np.arange(n), actions]
    action_prob = (pa * np.exp(rng.normal(0.0, 0.25, n))).astype(np.float32).clip(1e-6, 1.0)
    advantages = rng.normal(0.0, 1.0, n)
    advantages[rng.random(n) < 0.05] = 0.0
    values = rng.normal(0.0, 1.0, n).astype(np.float32)
    old_values = (values + rng.normal(0.0, 0.25, n)).astype(np.float32)
    returns = (values + rng.normal(0.0, 0.5, n)).astype(np.float32)
    return dict(values=values, policy=policy, actions=actions, action_prob=action_prob, old_values=old_values,
                returns=returns, advantages=advantages.astype(np.float32))


def near_a_kink(hyper, arrays):
    """bool [n]: the rows the generator will not keep (float64)."""
    w = {k: (v if k == "actions" else v.astype(np.float64)) for k, v in arrays.items()}
    b, pd, dv, sa, sb = branches(np, hyper, **w)
    clamped = (b[:, 1] == 1) | (b[:, 1] == 2)
    adv = np.abs(w["advantages"])
    return ((np.abs(pd + hyper[0]) < 1e-3) | (np.abs(np.abs(dv) - hyper[1]) < 1e-3)
            | (clamped & (np.abs(sa - sb) <= 1e-3 * np.maximum(sa, sb))) | ((adv > 0) & (adv < 1e-3)))


def mean_entropy64(policy):
    p = policy.astype(np.float64)
    return float(np.sum(-p * np.log(p + 1e-12), axis=1).mean())


def random_case(rng, n, A, scale, hyper, want_flag):
    while True:
        arrays = draw_rows(rng, n, A, scale, hyper)
        for _ in range(1000):
            bad = near_a_kink(hyper, arrays)
            if not bad.any():
                break
            fresh = draw_rows(rng, int(bad.sum()), A, scale, hyper)
            for k in arrays:
                arrays[k][bad] = fresh[k]
        else:
            raise AssertionError("rows keep landing near a kink")
        em = mean_entropy64(arrays["policy"])
        if abs(em - hyper[4]) >= 1e-3 and (em <= hyper[4]) == want_flag:
            return arrays
        scale *= 1.25 if want_flag else 0.8         # sharper policies have less entropy


def kink_rows():
    """16 dyadic rows, 9 actions; eps_policy = eps_value = 0.25."""
    P = np.array([16, 8, 8, 8, 8, 4, 4, 4, 4], np.float64) / 64            # the ordinary row
    rows = []

    def row(policy=P, a=1, old_p=8 / 64, adv=1.0, v=1.0, old_v=1.0, ret=0.5):
        rows.append((np.asarray(policy, np.float64), a, old_p, adv, v, old_v, ret))

    row()                                                                   # 0 nothing special
    row(adv=0.0)                                                            # 1 advantage exactly 0
    row(adv=-0.0, v=1.5, old_v=1.0, ret=2.0)                                # 2 ... and -0, value clamped above
    row(policy=np.array([10, 8, 8, 8, 8, 6, 4, 4, 8]) / 64, a=0, adv=2.0)   # 3 pd = -0.25 exactly, A > 0
    row(policy=np.array([10, 8, 8, 8, 8, 6, 4, 4, 8]) / 64, a=5, adv=-0.5)  # 4 pd = -0.25 exactly, A < 0
    row(policy=np.array([12, 8, 8, 8, 8, 4, 4, 4, 8]) / 64, a=0, adv=1.5)   # 5 pd = -0.5: clamped, no gradient
    row(v=1.0, old_v=0.75, ret=0.25)                                        # 6 v - v_old = +0.25 exactly
    row(v=1.0, old_v=1.25, ret=1.5)                                         # 7 v - v_old = -0.25 exactly
    row(v=1.0, old_v=0.5, ret=0.875)                                        # 8 clamped above, the squared errors tie
    row(v=-1.0, old_v=-0.5, ret=-0.875, adv=-1.0)                           # 9 clamped below, tie
    row(v=1.0, old_v=0.5, ret=2.0)                                          # 10 clamped above, the clipped error larger
    row(v=1.0, old_v=0.5, ret=0.0)                                          # 11 clamped above, the plain error larger
    row(policy=np.array([0, 16, 16, 8, 8, 4, 4, 4, 4]) / 64, a=1, old_p=16 / 64)        # 12 a zero probability
    row(policy=np.array([0, 16, 16, 8, 8, 4, 4, 4, 4]) / 64, a=0, old_p=4 / 64)         # 13 ... taken: pi_a = 0
    row(policy=np.array([0, 0, 0, 0, 32, 0, 0, 32, 0]) / 64, a=4, old_p=32 / 64, adv=-1.0)  # 14 seven zeros
    row(adv=-3.0, v=0.0, old_v=0.0, ret=0.0)                                # 15 zero value error
    return rows


def pack(rows):
    f32 = np.float32
    return dict(values=np.array([r[4] for r in rows], f32), policy=np.stack([r[0] for r in rows]).astype(f32),
                actions=np.array([r[1] for r in rows], np.int64), action_prob=np.array([r[2] for r in rows], f32),
                old_values=np.array([r[5] for r in rows], f32), returns=np.array([r[6] for r in rows], f32),
                advantages=np.array([r[3] for r in rows], f32))


def kink_cases():
    rows = kink_rows()
    yield "kink-bonus-off", (0.25, 0.25, 0.5, 0.01, 1.0), pack(rows)
    yield "kink-bonus-on", (0.25, 0.25, 0.5, 0.01, 4.0), pack(rows)
    hot = []
    for i in range(16):
        p = np.zeros(9)
        p[i % 9] = 1.0
        hot.append((p, i % 9, (32, 64, 16, 48)[i % 4] / 64, (1.0, -1.0, 0.5, 0.0)[i % 4], 0.25 * i, 0.25 * i - 0.125, 1.0))
    yield "kink-entropy-at-clip", (0.25, 0.25, 0.5, 0.01, 0.0), pack(hot)


def make_cases():
    rng = np.random.default_rng(20261020)
    for n in (1, 63, 64, 65, 257):
        for j in range(4):
            on = j % 2 == 0
            yield "n%d-a9-%s-%d" % (n, "on" if on else "off", j // 2), DEFAULTS, random_case(rng, n, 9, 4.0 if on else 1.0,
                                                                                          DEFAULTS, on)
    yield "n4099-a9-off-0", DEFAULTS, random_case(rng, 4099, 9, 1.0, DEFAULTS, False)
    yield "n65-a2-on-0", DEFAULTS, random_case(rng, 65, 2, 1.0, DEFAULTS, True)
    low = DEFAULTS[:4] + (0.25,)
    yield "n65-a2-off-0", low, random_case(rng, 65, 2, 0.5, low, False)
    yield "n65-a32-on-0", DEFAULTS, random_case(rng, 65, 32, 6.0, DEFAULTS, True)
    yield "n65-a32-off-0", DEFAULTS, random_case(rng, 65, 32, 1.0, DEFAULTS, False)
    for case in kink_cases():
        yield case


def reference_splits(PPO, torch, N, m):
    """The sizes of the minibatches the reference's train_batch asks calculate_loss about in one epoch -> split points."""
    Batch = collections.namedtuple("Batch", "obs actions action_prob values returns advantages")
    sizes = []

    class Loss(object):
        def backward(self):
            pass

    def calculate_loss(obs, *rest):
        sizes.append(len(obs))
        return None, Loss()

    opt = types.SimpleNamespace(zero_grad=lambda: None, step=lambda: None)
    stub = types.SimpleNamespace(num_minibatches=m, epochs_per_batch=1, calculate_loss=calculate_loss, optimizer=opt)
    x = torch.zeros(N)
    PPO.train_batch(stub, Batch(x, x, x, x, x, x))
    assert len(sizes) == m + 1 and sum(sizes) == N
    return np.cumsum(sizes)[:-1].astype(np.int64)


def main():
    import make_golden
    from make_golden_gae import write_npz
    make_golden.import_reference()
    import torch
    from training.ppo import PPO
    PPO.compute_device = torch.device("cpu")
    torch.set_num_threads(1)

    meta = {k: [] for k in ("n", "n_actions", "hyper", "kink", "name", "loss32", "loss64", "means32", "means64", "flag32",
                            "flag64")}
    names = ("values", "policy", "actions", "action_prob", "old_values", "returns", "advantages", "entropy32", "entropy64",
             "dvalues32", "dvalues64", "dpolicy32", "dpolicy64", "branch32", "branch64")
    flat = {k: [] for k in names}
    row_offsets, pol_offsets = [0], [0]
    for name, hyper, arrays in make_cases():
        n, A = arrays["policy"].shape
        got = {}
        for tag, dtype in (("32", np.float32), ("64", np.float64)):
            got[tag] = out = run_reference(PPO, torch, hyper, arrays, dtype)
            assert out["entropy"].dtype == out["dvalues"].dtype == out["dpolicy"].dtype == out["loss"].dtype == dtype
            w = {k: (v if k == "actions" else v.astype(dtype)) for k, v in arrays.items()}
            out["branch"] = branches(np, hyper, **w)[0]
            out["flag"] = int(dtype(out["means"][2]) <= dtype(hyper[4]))
            # the flag is what the gradient shows: with the bonus off, no entropy gradient reaches a column not taken
            others = np.ones((n, A), bool)
            others[np.arange(n), arrays["actions"]] = False
            assert bool(np.any(out["dpolicy"][others] != 0)) == bool(out["flag"]), name
        assert np.array_equal(got["32"]["branch"], got["64"]["branch"]) and got["32"]["flag"] == got["64"]["flag"], name
        meta["n"].append(n), meta["n_actions"].append(A), meta["hyper"].append(hyper)
        meta["kink"].append(int(name.startswith("kink"))), meta["name"].append(name)
        for k in ("values", "policy", "actions", "action_prob", "old_values", "returns", "advantages"):
            flat[k].append(arrays[k].ravel())
        for tag in ("32", "64"):
            for k in ("entropy", "dvalues", "dpolicy", "branch"):
                flat[k + tag].append(got[tag][k].ravel())
            meta["loss" + tag].append(got[tag]["loss"]), meta["means" + tag].append(got[tag]["means"])
            meta["flag" + tag].append(got[tag]["flag"])
        row_offsets.append(row_offsets[-1] + n), pol_offsets.append(pol_offsets[-1] + n * A)
        print("%-22s n=%4d A=%2d flag=%d loss32=%.7g loss64=%.15g" % (name, n, A, got["32"]["flag"], got["32"]["loss"],
                                                                     got["64"]["loss"]), flush=True)
    out = dict(n=np.array(meta["n"], np.int64), n_actions=np.array(meta["n_actions"], np.int32),
               hyper=np.array(meta["hyper"], np.float64), kink=np.array(meta["kink"], np.uint8), name=np.array(meta["name"]),
               loss32=np.array(meta["loss32"], np.float32), loss64=np.array(meta["loss64"], np.float64),
               means32=np.array(meta["means32"], np.float64), means64=np.array(meta["means64"], np.float64),
               flag32=np.array(meta["flag32"], np.uint8), flag64=np.array(meta["flag64"], np.uint8),
               row_offsets=np.array(row_offsets, np.int64), pol_offsets=np.array(pol_offsets, np.int64))
    for k, parts in flat.items():
        out[k] = np.concatenate(parts)
    pts, offs = [], [0]
    for N, m in SPLIT_PAIRS:
        s = reference_splits(PPO, torch, N, m)
        pts.append(s), offs.append(offs[-1] + len(s))
    out.update(split_N=np.array([p[0] for p in SPLIT_PAIRS], np.int64), split_m=np.array([p[1] for p in SPLIT_PAIRS], np.int64),
               split_offsets=np.array(offs, np.int64), split_points=np.concatenate(pts))
    path = os.path.join(HERE, "ppo_loss_cases.npz")
    write_npz(path, out)
    print("ppo_loss_cases: %d cases, %d bytes" % (len(meta["n"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
