"""The PPO update on the device (safelife_amd/ppo.py, sl_ppo.hip) against the reference's own results
(tests/golden/ppo_loss_cases.npz) and the host models of tests/ppo_loss_ref.py.

Bounds.  Every quantity of the fused loss is compared with the reference's FLOAT64 run.  The bound is twice the largest
deviation the reference's own float32 run shows from its float64 run over the fixture's cases of the same row count, and
never below one float32 ulp of the float64 value.  Twice: the kernel's per-row arithmetic IS the reference's float32
arithmetic, its sums are better than float32, and only `log` and the order of a few multiplications in the gradient may
differ.  BOUNDS below is computed from the fixture when the module loads; every test prints its figures before asserting.

Measured on an MI355X: see DESIGN.md section 6e."""
import collections
import os

import numpy as np
import pytest

from safelife_amd import _hip
from tests import ppo_loss_ref as ref
from tests import util

pytestmark = pytest.mark.gpu

HAVE = os.path.exists(os.path.join(util.GOLDEN, "ppo_loss_cases.npz"))
CASES = ref.load_cases() if HAVE else []
IDS = [c["id"] for c in CASES]
Batch = collections.namedtuple("Batch", "obs actions action_prob returns advantages values")
QUANTITIES = ("loss", "policy_mean", "value_mean", "entropy_mean", "entropy", "dvalues", "dpolicy")


def fixture_quantities(c, tag):
    m = c["means" + tag]
    return dict(loss=np.float64(c["loss" + tag]), policy_mean=m[0], value_mean=m[1], entropy_mean=m[2],
                entropy=c["entropy" + tag].astype(np.float64), dvalues=c["dvalues" + tag].astype(np.float64),
                dpolicy=c["dpolicy" + tag].astype(np.float64))


def _bounds():
    """BOUNDS[n][quantity] = twice the largest |float32 run - float64 run| over the fixture's cases of n rows."""
    b = collections.defaultdict(lambda: dict.fromkeys(QUANTITIES, 0.0))
    for c in CASES:
        lo, hi = fixture_quantities(c, "32"), fixture_quantities(c, "64")
        for q in QUANTITIES:
            b[c["n"]][q] = max(b[c["n"]][q], 2.0 * float(np.max(np.abs(lo[q] - hi[q]))))
    return b


BOUNDS = _bounds()


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def close(name, got, want64, bound):
    """|got - want| <= max(bound, one float32 ulp of want), elementwise; prints the figure first."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    dev = np.abs(got - want64)
    allowed = np.maximum(bound, ulp32(want64))
    print("  %-13s max deviation %.3e   bound %.3e   worst ratio %.3f" % (name, float(dev.max()), bound,
                                                                         float(np.max(dev / allowed))))
    return bool(np.all(dev <= allowed))


def device_batch(c, torch, dev, **replace):
    x = {k: torch.from_numpy(np.ascontiguousarray(replace.get(k, c[k]))).to(dev)
         for k in ("actions", "action_prob", "returns", "advantages")}
    x["values"] = torch.from_numpy(np.ascontiguousarray(replace.get("old_values", c["old_values"]))).to(dev)
    return Batch(None, x["actions"], x["action_prob"], x["returns"], x["advantages"], x["values"])


def run(c, batch=None, rows=None, values=None, policy=None, grad_loss=None, grad_entropy=None, status=None):
    """ppo_loss forward and backward on the device -> numpy results (sums included)."""
    import torch
    from safelife_amd import ppo
    dev = _hip.device()
    batch = device_batch(c, torch, dev) if batch is None else batch
    v = torch.from_numpy(np.ascontiguousarray(c["values"] if values is None else values)).to(dev).requires_grad_()
    p = torch.from_numpy(np.ascontiguousarray(c["policy"] if policy is None else policy)).to(dev).requires_grad_()
    r = None if rows is None else torch.from_numpy(np.asarray(rows, np.int64)).to(dev)
    kw = dict(zip(ref.HYPER, c["hyper"]))
    if status is not None:
        kw["status"] = status
    entropy, loss = ppo.ppo_loss(v, p, batch, r, **kw)
    sums = ppo.ppo_loss.sums
    assert entropy.shape == (len(c["values"] if values is None else values),) and loss.shape == () and loss.dtype == torch.float32
    total = loss if grad_loss is None else loss * grad_loss
    if grad_entropy is not None:
        total = total + (entropy * torch.from_numpy(grad_entropy).to(dev)).sum()
    total.backward()
    s = sums.cpu().numpy().copy()
    return dict(entropy=entropy.detach().cpu().numpy(), loss=loss.detach().cpu().numpy(), sums=s,
                loss_f32_slot=s.view(np.float32)[2 * _hip.PPO_SUM_LOSS_F32], dvalues=v.grad.cpu().numpy(),
                dpolicy=p.grad.cpu().numpy())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_and_backward_against_the_reference(case):
    out = run(case)
    want, bounds = fixture_quantities(case, "64"), BOUNDS[case["n"]]
    s = out["sums"]
    got = dict(loss=out["loss"], policy_mean=s[0], value_mean=s[1], entropy_mean=s[2], entropy=out["entropy"],
               dvalues=out["dvalues"], dpolicy=out["dpolicy"])
    print(case["id"])
    ok = [close(q, got[q], want[q], bounds[q]) for q in QUANTITIES]
    assert all(ok), [q for q, o in zip(QUANTITIES, ok) if not o]
    # the rest of the sums: the flag is the reference's branch, the total is the float32 loss before rounding
    assert s[5] == case["flag64"] == case["flag32"] and s[6] == case["n"]
    assert np.float32(s[4]) == out["loss"] == out["loss_f32_slot"]
    reg, clip, vf = (np.float64(np.float32(case["hyper"][k])) for k in (3, 4, 2))
    assert s[3] == -reg * (s[2] if s[5] else clip)
    assert s[4] == s[0] + vf * s[1] + s[3]
    assert out["entropy"].dtype == out["dvalues"].dtype == out["dpolicy"].dtype == np.float32
    from safelife_amd import ppo
    ppo.check_status()


@pytest.mark.parametrize("case", [c for c in CASES if c["kink"]], ids=[c["id"] for c in CASES if c["kink"]])
def test_kink_cases_take_the_reference_branch(case):
    """Dyadic inputs: the reference's two precisions agree exactly on every side, and so must the kernel.  A gradient that
    is exactly 0 in the fixture is exactly 0; the value gradient, which has no rounding at all on these numbers, equals the
    fixture's; so does the whole policy gradient while the bonus is off (identical float32 operations, no log)."""
    out = run(case)
    assert out["sums"][5] == case["flag32"]
    for name in ("dvalues", "dpolicy"):
        for tag in ("32", "64"):
            zero = case[name + tag] == 0
            assert np.all(out[name][zero] == 0), name
    assert np.array_equal(out["dvalues"], case["dvalues32"])
    if not case["flag32"]:
        assert np.array_equal(out["dpolicy"], case["dpolicy32"])
    if case["id"].startswith("kink-bonus"):
        n, vf = case["n"], case["hyper"][2]
        g = vf / n
        # rows 8, 9: clamped with tied squared errors -- half of the gradient through the plain error, none through the
        # clipped one; rows 6, 7: v - v_old exactly +-eps, the clamp passes the gradient
        assert out["dvalues"][8] == 0.5 * g * 2 * 0.125 and out["dvalues"][9] == 0.5 * g * 2 * -0.125
        v, old, ret = (case[k].astype(np.float64) for k in ("values", "old_values", "returns"))
        for i in (6, 7):
            assert abs(v[i] - old[i]) == 0.25 and out["dvalues"][i] == g * 2 * (v[i] - ret[i])
        # rows 3, 4: the policy clamp exactly at its edge passes the gradient; row 5, beyond it, has none; rows 1, 2: A = 0
        a = case["actions"]
        if not case["flag32"]:
            assert out["dpolicy"][3, a[3]] != 0 and out["dpolicy"][4, a[4]] != 0
            assert not out["dpolicy"][5].any() and not out["dpolicy"][1].any() and not out["dpolicy"][2].any()


def test_rows_equal_the_dense_evaluation_bit_for_bit():
    """A scrambled subset, a subset with repeated ids and rows=None: every result equals the dense evaluation of the same
    rows gathered on the host; what the batch holds at rows not named (NaN, actions out of range) is never read."""
    import torch
    from safelife_amd import ppo
    dev = _hip.device()
    c = next(c for c in CASES if c["id"] == "n257-a9-on-0")
    N = c["n"]
    rng = np.random.default_rng(5)
    subsets = {"scrambled": rng.permutation(N)[:100], "repeats": rng.integers(0, 40, 130), "all": None}
    fields = ("actions", "action_prob", "old_values", "returns", "advantages")
    for name, rows in subsets.items():
        n = N if rows is None else len(rows)
        pick = np.arange(N) if rows is None else rows
        values = rng.normal(0, 1, n).astype(np.float32)
        policy = c["policy"][rng.integers(0, N, n)]
        dense = dict(c, n=n, values=values, policy=policy, **{k: c[k][pick] for k in fields})
        want = run(dense)
        poisoned = {k: c[k].copy() for k in fields}
        if rows is not None:
            unnamed = np.setdiff1d(np.arange(N), rows)
            for k in fields[1:]:
                poisoned[k][unnamed] = np.nan
            poisoned["actions"][unnamed] = 1 << 40
        status = torch.zeros(1, dtype=torch.int64, device=dev)
        got = run(c, batch=device_batch(c, torch, dev, **poisoned), rows=rows, values=values, policy=policy, status=status)
        for k in ("entropy", "loss", "sums", "dvalues", "dpolicy"):
            assert same_bits(got[k], want[k]), (name, k)
        assert int(status.item()) == 0
        assert np.isfinite(got["dpolicy"]).all() and np.isfinite(got["sums"]).all()
    with pytest.raises(ValueError):         # without rows the outputs must cover the batch
        run(c, values=c["values"][:10], policy=c["policy"][:10])
    ppo.check_status()


def test_bad_ids_and_actions_are_flagged_and_contribute_nothing():
    """The comparison run holds, where the bad run has a bad id or a bad action, rows that add exactly zero to every sum
    (advantage 0, v = v_old = R, a one-hot policy: float32 entropy 0): sums and every other row's results must then be
    equal bit for bit."""
    import torch
    from safelife_amd import ppo
    dev = _hip.device()
    c = next(c for c in CASES if c["id"] == "n257-a9-on-0")
    N = c["n"]
    rng = np.random.default_rng(6)
    rows = rng.permutation(N)[:150].astype(np.int64)
    at_id, at_action = (3, 77), (64, 149)                    # positions in the minibatch
    special = at_id + at_action
    values, policy = c["values"][rows].copy(), c["policy"][rows].copy()
    fields = {k: c[k].copy() for k in ("actions", "action_prob", "old_values", "returns", "advantages")}
    for i in special:
        r = rows[i]
        fields["advantages"][r] = 0.0
        fields["old_values"][r] = fields["returns"][r] = values[i] = 0.5
        policy[i] = 0.0
        policy[i, 2] = 1.0
        fields["actions"][r] = 2
    clean_status = torch.zeros(1, dtype=torch.int64, device=dev)
    clean = run(c, batch=device_batch(c, torch, dev, **fields), rows=rows, values=values, policy=policy, status=clean_status)
    assert int(clean_status.item()) == 0 and not clean["entropy"][list(special)].any()

    for which, bit in (("id", _hip.PPO_BAD_INDEX), ("action", _hip.PPO_BAD_ACTION), ("both", 3)):
        bad_rows, bad_fields = rows.copy(), {k: v.copy() for k, v in fields.items()}
        hit = []
        if which in ("id", "both"):
            bad_rows[at_id[0]], bad_rows[at_id[1]] = -1, N
            hit += at_id
        if which in ("action", "both"):
            bad_fields["actions"][rows[at_action[0]]], bad_fields["actions"][rows[at_action[1]]] = -1, 9
            hit += at_action
        status = torch.zeros(1, dtype=torch.int64, device=dev)
        got = run(c, batch=device_batch(c, torch, dev, **bad_fields), rows=bad_rows, values=values, policy=policy,
                  status=status)
        assert int(status.item()) == bit, which
        with pytest.raises(ValueError):
            ppo.check_status(status)
        assert same_bits(got["sums"], clean["sums"]) and same_bits(got["loss"], clean["loss"]), which
        assert not got["entropy"][hit].any() and not got["dvalues"][hit].any() and not got["dpolicy"][hit].any()
        others = np.setdiff1d(np.arange(len(rows)), hit)
        for k in ("entropy", "dvalues", "dpolicy"):
            assert same_bits(got[k][others], clean[k][others]), (which, k)


def test_two_calls_are_equal_bit_for_bit():
    for name in ("n4099-a9-off-0", "n257-a9-on-1"):
        c = next(c for c in CASES if c["id"] == name)
        a, b = run(c), run(c)
        for k in ("entropy", "loss", "sums", "dvalues", "dpolicy"):
            assert same_bits(a[k], b[k]), (name, k)


def test_grad_loss_scales_and_grad_entropy_adds():
    import torch
    c = next(c for c in CASES if c["id"] == "n257-a9-on-0")
    one, half = run(c), run(c, grad_loss=0.5)
    assert same_bits(half["dvalues"], (0.5 * one["dvalues"]).astype(np.float32))
    assert same_bits(half["dpolicy"], (0.5 * one["dpolicy"]).astype(np.float32))
    # d/dp of a row's own entropy is -log(p + e) - p / (p + e); weighted by w and added to the loss's gradient.  The kernel
    # forms ge * log(x) and ge * p / x with ge = w - reg / n and adds them (and the policy term): each float32 result below
    # carries a few roundings of terms no larger than (|w| + reg / n) * (|log x| + 1) or than the result itself; eight
    # half-ulps of their sum bound the error.
    w = np.linspace(-1.0, 1.0, c["n"]).astype(np.float32)
    both = run(c, grad_entropy=w)
    p = c["policy"].astype(np.float64)
    x = p + np.float64(np.float32(1e-12))
    own = w[:, None].astype(np.float64) * (-np.log(x) - p / x)
    diff = both["dpolicy"].astype(np.float64) - one["dpolicy"].astype(np.float64)
    scale = ((np.abs(w[:, None]) + c["hyper"][3] / c["n"]) * (np.abs(np.log(x)) + 1.0)
             + np.abs(both["dpolicy"]) + np.abs(one["dpolicy"]))
    err = np.abs(diff - own)
    print("grad_entropy: max error %.3e, worst ratio %.3f" % (err.max(), np.max(err / (8 * 2.0 ** -24 * scale + 1e-45))))
    assert np.all(err <= 8 * 2.0 ** -24 * scale)
    assert same_bits(both["dvalues"], one["dvalues"])
    # entropy alone: no loss gradient at all
    import torch
    from safelife_amd import ppo
    dev = _hip.device()
    v = torch.from_numpy(c["values"]).to(dev).requires_grad_()
    q = torch.from_numpy(c["policy"]).to(dev).requires_grad_()
    entropy, _loss = ppo.ppo_loss(v, q, device_batch(c, torch, dev), **dict(zip(ref.HYPER, c["hyper"])))
    (entropy * torch.from_numpy(w).to(dev)).sum().backward()
    assert not v.grad.cpu().numpy().any()
    err = np.abs(q.grad.cpu().numpy().astype(np.float64) - own)
    assert np.all(err <= 8 * 2.0 ** -24 * scale)


# ------------------------------------------------------------------------------------------------------- minibatch_obs

@pytest.mark.parametrize("n", (1, 65, 257))
@pytest.mark.parametrize("mode", ("u8-u8", "u8-f32", "f32-f32"))
@pytest.mark.parametrize("width", (3125, 6250, 16))
def test_minibatch_obs_is_byte_exact(width, mode, n):
    """`width` elements per row: for the uint8 stores that is obs_bytes (3125 = 25 * 25 * 5 is odd: byte lanes; 6250: two-byte
    lanes; 16: sixteen-byte lanes), for the float32 store four times as many.  Source and output are also shifted off their
    alignment, which changes the lane width the launcher may pick."""
    import torch
    from safelife_amd import ppo
    dev = _hip.device()
    rng = np.random.default_rng(width * 7 + n)
    N = 40
    src_dtype = np.uint8 if mode.startswith("u8") else np.float32
    out_dtype = np.float32 if mode.endswith("f32") else np.uint8
    if src_dtype is np.uint8:
        store = rng.integers(0, 256, (N + 1, width)).astype(np.uint8)
    else:
        store = rng.normal(0, 1, (N + 1, width)).astype(np.float32)
    rows = rng.integers(0, N, n).astype(np.int64)
    d_store_all = torch.from_numpy(store).to(dev)
    d_rows = torch.from_numpy(rows).to(dev)
    for src_shift in (0, 1):                    # the store as a whole, and from its second row on (odd rows: odd addresses)
        d_store, h_store = d_store_all[src_shift:src_shift + N], store[src_shift:src_shift + N]
        want = h_store[rows].astype(out_dtype)
        got = ppo.minibatch_obs(d_store, d_rows, float32=mode.endswith("f32"))
        assert got.dtype == (torch.float32 if out_dtype is np.float32 else torch.uint8) and tuple(got.shape) == (n, width)
        assert same_bits(got.cpu().numpy(), want), (src_shift, "fresh")
        for out_shift in (1, 2, 3, 4, 8):       # elements in front of the output
            room = torch.zeros(n * width + 16, dtype=got.dtype, device=dev)
            out = room[out_shift:out_shift + n * width].view(n, width)
            back = ppo.minibatch_obs(d_store, d_rows, float32=mode.endswith("f32"), out=out)
            assert back is out and same_bits(out.cpu().numpy(), want), (src_shift, out_shift)
            assert not room[:out_shift].cpu().numpy().any() and not room[out_shift + n * width:].cpu().numpy().any()
    # a bad id is flagged and its output row is left as it was
    status = torch.zeros(1, dtype=torch.int64, device=dev)
    bad = rows.copy()
    bad[n // 2] = N if n % 2 else -1
    out = torch.full((n, width), 7, dtype=got.dtype, device=dev)
    ppo.minibatch_obs(d_store_all[:N], torch.from_numpy(bad).to(dev), float32=mode.endswith("f32"), out=out, status=status)
    want = store[:N][np.where((bad < 0) | (bad >= N), 0, bad)].astype(out_dtype)
    want[n // 2] = 7
    assert same_bits(out.cpu().numpy(), want)
    assert int(status.item()) == _hip.PPO_BAD_INDEX
    ppo.check_status()                          # the shared word was never touched


def test_minibatch_obs_keeps_the_observation_shape():
    import torch
    from safelife_amd import ppo
    dev = _hip.device()
    store = torch.randint(0, 256, (12, 5, 5, 5), dtype=torch.uint8, device=dev)
    rows = torch.tensor([11, 0, 3, 3], dtype=torch.int64, device=dev)
    got = ppo.minibatch_obs(store, rows)
    assert got.shape == (4, 5, 5, 5) and got.dtype == torch.float32 and torch.equal(got, store[rows].float())
    assert torch.equal(ppo.minibatch_obs(store, rows, float32=False), store[rows])


# ------------------------------------------------------------------------------------------------------- MinibatchDeal

@pytest.mark.parametrize("N", (1, 5, 4099, 65536))
def test_deal_equals_the_host_model(N):
    import torch
    from safelife_amd import ppo
    dev = _hip.device()
    for m, seed in ((4, 0), (7, 12345678901234567890)):
        deal = ppo.MinibatchDeal(N, m, seed, device=dev)
        for epoch in (0, 3):
            pieces = deal.epoch(epoch)
            assert same_bits(deal.keys.cpu().numpy().view(np.uint64), ref.keys(N, seed, epoch))
            want = ref.deal(N, m, seed, epoch)
            assert len(pieces) == len(want) == min(N, m + 1) and all(len(p) for p in pieces)
            for got, w in zip(pieces, want):
                assert got.dtype == torch.int64 and same_bits(got.cpu().numpy(), w)
            # views of one permutation, which they partition
            perm = deal.permutation
            assert all(p.untyped_storage().data_ptr() == perm.untyped_storage().data_ptr() for p in pieces)
            assert torch.equal(torch.cat(pieces), perm)
            assert np.array_equal(np.sort(perm.cpu().numpy()), np.arange(N))
        if N >= 4099:
            assert not torch.equal(torch.cat(deal.epoch(0)), torch.cat(deal.epoch(1)))


# ---------------------------------------------------------------------------------------------------------- train_batch

def _torch_loss(values, policy, batch, rows, eps_policy=0.2, eps_value=0.2, vf_coef=0.5, entropy_reg=0.01, entropy_clip=1.0):
    """The reference's expression (training/ppo.py:150-166) on tensors of any float dtype."""
    import torch
    actions, old_policy, old_values = batch.actions[rows], batch.action_prob[rows], batch.values[rows]
    returns, advantages = batch.returns[rows], batch.advantages[rows]
    a_policy = torch.gather(policy, -1, actions[..., None])[..., 0]
    prob_diff = advantages.sign() * (1 - a_policy / old_policy)
    policy_loss = (advantages.abs() * torch.clamp(prob_diff, min=-eps_policy)).mean()
    v_clip = old_values + torch.clamp(values - old_values, min=-eps_value, max=+eps_value)
    value_loss = torch.max((v_clip - returns) ** 2, (values - returns) ** 2).mean()
    entropy = torch.sum(-policy * torch.log(policy + 1e-12), dim=-1)
    entropy_loss = torch.clamp(entropy.mean(), max=entropy_clip)
    entropy_loss = entropy_loss * -entropy_reg
    return entropy, policy_loss + value_loss * vf_coef + entropy_loss


def test_train_batch_end_to_end():
    """65 envs x 4 steps of synthetic rows, a linear model to a value and a softmax head over 9 actions, Adam, 2 epochs of 5
    minibatches.  The parameters after `train_batch` are compared with those of the same loop -- same deal, same rows --
    around the reference's expression written in torch: in float64 as the yardstick, in float32 for the bound, which is twice
    the largest deviation of that float32 loop from the float64 one (never below a float32 ulp of the float64 value)."""
    import torch
    from safelife_amd import ppo
    dev = _hip.device()
    rng = np.random.default_rng(11)
    N, D, A = 65 * 4, 16, 9
    obs = torch.from_numpy(rng.integers(0, 4, (N, D)).astype(np.uint8)).to(dev)
    logits = rng.normal(0, 1, (N, A))
    old = np.exp(logits) / np.exp(logits).sum(1, keepdims=True)
    actions = rng.integers(0, A, N)
    f32 = lambda x: torch.from_numpy(np.asarray(x, np.float32)).to(dev)
    batch = Batch(obs, torch.from_numpy(actions).to(dev), f32(old[np.arange(N), actions]), f32(rng.normal(0, 1, N)),
                  f32(rng.normal(0, 1, N)), f32(rng.normal(0, 0.5, N)))

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.layer = torch.nn.Linear(D, 1 + A)

        def forward(self, x):
            y = self.layer(x)
            return y[:, 0], torch.softmax(y[:, 1:], dim=-1)

    torch.manual_seed(3)
    start = Model().state_dict()

    def fresh(dtype):
        model = Model()
        model.load_state_dict(start)
        model = model.to(device=dev, dtype=dtype)
        return model, torch.optim.Adam(model.parameters(), lr=3e-4)

    def params(model):
        return np.concatenate([p.detach().double().cpu().numpy().ravel() for p in model.parameters()])

    def torch_loop(dtype):
        model, opt = fresh(dtype)
        cast = Batch(None, batch.actions, *(x.to(dtype) for x in batch[2:]))
        deal = ppo.MinibatchDeal(N, 4, seed=9, device=dev)
        for e in range(2):
            for rows in deal.epoch(5 + e):
                values, policy = model(obs[rows].to(dtype))
                _entropy, loss = _torch_loss(values, policy, cast, rows)
                opt.zero_grad()
                loss.backward()
                opt.step()
        return params(model)

    model, opt = fresh(torch.float32)
    before = params(model)
    sums = ppo.train_batch(model, opt, batch, ppo.MinibatchDeal(N, 4, seed=9, device=dev), first_epoch=5, epochs_per_batch=2)
    got = params(model)
    p32, p64 = torch_loop(torch.float32), torch_loop(torch.float64)
    bound = 2.0 * float(np.max(np.abs(p32 - p64)))
    dev_fused = np.abs(got - p64)
    print("train_batch: parameters moved by up to %.3e; torch float32 loop vs float64 %.3e; fused vs float64 %.3e; bound %.3e"
          % (np.max(np.abs(got - before)), bound / 2, dev_fused.max(), bound))
    assert np.max(np.abs(got - before)) > 1e-3              # ten Adam steps of 3e-4 moved them
    assert np.all(dev_fused <= np.maximum(bound, ulp32(p64)))
    s = sums.cpu().numpy()
    assert s[6] == N - ppo.split_points(N, 4)[-1] and s[5] in (0.0, 1.0) and np.isfinite(s[:5]).all()
    ppo.check_status()
