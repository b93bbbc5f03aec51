#!/usr/bin/env python
"""
Times the device-side PPO update (safelife_amd.ppo -> csrc/sl_ppo.hip) against the reference's expressions written with
torch alone, in the same process:

    loss          ppo_loss forward + backward  vs  the expression of PPO.calculate_loss (training/ppo.py:150-166) forward +
                  backward, at 4096 and 32768 rows x 9 actions; `dense`: the minibatch is the batch (rows=None, no gather on
                  either side); `rows`: the minibatch is one of the five pieces of a batch five times as large, the fused
                  loss reading the five scalars through the row ids, torch gathering them first (`batch.x[k]`)
    minibatch_obs 32768 rows of 3125-byte uint8 observations out of 163840 (8192 envs x 20 steps), widened to float32
                  vs  index_select + .float()
    minibatch     one minibatch of train_batch -- observations, model, loss, zero_grad, backward, step -- with a do-nothing
                  model (a value and nine logits that ignore the observation) and SGD, both ways

Before anything is timed the two ways are compared on the timed inputs (loss and both gradients to a few float32 ulps of
their largest element; the observations byte exact).  A mismatch ends the run with status 1.

Device time: HIP events (torch.cuda.Event) around `--inner` back-to-back repetitions of a variant, every input allocated
before the events, one warm-up window, the two ways alternating, the median of `--repeats` windows divided by `--inner`.
The span between the events includes the gaps the host leaves between launches: that is what a training loop waits for.
Writes profiles/ppo_update_bench.json.

    python tools/ppo_update_bench.py [--repeats 7] [--inner 200] [--out DIR]
"""
import argparse
import collections
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

Batch = collections.namedtuple("Batch", "obs actions action_prob returns advantages values")
N_ACTIONS, OBS_BYTES = 9, 3125


def torch_loss(torch, values, policy, actions, old_policy, old_values, returns, advantages, eps_policy=0.2, eps_value=0.2,
               vf_coef=0.5, entropy_reg=0.01, entropy_clip=1.0):
    a_policy = torch.gather(policy, -1, actions[..., None])[..., 0]
    prob_diff = advantages.sign() * (1 - a_policy / old_policy)
    policy_loss = (advantages.abs() * torch.clamp(prob_diff, min=-eps_policy)).mean()
    v_clip = old_values + torch.clamp(values - old_values, min=-eps_value, max=+eps_value)
    value_loss = torch.max((v_clip - returns) ** 2, (values - returns) ** 2).mean()
    entropy = torch.sum(-policy * torch.log(policy + 1e-12), dim=-1)
    entropy_loss = torch.clamp(entropy.mean(), max=entropy_clip)
    entropy_loss = entropy_loss * -entropy_reg
    return entropy, policy_loss + value_loss * vf_coef + entropy_loss


def torch_loss_rows(torch, values, policy, batch, rows):
    if rows is None:
        return torch_loss(torch, values, policy, batch.actions, batch.action_prob, batch.values, batch.returns, batch.advantages)
    return torch_loss(torch, values, policy, batch.actions[rows], batch.action_prob[rows], batch.values[rows],
                      batch.returns[rows], batch.advantages[rows])


def windows(torch, variants, repeats, inner):
    """variants: name -> fn.  One warm-up window each, then `repeats` rounds in which the variants take turns."""
    runs = {name: [] for name in variants}
    for r in range(repeats + 1):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if r:
                runs[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    return {name: {"us_runs": [round(x, 1) for x in v], "us_median": round(statistics.median(v), 1)}
            for name, v in runs.items()}


def make_batch(torch, dev, g, N, obs=None):
    policy = torch.softmax(torch.randn((N, N_ACTIONS), generator=g), dim=1)
    actions = torch.randint(0, N_ACTIONS, (N,), generator=g)
    prob = policy.gather(1, actions.view(N, 1)).view(N) * torch.exp(0.25 * torch.randn(N, generator=g))
    return Batch(obs, actions.to(dev), prob.to(dev), torch.randn(N, generator=g).to(dev), torch.randn(N, generator=g).to(dev),
                 torch.randn(N, generator=g).to(dev))


def close(torch, a, b, ulps=16):
    scale = float(b.abs().max())
    return bool((a - b).abs().max() <= ulps * 2.0 ** -24 * max(scale, 1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of ppo_update_bench.json")
    args = ap.parse_args()
    from safelife_amd import _hip, ppo
    import torch
    dev = _hip.device()
    g = torch.Generator(device="cpu").manual_seed(0)
    report = {"device": torch.cuda.get_device_name(dev), "n_actions": N_ACTIONS, "inner": args.inner, "checks": {}}

    # ---- the loss, forward + backward
    for n in (4096, 32768):
        for kind, N in (("dense", n), ("rows", 5 * n)):
            batch = make_batch(torch, dev, g, N)
            rows = None if kind == "dense" else ppo.MinibatchDeal(N, 4, seed=1, device=dev).epoch(0)[0]
            assert rows is None or rows.numel() == n
            values = torch.randn(n, generator=g).to(dev).requires_grad_()
            policy = torch.softmax(2.0 * torch.randn((n, N_ACTIONS), generator=g), dim=1).to(dev).requires_grad_()

            def fused():
                values.grad = policy.grad = None
                _e, loss = ppo.ppo_loss(values, policy, batch, rows)
                loss.backward()

            def plain():
                values.grad = policy.grad = None
                _e, loss = torch_loss_rows(torch, values, policy, batch, rows)
                loss.backward()

            fused()
            e_f, l_f = ppo.ppo_loss(values.detach(), policy.detach(), batch, rows)
            gv, gp = values.grad.clone(), policy.grad.clone()
            plain()
            e_t, l_t = torch_loss_rows(torch, values.detach(), policy.detach(), batch, rows)
            ok = {"loss": close(torch, l_f, l_t), "entropy": close(torch, e_f, e_t), "d_values": close(torch, gv, values.grad),
                  "d_policy": close(torch, gp, policy.grad)}
            report["checks"]["loss_%d_%s" % (n, kind)] = ok
            if not all(ok.values()):
                print(json.dumps(report["checks"], sort_keys=True))
                raise SystemExit("ppo_update_bench: the fused loss and the torch expression disagree; nothing timed")
            t = windows(torch, {"fused": fused, "torch": plain}, args.repeats, args.inner)
            t["torch_over_fused"] = round(t["torch"]["us_median"] / t["fused"]["us_median"], 2)
            report["loss_fwd_bwd_%d_%s" % (n, kind)] = t
            print("loss %d %s" % (n, kind), json.dumps(t, sort_keys=True), flush=True)

    # ---- the observations of a minibatch
    N, n = 163840, 32768
    obs = torch.randint(0, 256, (N, OBS_BYTES), dtype=torch.uint8, device=dev)
    batch = make_batch(torch, dev, g, N, obs)
    deal = ppo.MinibatchDeal(N, 4, seed=2, device=dev)
    rows = deal.epoch(0)[0]
    assert rows.numel() == n
    out = torch.empty((n, OBS_BYTES), dtype=torch.float32, device=dev)
    ok = bool(torch.equal(ppo.minibatch_obs(obs, rows, out=out), obs.index_select(0, rows).float()))
    report["checks"]["minibatch_obs"] = ok
    if not ok:
        raise SystemExit("ppo_update_bench: minibatch_obs and index_select + float disagree; nothing timed")
    t = windows(torch, {"fused": lambda: ppo.minibatch_obs(obs, rows, out=out),
                        "fused_alloc": lambda: ppo.minibatch_obs(obs, rows),
                        "torch": lambda: obs.index_select(0, rows).float()}, args.repeats, args.inner)
    moved = n * OBS_BYTES * 5           # bytes read as uint8 and written as float32
    for k in ("fused", "fused_alloc", "torch"):
        t[k]["GB_per_s"] = round(moved / t[k]["us_median"] / 1e3, 1)
    t["torch_over_fused"] = round(t["torch"]["us_median"] / t["fused_alloc"]["us_median"], 2)
    report["minibatch_obs_%d_of_%d_x%d" % (n, N, OBS_BYTES)] = t
    print("minibatch_obs", json.dumps(t, sort_keys=True), flush=True)

    # ---- one minibatch of train_batch, a model that does nothing
    class Nothing(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.value = torch.nn.Parameter(torch.zeros(1))
            self.logits = torch.nn.Parameter(torch.zeros(N_ACTIONS))

        def forward(self, x):
            k = x.shape[0]
            return self.value.expand(k), torch.softmax(self.logits, dim=0).expand(k, N_ACTIONS)

    def minibatch(fused):
        model = Nothing().to(dev)
        opt = torch.optim.SGD(model.parameters(), lr=1e-3)

        def step():
            if fused:
                x = ppo.minibatch_obs(obs, rows)
                values, policy = model(x)
                _e, loss = ppo.ppo_loss(values, policy, batch, rows)
            else:
                x = obs[rows].float()
                values, policy = model(x)
                _e, loss = torch_loss_rows(torch, values, policy, batch, rows)
            opt.zero_grad()
            loss.backward()
            opt.step()
        return step

    t = windows(torch, {"fused": minibatch(True), "torch": minibatch(False)}, args.repeats, args.inner)
    t["torch_over_fused"] = round(t["torch"]["us_median"] / t["fused"]["us_median"], 2)
    report["train_minibatch_%d_of_%d" % (n, N)] = t
    print("minibatch", json.dumps(t, sort_keys=True), flush=True)
    ppo.check_status()

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "ppo_update_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
