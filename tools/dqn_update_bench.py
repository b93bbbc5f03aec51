#!/usr/bin/env python
"""
Times the device-side DQN update (safelife_amd.dqn -> csrc/sl_dqn.hip) against the reference's expressions written with torch
alone, in the same process:

    loss          dqn_loss forward + backward  vs  the expression of DQN.optimize (training/dqn.py:152-157) forward +
                  backward, at 96 and 4096 rows x 9 actions, from a gathered batch on both sides
    launches      dqn_loss forward alone at 256 rows (the row pass finishes its own sums: ONE launch) and at 257 rows (the
                  row pass and the one-workgroup finish: TWO launches) -- the same work but for one row, so the difference
                  is what the second launch costs
    optimize      one `optimize` -- sample, observations, both models, loss, zero_grad, backward, step -- with a do-nothing
                  model (nine Q-values that ignore the observation) and SGD  vs  `replay.sample` + the torch expression;
                  96 rows of 3125-byte uint8 observations out of a ring of 100000
    sync_target   sync_target  vs  load_state_dict for a model shaped like SafeLifeQNetwork (three convolutions, two dense
                  heads, a 15-channel 25x25 view)

Before anything is timed the two ways are compared on the timed inputs (td and the gradient bit for bit, the loss to a few
float32 ulps; the synced parameters equal).  A mismatch ends the run with status 1.

Device time: HIP events (torch.cuda.Event) around `--inner` back-to-back repetitions of a variant, every input allocated
before the events, `--warmup` warm-up windows (three: with one, the first section of a fresh process was timed while host
and device were still ramping up -- both ways came out at 175 us for four windows and then fell to their steady 68 and
122 us), the two ways alternating, the median of `--repeats` windows divided by `--inner`.  The span between the events
includes the gaps the host leaves between launches: that is what a training loop waits for.
Writes profiles/dqn_update_bench.json.

    python tools/dqn_update_bench.py [--repeats 7] [--inner 1000] [--warmup 3] [--out DIR]
"""
import argparse
import collections
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N_ACTIONS, OBS_BYTES = 9, 3125
GAMMA, MULTI_STEP = 0.97, 5
Step = collections.namedtuple("Step", "obs actions rewards done next_obs")


def torch_loss(torch, q_values, next_q_values, action, reward, done):
    q_value = q_values.gather(1, action.unsqueeze(1)).squeeze(1)
    next_q_value, _next_action = next_q_values.max(1)
    discount = GAMMA ** MULTI_STEP * (1 - done)
    expected_q_value = reward + discount * next_q_value
    td = q_value - expected_q_value
    return td, torch.mean(td ** 2)


def windows(torch, variants, repeats, inner, warmup):
    """variants: name -> fn.  `warmup` warm-up windows each, then `repeats` rounds in which the variants take turns."""
    runs = {name: [] for name in variants}
    for r in range(-warmup, repeats):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if r >= 0:
                runs[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    return {name: {"us_runs": [round(x, 1) for x in v], "us_median": round(statistics.median(v), 1)}
            for name, v in runs.items()}


def make_batch(torch, dev, g, n):
    from safelife_amd.replay import ReplayBatch
    reward = torch.randn(n, generator=g)
    reward[torch.rand(n, generator=g) < 0.2] = 0.0
    return ReplayBatch(None, torch.randint(0, N_ACTIONS, (n,), generator=g).to(dev), reward.to(dev), None,
                       (torch.rand(n, generator=g) < 0.2).float().to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3, help="warm-up windows per variant")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of dqn_update_bench.json")
    args = ap.parse_args()
    from safelife_amd import _hip, dqn
    from safelife_amd.replay import ReplayBuffer
    import torch
    dev = _hip.device()
    g = torch.Generator(device="cpu").manual_seed(0)
    report = {"device": torch.cuda.get_device_name(dev), "n_actions": N_ACTIONS, "inner": args.inner, "warmup_windows": args.warmup,
              "checks": {}}

    # ---- the loss, forward + backward
    for n in (96, 4096):
        batch = make_batch(torch, dev, g, n)
        q = (2.0 * torch.randn((n, N_ACTIONS), generator=g)).to(dev).requires_grad_()
        nq = (2.0 * torch.randn((n, N_ACTIONS), generator=g)).to(dev)

        def fused():
            q.grad = None
            _td, loss = dqn.dqn_loss(q, nq, batch, gamma=GAMMA, multi_step=MULTI_STEP)
            loss.backward()

        def plain():
            q.grad = None
            _td, loss = torch_loss(torch, q, nq, batch.action, batch.reward, batch.done)
            loss.backward()

        fused()
        td_f, l_f = dqn.dqn_loss(q.detach(), nq, batch, gamma=GAMMA, multi_step=MULTI_STEP)
        grad_f = q.grad.clone()
        plain()
        td_t, l_t = torch_loss(torch, q.detach(), nq, batch.action, batch.reward, batch.done)
        ok = {"td": bool(torch.equal(td_f, td_t)), "d_q": bool(torch.equal(grad_f, q.grad)),
              "loss": bool((l_f - l_t).abs() <= 16 * 2.0 ** -24 * l_t.abs())}
        report["checks"]["loss_%d" % n] = ok
        if not all(ok.values()):
            print(json.dumps(report["checks"], sort_keys=True))
            raise SystemExit("dqn_update_bench: the fused loss and the torch expression disagree; nothing timed")
        t = windows(torch, {"fused": fused, "torch": plain}, args.repeats, args.inner, max(0, args.warmup))
        t["torch_over_fused"] = round(t["torch"]["us_median"] / t["fused"]["us_median"], 2)
        report["loss_fwd_bwd_%d" % n] = t
        print("loss %d" % n, json.dumps(t, sort_keys=True), flush=True)

    # ---- one launch or two: the forward alone on either side of the switch
    variants = {}
    for n in (256, 257):
        batch = make_batch(torch, dev, g, n)
        q = (2.0 * torch.randn((n, N_ACTIONS), generator=g)).to(dev)
        nq = (2.0 * torch.randn((n, N_ACTIONS), generator=g)).to(dev)
        variants["rows_%d_%s" % (n, "one_launch" if n <= 256 else "two_launches")] = (
            lambda q=q, nq=nq, batch=batch: dqn.dqn_loss(q, nq, batch, gamma=GAMMA, multi_step=MULTI_STEP))
    t = windows(torch, variants, args.repeats, args.inner, max(0, args.warmup))
    one, two = (t[k]["us_median"] for k in sorted(t))
    t["two_over_one"] = round(two / one, 2)
    report["forward_launches"] = t
    print("launches", json.dumps(t, sort_keys=True), flush=True)

    # ---- one optimize, a model that does nothing
    B, n_step, cap, k = 64, MULTI_STEP, 100000, 96
    replay = ReplayBuffer(cap, B, multi_step=n_step, gamma=GAMMA, obs_shape=(OBS_BYTES,), obs_dtype=torch.uint8,
                          reward_dtype=torch.float32, device=dev, seed=1)
    for t_ in range(24):
        replay.add(Step(torch.randint(0, 256, (B, OBS_BYTES), dtype=torch.uint8, device=dev),
                        torch.randint(0, N_ACTIONS, (B,), dtype=torch.int32, device=dev), torch.randn(B, device=dev),
                        torch.rand(B, device=dev) < 0.1, torch.randint(0, 256, (B, OBS_BYTES), dtype=torch.uint8, device=dev)))
    assert len(replay) >= 10 * k

    class Nothing(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.q = torch.nn.Parameter(torch.linspace(-1.0, 1.0, N_ACTIONS))

        def forward(self, x):
            return self.q.expand(x.shape[0], N_ACTIONS)

    def optimize(fused):
        model, target = Nothing().to(dev), Nothing().to(dev)
        opt = torch.optim.SGD(model.parameters(), lr=1e-3)

        def step():
            if fused:
                dqn.optimize(model, target, opt, replay, k, gamma=GAMMA, multi_step=MULTI_STEP)
                return
            b = replay.sample(k)
            q_values = model(b.obs)
            next_q_values = target(b.next_obs).detach()
            _td, loss = torch_loss(torch, q_values, next_q_values, b.action, b.reward, b.done)
            opt.zero_grad()
            loss.backward()
            opt.step()
        return step

    t = windows(torch, {"fused": optimize(True), "torch": optimize(False)}, args.repeats, args.inner, max(0, args.warmup))
    t["torch_over_fused"] = round(t["torch"]["us_median"] / t["fused"]["us_median"], 2)
    report["optimize_%d_of_%d_x%d" % (k, cap, OBS_BYTES)] = t
    print("optimize", json.dumps(t, sort_keys=True), flush=True)
    replay.check_status()
    dqn.check_status()

    # ---- the target update
    def q_network():
        """The tensors of SafeLifeQNetwork on a 25x25x15 view: three convolutions and two dense heads of 256 (only the
        state dict matters here: seven weights and seven biases, 0.37 M parameters)."""
        features = 64 * 3 * 3
        head = lambda out: torch.nn.Sequential(torch.nn.Linear(features, 256), torch.nn.ReLU(), torch.nn.Linear(256, out))  # noqa: E731
        return torch.nn.ModuleDict(dict(
            cnn=torch.nn.Sequential(torch.nn.Conv2d(15, 32, 5, stride=2), torch.nn.ReLU(), torch.nn.Conv2d(32, 64, 3, stride=2),
                                    torch.nn.ReLU(), torch.nn.Conv2d(64, 64, 3, stride=1), torch.nn.ReLU()),
            advantages=head(N_ACTIONS), value_func=head(1))).to(dev)

    training, target, twin = q_network(), q_network(), q_network()
    dqn.sync_target(training, target)
    twin.load_state_dict(training.state_dict())
    ok = all(bool(torch.equal(a, b)) for a, b in zip(target.state_dict().values(), twin.state_dict().values()))
    report["checks"]["sync_target"] = ok
    if not ok:
        raise SystemExit("dqn_update_bench: sync_target and load_state_dict disagree; nothing timed")
    t = windows(torch, {"fused": lambda: dqn.sync_target(training, target),
                        "torch": lambda: twin.load_state_dict(training.state_dict())}, args.repeats, args.inner, max(0, args.warmup))
    t["torch_over_fused"] = round(t["torch"]["us_median"] / t["fused"]["us_median"], 2)
    t["tensors"] = len(training.state_dict())
    t["parameters"] = sum(p.numel() for p in training.parameters())
    report["sync_target_q_network"] = t
    print("sync_target", json.dumps(t, sort_keys=True), flush=True)

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "dqn_update_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
