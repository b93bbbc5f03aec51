#!/usr/bin/env python
"""
Times the device-side PPO batch builder (safelife_amd.rollout.RolloutBuffer -> slhip_rollout_record /
slhip_training_batch, csrc/sl_rollout.hip) at 8192 envs x 20 steps, float32 rewards, against the same result computed
with torch alone in the same process:

    hip    20 record calls (one kernel each) + one slhip_training_batch
    torch  20 x (a gather and four row copies) + a reverse loop over the 20 steps that carries the float32 and the
           float64 running advantage, the running return and the width flag as [B] tensors (about fifteen small
           kernels per step)

Before anything is timed the torch loop is checked against the kernel: bit-equal on a window without a single done flag
(every trajectory open and float32 -- the case a textbook GAE computes), and the full contract on the timed window, whose
done flags are drawn with probability 0.05.  A mismatch ends the run with status 1.

Device time: HIP events (torch.cuda.Event) around each variant, every buffer allocated before the events, one full
warm-up, median of five.  The span between the events includes the gaps the host leaves between launches: that is what a
training loop waits for.  Writes profiles/training_batch_bench.json.

    python tools/training_batch_bench.py [--envs 8192] [--steps 20] [--repeats 5] [--out DIR]
"""
import argparse
import collections
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

Step = collections.namedtuple("Step", "obs actions rewards done policies values")
GAMMA, LMDA, N_ACTIONS = 0.97, 0.95, 9


def torch_record(bufs, t, step):
    B = step.actions.shape[0]
    bufs["actions"][t].copy_(step.actions)
    bufs["action_prob"][t].copy_(step.policies.gather(1, step.actions.to(step.policies.device).long().view(B, 1)).view(B))
    bufs["rewards"][t].copy_(step.rewards)
    bufs["values"][t].copy_(step.values)
    bufs["done"][t].copy_(step.done)


def torch_training_batch(torch, R, V, D, fv, gamma, lmda, returns, advantages):
    """The contract of slhip_training_batch for float32 rewards, one reverse step at a time, [B] tensors throughout."""
    T, B = R.shape
    Dn = D != 0
    zero32, zero64 = torch.zeros_like(fv), torch.zeros(B, dtype=torch.float64, device=fv.device)
    ret = adv_n = adv_w = wide = None
    for t in range(T - 1, -1, -1):
        d = Dn[t]
        r, v = R[t], V[t]
        r64, v64 = r.double(), v.double()
        if t == T - 1:
            before = Dn[t - 1] if t > 0 else torch.ones_like(d)
            wide = d | before
            vn = torch.where(d, zero32, fv)
            ret = r + gamma * vn
            adv_n = (r + gamma * vn) - v
            adv_w = (r64 + gamma * vn.double()) - v64
        else:
            wide = wide | d
            vn = torch.where(d, zero32, V[t + 1])
            ret = r + gamma * torch.where(d, zero32, ret)
            adv_n = ((r + gamma * vn) - v) + lmda * torch.where(d, zero32, adv_n)
            adv_w = ((r64 + gamma * vn.double()) - v64) + lmda * torch.where(d, zero64, adv_w)
        returns[t].copy_(ret)
        advantages[t].copy_(torch.where(wide, adv_w.float(), adv_n))


def timed(torch, fn, repeats):
    fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3)
    return {"us_runs": [round(x, 1) for x in runs], "us_median": round(statistics.median(runs), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of training_batch_bench.json")
    args = ap.parse_args()
    import torch
    from safelife_amd import _hip
    from safelife_amd.rollout import RolloutBuffer
    dev = _hip.device()
    T, B = args.steps, args.envs
    g = torch.Generator(device="cpu").manual_seed(0)

    def window(p_done):
        return [Step(None, torch.randint(0, N_ACTIONS, (B,), generator=g, dtype=torch.int32).to(dev),
                     torch.randn(B, generator=g).to(dev), (torch.rand(B, generator=g) < p_done).to(torch.uint8).to(dev),
                     torch.softmax(torch.randn((B, N_ACTIONS), generator=g), dim=1).to(dev), torch.randn(B, generator=g).to(dev))
                for _ in range(T)]
    fv = torch.randn(B, generator=g).to(dev)
    buf = RolloutBuffer(B, T, None, None, torch.float32, dev)
    tb = dict(actions=torch.zeros((T, B), dtype=torch.int32, device=dev), action_prob=torch.zeros((T, B), device=dev),
              rewards=torch.zeros((T, B), device=dev), values=torch.zeros((T, B), device=dev),
              done=torch.zeros((T, B), dtype=torch.uint8, device=dev))
    t_ret, t_adv = torch.zeros((T, B), device=dev), torch.zeros((T, B), device=dev)

    def hip_record(steps):
        for t, s in enumerate(steps):
            buf.record(t, s)

    def torch_records(steps):
        for t, s in enumerate(steps):
            torch_record(tb, t, s)

    def same(a, b):
        return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))

    checks = {}
    for name, p_done in (("open_float32", 0.0), ("timed_window", 0.05)):
        steps = window(p_done)
        hip_record(steps), torch_records(steps)
        buf.finish(fv, GAMMA, LMDA)
        torch_training_batch(torch, tb["rewards"], tb["values"], tb["done"], fv, GAMMA, LMDA, t_ret, t_adv)
        torch.cuda.synchronize()
        buf.check_status()
        checks[name] = {"records_equal": all(bool(torch.equal(getattr(buf, k), tb[k])) for k in tb),
                        "returns_bit_equal": same(buf.returns, t_ret), "advantages_bit_equal": same(buf.advantages, t_adv)}
    print(json.dumps(checks, sort_keys=True))
    if not all(all(c.values()) for c in checks.values()):
        raise SystemExit("training_batch_bench: the torch loop and the kernel disagree; nothing timed")

    report = {"envs": B, "steps": T, "reward_dtype": "float32", "gamma": GAMMA, "lmda": LMDA, "checks": checks,
              "device": torch.cuda.get_device_name(dev),
              "hip_record_x%d" % T: timed(torch, lambda: hip_record(steps), args.repeats),
              "hip_training_batch": timed(torch, lambda: buf.finish(fv, GAMMA, LMDA), args.repeats),
              "hip_total": timed(torch, lambda: (hip_record(steps), buf.finish(fv, GAMMA, LMDA)), args.repeats),
              "torch_record_x%d" % T: timed(torch, lambda: torch_records(steps), args.repeats),
              "torch_training_batch": timed(torch, lambda: torch_training_batch(
                  torch, tb["rewards"], tb["values"], tb["done"], fv, GAMMA, LMDA, t_ret, t_adv), args.repeats)}
    report["torch_total"] = timed(torch, lambda: (torch_records(steps), torch_training_batch(
        torch, tb["rewards"], tb["values"], tb["done"], fv, GAMMA, LMDA, t_ret, t_adv)), args.repeats)
    report["torch_over_hip"] = round(report["torch_total"]["us_median"] / report["hip_total"]["us_median"], 2)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "training_batch_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
