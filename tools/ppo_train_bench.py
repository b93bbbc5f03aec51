#!/usr/bin/env python
"""
Times the pieces the PPO train loop adds (safelife_amd.ppo.ppo_report / PPOTrainer, runner.VectorRunner(seed=)) against
what they replace, in the same process:

    report        ppo_report on GIVEN model outputs (the model hands back slices of stored tensors) at 4096 and 32768 rows x
                  9 actions, in one chunk and in 8192-row chunks  vs  the torch expression of training/ppo.py:199-205 --
                  calculate_loss on the whole batch and its two .mean() calls -- and vs ppo_loss forward plus the two torch
                  means (what a caller would write without the report pass)
    trainer       one PPOTrainer iteration (1024 envs x 20 steps of the benchmark pool, a do-nothing model, no report due)
                  vs  the same gen_training_batch + train_batch calls made by hand: the loop's own overhead
    take_one_step VectorRunner.take_one_step with seed= (slhip_sample_actions)  vs  seed=None (torch.multinomial) at 1024
                  and 8192 envs with a do-nothing policy

Before the report is timed the two ways are compared on the timed inputs (the four scalars to a few float32 ulps).  A
mismatch ends the run with status 1.

Device time: HIP events (torch.cuda.Event) around `--inner` back-to-back repetitions of a variant, one warm-up window, the
variants alternating, the median of `--repeats` windows divided by `--inner`.  The span between the events includes the
gaps the host leaves between launches: that is what a training loop waits for.  Writes profiles/ppo_train_bench.json.

    python tools/ppo_train_bench.py [--repeats 7] [--inner 200] [--out DIR]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

N_ACTIONS = 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of ppo_train_bench.json")
    args = ap.parse_args()
    import bench
    from ppo_update_bench import make_batch, torch_loss, windows
    from safelife_amd import _hip, ppo
    from safelife_amd.levels import _device_counts
    from safelife_amd.runner import VectorRunner
    from safelife_amd.vector_env import SafeLifeVectorEnv
    import torch
    dev = _hip.device()
    g = torch.Generator(device="cpu").manual_seed(0)
    report = {"device": torch.cuda.get_device_name(dev), "n_actions": N_ACTIONS, "inner": args.inner, "checks": {}}

    # ---- the report on given model outputs
    for n in (4096, 32768):
        batch = make_batch(torch, dev, g, n, obs=torch.zeros((n, 1), dtype=torch.float32, device=dev))
        values = torch.randn(n, generator=g).to(dev)
        policy = torch.softmax(2.0 * torch.randn((n, N_ACTIONS), generator=g), dim=1).to(dev)
        at = [0]

        def model(x):
            lo, k = at[0], x.shape[0]
            at[0] = (lo + k) % n
            return values[lo:lo + k], policy[lo:lo + k]

        def plain():
            entropy, loss = torch_loss(torch, values, policy, batch.actions, batch.action_prob, batch.values, batch.returns,
                                       batch.advantages)
            return loss, entropy.mean(), batch.values.mean(), batch.advantages.mean()

        def loss_and_means():
            ppo.ppo_loss(values, policy, batch)
            return ppo.ppo_loss.sums, batch.values.mean(), batch.advantages.mean()

        fused = ppo.ppo_report.scalars(ppo.ppo_report(model, batch, chunk_rows=n))
        chunked = ppo.ppo_report.scalars(ppo.ppo_report(model, batch, chunk_rows=8192))
        want = [float(x) for x in plain()]
        ok = chunked == fused and all(abs(fused[k] - w) <= 16 * 2.0 ** -24 * max(abs(w), 1e-3)
                                      for k, w in zip(("loss", "entropy", "values", "advantages"), want))
        report["checks"]["report_%d" % n] = ok
        if not ok:
            print(fused, chunked, want)
            raise SystemExit("ppo_train_bench: the report and the torch expression disagree; nothing timed")
        t = windows(torch, {"report_one_chunk": lambda: ppo.ppo_report(model, batch, chunk_rows=n),
                            "report_8192_row_chunks": lambda: ppo.ppo_report(model, batch, chunk_rows=8192),
                            "ppo_loss_forward_plus_two_means": loss_and_means, "torch": plain}, args.repeats, args.inner)
        t["torch_over_report"] = round(t["torch"]["us_median"] / t["report_8192_row_chunks"]["us_median"], 2)
        report["report_%d" % n] = t
        print("report %d" % n, json.dumps(t, sort_keys=True), flush=True)

    # ---- a do-nothing model and policy
    class Nothing(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.value = torch.nn.Parameter(torch.zeros(1))
            self.logits = torch.nn.Parameter(torch.zeros(N_ACTIONS))

        def forward(self, x):
            k = x.shape[0]
            return self.value.expand(k), torch.softmax(self.logits, dim=0).expand(k, N_ACTIONS)

    pool = bench.load_pool("prune_still_25", _device_counts)

    def make_env(B):
        return SafeLifeVectorEnv(pool, B, time_limit=1000, view_shape=(25, 25), output_channels=bench.TRAIN_CHANNELS,
                                 auto_reset=True, with_obs=False, policy_layout="uint8")

    # ---- one trainer iteration against the same calls by hand
    B, T = 1024, 20

    def loop(by_hand):
        model = Nothing().to(dev)
        opt = torch.optim.SGD(model.parameters(), lr=1e-3)
        runner = VectorRunner(make_env(B), model, seed=1, cast_obs=False)
        if by_hand:
            deal, epoch = ppo.MinibatchDeal(B * T, 4, seed=1), [0]

            def iteration():
                batch = runner.gen_training_batch(T, 0.97, 0.95)
                ppo.train_batch(model, opt, batch, deal, epoch[0], 3)
                epoch[0] += 3
            return iteration
        trainer = ppo.PPOTrainer(runner, model, opt, steps_per_env=T, seed=1, report_interval=10 ** 12, test_interval=10 ** 12)
        return lambda: trainer.train(B * T)

    t = windows(torch, {"trainer": loop(False), "by_hand": loop(True)}, args.repeats, max(1, args.inner // 100))
    t["trainer_over_by_hand"] = round(t["trainer"]["us_median"] / t["by_hand"]["us_median"], 3)
    report["trainer_iteration_%d_envs_x_%d_steps" % (B, T)] = t
    print("trainer", json.dumps(t, sort_keys=True), flush=True)

    # ---- take_one_step: the library's draw against torch.multinomial
    for B in (1024, 8192):
        def stepper(seed):
            probs = torch.full((B, N_ACTIONS), 1.0 / N_ACTIONS, device=dev)
            zeros = torch.zeros(B, device=dev)
            runner = VectorRunner(make_env(B), lambda obs: (zeros, probs), seed=seed, copy_obs=False, cast_obs=False)
            return runner.take_one_step
        t = windows(torch, {"seed": stepper(1), "multinomial": stepper(None)}, args.repeats, args.inner)
        t["multinomial_over_seed"] = round(t["multinomial"]["us_median"] / t["seed"]["us_median"], 2)
        report["take_one_step_%d_envs" % B] = t
        print("take_one_step %d" % B, json.dumps(t, sort_keys=True), flush=True)
    ppo.check_status()

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "ppo_train_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
