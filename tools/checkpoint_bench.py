#!/usr/bin/env python
"""
Times checkpoints (safelife_amd.checkpoint, sl_digest.hip), every comparison in the same process:

    digest        slhip_state_digest over ONE segment of 1 MiB, 64 MiB and 1 GiB, and over the segment table of a DQN
                  run's state at the reference's replay_size (100 000 rows of 15 x 25 x 25 uint8 observations: the ring's
                  obs and next_obs are 0.94 GB each), table and prefix already on the device  vs  a read-only pass of stock
                  kernels over the same bytes, torch.sum of the int64 view (one per segment).  Both in GB/s, and the ratio.
    save / load   wall time of checkpoint.save and checkpoint.load for that DQN state and for a PPO state at 1024 envs,
                  with the pieces timed again on their own: the digest (state_digest: table upload, two launches, read-back),
                  the device <-> host copies, and torch.save / torch.load of the blob.
    not due       a PPOTrainer iteration at 1024 envs x 20 steps with a Checkpointer that is not due  vs  the same loop with
                  checkpointer=None: the time between consecutive on_batch calls inside one train() call (a device
                  synchronisation in each), `--repeats` windows of `--inner` iterations each, the variants alternating.  The
                  hook is a comparison of two integers: the two ranges must overlap, or the run ends with status 1.

Writes profiles/checkpoint_bench.json.

    python tools/checkpoint_bench.py [--repeats 5] [--inner 10] [--replay-size 100000] [--out DIR] [--scratch DIR]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

MIB = 1 << 20


def prepared_digest(torch, _hip, dev, segments, salt=0):
    """-> (launch, out): the table and the prefix uploaded once; ``launch()`` is the two launches alone."""
    lib, n = _hip.lib(), len(segments)
    sizes = (C.c_ulonglong * n)(*[b for _, b in segments])
    words = int(lib.slhip_state_digest_workspace_bytes(sizes, n)) // 8
    prefix = np.zeros(n + 1, np.uint64)
    _hip.check(lib.slhip_state_digest_prefix(sizes, n, prefix.ctypes.data_as(C.c_void_p)))
    table = torch.from_numpy(np.array(segments, np.uint64).reshape(n, 2).view(np.int64)).to(dev)
    work = torch.zeros(words, dtype=torch.int64, device=dev)
    work[:n + 1] = torch.from_numpy(prefix.view(np.int64)).to(dev)
    out = torch.zeros(n, dtype=torch.int64, device=dev)

    def launch():
        rc = lib.slhip_state_digest(_hip.ptr(table), n, salt, _hip.ptr(out), _hip.ptr(work), _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)
    launch.keep = (table, work)
    return launch, out


def wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--replay-size", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of checkpoint_bench.json")
    ap.add_argument("--scratch", default=None, help="where the checkpoint files are written (default: a temporary directory)")
    args = ap.parse_args()
    import bench
    from ppo_update_bench import windows
    from safelife_amd import _hip, checkpoint, dqn, ppo
    from safelife_amd.levels import _device_counts
    from safelife_amd.replay import ReplayBuffer
    from safelife_amd.runner import DQNRunner, VectorRunner
    from safelife_amd.vector_env import SafeLifeVectorEnv
    from tests import checkpoint_ref
    import torch
    dev = _hip.device()
    report = {"device": torch.cuda.get_device_name(dev), "repeats": args.repeats, "checks": {}}
    pool = bench.load_pool("prune_still_25", _device_counts)

    def make_env(B):
        return SafeLifeVectorEnv(pool, B, time_limit=1000, view_shape=(25, 25), output_channels=bench.TRAIN_CHANNELS,
                                 auto_reset=True, with_obs=False, policy_layout="uint8")

    def throughput(name, tensors, inner):
        segments = [(t.data_ptr(), t.numel() * t.element_size()) for t in tensors]
        total = sum(b for _, b in segments)
        views = [t.view(-1).view(torch.uint8)[:t.numel() * t.element_size() // 8 * 8].view(torch.int64) for t in tensors]
        launch, _out = prepared_digest(torch, _hip, dev, segments)
        t = windows(torch, {"digest": launch, "torch_sum_int64": lambda: [v.sum() for v in views]}, args.repeats, inner)
        for k in ("digest", "torch_sum_int64"):
            t[k]["GB_per_s"] = round(total / t[k]["us_median"] / 1e3, 1)
        t["bytes"], t["segments"] = total, len(segments)
        t["digest_over_sum"] = round(t["digest"]["us_median"] / t["torch_sum_int64"]["us_median"], 2)
        report["digest_" + name] = t
        print("digest", name, json.dumps(t, sort_keys=True), flush=True)

    # ---- the digest's throughput on one segment
    g = torch.Generator(device="cpu").manual_seed(0)
    small = torch.randint(0, 256, (MIB,), dtype=torch.uint8, generator=g)
    x = small.to(dev)
    launch, out = prepared_digest(torch, _hip, dev, [(x.data_ptr(), MIB)])
    launch()
    ok = int(out.cpu().numpy().view(np.uint64)[0]) == checkpoint_ref.digest(small.numpy().tobytes())
    report["checks"]["digest_1MiB_equals_the_host_model"] = ok
    if not ok:
        raise SystemExit("checkpoint_bench: the digest disagrees with the host model; nothing timed")
    for name, n, inner in (("1MiB", MIB, 200), ("64MiB", 64 * MIB, 50), ("1GiB", 1024 * MIB, 10)):
        data = torch.empty(n, dtype=torch.uint8, device=dev)
        data.view(torch.int64).random_()
        throughput(name, [data], inner)
        del data

    # ---- a DQN run's state at the reference's replay_size
    class QNet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.bias = torch.nn.Parameter(torch.zeros(9))

        def forward(self, x):
            return self.bias.expand(x.shape[0], 9)

    def dqn_stack():
        env = make_env(16)
        model, target = QNet().to(dev), QNet().to(dev)
        replay = ReplayBuffer(args.replay_size, 16, multi_step=5, obs_shape=tuple(env.policy_tensor.shape[1:]),
                              obs_dtype=torch.uint8, device=dev, seed=1)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        trainer = dqn.DQNTrainer(DQNRunner(env, model, seed=1, cast_obs=False), replay, model, target, opt,
                                 replay_initial=10 ** 9)
        return trainer, {"training_model": model, "target_model": target}, opt

    def ppo_stack(checkpointer=None, on_batch=None):
        class Nothing(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.value = torch.nn.Parameter(torch.zeros(1))
                self.logits = torch.nn.Parameter(torch.zeros(9))

            def forward(self, x):
                k = x.shape[0]
                return self.value.expand(k), torch.softmax(self.logits, dim=0).expand(k, 9)

        model = Nothing().to(dev)
        opt = torch.optim.SGD(model.parameters(), lr=1e-3)
        runner = VectorRunner(make_env(1024), model, seed=1, cast_obs=False)
        trainer = ppo.PPOTrainer(runner, model, opt, steps_per_env=20, seed=1, report_interval=10 ** 12,
                                 test_interval=10 ** 12, checkpointer=checkpointer, on_batch=on_batch)
        return trainer, {"model": model}, opt

    scratch = tempfile.TemporaryDirectory(dir=args.scratch)

    def save_load(name, build, steps):
        trainer, models, opt = build()
        trainer.train(steps)
        tensors = checkpoint._flat(checkpoint._states(trainer))
        if name == "dqn":
            for ring in (trainer.replay.obs, trainer.replay.next_obs):      # (a ring that is full of something)
                flat = ring.view(-1)
                flat[:flat.numel() // 8 * 8].view(torch.int64).random_()
            throughput("dqn_state_table", list(tensors.values()), 10)
        path = os.path.join(scratch.name, name + ".data")
        r = {"tensors": len(tensors), "bytes": sum(t.numel() * t.element_size() for t in tensors.values())}
        r["save_ms"], digests = wall(torch, lambda: checkpoint.save(path, trainer, model=models, optimizer=opt))
        r["file_bytes"] = os.path.getsize(path)
        r["digest_ms"], again = wall(torch, lambda: checkpoint.state_digest(trainer))
        r["device_to_host_ms"], host = wall(torch, lambda: {k: t.cpu() for k, t in tensors.items()})
        r["torch_save_ms"], _ = wall(torch, lambda: torch.save(host, os.path.join(scratch.name, "blob.data")))
        fresh, fresh_models, fresh_opt = build()
        r["load_ms"], _ = wall(torch, lambda: checkpoint.load(path, fresh, model=fresh_models, optimizer=fresh_opt))
        r["torch_load_ms"], blob = wall(torch, lambda: torch.load(os.path.join(scratch.name, "blob.data"), weights_only=True))
        into = checkpoint._flat(checkpoint._states(fresh))
        r["host_to_device_ms"], _ = wall(torch, lambda: [into[k].copy_(blob[k]) for k in into])
        ok = digests == again == checkpoint.state_digest(fresh)
        report["checks"][name + "_state_round_trip"] = ok
        if not ok:
            raise SystemExit("checkpoint_bench: the %s state did not come back as it was saved" % name)
        os.remove(path), os.remove(os.path.join(scratch.name, "blob.data"))
        r = {k: round(v, 2) if isinstance(v, float) else v for k, v in r.items()}
        report[name + "_state"] = r
        print(name, json.dumps(r, sort_keys=True), flush=True)

    save_load("dqn", dqn_stack, 16 * 8)
    save_load("ppo_1024_envs", ppo_stack, 1024 * 20)

    # ---- a checkpointer that is not due, inside one train() call
    B, T = 1024, 20
    stamps = []

    def on_batch(num_steps):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())

    ck = checkpoint.Checkpointer(os.path.join(scratch.name, "run"), interval=10 ** 15, keep=1)
    loops = {"checkpointer_not_due": ppo_stack(ck, on_batch)[0], "checkpointer_none": ppo_stack(None, on_batch)[0]}
    runs = {k: [] for k in loops}
    for r in range(args.repeats + 1):
        for name, trainer in loops.items():
            del stamps[:]
            trainer.train((args.inner + 1) * B * T)         # (the first iteration's save and train()'s last one lie outside)
            gaps = np.diff(stamps) * 1e3
            if r:
                runs[name].append(float(np.median(gaps)))
    t = {name: {"ms_runs": [round(x, 3) for x in v], "ms_median": round(statistics.median(v), 3)} for name, v in runs.items()}
    lo = max(min(v) for v in runs.values())
    hi = min(max(v) for v in runs.values())
    t["ranges_overlap"] = bool(lo <= hi)
    t["saves_made"] = ck.saved
    report["ppo_iteration_%d_envs_x_%d_steps" % (B, T)] = t
    report["checks"]["not_due_ranges_overlap"] = t["ranges_overlap"]
    print("not due", json.dumps(t, sort_keys=True), flush=True)
    scratch.cleanup()

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "checkpoint_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, indent=1, sort_keys=True))
    if not t["ranges_overlap"]:
        raise SystemExit("checkpoint_bench: a checkpointer that is not due costs time: the two ranges do not overlap")


if __name__ == "__main__":
    main()
