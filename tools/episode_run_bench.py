#!/usr/bin/env python
"""
Times what an evaluation run (safelife_amd.episode_run.EpisodeRun -> slhip_episode_run_start / _harvest / _tickets;
csrc/sl_episode_run.hip) costs.

    step       us per SafeLifeVectorEnv.step() with the training observation at 8192 and 1024 envs (25x25, the prune-still
               fixture pool cycled to 80 slots), without a run and with a started one, in the same process and built with
               the same ``run.env_arguments()``; the run has 16 tickets per env, so nobody retires while the clock runs,
               and the envs' episodes are spread over the time limit, so about B / 1000 envs end an episode inside every
               step.  `harvest_alone`: the harvest kernel back to back on one stream over step records of which about
               B / 1000 per step are done (the span includes the gaps the host leaves between launches, and one
               slhip_episode_run_start per 200 calls, under 0.1 us per call)
    run        a whole ``VectorRunner.run_episodes`` of 1000 tickets on 1024 envs over a 100-slot archive (the prune-still
               fixture cycled to 100 slots: the reference's benchmark archives are not part of this repository), time limit
               1000, a fixed uniform random policy, the counter polled every 16 steps: wall-clock milliseconds from the
               call to the returned result table, the steps it took and the episode lengths it saw

Device time for `step`: HIP events around a loop of calls, every buffer allocated before the events, one loop of warm-up
first, median of five loops.  Wall clock for `run` (it ends with a host read): one warm-up run, median of five.

    python tools/episode_run_bench.py [--repeats 5] [--out DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.episode_log_bench import LOOP, TRAIN_CHANNELS, cycled_levels, step_records, timed    # noqa: E402


def run_steps(torch, dev, B, repeats):
    from safelife_amd import _hip
    from safelife_amd.episode_run import EpisodeRun
    from safelife_amd.levels import LevelPool
    from safelife_amd.vector_env import SafeLifeVectorEnv
    lv = cycled_levels("prune_still_25", 80)
    actions = torch.randint(0, 9, (LOOP, B), device=dev, dtype=torch.int32)
    kw = dict(time_limit=1000, view_shape=(25, 25), output_channels=TRAIN_CHANNELS)
    out = {"envs": B}
    for label in ("plain", "with_run"):
        pool = LevelPool(lv)
        run = EpisodeRun(pool, B, 16 * B)
        env = SafeLifeVectorEnv(pool, B, episode_run=run if label == "with_run" else None, **kw, **run.env_arguments())
        if label == "with_run":
            run.start()
        else:
            env.reset()
        env.t["scalars"][:, _hip.SCALAR_COLS["num_steps"]] = (torch.arange(B, device=dev, dtype=torch.int64) * 997 % 1000).to(torch.int32)

        def loop():
            for t in range(LOOP):
                env.step(actions[t])
        out[label] = timed(torch, loop, repeats, LOOP)
        if label == "with_run":
            c = run.counters()
            assert c["in_progress"] == B            # nobody retired while the clock ran
            out[label]["episodes_filed"] = c["completed"]
            out[label]["over_plain_us"] = round(out[label]["us_per_call_median"] - out["plain"]["us_per_call_median"], 2)
        del env, run, pool
        torch.cuda.empty_cache()
    return out


def run_harvest(torch, dev, B, repeats):
    import types
    from safelife_amd import _hip
    from safelife_amd.episode_run import EpisodeRun
    from safelife_amd.levels import LevelPool
    rng = np.random.default_rng(B)
    pool = LevelPool(cycled_levels("prune_still_25", 80))
    # (the eight record sets come round every eight calls: an env that is done in one of them files a ticket 25 times per
    #  loop.  Every loop starts the run afresh -- one more launch per 200, a 64-tickets-per-env table zeroed: under 0.1 us
    #  per call -- so that nobody retires while the clock runs)
    run = EpisodeRun(pool, B, 64 * B)
    outs, scalars = step_records(torch, dev, _hip, rng, B, 80)
    run._attach(types.SimpleNamespace(torch=torch, device=dev))
    lib = _hip.lib()
    first = torch.from_numpy(scalars[0]).to(dev)

    def harvest():
        _hip.check(lib.slhip_episode_run_start(run._sref, _hip.ptr(first), _hip.current_stream_ptr()))
        for k in range(LOOP):
            lib.slhip_episode_run_harvest(run._sref, _hip.ptr(outs[k % 8]), k + 1, _hip.current_stream_ptr())
    res = timed(torch, harvest, repeats, LOOP)
    assert run.counters()["in_progress"] == B
    return {"envs": B, "harvest_alone": res}


def run_whole(torch, dev, repeats):
    from safelife_amd.episode_run import EpisodeRun
    from safelife_amd.levels import LevelPool
    from safelife_amd.runner import VectorRunner
    from safelife_amd.vector_env import SafeLifeVectorEnv
    B, N, L = 1024, 1000, 100
    pool = LevelPool(cycled_levels("prune_still_25", L))
    run = EpisodeRun(pool, B, N)
    env = SafeLifeVectorEnv(pool, B, episode_run=run, time_limit=1000, view_shape=(25, 25), output_channels=TRAIN_CHANNELS,
                            policy_layout="uint8", with_obs=False, **run.env_arguments())
    probs = torch.full((B, 9), 1.0 / 9.0, device=dev)
    values = torch.zeros(B, device=dev)
    runner = VectorRunner(env, lambda obs: (values, probs), generator=torch.Generator(device=dev).manual_seed(1),
                          copy_obs=False, cast_obs=False)
    ms, steps, res = [], [], None
    for k in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = runner.run_episodes(poll_every=16)
        t1 = time.perf_counter()
        if k:                                       # (the first run warms up)
            ms.append((t1 - t0) * 1e3)
            steps.append(run.steps)
    assert (res["flags"] & 1).all() and run.counters()["completed"] == N
    return {"envs": B, "tickets": N, "slots": L, "time_limit": 1000, "poll_every": 16,
            "ms_runs": [round(x, 2) for x in ms], "ms_median": round(statistics.median(ms), 2), "steps_runs": steps,
            "us_per_step_median": round(statistics.median(m * 1e3 / s for m, s in zip(ms, steps)), 2),
            "episode_length_mean": round(float(res["length"].mean()), 2), "episode_length_max": int(res["length"].max()),
            "success_rate": round(float(res["success"].mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of episode_run_bench.json")
    args = ap.parse_args()
    import torch
    from safelife_amd import _hip
    dev = _hip.device()
    report = {"calls_per_loop": LOOP, "device": torch.cuda.get_device_name(dev), "step": {}, "kernels": {}}
    for B in (8192, 1024):
        report["step"]["envs_%d" % B] = run_steps(torch, dev, B, args.repeats)
        print("step", json.dumps(report["step"]["envs_%d" % B], sort_keys=True), flush=True)
        report["kernels"]["envs_%d" % B] = run_harvest(torch, dev, B, args.repeats)
        print("kernels", json.dumps(report["kernels"]["envs_%d" % B], sort_keys=True), flush=True)
    report["run"] = run_whole(torch, dev, args.repeats)
    print("run", json.dumps(report["run"], sort_keys=True), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "episode_run_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
