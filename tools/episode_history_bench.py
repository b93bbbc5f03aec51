#!/usr/bin/env python
"""
Times what an episode history (safelife_amd.episode_history.EpisodeHistory -> slhip_history_capture; csrc/sl_history.hip)
costs.

    step       us per SafeLifeVectorEnv.step() with the training observation at 8192 and 1024 envs (25x25, the prune-still
               fixture pool cycled to 80 slots): `plain` (no queue), `queue` (side_effects=, which a history needs, and no
               history) and `history` (the same env with a recorder that watches 64 envs, 96 slots, interval 1), all three in
               one process, their loops ALTERNATING, so that a drift of the machine meets all of them alike.  The envs'
               episodes are spread over the time limit, so about B / 1000 envs reload inside every step.  The cost of a
               history is `history` minus `queue`: never a number from another run.
    capture    the two launches back to back on one stream over the last step's state, nobody done
    frames     EpisodeHistory.frames(i) of the longest kept history, per frame

Device time: HIP events around a loop of calls, every buffer allocated before the events, one loop of warm-up first,
median of five loops.

    python tools/episode_history_bench.py [--repeats 5] [--out DIR]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.episode_log_bench import LOOP, TRAIN_CHANNELS, cycled_levels    # noqa: E402

WATCHED, SLOTS = 64, 96


def span(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def summary(runs):
    return {"us_per_call_runs": [round(x, 2) for x in runs], "us_per_call_median": round(statistics.median(runs), 2)}


def run_steps(torch, dev, B, repeats):
    from safelife_amd import _hip
    from safelife_amd.episode_history import EpisodeHistory
    from safelife_amd.levels import LevelPool
    from safelife_amd.vector_env import SafeLifeVectorEnv
    lv = cycled_levels("prune_still_25", 80)
    actions = torch.randint(0, 9, (LOOP, B), device=dev, dtype=torch.int32)
    kw = dict(time_limit=1000, view_shape=(25, 25), output_channels=TRAIN_CHANNELS, auto_reset=True, level_stride=1)
    queue = dict(capacity=2 * B, num_samples=8)         # holds the (1 + repeats) * LOOP * B / 1000 episodes of the run
    envs, hist = {}, None
    for label in ("plain", "queue", "history"):
        pool = LevelPool(lv)
        if label == "history":
            hist = EpisodeHistory(pool, B, np.arange(WATCHED) * (B // WATCHED), SLOTS)
        env = SafeLifeVectorEnv(pool, B, side_effects=None if label == "plain" else queue,
                                episode_history=hist if label == "history" else None, **kw)
        env.reset()
        env.t["scalars"][:, _hip.SCALAR_COLS["num_steps"]] = (torch.arange(B, device=dev, dtype=torch.int64) * 997 % 1000).to(torch.int32)
        envs[label] = env

    def loop(env):
        for t in range(LOOP):
            env.step(actions[t])
    runs = {label: [] for label in envs}
    for r in range(repeats + 1):                        # (the first round warms up)
        for label, env in envs.items():
            us = span(torch, lambda: loop(env)) / LOOP
            if r:
                runs[label].append(us)
    out = {"envs": B, "watched": WATCHED, "slots": SLOTS}
    for label in envs:
        out[label] = summary(runs[label])
    out["history"]["over_queue_us"] = round(out["history"]["us_per_call_median"] - out["queue"]["us_per_call_median"], 2)
    out["queue"]["over_plain_us"] = round(out["queue"]["us_per_call_median"] - out["plain"]["us_per_call_median"], 2)
    out["history"]["counters"] = hist.counters()

    def capture():
        for _ in range(LOOP):
            hist._after_step()
    envs["history"].t["out"].zero_()                    # nobody done: the capture's steady state
    span(torch, capture)
    out["capture_alone"] = summary([span(torch, capture) / LOOP for _ in range(repeats)])

    listing = hist.entries()
    if len(listing):
        i = int(np.argmax(listing["length"]))
        n = int(listing["length"][i])
        frames = hist.frames(i)
        span(torch, lambda: hist.frames(i, out=frames))
        per = [span(torch, lambda: hist.frames(i, out=frames)) / n for _ in range(repeats)]
        out["frames"] = dict(summary(per), frames=n)
        out["frames"]["us_per_frame_median"] = out["frames"].pop("us_per_call_median")
        out["frames"]["us_per_frame_runs"] = out["frames"].pop("us_per_call_runs")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of episode_history_bench.json")
    args = ap.parse_args()
    import torch
    from safelife_amd import _hip
    dev = _hip.device()
    report = {"calls_per_loop": LOOP, "device": torch.cuda.get_device_name(dev), "step": {}}
    for B in (8192, 1024):
        report["step"]["envs_%d" % B] = run_steps(torch, dev, B, args.repeats)
        print("step", json.dumps(report["step"]["envs_%d" % B], sort_keys=True), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "episode_history_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
