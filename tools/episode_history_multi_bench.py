#!/usr/bin/env python
"""
Times what an episode history of a multi-agent env (safelife_amd.episode_history.MultiAgentEpisodeHistory ->
slhip_history_capture_multi; csrc/sl_history.hip) costs.

    step       us per SafeLifeMultiAgentVectorEnv.step() with the training observation at 8192 and 1024 envs of 2 agents
               (the 26x26 multi-agent families of tools/episode_log_multi_bench.py): `queue` (side_effects=, which a history
               needs, and no history: what the env did before there was a recorder) and `history` (the same env with a
               recorder that watches 64 envs, 96 slots, interval 1), both in one process, their loops ALTERNATING, so that a
               drift of the machine meets both alike.  The envs' episodes are spread over the time limit, so about B / 1000
               envs reload inside every step.  The cost of a history is `history` minus `queue`: never a number from
               another run.
    capture    the two launches back to back on one stream over the last step's state, nobody done

Device time: HIP events around a loop of calls, every buffer allocated before the events, one loop of warm-up first,
median of five loops.

    python tools/episode_history_multi_bench.py [--repeats 5] [--out DIR]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from episode_history_bench import SLOTS, WATCHED, span, summary      # noqa: E402
from episode_log_multi_bench import A, LOOP, TRAIN_CHANNELS, bench_levels    # noqa: E402


def run_steps(torch, dev, B, repeats):
    from safelife_amd import _hip
    from safelife_amd.episode_history import MultiAgentEpisodeHistory
    from safelife_amd.levels import LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    lv = bench_levels()
    actions = torch.randint(0, 9, (LOOP, B, A), device=dev, dtype=torch.int32)
    kw = dict(time_limit=1000, view_shape=(25, 25), output_channels=TRAIN_CHANNELS, auto_reset=True, level_stride=1)
    queue = dict(capacity=2 * B, num_samples=8)         # holds the (1 + repeats) * LOOP * B / 1000 episodes of the run
    envs, hist = {}, None
    for label in ("queue", "history"):
        pool = LevelPool(lv, n_agents=A)
        if label == "history":
            hist = MultiAgentEpisodeHistory(pool, B, np.arange(WATCHED) * (B // WATCHED), SLOTS)
        env = SafeLifeMultiAgentVectorEnv(pool, B, side_effects=queue, episode_history=hist if label == "history" else None,
                                          **kw)
        env.reset()
        env.base.t["scalars"][:, _hip.SCALAR_COLS["num_steps"]] = (torch.arange(B, device=dev, dtype=torch.int64) * 997
                                                                   % 1000).to(torch.int32)
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
    out = {"envs": B, "agents": A, "watched": WATCHED, "slots": SLOTS}
    for label in envs:
        out[label] = summary(runs[label])
    out["history"]["over_queue_us"] = round(out["history"]["us_per_call_median"] - out["queue"]["us_per_call_median"], 2)
    out["history"]["counters"] = hist.counters()

    def capture():
        for _ in range(LOOP):
            hist._after_step()
    envs["history"].t["out"].zero_()                    # nobody done: the capture's steady state
    span(torch, capture)
    out["capture_alone"] = summary([span(torch, capture) / LOOP for _ in range(repeats)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of episode_history_multi_bench.json")
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
    with open(os.path.join(args.out, "episode_history_multi_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
