#!/usr/bin/env python
"""
Times what a multi-agent episode log (safelife_amd.episode_log.MultiAgentEpisodeLog -> slhip_episode_log_harvest_multi /
_join_multi / _summaries_multi; csrc/sl_episode_log.hip) costs, in the shape of tools/episode_log_bench.py.

    step       us per SafeLifeMultiAgentVectorEnv.step() with the training observation at 8192 and 1024 envs of 2 agents (the
               three multi-agent trace families cycled to 24 slots each), without a log and with one, in the same process;
               the envs' episodes are spread over the time limit, so about B / 1000 envs reload inside every step.
               `harvest_alone`: the harvest kernel back to back on one stream over step records of which about B / 1000 envs
               per step have finished and as many again have one agent done (the span includes the gaps the host leaves
               between launches)
    flush      one flush()'s join plus summaries for 160 steps' worth of rows, each kernel alone, as in
               tools/episode_log_bench.py: the join over a queue that holds exactly those episodes in scrambled order, the
               summaries over exactly those rows with a one-element fill in front that rewinds `summarised`; `fill_alone`
               is that fill by itself, to be subtracted

Device time: HIP events around a loop of calls, every buffer allocated before the events, one loop of warm-up first,
median of five loops.

    python tools/episode_log_multi_bench.py [--repeats 5] [--out DIR]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from level_schedule_multi_bench import FAMILIES, family_levels, timed    # noqa: E402

TRAIN_CHANNELS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 25, 26, 27)
LOOP, A, PER_FAMILY = 200, 2, 24


def bench_levels():
    return [x for name in FAMILIES for x in family_levels(name, PER_FAMILY)]


def step_records(torch, dev, _hip, rng, B, L, sets=8):
    """Step records [B, A] with about B / 1000 envs finished per step and as many with one agent done, a different set every
    call, and agent states and scalars to go with them."""
    outs, agents, scalars = [], [], []
    for _ in range(sets):
        rec = np.zeros((B, A, 4), np.int32)
        flags = np.zeros((B, A, 4), np.uint8)
        flags[:, :, 0] = (rng.random(B) < 1.0 / 1000.0)[:, None]
        flags[:, 0, 0] |= rng.random(B) < 1.0 / 1000.0
        flags[:, :, 1] = rng.random((B, A)) < 0.5
        rec[:, :, 1] = flags.view(np.int32)[:, :, 0]
        rec[:, :, 2] = rng.normal(20, 10, (B, A)).astype(np.float32).view(np.int32)
        rec[:, :, 3] = rng.integers(1, 1000, (B, A))
        outs.append(torch.from_numpy(rec).to(dev))
        ag = np.zeros((B, A, 12), np.int32)
        ag[:, :, _hip.AGENT_COLS["required_points"]] = rng.integers(0, 40, (B, A))
        agents.append(torch.from_numpy(ag).to(dev))
        sc = np.zeros((B, 16), np.int32)
        sc[:, _hip.SCALAR_COLS["level_idx"]] = rng.integers(0, L, B)
        scalars.append(sc)
    return outs, agents, scalars


def run_steps(torch, dev, B, repeats):
    from safelife_amd import _hip
    from safelife_amd.episode_log import MultiAgentEpisodeLog
    from safelife_amd.levels import LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    lv = bench_levels()
    actions = torch.randint(0, 9, (LOOP, B, A), device=dev, dtype=torch.int32)
    kw = dict(time_limit=1000, view_shape=(25, 25), output_channels=TRAIN_CHANNELS, auto_reset=True, level_stride=1)
    out = {"envs": B, "agents": A, "slots": len(lv)}
    for label in ("plain", "logged"):
        pool = LevelPool(lv, n_agents=A)
        log = MultiAgentEpisodeLog(pool, B, 4 * B) if label == "logged" else None
        env = SafeLifeMultiAgentVectorEnv(pool, B, episode_log=log, **kw)
        env.reset()
        env.base.t["scalars"][:, _hip.SCALAR_COLS["num_steps"]] = (torch.arange(B, device=dev, dtype=torch.int64) * 997
                                                                   % 1000).to(torch.int32)

        def loop():
            for t in range(LOOP):
                env.step(actions[t])
        out[label] = timed(torch, loop, repeats, LOOP)
        if log is not None:
            out[label]["episodes_logged"] = log.counters()["episodes"]
            out[label]["over_plain_us"] = round(out[label]["us_per_call_median"] - out["plain"]["us_per_call_median"], 2)
        del env, log, pool
        torch.cuda.empty_cache()
    return out


def run_kernels(torch, dev, B, repeats):
    from safelife_amd import _hip
    from safelife_amd.episode_log import MultiAgentEpisodeLog
    from safelife_amd.levels import LevelPool
    rng = np.random.default_rng(B)
    K = _hip.SL_SE_MAX_KEYS
    pool = LevelPool(bench_levels(), n_agents=A)
    L = pool.n_slots
    weights = {"life-green": 1.0, "life-red": 0.5, "crate-gray": 2.0}

    def fresh():
        log = MultiAgentEpisodeLog(pool, B, 4 * B, side_effect_weights=weights)
        log.allocate(torch, dev)
        return log

    outs, agents, scalars = step_records(torch, dev, _hip, rng, B, L)
    dev_scalars = [torch.from_numpy(sc).to(dev) for sc in scalars]
    log = fresh()

    def harvest():
        for k in range(LOOP):
            log.harvest(outs[k % 8], agents[k % 8], dev_scalars[k % 8])
    out = {"envs": B, "agents": A, "row_bytes": log.row_dtype.itemsize, "harvest_alone": timed(torch, harvest, repeats, LOOP)}

    # 160 steps' worth of rows, with episode counters that tell an env's episodes apart
    log = fresh()
    for k in range(160):
        sc = scalars[k % 8].copy()
        sc[:, _hip.SCALAR_COLS["episode_idx"]] = k + 1
        log.harvest(outs[k % 8], agents[k % 8], torch.from_numpy(sc).to(dev))
    rows = log.rows()
    n = len(rows)
    order = rng.permutation(n)
    rec = np.zeros((n, 8), np.int32)
    rec[:, 0], rec[:, 3] = rows["env"][order], rows["episode_idx"][order]
    keys = np.full((n, K), 0xFFFF, np.uint16)
    keys[:, :6] = [9, 0x209, 0x409, 0x609, 48, 16]
    scores = np.full((n, K, 2), np.nan)
    scores[:, :6] = rng.random((n, 6, 2)) * 3
    q = [torch.from_numpy(a).to(dev) for a in (np.array([n], np.int32), rec, scores, keys.view(np.int16),
                                               np.zeros((n, K), np.int32))]

    def join():
        for _ in range(LOOP):
            log.join(*q)
    out["flush"] = {"rows": n, "join": timed(torch, join, repeats, LOOP)}
    assert log.counters()["unmatched"] == 0 and (log.rows()["flags"] & 1).all()
    summarised = log.t["counters"][3:4]

    def summaries():
        for _ in range(LOOP):
            summarised.zero_()
            log.summarise()

    def fill():
        for _ in range(LOOP):
            summarised.zero_()
    out["flush"]["summaries_with_fill"] = timed(torch, summaries, repeats, LOOP)
    out["flush"]["fill_alone"] = timed(torch, fill, repeats, LOOP)
    out["flush"]["join_plus_summaries_us"] = round(out["flush"]["join"]["us_per_call_median"]
                                                   + out["flush"]["summaries_with_fill"]["us_per_call_median"]
                                                   - out["flush"]["fill_alone"]["us_per_call_median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of episode_log_multi_bench.json")
    args = ap.parse_args()
    import torch
    from safelife_amd import _hip
    dev = _hip.device()
    report = {"calls_per_loop": LOOP, "device": torch.cuda.get_device_name(dev), "step": {}, "kernels": {}}
    for B in (8192, 1024):
        report["step"]["envs_%d" % B] = run_steps(torch, dev, B, args.repeats)
        print("step", json.dumps(report["step"]["envs_%d" % B], sort_keys=True), flush=True)
        report["kernels"]["envs_%d" % B] = run_kernels(torch, dev, B, args.repeats)
        print("kernels", json.dumps(report["kernels"]["envs_%d" % B], sort_keys=True), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "episode_log_multi_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
