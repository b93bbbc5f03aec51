#!/usr/bin/env python
"""
Times what a level schedule adds to SafeLifeMultiAgentVectorEnv.step() (safelife_amd.schedule.LevelSchedule on a pool with
two agents per level -> slhip_schedule_draw / _required_multi / _harvest_multi / _curriculum; csrc/sl_schedule.hip) at 1024
and 8192 envs of 26x26 boards -- the levels of the reference's multi-agent specs asym1, build-coop and build-compete
(tests/golden/trace_multi_*.npz) cycled up to 90 slots, three groups -- and the kernels alone.

    step          us per env.step() without a schedule (the yardstick: today's multi-agent step), with a uniform schedule
                  (draw + harvest per step), with a moving exit difficulty on top (draw + required + harvest) and in
                  curriculum mode (curriculum + draw + harvest); the envs' episodes are spread over the time limit, so a few
                  envs reload inside every step, as in a training run's steady state
    kernels       us per call of each entry point alone, back to back on one stream (the span includes the gaps the host
                  leaves between launches): the draw, the per-agent required points (1000 slots x 2 agents), the multi-agent
                  harvest over [B, 2] records with about B / 1000 envs finished per call and a third of the others with one
                  agent done -- and, beside it, the single-agent harvest at the same B with the same envs finished

Device time: HIP events around a loop of calls, every buffer allocated before the events, one loop of warm-up first,
median of five loops.

    python tools/level_schedule_multi_bench.py [--repeats 5] [--out DIR]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TRAIN_CHANNELS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 25, 26, 27)
FAMILIES = ("multi_asym1", "multi_build_coop", "multi_build_compete")
LOOP, A, PER_GROUP = 200, 2, 30


def timed(torch, fn, repeats, calls):
    fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / calls)
    return {"us_per_call_runs": [round(x, 2) for x in runs], "us_per_call_median": round(statistics.median(runs), 2)}


def family_levels(name, n):
    from safelife_amd.levels import Level
    with np.load(os.path.join(REPO, "tests", "golden", "trace_%s.npz" % name)) as d:
        base = int(d["n_levels"])
        out = []
        for k in range(n):
            pre = "level%d_" % (k % base)
            out.append(Level(d[pre + "board"], d[pre + "goals"], d[pre + "agent_locs"], spawn_prob=float(d[pre + "spawn_prob"]),
                             min_performance=float(d[pre + "min_performance"]), points_table=d[pre + "points_table"],
                             rng_words=np.array(d[pre + "rng"], np.uint64)))
        return out


def run_steps(torch, dev, B, repeats):
    from safelife_amd import _hip
    from safelife_amd.levels import LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    from safelife_amd.schedule import LevelSchedule, LinearSchedule
    lv = [x for name in FAMILIES for x in family_levels(name, PER_GROUP)]
    groups = [(k * PER_GROUP, PER_GROUP) for k in range(len(FAMILIES))]
    actions = torch.randint(0, 9, (LOOP, B, A), device=dev, dtype=torch.int32)
    kw = dict(time_limit=1000, view_shape=(25, 25), output_channels=TRAIN_CHANNELS, auto_reset=True, level_stride=1)
    moving = LinearSchedule([0, 10 ** 9], [0.001, 1.0])         # another value at every step: the kernel runs every time
    variants = (("plain", None),
                ("uniform", dict(mode="uniform")),
                ("uniform_moving_difficulty", dict(mode="uniform", min_performance_fraction=moving)),
                ("curriculum", dict(mode="curriculum")))
    out = {"slots": len(lv), "agents": A}
    for label, skw in variants:
        pool = LevelPool(lv, n_agents=A)
        sched = None if skw is None else LevelSchedule(pool, groups, seed=1, **skw)
        env = SafeLifeMultiAgentVectorEnv(pool, B, level_schedule=sched, **kw)
        env.reset()
        env.base.t["scalars"][:, _hip.SCALAR_COLS["num_steps"]] = (torch.arange(B, device=dev, dtype=torch.int64) * 997
                                                                   % 1000).to(torch.int32)
        clock = [0]

        def loop():
            for t in range(LOOP):
                if sched is not None:
                    sched.training_steps = clock[0]
                    clock[0] += B
                env.step(actions[t])
        out[label] = timed(torch, loop, repeats, LOOP)
        if sched is not None:
            out[label]["episodes_harvested"] = int(sched.stats()["episodes"].sum())
            out[label]["over_plain_us"] = round(out[label]["us_per_call_median"] - out["plain"]["us_per_call_median"], 2)
        del env, sched, pool
        torch.cuda.empty_cache()
    return out


def run_kernels(torch, _hip, dev, L, B, repeats):
    lib = _hip.lib()
    G, lookback = 3, 100
    rng = np.random.default_rng(L + B)
    t = {"min_performance": torch.full((L,), 0.5, dtype=torch.float64, device=dev),
         "cur_slot": torch.from_numpy(rng.integers(0, L, B).astype(np.int32)).to(dev),
         "ring": torch.zeros((G, lookback), dtype=torch.float64, device=dev),
         "count": torch.ones(G, dtype=torch.int64, device=dev), "episodes": torch.zeros(G, dtype=torch.int64, device=dev),
         "pos": torch.ones(G, dtype=torch.int32, device=dev), "best": torch.zeros(G, dtype=torch.float64, device=dev),
         "mean": torch.zeros(G, dtype=torch.float64, device=dev), "status": torch.zeros(1, dtype=torch.int32, device=dev)}
    available = torch.from_numpy(rng.integers(10, 80, (L, A)).astype(np.int32)).to(dev)
    possible = torch.from_numpy(rng.integers(10, 80, (L, A)).astype(np.int32)).to(dev)
    pool_agents = torch.zeros((L, A, 8), dtype=torch.int32, device=dev)
    m = _hip.LevelScheduleMulti()
    m.s.G, m.s.lookback, m.s.L, m.n_agents = G, lookback, L, A
    third = L // 3
    for g, (a, n) in enumerate(((0, third), (third, third), (2 * third, L - 2 * third))):
        m.s.start[g], m.s.len[g] = a, n
    for name in t:
        setattr(m.s, name, t[name].data_ptr())
    m.available, m.reward_possible, m.pool_agents = available.data_ptr(), possible.data_ptr(), pool_agents.data_ptr()
    # the single-agent harvest reads agent 0's column of the same table
    single_possible = possible[:, 0].contiguous()
    m.s.reward_possible = single_possible.data_ptr()
    ref, sref = C.byref(m), C.byref(m.s)
    pool_next = torch.zeros(L, dtype=torch.int32, device=dev)
    probs = (C.c_double * G)(0.2, 0.3, 0.5)
    # step records with about B / 1000 envs finished per step and a third of the others with one agent done, a different set
    # every call; the single-agent records: the same envs finished
    outs, singles, scalars = [], [], []
    for k in range(8):
        finished = rng.random(B) < 1.0 / 1000.0
        finished[k] = True
        done = np.repeat(finished, A).reshape(B, A)
        some = rng.random(B) < 1.0 / 3.0
        done[some & ~finished, 0] = True
        rec = np.zeros((B, A, 4), np.int32)
        flags = np.zeros((B, A, 4), np.uint8)
        flags[:, :, 0] = done
        rec[:, :, 1] = flags.view(np.int32)[:, :, 0]
        rec[:, :, 2] = rng.normal(20, 10, (B, A)).astype(np.float32).view(np.int32)
        outs.append(torch.from_numpy(rec).to(dev))
        one = rec[:, 1].copy()                                  # (agent 1 is done exactly where the env has finished)
        singles.append(torch.from_numpy(one).to(dev))
        sc = np.zeros((B, 16), np.int32)
        sc[:, _hip.SCALAR_COLS["level_idx"]] = rng.integers(0, L, B)
        scalars.append(torch.from_numpy(sc).to(dev))
    st = _hip.current_stream_ptr()
    counter = [0]

    def draw():
        for _ in range(LOOP):
            lib.slhip_schedule_draw(sref, probs, None, 5, counter[0], _hip.ptr(pool_next), L, st)
            counter[0] += 1

    def required_multi():
        for k in range(LOOP):
            lib.slhip_schedule_required_multi(ref, 0.001 * (k + 1), st)

    def harvest_multi():
        for k in range(LOOP):
            m.out = outs[k % 8].data_ptr()
            lib.slhip_schedule_harvest_multi(ref, _hip.ptr(scalars[k % 8]), B, st)

    def harvest_single():
        for k in range(LOOP):
            lib.slhip_schedule_harvest(sref, _hip.ptr(singles[k % 8]), _hip.ptr(scalars[k % 8]), B, st)

    out = {"slots": L, "envs": B, "agents": A}
    for name, fn in (("draw", draw), ("required_multi", required_multi), ("harvest_multi", harvest_multi),
                     ("harvest_single_agent", harvest_single)):
        out[name] = timed(torch, fn, repeats, LOOP)
    assert int(t["status"].item()) == 0 and int(t["episodes"].sum().item()) > 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of level_schedule_multi_bench.json")
    args = ap.parse_args()
    import torch
    from safelife_amd import _hip
    dev = _hip.device()
    report = {"calls_per_loop": LOOP, "device": torch.cuda.get_device_name(dev), "step": {}, "kernels": {}}
    for B in (1024, 8192):
        report["step"]["B_%d" % B] = run_steps(torch, dev, B, args.repeats)
        print("step B=%d" % B, json.dumps(report["step"]["B_%d" % B], sort_keys=True), flush=True)
        report["kernels"]["B_%d" % B] = run_kernels(torch, _hip, dev, 1000, B, args.repeats)
        print("kernels B=%d" % B, json.dumps(report["kernels"]["B_%d" % B], sort_keys=True), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "level_schedule_multi_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
