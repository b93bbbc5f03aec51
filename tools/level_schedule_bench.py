#!/usr/bin/env python
"""
Times what a level schedule (safelife_amd.schedule.LevelSchedule -> slhip_schedule_draw / _required / _harvest /
_curriculum; csrc/sl_schedule.hip) adds to SafeLifeVectorEnv.step() at the C3 and C4 shapes -- 8192 envs, 25x25, the
training observation, the fixture pools of the reference's prune-still and append-spawn procgen cycled up to 80 and 2000
slots -- and the kernels alone at pools of 1e3, 1e4 and 1e5 slots.

    step          us per env.step() without a schedule, with a switching schedule (two groups, p = 0.5: draw + harvest per
                  step), with a moving exit difficulty on top (draw + required + harvest) and in curriculum mode
                  (curriculum + draw + harvest); the envs' episodes are spread over the time limit, so about 8 envs reload
                  inside every step, as in a training run's steady state
    kernels       us per call of each entry point alone, back to back on one stream (the span includes the gaps the host
                  leaves between launches); the harvest with 8192 envs of which about 8 per step are done

Device time: HIP events around a loop of calls, every buffer allocated before the events, one loop of warm-up first,
median of five loops.

    python tools/level_schedule_bench.py [--envs 8192] [--repeats 5] [--out DIR]
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
LOOP = 200


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


def cycled_levels(name, n):
    from safelife_amd.levels import Level
    with np.load(os.path.join(REPO, "tests", "golden", "pool_%s.npz" % name)) as d:
        base = int(d["n_levels"])
        return [Level(d["board"][k % base], d["goals"][k % base], d["agent_locs"][k % base],
                      spawn_prob=float(d["spawn_prob"][k % base]), min_performance=float(d["min_performance"][k % base]),
                      points_table=d["points_table"][k % base], rng_words=d["rng"][k % base]) for k in range(n)]


def run_steps(torch, dev, name, slots, B, repeats):
    from safelife_amd import _hip
    from safelife_amd.levels import LevelPool
    from safelife_amd.schedule import LevelSchedule, LinearSchedule
    from safelife_amd.vector_env import SafeLifeVectorEnv
    lv = cycled_levels(name, slots)
    actions = torch.randint(0, 9, (LOOP, B), device=dev, dtype=torch.int32)
    kw = dict(time_limit=1000, view_shape=(25, 25), output_channels=TRAIN_CHANNELS, auto_reset=True, level_stride=1)
    half = slots // 2
    moving = LinearSchedule([0, 10 ** 9], [0.001, 1.0])         # another value at every step: the kernel runs every time
    variants = (("plain", None),
                ("switching", dict(mode="switching", p_switch=0.5)),
                ("switching_moving_difficulty", dict(mode="switching", p_switch=0.5, min_performance_fraction=moving)),
                ("curriculum", dict(mode="curriculum")))
    out = {"slots": slots}
    for label, skw in variants:
        pool = LevelPool(lv)
        sched = None if skw is None else LevelSchedule(pool, [(0, half), (half, slots - half)], seed=1, **skw)
        env = SafeLifeVectorEnv(pool, B, level_schedule=sched, **kw)
        env.reset()
        env.t["scalars"][:, _hip.SCALAR_COLS["num_steps"]] =(torch.arange(B, device=dev, dtype=torch.int64) * 997 % 1000).to(torch.int32)
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
    rng = np.random.default_rng(L)
    t = {"min_performance": torch.full((L,), 0.5, dtype=torch.float64, device=dev),
         "available": torch.from_numpy(rng.integers(10, 80, L).astype(np.int32)).to(dev),
         "reward_possible": torch.from_numpy(rng.integers(10, 80, L).astype(np.int32)).to(dev),
         "cur_slot": torch.from_numpy(rng.integers(0, L, B).astype(np.int32)).to(dev),
         "ring": torch.zeros((G, lookback), dtype=torch.float64, device=dev),
         "count": torch.ones(G, dtype=torch.int64, device=dev), "episodes": torch.zeros(G, dtype=torch.int64, device=dev),
         "pos": torch.ones(G, dtype=torch.int32, device=dev), "best": torch.zeros(G, dtype=torch.float64, device=dev),
         "mean": torch.zeros(G, dtype=torch.float64, device=dev), "status": torch.zeros(1, dtype=torch.int32, device=dev)}
    s = _hip.LevelSchedule()
    s.G, s.lookback, s.L = G, lookback, L
    third = L // 3
    for g, (a, n) in enumerate(((0, third), (third, third), (2 * third, L - 2 * third))):
        s.start[g], s.len[g] = a, n
    for name in t:
        setattr(s, name, t[name].data_ptr())
    ref = C.byref(s)
    pool_next = torch.zeros(L, dtype=torch.int32, device=dev)
    pool_scalars = torch.zeros((L, 8), dtype=torch.int32, device=dev)
    probs = (C.c_double * G)(0.2, 0.3, 0.5)
    dprobs = torch.full((G,), 1.0 / G, dtype=torch.float64, device=dev)
    # step records with about 8 of 8192 envs done per step, a different set every call
    outs, scalars = [], []
    for k in range(8):
        rec = np.zeros((B, 4), np.int32)
        flags = np.zeros((B, 4), np.uint8)
        flags[:, 0] = rng.random(B) < 8.0 / 8192.0
        rec[:, 1] = flags.view(np.int32)[:, 0]
        rec[:, 2] = rng.normal(20, 10, B).astype(np.float32).view(np.int32)
        outs.append(torch.from_numpy(rec).to(dev))
        sc = np.zeros((B, 16), np.int32)
        sc[:, _hip.SCALAR_COLS["level_idx"]] = rng.integers(0, L, B)
        scalars.append(torch.from_numpy(sc).to(dev))
    st = _hip.current_stream_ptr()
    counter = [0]

    def draw():
        for _ in range(LOOP):
            lib.slhip_schedule_draw(ref, probs, None, 5, counter[0], _hip.ptr(pool_next), L, st)
            counter[0] += 1

    def required():
        for k in range(LOOP):
            lib.slhip_schedule_required(ref, 0.001 * (k + 1), _hip.ptr(pool_scalars), L, st)

    def harvest():
        for k in range(LOOP):
            lib.slhip_schedule_harvest(ref, _hip.ptr(outs[k % 8]), _hip.ptr(scalars[k % 8]), B, st)

    def curriculum():
        for _ in range(LOOP):
            lib.slhip_schedule_curriculum(ref, _hip.ptr(dprobs), st)

    out = {"slots": L, "envs": B}
    for name, fn in (("draw", draw), ("required", required), ("harvest", harvest), ("curriculum", curriculum)):
        out[name] = timed(torch, fn, repeats, LOOP)
    assert int(t["status"].item()) == 0 and int(t["episodes"].sum().item()) > 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"), help="directory of level_schedule_bench.json")
    args = ap.parse_args()
    import torch
    from safelife_amd import _hip
    dev = _hip.device()
    B = args.envs
    report = {"envs": B, "calls_per_loop": LOOP, "device": torch.cuda.get_device_name(dev), "step": {}, "kernels": {}}
    for config, name in (("C3", "prune_still_25"), ("C4", "append_spawn_25")):
        for slots in (80, 2000):
            key = "%s_%s_%d_slots" % (config, name, slots)
            report["step"][key] = run_steps(torch, dev, name, slots, B, args.repeats)
            print(key, json.dumps(report["step"][key], sort_keys=True), flush=True)
    for L in (1000, 10000, 100000):
        report["kernels"]["L_%d" % L] = run_kernels(torch, _hip, dev, L, B, args.repeats)
        print("kernels", json.dumps(report["kernels"]["L_%d" % L], sort_keys=True), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "level_schedule_bench.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
