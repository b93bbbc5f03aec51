#!/usr/bin/env python3
"""Microseconds per step of the multi-agent fused step with and without the training stack: 8192 envs x 2 agents on the
reference's 26x26 multi-agent specs (levels of tests/golden/trace_multi_*.npz), no observation, random actions, reloads
inside the step.  Variants: unwrapped (slhip_env_step_multi), the env_factory stack with the starting-state baseline, the
same with the inaction baseline, and the stack with the finished-episode queue flushed every 100 steps.
    python tools/multi_wrapped_bench.py [steps] [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from safelife_amd.levels import LevelPool, _device_counts
from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
from tests import util

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 400
OUT = sys.argv[2] if len(sys.argv) > 2 else None
B = 8192
TRAIN = dict(movement_bonus=0.1, as_penalty=True, exit_bonus=0.5, penalty_coef=0.3)
VARIANTS = [("unwrapped", {}), ("stack_starting_state", dict(wrappers=TRAIN)),
            ("stack_inaction", dict(wrappers=dict(TRAIN, baseline="inaction", inaction_seed=1))),
            ("stack_queue_flush100", dict(wrappers=TRAIN, side_effects=dict(capacity=8192, num_samples=100)))]

levels = []
for name in ("multi_asym1", "multi_build_coop", "multi_build_compete"):
    levels += util.levels_from_trace(util.load_trace(name))
pool = LevelPool(levels, counts_fn=_device_counts, n_agents=2, min_performance_fraction=0.3)
acts = torch.randint(0, 9, (64, B, 2), dtype=torch.int32, device="cuda")
res = {"B": B, "agents": 2, "shape": [26, 26], "steps": STEPS}
for name, extra in VARIANTS:
    env = SafeLifeMultiAgentVectorEnv(pool, B, time_limit=100, with_obs=False, first_level=np.arange(B) % len(levels),
                                      **extra)
    env.reset()
    for t in range(20):
        env.step(acts[t % 64])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(STEPS):
        env.step(acts[t % 64])
        if "side_effects" in extra and (t + 1) % 100 == 0:
            env.side_effects_flush()
    torch.cuda.synchronize()
    res[name + "_us_per_step"] = (time.perf_counter() - t0) / STEPS * 1e6
    print(name, "%.1f us per step" % res[name + "_us_per_step"], flush=True)
    del env
    torch.cuda.synchronize()
res["stack_over_unwrapped"] = res["stack_starting_state_us_per_step"] / res["unwrapped_us_per_step"]
print(json.dumps(res))
if OUT:
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
