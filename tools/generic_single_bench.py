#!/usr/bin/env python3
"""Microseconds per step of a single-agent batch that falls to the size-generic family: 8192 envs at 25x41, the levels,
channels and wrappers of tests/step_matrix_cases.py (the shape is one of tests/step_generic_cases.py's),
training wrappers and a uint8 observation, 400 timed steps between two HIP events.  Library: SAFELIFE_HIP_LIB."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from safelife_amd.levels import LevelPool, _device_counts
from safelife_amd.vector_env import SafeLifeVectorEnv
from tests import step_matrix_cases as smc

B = 8192
levels = smc.build_levels(25, 41, "one", "spawn")
pool = LevelPool(levels, counts_fn=_device_counts, min_performance_fraction=1.0)
env = SafeLifeVectorEnv(pool, B, time_limit=100, view_shape=(15, 15), output_channels=smc.CHANNELS_15, with_obs=True,
                        first_level=(np.arange(B) % len(levels)).astype(np.int32), wrappers=dict(smc.TRAINING_WRAPPERS))
assert not env.row_kernels()
env.reset()
acts = torch.randint(0, 9, (440, B), device=env.device, dtype=torch.int32,
                     generator=torch.Generator(device=env.device).manual_seed(5))
for t in range(40):
    env.step(acts[t])
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for t in range(40, 440):
    env.step(acts[t])
e1.record()
torch.cuda.synchronize()
print(json.dumps({"single_25x41_wrap_obs15_us_per_step": e0.elapsed_time(e1) / 400 * 1e3}))
