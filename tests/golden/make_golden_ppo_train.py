#!/usr/bin/env python3
"""
Writes tests/golden/ppo_train_cases.npz by RUNNING THE REFERENCE's PPO.train (training/ppo.py:184-219) on the CPU: what
safelife_amd.ppo.PPOTrainer, ppo_report (slhip_ppo_report_rows / _finish) and tests/ppo_train_ref.py are held to.  The fixture
holds data only.

    python tests/golden/make_golden_ppo_train.py

Runs where make_golden.py runs (it needs the reference's Python, loaded through make_golden.import_reference()).

TRAIN-LOOP CASES.  PPO.train runs on a stub `self`: gen_training_batch adds steps_per_env * num_envs to num_steps and hands out
a tiny batch, train_batch does nothing, calculate_loss returns two constants, save_checkpoint* are no-ops, and the data
logger's log_scalars and run_episodes are recorders.  Per iteration the recorders leave (num_steps after the batch, reported,
tested).  Per case: t_params (num_envs, steps_per_env, report_interval, test_interval, start, has_logger, has_testing_envs),
t_calls (the `steps` of consecutive train() calls) and the events.  The cases: 1, 5, 16 and 96 envs; steps_per_env 1, 7 and 20;
intervals that num_envs * steps_per_env does not divide, and intervals it divides exactly (num_steps lands ON a multiple, where
round_up answers the NEXT one and `>=` decides); a start that is not 0 and one that is itself a multiple of both intervals; two
consecutive train() calls; a run without a logger (nothing is reported) and a run without testing envs (nothing is tested).

REPORT CASES.  What lines 199-205 hand to log_scalars: PPO.train runs ONE iteration on a stub whose gen_training_batch returns
the case's batch, whose model returns the case's stored outputs (values, policy) and whose calculate_loss is the reference's
own; the logger keeps loss, entropy, values, advantages (Python floats).  Every case runs twice on the same numbers: with
float32 tensors, and with the same numbers widened to float64.  Per case (flat arrays; rows of case i at [row_offsets[i],
row_offsets[i+1]), its policy elements at [pol_offsets[i], pol_offsets[i+1])):
    n, n_actions, hyper [5] (eps_policy, eps_value, vf_coef, entropy_reg, entropy_clip), edge (1: a dyadic edge case), name
    values, policy, action_prob, old_values, returns, advantages float32; actions uint8            the inputs
    scalars32 / scalars64 [4] float64: loss, entropy, values, advantages as the logger got them
Random cases: 1, 63, 64, 65, 255, 256, 257 and 4099 rows, each with 2, 9 and 32 actions (drawn as make_golden_ppo_loss.py draws
its rows).  The three cases of one row count share their values, old_values, returns and advantages (stored once: `shared` is
the index of the case that holds them), which keeps the file under the size limit; policy, actions and action_prob are each
case's own.  Edge cases, dyadic numbers, 16 rows: one-hot policies with entropy_clip = 0 (the float32 mean entropy is exactly
0: AT the clip, the bonus stays on); policies (1/2, 1/2) with entropy_clip just below ln 2 (just OVER the clip: the bonus is
the constant); all advantages 0; and old_values of +-2^24 and 1 in turn, whose float32 sum loses the ones.
"""
import collections
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

DEFAULTS = (0.2, 0.2, 0.5, 0.01, 1.0)
SCALARS = ("loss", "entropy", "values", "advantages")
ROWS, ACTIONS = (1, 63, 64, 65, 255, 256, 257, 4099), (2, 9, 32)
Batch = collections.namedtuple("Batch", "obs actions action_prob returns advantages values")


# -------------------------------------------------------------------------------------------------------- the train loop

def train_cases():
    def case(name, B, T, report, test, start, calls, logger=True, testing=True):
        return dict(name=name, params=(B, T, report, test, start, int(logger), int(testing)), calls=calls)

    yield case("envs1-T1", 1, 1, 7, 13, 0, (40,))
    yield case("envs1-T20", 1, 20, 960, 100, 0, (3000,))
    yield case("envs5-T7", 5, 7, 100, 250, 0, (700,))
    yield case("envs5-T7-divides", 5, 7, 35, 70, 0, (350,))
    yield case("envs5-T7-divides-twice", 5, 7, 70, 105, 0, (700,))
    yield case("envs16-T20-reference-intervals", 16, 20, 960, 500000, 0, (6400,))
    yield case("envs16-T20-test-divides", 16, 20, 960, 3200, 0, (9600,))
    yield case("envs16-T7-start-37", 16, 7, 960, 1000, 37, (3000,))
    yield case("envs96-T20", 96, 20, 960, 5000, 0, (20000,))
    yield case("envs96-T1-start-on-a-multiple", 96, 1, 960, 1920, 1920, (4000,))
    yield case("envs5-T20-two-calls", 5, 20, 250, 600, 0, (1000, 730))
    yield case("envs5-T7-no-logger", 5, 7, 100, 250, 0, (700,), logger=False)
    yield case("envs5-T7-no-testing-envs", 5, 7, 100, 250, 0, (700,), testing=False)


def run_train(PPO, torch, case):
    B, T, report, test, start, has_logger, has_testing = case["params"]
    events = []
    one = torch.ones(2)

    def gen_training_batch(steps_per_env):
        assert steps_per_env == T
        stub.num_steps += steps_per_env * B
        events.append([stub.num_steps, 0, 0])
        return Batch(one, one, one, one, one, one)

    def log_scalars(data, steps, tag):
        assert steps == events[-1][0] and tag == "ppo" and sorted(data) == sorted(SCALARS) and not events[-1][1]
        events[-1][1] = 1

    def run_episodes(envs):
        assert envs is stub.testing_envs and not events[-1][2]
        events[-1][2] = 1

    stub = types.SimpleNamespace(
        num_steps=start, steps_per_env=T, report_interval=report, test_interval=test, gen_training_batch=gen_training_batch,
        train_batch=lambda batch: None, calculate_loss=lambda *a: (one, one.sum()),
        data_logger=types.SimpleNamespace(log_scalars=log_scalars) if has_logger else None,
        testing_envs=[None] * 3 if has_testing else None, run_episodes=run_episodes,
        save_checkpoint_if_needed=lambda: None, save_checkpoint=lambda: None)
    for steps in case["calls"]:
        PPO.train(stub, steps)
    return events


# ------------------------------------------------------------------------------------------------------------ the report

def run_report(PPO, torch, hyper, arrays, dtype):
    """Lines 199-205 on the arrays in `dtype`: one iteration of the reference's train -> the four logged floats."""
    t = {k: torch.tensor(v.astype(np.int64) if k == "actions" else v.astype(dtype)) for k, v in arrays.items()}
    logged = {}
    batch = Batch(torch.zeros(len(arrays["values"])), t["actions"], t["action_prob"], t["returns"], t["advantages"],
                  t["old_values"])

    def gen_training_batch(steps_per_env):
        stub.num_steps += 1
        return batch

    stub = types.SimpleNamespace(
        num_steps=0, steps_per_env=1, report_interval=1, test_interval=10 ** 12, gen_training_batch=gen_training_batch,
        train_batch=lambda b: None, model=lambda obs: (t["values"], t["policy"]), eps_policy=hyper[0], eps_value=hyper[1],
        vf_coef=hyper[2], entropy_reg=hyper[3], entropy_clip=hyper[4],
        data_logger=types.SimpleNamespace(log_scalars=lambda data, steps, tag: logged.update(data)), testing_envs=None,
        save_checkpoint_if_needed=lambda: None, save_checkpoint=lambda: None)
    stub.calculate_loss = lambda *a: PPO.calculate_loss(stub, *a)
    with torch.no_grad():
        PPO.train(stub, 1)
    assert sorted(logged) == sorted(SCALARS) and all(isinstance(v, float) for v in logged.values())
    return np.array([logged[k] for k in SCALARS], np.float64)


def edge_cases():
    f32 = np.float32
    n, A = 16, 9
    i = np.arange(n)
    base = dict(values=(0.25 * i).astype(f32), old_values=(0.25 * i - 0.125).astype(f32), returns=np.ones(n, f32),
                advantages=np.array([1.0, -1.0, 0.5, 0.0] * 4, f32), actions=(i % A).astype(np.uint8),
                action_prob=np.array([32, 64, 16, 48] * 4, f32) / 64)
    hot = np.zeros((n, A), f32)
    hot[i, i % A] = 1.0
    yield "edge-entropy-at-clip", (0.25, 0.25, 0.5, 0.01, 0.0), dict(base, policy=hot)
    half = dict(base, policy=np.full((n, 2), 0.5, f32), actions=(i % 2).astype(np.uint8))
    yield "edge-entropy-over-clip", (0.25, 0.25, 0.5, 0.01, 0.693147), half
    spread = np.tile(np.array([16, 8, 8, 8, 8, 4, 4, 4, 4], f32) / 64, (n, 1))
    yield "edge-advantages-zero", (0.25, 0.25, 0.5, 0.01, 4.0), dict(base, policy=spread, advantages=np.zeros(n, f32))
    big = np.array([2.0 ** 24, 1.0, -2.0 ** 24, 1.0] * 4, f32)
    yield "edge-values-cancel", (0.25, 0.25, 0.5, 0.01, 4.0), dict(base, policy=spread, values=big, old_values=big, returns=big)


def report_cases():
    from make_golden_ppo_loss import draw_rows
    rng = np.random.default_rng(20261021)
    for n in ROWS:
        first = None
        for A in ACTIONS:
            arrays = draw_rows(rng, n, A, 1.0 if A == 2 else 2.0, DEFAULTS)
            if first is None:
                first = arrays
            else:
                for k in ("values", "old_values", "returns", "advantages"):
                    arrays[k] = first[k]
            arrays["actions"] = arrays["actions"].astype(np.uint8)
            yield "n%d-a%d" % (n, A), DEFAULTS, arrays, A != ACTIONS[0]
    for name, hyper, arrays in edge_cases():
        yield name, hyper, arrays, False


def main():
    import make_golden
    from make_golden_gae import write_npz
    make_golden.import_reference()
    import torch
    from training.ppo import PPO
    PPO.compute_device = torch.device("cpu")
    torch.set_num_threads(1)

    t = {k: [] for k in ("name", "params", "calls", "steps", "flags")}
    event_offsets, call_offsets = [0], [0]
    for case in train_cases():
        events = run_train(PPO, torch, case)
        t["name"].append(case["name"]), t["params"].append(case["params"]), t["calls"].append(np.array(case["calls"], np.int64))
        t["steps"].append(np.array([e[0] for e in events], np.int64))
        t["flags"].append(np.array([e[1:] for e in events], np.uint8).reshape(-1, 2))
        event_offsets.append(event_offsets[-1] + len(events)), call_offsets.append(call_offsets[-1] + len(case["calls"]))
        f = t["flags"][-1]
        print("%-34s %4d iterations: %3d reported, %3d tested" % (case["name"], len(events), f[:, 0].sum(), f[:, 1].sum()),
              flush=True)
    out = dict(t_name=np.array(t["name"]), t_params=np.array(t["params"], np.int64), t_calls=np.concatenate(t["calls"]),
               t_event_steps=np.concatenate(t["steps"]), t_event_flags=np.concatenate(t["flags"]),
               t_event_offsets=np.array(event_offsets, np.int64), t_call_offsets=np.array(call_offsets, np.int64))

    meta = {k: [] for k in ("n", "n_actions", "hyper", "edge", "name", "shared", "scalars32", "scalars64")}
    own, shared = ("policy", "actions", "action_prob"), ("values", "old_values", "returns", "advantages")
    flat = {k: [] for k in own + shared}
    row_offsets, pol_offsets, shared_offsets = [0], [0], [0]
    holder = None
    for name, hyper, arrays, shares in report_cases():
        n, A = arrays["policy"].shape
        got = {tag: run_report(PPO, torch, hyper, arrays, dtype) for tag, dtype in (("32", np.float32), ("64", np.float64))}
        index = len(meta["n"])
        if not shares:
            holder = index
            for k in shared:
                flat[k].append(arrays[k])
            shared_offsets.append(shared_offsets[-1] + n)
        else:
            shared_offsets.append(shared_offsets[-1])
        meta["n"].append(n), meta["n_actions"].append(A), meta["hyper"].append(hyper), meta["name"].append(name)
        meta["edge"].append(int(name.startswith("edge"))), meta["shared"].append(holder)
        meta["scalars32"].append(got["32"]), meta["scalars64"].append(got["64"])
        for k in own:
            flat[k].append(arrays[k].ravel())
        row_offsets.append(row_offsets[-1] + n), pol_offsets.append(pol_offsets[-1] + n * A)
        print("%-24s n=%4d A=%2d  float32 %s  float64 %s" % (name, n, A, got["32"], got["64"]), flush=True)
    out.update(n=np.array(meta["n"], np.int64), n_actions=np.array(meta["n_actions"], np.int32),
               hyper=np.array(meta["hyper"], np.float64), edge=np.array(meta["edge"], np.uint8), name=np.array(meta["name"]),
               shared=np.array(meta["shared"], np.int32), scalars32=np.array(meta["scalars32"], np.float64),
               scalars64=np.array(meta["scalars64"], np.float64), row_offsets=np.array(row_offsets, np.int64),
               pol_offsets=np.array(pol_offsets, np.int64), shared_offsets=np.array(shared_offsets, np.int64))
    for k, parts in flat.items():
        out[k] = np.concatenate(parts)
    path = os.path.join(HERE, "ppo_train_cases.npz")
    write_npz(path, out)
    size = os.path.getsize(path)
    print("ppo_train_cases: %d train cases, %d report cases, %d bytes" % (len(t["name"]), len(meta["n"]), size))
    assert size < 1024 * 1024


if __name__ == "__main__":
    main()
