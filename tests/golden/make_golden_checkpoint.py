#!/usr/bin/env python3
"""
Writes tests/golden/checkpoint_cases.npz by RUNNING THE REFERENCE's PPO.train (training/ppo.py:184-219) and DQN.train
(training/dqn.py:177-214) on the CPU with the reference's own checkpointing (BaseAlgo, training/base_algo.py:56-139) writing
into a temporary directory: what safelife_amd.checkpoint.Checkpointer, the trainers' ``checkpointer=`` and ``test_runner=``
and tests/checkpoint_ref.py are held to.  The fixture holds data only.

    python tests/golden/make_golden_checkpoint.py

Runs where make_golden.py runs (it needs the reference's Python, loaded through make_golden.import_reference()).

The trainers run on the stub envs of the train fixtures (make_golden_ppo_train.py, make_golden_dqn_update.py): a stub `self`
whose gen_training_batch / take_one_step only count, with BaseAlgo's get_all_checkpoints, save_checkpoint_if_needed,
save_checkpoint and load_checkpoint bound to it UNCHANGED; save_checkpoint is wrapped by a recorder that notes num_steps.

Per schedule: params (kind 0 PPO / 1 DQN, num_envs, steps_per_env, checkpoint_interval, max_checkpoints, reload_after,
replay_initial, test_interval), calls (the `steps` of consecutive train() calls; behind call `reload_after` a FRESH stub
calls load_checkpoint() and goes on -- its replay buffer is empty again, the reference does not checkpoint it), before (file
names put into the directory before the run, oldest first), saves (num_steps of every save in order), left (the directory's
file names at the end), and for DQN with testing envs test_steps / test_eps (the steps at which run_episodes ran and the
epsilon it saw) and eps_testing.
"""
import os
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

JUNK = ("checkpoint-abc.data", "notes.txt", "checkpoint-12.data.bak")


def cases():
    def case(name, kind, B, T, interval, keep, calls, reload_after=-1, replay_initial=0, test_interval=0, before=()):
        return dict(name=name, params=(kind, B, T, interval, keep, reload_after, replay_initial, test_interval), calls=calls,
                    before=before)

    # PPO: 5 envs x 7 steps = 35 steps per batch
    yield case("ppo-interval-divides", 0, 5, 7, 70, 3, (700,))
    yield case("ppo-interval-equals-batch", 0, 5, 7, 35, 3, (350,))
    yield case("ppo-interval-does-not-divide", 0, 5, 7, 100, 3, (700,))
    yield case("ppo-interval-below-batch", 0, 5, 7, 10, 3, (350,))
    yield case("ppo-keep-1", 0, 5, 7, 100, 1, (700,))
    yield case("ppo-second-train-call", 0, 5, 7, 100, 3, (350, 360))
    yield case("ppo-resumed", 0, 5, 7, 100, 3, (350, 360), reload_after=0)
    yield case("ppo-16-envs-reference-interval", 0, 16, 20, 100000, 3, (330000,))
    yield case("ppo-old-files-in-the-directory", 0, 5, 7, 100, 3, (500,),
               before=JUNK + ("checkpoint-7.data", "checkpoint-900000.data", "checkpoint-40.data"))
    # DQN: 5 envs, the replay gate at 60 rows is crossed in mid-run
    yield case("dqn-gate-in-mid-run", 1, 5, 1, 20, 3, (300,), replay_initial=60)
    yield case("dqn-interval-does-not-divide", 1, 5, 1, 33, 3, (300,), replay_initial=60)
    yield case("dqn-keep-1-two-calls", 1, 5, 1, 50, 1, (150, 160), replay_initial=60)
    yield case("dqn-resumed", 1, 5, 1, 50, 3, (150, 160), reload_after=0, replay_initial=60)
    yield case("dqn-gate-never-crossed", 1, 5, 1, 20, 3, (50,), replay_initial=1000)
    yield case("dqn-tests", 1, 5, 1, 50, 3, (300,), replay_initial=60, test_interval=40)
    yield case("dqn-tests-interval-not-a-multiple", 1, 5, 1, 50, 3, (200, 100), replay_initial=85, test_interval=33)


def bind_checkpointing(BaseAlgo, stub, directory, interval, keep, saves):
    stub.checkpoint_directory, stub.checkpoint_interval, stub.max_checkpoints = directory, interval, keep
    stub._last_checkpoint = -1
    stub.checkpoint_attribs = ("marker",)
    stub.marker = {"made_by": "make_golden_checkpoint"}
    stub.get_all_checkpoints = lambda: BaseAlgo.get_all_checkpoints(stub)
    stub.save_checkpoint_if_needed = lambda: BaseAlgo.save_checkpoint_if_needed(stub)
    stub.load_checkpoint = lambda name=None: BaseAlgo.load_checkpoint(stub, name)

    def save_checkpoint():
        saves.append(stub.num_steps)
        BaseAlgo.save_checkpoint(stub)
        assert os.path.exists(os.path.join(directory, "checkpoint-%d.data" % stub.num_steps))

    stub.save_checkpoint = save_checkpoint


def ppo_stub(B, T):
    def gen_training_batch(steps_per_env):
        assert steps_per_env == T
        stub.num_steps += steps_per_env * B

    stub = types.SimpleNamespace(num_steps=0, steps_per_env=T, report_interval=10 ** 12, test_interval=10 ** 12,
                                 gen_training_batch=gen_training_batch, train_batch=lambda batch: None, data_logger=None,
                                 testing_envs=None)
    return stub


def dqn_stub(B, replay_initial, test_interval, eps_testing, tests):
    class Replay(list):
        pass

    def take_one_step(envs):
        assert envs is stub.training_envs
        return [None] * B

    def run_episodes(envs):
        assert envs is stub.testing_envs
        tests.append((stub.num_steps, stub.epsilon))

    model = types.SimpleNamespace(state_dict=lambda: {}, load_state_dict=lambda state: None)
    stub = types.SimpleNamespace(
        num_steps=0, optimize_interval=32, target_update_interval=100, report_interval=256,
        test_interval=test_interval or 10 ** 12, epsilon_schedule=lambda n: 1.0 - 1e-3 * n, epsilon=None,
        epsilon_testing=eps_testing, training_envs=[None] * B, testing_envs=[None] * 2 if test_interval else None,
        take_one_step=take_one_step, replay_buffer=Replay(), replay_initial=replay_initial,
        optimize=lambda report: None, training_model=model, target_model=model, run_episodes=run_episodes)
    stub.add_to_replay = lambda step_data: stub.replay_buffer.extend(step_data)
    return stub


def run_case(BaseAlgo, PPO, DQN, case, directory):
    kind, B, T, interval, keep, reload_after, replay_initial, test_interval = case["params"]
    for name in case["before"]:
        with open(os.path.join(directory, name), "wb") as f:
            f.write(b"old")
        time.sleep(0.01)            # (distinct modification times, oldest first)
    saves, tests = [], []
    eps_testing = 0.01 if kind else 0.0

    def fresh():
        stub = dqn_stub(B, replay_initial, test_interval, eps_testing, tests) if kind else ppo_stub(B, T)
        bind_checkpointing(BaseAlgo, stub, directory, interval, keep, saves)
        return stub

    stub = fresh()
    for k, steps in enumerate(case["calls"]):
        (DQN if kind else PPO).train(stub, steps)
        if k == reload_after:
            at = stub.num_steps
            stub = fresh()
            stub.load_checkpoint()
            assert stub.num_steps == at and stub._last_checkpoint == at
    return saves, sorted(os.listdir(directory)), tests, eps_testing


def main():
    import make_golden
    from make_golden_gae import write_npz
    make_golden.import_reference()
    import torch
    from training.base_algo import BaseAlgo
    from training.dqn import DQN
    from training.ppo import PPO
    torch.set_num_threads(1)

    keys = ("calls", "saves", "before", "left", "test_steps", "test_eps")
    flat = {k: [] for k in keys}
    offsets = {k: [0] for k in ("calls", "saves", "before", "left", "test")}
    names, params, eps = [], [], []
    for case in cases():
        with tempfile.TemporaryDirectory() as directory:
            saves, left, tests, eps_testing = run_case(BaseAlgo, PPO, DQN, case, directory)
        names.append(case["name"]), params.append(case["params"]), eps.append(eps_testing)
        flat["calls"] += list(case["calls"])
        flat["saves"] += saves
        flat["before"] += list(case["before"])
        flat["left"] += left
        flat["test_steps"] += [t[0] for t in tests]
        flat["test_eps"] += [t[1] for t in tests]
        for k, n in (("calls", len(case["calls"])), ("saves", len(saves)), ("before", len(case["before"])),
                     ("left", len(left)), ("test", len(tests))):
            offsets[k].append(offsets[k][-1] + n)
        print("%-36s %3d saves %s ... left %s  tests %s" % (case["name"], len(saves), saves[:6], left, [t[0] for t in tests][:8]),
              flush=True)
    out = dict(name=np.array(names), params=np.array(params, np.int64), eps_testing=np.array(eps, np.float64),
               calls=np.array(flat["calls"], np.int64), saves=np.array(flat["saves"], np.int64),
               before=np.array(flat["before"] or [""])[:len(flat["before"])], left=np.array(flat["left"]),
               test_steps=np.array(flat["test_steps"], np.int64), test_eps=np.array(flat["test_eps"], np.float64),
               call_offsets=np.array(offsets["calls"], np.int64), save_offsets=np.array(offsets["saves"], np.int64),
               before_offsets=np.array(offsets["before"], np.int64), left_offsets=np.array(offsets["left"], np.int64),
               test_offsets=np.array(offsets["test"], np.int64))
    path = os.path.join(HERE, "checkpoint_cases.npz")
    write_npz(path, out)
    size = os.path.getsize(path)
    print("checkpoint_cases: %d schedules, %d bytes" % (len(names), size))
    assert size < 1024 * 1024


if __name__ == "__main__":
    main()
