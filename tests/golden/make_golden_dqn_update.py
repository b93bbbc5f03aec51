#!/usr/bin/env python3
"""
Writes tests/golden/dqn_update_cases.npz by RUNNING THE REFERENCE's DQN.optimize (training/dqn.py:136-175) and DQN.train
(:177-214) on the CPU: what slhip_dqn_loss_forward / _backward, safelife_amd.dqn.DQNTrainer and tests/dqn_loss_ref.py are held
to.  The fixture holds data only.

    python tests/golden/make_golden_dqn_update.py

Runs where make_golden.py runs (it needs the reference's Python, loaded through make_golden.import_reference()).

LOSS CASES.  optimize is called on a stub `self`: its replay buffer hands out the case's rows, its two models return preset
tensors (q_values a leaf that requires grad), its optimiser does nothing and its data logger keeps what optimize reports.
loss.backward() -- the reference's own call -- leaves d loss / d q_values in the leaf.  Every case runs twice on the same
numbers: with the reference's float32 tensors, and with `self.tensor` handing out float64 whatever dtype optimize asks for,
so that lines 149-157 and 165-170 run in float64 (Q-values widened; a ring case's reward is then its unrounded float64 sum).
Per case (flat arrays; rows of case i at [row_offsets[i], row_offsets[i+1]), its Q elements at [q_offsets[i], q_offsets[i+1])):
    n, n_actions, gamma, multi_step, ring (1: the ring's storage, 0: a gathered batch), edge (1: a dyadic edge case), name
    q_values, next_q_values [n, A] float32;  action int64, reward float64, done uint8 [n]     the inputs
    td32 / td64 [n]       q_value - expected_q_value: optimize does not return it, so its lines are evaluated here again on the
                          same tensors and checked to recombine into its loss bit for bit
    dq32 / dq64 [n]       d loss / d q_values in the column of the action taken (every other column is exactly 0: asserted)
    scalars32 / scalars64 [5] float64: loss, q_model_mean, q_model_max, q_target_mean, q_target_max as optimize logged them
A ring case's rewards are float64 numbers that are NOT float32-representable (the n-step sums of the ring); a batch case's
are float32 numbers.  No row of the fixture has a maximum that is a zero of both signs (+0 in one column, -0 in another):
which of the two torch.max returns is not defined, and main() asserts that no such row got in.

Random cases: rows 1, 63, 64, 65, 257 with 9 actions in both source forms; 4099 rows as a ring of 9 actions and as a batch of
2; 65 rows with 2 and 32 actions in both forms; 257 rows with 32 actions from the ring.  (gamma, multi_step) cycles through
(0.97, 5), (0.9, 1), (0.99, 16) so that each meets both forms.  A fifth of the rows are done.

Edge cases, dyadic numbers (gamma = 0.5, multi_step = 2: a discount of exactly 0.25; everything a multiple of 2^-6), in both
forms: all rows done; no row done; a mixed case with a row whose maximum is tied in two columns, rows whose action is not the
greedy column, a row with td exactly 0; n = 1; a case with +inf in next_q_values (loss +inf); a case with a NaN in
next_q_values, one NaN row done and one not, and a done row with +inf (0 * inf: NaN).

main() also checks that the fixture separates the readings a kernel could get wrong without anyone noticing: contracting
`reward + disc * m` into one FMA, and adding the ring's float64 reward in float64 and rounding afterwards, must each change
td32 on at least one row.

TRAIN-LOOP CASES.  DQN.train runs on a stub `self`: take_one_step and add_to_replay do nothing but count -- the replay
buffer is the reference's own ReplayBuffer, pushed `pushes[k]` times in iteration k -- optimize and
target_model.load_state_dict are recorders, the epsilon schedule is the reference's spline.  Per iteration the recorders leave
(num_steps after the step, epsilon, optimized, reported, target_updated).  Per case: t_params (num_envs, optimize_interval,
target_update_interval, report_interval, replay_initial, start, capacity), t_calls (the `steps` of consecutive train() calls),
t_pushes and the events.  The cases: 1, 5, 16 and 96 envs; intervals the env count does not divide; optimize_interval below
the env count; replay_initial crossed in mid-run; a ring too small ever to reach replay_initial; two consecutive train()
calls; and runs that start just below each knot of the epsilon spline (5e4, 5e5, 4e6) and cross it, one sample ON the knot.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

HYPERS = ((0.97, 5), (0.9, 1), (0.99, 16))
SCALARS = ("loss", "q_model_mean", "q_model_max", "q_target_mean", "q_target_max")


def run_reference(DQN, torch, case, wide):
    """The reference's optimize on the case; wide: every tensor optimize builds is float64."""
    n = case["n"]
    reward = case["reward"]             # float64 numbers either way: optimize casts them
    dtype = torch.float64 if wide else torch.float32
    q = torch.tensor(case["q_values"].astype(np.float64 if wide else np.float32), requires_grad=True)
    nq = torch.tensor(case["next_q_values"].astype(np.float64 if wide else np.float32))
    logged = {}

    def tensor(data, want):
        data = np.asanyarray(data)
        if wide and want == torch.float32:
            want = torch.float64
        return torch.as_tensor(data, dtype=want)

    rows = [(0.0, int(a), r, 0.0, bool(d)) for a, r, d in zip(case["action"], reward, case["done"])]

    class Replay(object):
        def __len__(self):
            return n

        def sample(self, k):
            return list(zip(*rows[:k]))

    stub = types.SimpleNamespace(
        replay_buffer=Replay(), replay_initial=0, training_batch_size=n, tensor=tensor,
        training_model=lambda obs: q, target_model=lambda obs: nq, gamma=case["gamma"],
        multi_step_learning=case["multi_step"], optimizer=types.SimpleNamespace(zero_grad=lambda: None, step=lambda: None),
        data_logger=types.SimpleNamespace(log_scalars=lambda data, steps, tag: logged.update(data)), epsilon=0.0, num_steps=0)
    with np.errstate(all="ignore"):
        DQN.optimize(stub, report=True)
    assert q.grad is not None and q.grad.dtype == dtype
    with torch.no_grad():       # the reference's lines again, for td
        action = tensor(case["action"], torch.int64)
        rew = tensor(reward, torch.float32)
        done = tensor(case["done"].astype(bool), torch.float32)
        q_value = q.gather(1, action.unsqueeze(1)).squeeze(1)
        next_q_value, _ = nq.max(1)
        discount = case["gamma"] ** case["multi_step"] * (1 - done)
        expected = rew + discount * next_q_value
        td = q_value - expected
        again = torch.mean(td ** 2).item()
        assert td.dtype == dtype
        assert again == logged["loss"] or (np.isnan(again) and np.isnan(logged["loss"])), (again, logged["loss"])
    grad = q.grad.numpy()
    others = np.ones(grad.shape, bool)
    others[np.arange(n), case["action"]] = False
    assert not grad[others].any(), "a gradient outside the column of the action taken"
    return dict(td=td.numpy(), dq=grad[np.arange(n), case["action"]].copy(),
                scalars=np.array([logged[k] for k in SCALARS], np.float64))


def random_case(rng, n, A, hyper, ring):
    q = rng.normal(0.0, 2.0, (n, A)).astype(np.float32)
    nq = rng.normal(0.0, 2.0, (n, A)).astype(np.float32)
    action = rng.integers(0, A, n).astype(np.int64)
    done = (rng.random(n) < 0.2).astype(np.uint8)
    reward = rng.normal(0.0, 1.0, n)
    reward[rng.random(n) < 0.2] = 0.0
    if ring:                    # n-step sums: float64 numbers with bits below float32's last
        assert n < 8 or np.any(reward.astype(np.float32).astype(np.float64) != reward)
    else:
        reward = reward.astype(np.float32).astype(np.float64)
    return dict(n=n, n_actions=A, gamma=hyper[0], multi_step=hyper[1], ring=ring, edge=False, q_values=q, next_q_values=nq,
                action=action, reward=reward, done=done)


def edge_rows():
    """The mixed edge case: 8 dyadic rows of 9 actions -> (q row, next_q row, action, reward, done)."""
    base_q = np.array([16, -8, 40, 24, 0, 8, -32, 4, 12], np.float64) / 64
    base_n = np.array([8, 72, -16, 24, 32, 4, 0, -40, 16], np.float64) / 64       # maximum 72/64 in column 1
    rows = []

    def row(q=base_q, nq=base_n, a=2, r=0.5, d=0):
        rows.append((np.asarray(q, np.float64), np.asarray(nq, np.float64), a, r, d))

    row()                                                                   # 0 the action taken is the greedy column
    row(a=5)                                                                # 1 ... is not
    row(a=6, d=1)                                                           # 2 ... is the smallest, the row is done
    tied = base_n.copy()
    tied[7] = tied[1]
    row(nq=tied, a=3)                                                       # 3 the maximum is tied in two columns
    both = base_q.copy()
    both[0] = both[2]
    row(q=both, a=0)                                                        # 4 the greedy Q-value is tied, the second one taken
    row(a=2, r=40 / 64 - 0.25 * 72 / 64)                                    # 5 td exactly 0: q = r + 0.25 * m
    row(a=2, r=40 / 64, d=1)                                                # 6 td exactly 0 on a done row
    row(q=-base_q, nq=-base_n, a=8, r=-1.25)                                # 7 negative maxima
    return rows


def pack(rows, ring, name):
    return dict(n=len(rows), n_actions=len(rows[0][0]), gamma=0.5, multi_step=2, ring=ring, edge=True, name=name,
                q_values=np.stack([r[0] for r in rows]).astype(np.float32),
                next_q_values=np.stack([r[1] for r in rows]).astype(np.float32),
                action=np.array([r[2] for r in rows], np.int64), reward=np.array([r[3] for r in rows], np.float64),
                done=np.array([r[4] for r in rows], np.uint8))


def edge_cases():
    rows = edge_rows()
    for ring in (True, False):
        tag = "ring" if ring else "batch"
        yield pack(rows, ring, "edge-mixed-" + tag)
        yield pack([r[:4] + (1,) for r in rows], ring, "edge-all-done-" + tag)
        yield pack([r[:4] + (0,) for r in rows], ring, "edge-none-done-" + tag)
        yield pack(rows[1:2], ring, "edge-n1-" + tag)
        inf = [list(r) for r in rows[:4]]
        inf[1][1] = inf[1][1].copy()
        inf[1][1][4] = np.inf                                               # not done: expected = +inf, td = -inf
        yield pack([tuple(r) for r in inf], ring, "edge-inf-" + tag)
        nan = [list(r) for r in rows[:5]]
        for k in (0, 2):                                                    # row 0 not done, row 2 done: NaN either way
            nan[k][1] = nan[k][1].copy()
            nan[k][1][k + 3] = np.nan
        nan[4][1] = nan[4][1].copy()
        nan[4][1][0] = np.inf
        nan[4][4] = 1                                                       # done and +inf: 0 * inf
        yield pack([tuple(r) for r in nan], ring, "edge-nan-" + tag)


def make_cases():
    rng = np.random.default_rng(20261020)
    k = 0

    def nxt(n, A, ring):
        nonlocal k
        hyper = HYPERS[k % 3]
        k += 1
        c = random_case(rng, n, A, hyper, ring)
        c["name"] = "n%d-a%d-g%g-m%d-%s" % (n, A, hyper[0], hyper[1], "ring" if ring else "batch")
        return c

    for n in (1, 63, 64, 65, 257):
        for ring in (True, False):
            yield nxt(n, 9, ring)
    k += 1
    yield nxt(4099, 9, True)
    yield nxt(4099, 2, False)
    for A in (2, 32):
        for ring in (True, False):
            yield nxt(65, A, ring)
    yield nxt(257, 32, True)
    for c in edge_cases():
        yield c


def float32_td(case, how):
    """td of the float32 run under a reading of `reward + disc * m`: "plain", "fma" or "late" (tests/dqn_loss_ref.py)."""
    from tests import dqn_loss_ref as ref
    kw = {"fma": dict(fused_multiply_add=True), "late": dict(late_reward_rounding=True), "plain": {}}[how]
    c = dict(case, id=case["name"])
    return ref.restate(c, np.float32, **kw)["td"]


# -------------------------------------------------------------------------------------------------------- the train loop

def train_cases():
    rng = np.random.default_rng(20261021)

    def case(name, B, opt, upd, rep, initial, start, calls, capacity=10 ** 6, full=False):
        iters, steps = 0, start
        for c in calls:
            end = steps + c
            while steps < end:
                steps += B
                iters += 1
        pushes = np.full(iters, B) if full else rng.integers(0, 2 * B + 1, iters)
        return dict(name=name, params=(B, opt, upd, rep, initial, start, capacity), calls=calls, pushes=pushes.astype(np.int32))

    yield case("envs1", 1, 32, 100, 64, 50, 0, (300,))
    yield case("envs5-two-calls", 5, 32, 70, 64, 100, 0, (400, 333))
    yield case("envs16-open-from-the-start", 16, 32, 200, 256, 0, 0, (1000,))
    yield case("envs96-interval-below-envs", 96, 32, 1000, 256, 500, 0, (3000, 289))
    yield case("envs5-odd-intervals", 5, 7, 11, 13, 60, 3, (200, 200))
    yield case("envs5-ring-too-small", 5, 7, 11, 13, 41, 0, (150,), capacity=40)
    yield case("envs16-defaults", 16, 32, 10000, 256, 40000, 0, (48000,), full=True)
    for knot in (50000, 500000, 4000000):
        yield case("envs16-knot-%d" % knot, 16, 32, 10000, 256, 0, knot - 48, (128,))
        yield case("envs5-knot-%d" % knot, 5, 32, 10000, 256, 0, knot - 12, (30,))


def run_train(dqn_module, case):
    DQN = dqn_module.DQN
    B, opt, upd, rep, initial, start, capacity = case["params"]
    events = []
    replay = dqn_module.ReplayBuffer(capacity)
    pushes = iter(case["pushes"])

    def take_one_step(envs):
        events.append([stub.num_steps + B, stub.epsilon, 0, 0, 0])

    def add_to_replay(step):
        for _ in range(int(next(pushes))):
            replay.push(None)

    def optimize(report=False):
        assert not events[-1][2]
        events[-1][2], events[-1][3] = 1, int(bool(report))

    def load_state_dict(state):
        assert state == "the training model's state" and not events[-1][4]
        events[-1][4] = 1

    stub = types.SimpleNamespace(
        num_steps=start, optimize_interval=opt, target_update_interval=upd, report_interval=rep, test_interval=10 ** 12,
        epsilon_schedule=DQN.epsilon_schedule, epsilon=None, training_envs=[None] * B, take_one_step=take_one_step,
        add_to_replay=add_to_replay, replay_buffer=replay, replay_initial=initial, optimize=optimize,
        target_model=types.SimpleNamespace(load_state_dict=load_state_dict),
        training_model=types.SimpleNamespace(state_dict=lambda: "the training model's state"),
        save_checkpoint_if_needed=lambda: None, save_checkpoint=lambda: None, testing_envs=None)
    for steps in case["calls"]:
        DQN.train(stub, steps)
    assert len(events) == len(case["pushes"]) and next(pushes, None) is None
    return events


def main():
    import make_golden
    from make_golden_gae import write_npz
    make_golden.import_reference()
    import torch
    import training.dqn as dqn_module
    DQN = dqn_module.DQN
    DQN.compute_device = torch.device("cpu")
    torch.set_num_threads(1)

    meta = {k: [] for k in ("n", "n_actions", "gamma", "multi_step", "ring", "edge", "name", "scalars32", "scalars64")}
    names = ("q_values", "next_q_values", "action", "reward", "done", "td32", "td64", "dq32", "dq64")
    flat = {k: [] for k in names}
    row_offsets, q_offsets = [0], [0]
    differs = dict(fma=0, late=0)
    for case in make_cases():
        n, A = case["q_values"].shape
        for x in (case["q_values"], case["next_q_values"]):        # no maximum that is a zero of both signs
            mx = np.nanmax(x, axis=1, keepdims=True)
            zeros = (x == 0) & (mx == 0)
            assert not np.any(np.any(zeros & np.signbit(x), axis=1) & np.any(zeros & ~np.signbit(x), axis=1)), case["name"]
        got = {"32": run_reference(DQN, torch, case, False), "64": run_reference(DQN, torch, case, True)}
        assert got["32"]["td"].dtype == got["32"]["dq"].dtype == np.float32
        assert got["64"]["td"].dtype == got["64"]["dq"].dtype == np.float64
        plain = float32_td(case, "plain")
        assert np.array_equal(plain, got["32"]["td"], equal_nan=True), case["name"]
        for how in differs:
            with np.errstate(all="ignore"):
                other = float32_td(case, how)
            differs[how] += int(np.sum(~((other == plain) | (np.isnan(other) & np.isnan(plain)))))
        for k in ("n_actions", "gamma", "multi_step", "name"):
            meta[k].append(case[k])
        meta["n"].append(n), meta["ring"].append(int(case["ring"])), meta["edge"].append(int(case["edge"]))
        for k in ("q_values", "next_q_values", "action", "reward", "done"):
            flat[k].append(case[k].ravel())
        for tag in ("32", "64"):
            flat["td" + tag].append(got[tag]["td"]), flat["dq" + tag].append(got[tag]["dq"])
            meta["scalars" + tag].append(got[tag]["scalars"])
        row_offsets.append(row_offsets[-1] + n), q_offsets.append(q_offsets[-1] + n * A)
        print("%-28s n=%4d A=%2d loss32=%.7g loss64=%.15g" % (case["name"], n, A, got["32"]["scalars"][0],
                                                             got["64"]["scalars"][0]), flush=True)
    print("rows on which td32 changes under the FMA reading: %d, under late rounding of the ring's reward: %d"
          % (differs["fma"], differs["late"]))
    assert differs["fma"] > 0 and differs["late"] > 0

    out = dict(n=np.array(meta["n"], np.int64), n_actions=np.array(meta["n_actions"], np.int32),
               gamma=np.array(meta["gamma"], np.float64), multi_step=np.array(meta["multi_step"], np.int32),
               ring=np.array(meta["ring"], np.uint8), edge=np.array(meta["edge"], np.uint8), name=np.array(meta["name"]),
               scalars32=np.array(meta["scalars32"], np.float64), scalars64=np.array(meta["scalars64"], np.float64),
               row_offsets=np.array(row_offsets, np.int64), q_offsets=np.array(q_offsets, np.int64))
    for k, parts in flat.items():
        out[k] = np.concatenate(parts)

    t = {k: [] for k in ("name", "params", "calls", "pushes", "steps", "epsilon", "flags")}
    event_offsets, call_offsets = [0], [0]
    for case in train_cases():
        events = run_train(dqn_module, case)
        t["name"].append(case["name"]), t["params"].append(case["params"])
        t["calls"].append(np.array(case["calls"], np.int64)), t["pushes"].append(case["pushes"])
        t["steps"].append(np.array([e[0] for e in events], np.int64))
        t["epsilon"].append(np.array([e[1] for e in events], np.float64))
        t["flags"].append(np.array([e[2:] for e in events], np.uint8).reshape(-1, 3))
        event_offsets.append(event_offsets[-1] + len(events)), call_offsets.append(call_offsets[-1] + len(case["calls"]))
        f = t["flags"][-1]
        print("%-30s %5d iterations: %4d optimised, %3d reported, %3d target updates" % (
            case["name"], len(events), f[:, 0].sum(), f[:, 1].sum(), f[:, 2].sum()), flush=True)
    out.update(t_name=np.array(t["name"]), t_params=np.array(t["params"], np.int64), t_calls=np.concatenate(t["calls"]),
               t_pushes=np.concatenate(t["pushes"]), t_event_steps=np.concatenate(t["steps"]),
               t_event_epsilon=np.concatenate(t["epsilon"]), t_event_flags=np.concatenate(t["flags"]),
               t_event_offsets=np.array(event_offsets, np.int64), t_call_offsets=np.array(call_offsets, np.int64))
    path = os.path.join(HERE, "dqn_update_cases.npz")
    write_npz(path, out)
    print("dqn_update_cases: %d loss cases, %d train cases, %d bytes" % (len(meta["n"]), len(t["name"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
