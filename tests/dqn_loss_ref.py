"""The DQN update restated in numpy: the TD loss of the reference's DQN.optimize (training/dqn.py:152-157) with its gradient
WRITTEN OUT BY HAND -- no autograd, so the restatement shares nothing with torch's backward and nothing with sl_dqn.hip --
in float64 or in float32, the four report scalars (:165-170), and a pure-Python model of the schedule of DQN.train (:177-208).
What the fixture tests/golden/dqn_update_cases.npz (the reference's own results) holds both this and the kernels to.

Every numpy operation below is one elementwise IEEE operation of the arrays' dtype, in the reference's order; the means are
float64 sums of those terms (the kernel's rule; the reference's float32 means are in the fixture).

WRONG_VARIANTS names deliberately wrong readings of the rule; ``td_loss_and_grads(..., **{variant: True})`` computes one."""
import os

import numpy as np

from tests import util

WRONG_VARIANTS = ("gamma_not_powered", "done_ignored", "greedy_column", "fused_multiply_add", "late_reward_rounding",
                  "gradient_over_cells")
SCALARS = ("loss", "q_model_mean", "q_model_max", "q_target_mean", "q_target_max")
FLAGS = ("optimized", "reported", "target_updated")


def load_cases(path=None):
    z = np.load(path or os.path.join(util.GOLDEN, "dqn_update_cases.npz"))
    ro, qo = z["row_offsets"], z["q_offsets"]
    cases = []
    for i, name in enumerate(z["name"]):
        n, A = int(z["n"][i]), int(z["n_actions"][i])
        c = dict(id=str(name), n=n, n_actions=A, gamma=float(z["gamma"][i]), multi_step=int(z["multi_step"][i]),
                 ring=bool(z["ring"][i]), edge=bool(z["edge"][i]))
        for k in ("action", "reward", "done", "td32", "td64", "dq32", "dq64"):
            c[k] = z[k][ro[i]:ro[i + 1]]
        for k in ("q_values", "next_q_values"):
            c[k] = z[k][qo[i]:qo[i + 1]].reshape(n, A)
        c["scalars32"], c["scalars64"] = z["scalars32"][i], z["scalars64"][i]
        cases.append(c)
    return cases


def source_arrays(case):
    """action, reward, done in the storage types of the case's source form: the ring's (int32, float64, uint8) or a gathered
    batch's (int64, float32, float32).  The fixture keeps rewards as float64; a batch case's are float32 numbers."""
    if case["ring"]:
        return case["action"].astype(np.int32), case["reward"].astype(np.float64), case["done"].astype(np.uint8)
    reward = case["reward"].astype(np.float32)
    assert np.array_equal(reward.astype(np.float64), case["reward"])
    return case["action"].astype(np.int64), reward, case["done"].astype(np.float32)


def full_gradient(case, tag):
    """The fixture's d loss / d q_values as [n, A]: the reference's gradient is zero outside the column of the action
    taken (the generator asserts it), so only that column is kept."""
    d = np.zeros((case["n"], case["n_actions"]), case["dq" + tag].dtype)
    d[np.arange(case["n"]), case["action"]] = case["dq" + tag]
    return d


def _fma32(a, b, c):
    """fma(a, b, c) of float32 numbers: the product is exact in float64; the sum is rounded to float64 and then to float32
    (a double rounding in rare cases, which does not matter to a reading that is meant to be wrong)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def td_loss_and_grads(q_values, next_q_values, action, reward, done, gamma, multi_step, dtype, grad_loss=1.0, grad_td=None,
                      gamma_not_powered=False, done_ignored=False, greedy_column=False, fused_multiply_add=False,
                      late_reward_rounding=False, gradient_over_cells=False):
    """-> dict(td [n], loss, scalars [5] float64 (SCALARS), dq [n, A]) in `dtype`.  `reward` may be float64 (the ring's n-step
    sum): it is rounded to `dtype` ONCE, before anything is added to it."""
    dt = np.dtype(dtype).type
    q, nq = q_values.astype(dt), next_q_values.astype(dt)
    n, A = q.shape
    idx = np.arange(n)
    a = np.asarray(action, np.int64)
    discount = dt(float(gamma) if gamma_not_powered else float(gamma) ** int(multi_step))   # a Python float meets a tensor
    rew = np.asarray(reward).astype(dt)
    d = np.asarray(done).astype(dt)

    # torch.max's value: NaN if any element is NaN (np.max propagates NaN too)
    with np.errstate(invalid="ignore", over="ignore"):
        m = nq.max(axis=1)
        taken = q[idx, np.argmax(q, axis=1)] if greedy_column else q[idx, a]
        nd = dt(1) - (np.zeros_like(d) if done_ignored else d)
        disc = discount * nd
        if fused_multiply_add and dt is np.float32:
            expected = _fma32(disc, m, rew)
        elif late_reward_rounding and dt is np.float32:
            expected = (np.asarray(reward, np.float64) + (disc * m).astype(np.float64)).astype(np.float32)
        else:
            expected = rew + disc * m
        td = taken - expected
        sq = td * td

        loss = sq.sum(dtype=np.float64) / n
        scalars = np.array([loss, q.sum(dtype=np.float64) / (n * A), q.max(axis=1).sum(dtype=np.float64) / n,
                            nq.sum(dtype=np.float64) / (n * A), m.sum(dtype=np.float64) / n], np.float64)

        # ---- backward, by hand: mean's backward divides by n, pow's multiplies by 2 * td, gather's scatters
        g = dt(grad_loss) / dt(n * A if gradient_over_cells else n)
        col = g * (dt(2) * td)
        if grad_td is not None:
            col = col + np.asarray(grad_td).astype(dt)
    dq = np.zeros((n, A), dt)
    dq[idx, a] = col
    return dict(td=td, loss=dt(loss), scalars=scalars, dq=dq)


def restate(case, dtype, **kw):
    action, reward, done = source_arrays(case)
    return td_loss_and_grads(case["q_values"], case["next_q_values"], action, reward, done, case["gamma"],
                             case["multi_step"], dtype, **kw)


def same_values(a, b):
    """Bit for bit, except that a NaN equals a NaN whatever its sign and payload (two IEEE machines need not agree on
    those); shapes and dtypes must agree."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    u = np.dtype("u%d" % a.dtype.itemsize)
    return bool(np.array_equal(a.view(u)[~nan], b.view(u)[~nan]))


# -------------------------------------------------------------------------------------------------------- the train loop

def load_train_cases(path=None):
    z = np.load(path or os.path.join(util.GOLDEN, "dqn_update_cases.npz"))
    eo, co = z["t_event_offsets"], z["t_call_offsets"]
    cases = []
    for i, name in enumerate(z["t_name"]):
        lo, hi = eo[i], eo[i + 1]
        events = [(int(s), float(e), bool(f[0]), bool(f[1]), bool(f[2]))
                  for s, e, f in zip(z["t_event_steps"][lo:hi], z["t_event_epsilon"][lo:hi], z["t_event_flags"][lo:hi])]
        p = z["t_params"][i]
        cases.append(dict(id=str(name), num_envs=int(p[0]), optimize_interval=int(p[1]), target_update_interval=int(p[2]),
                          report_interval=int(p[3]), replay_initial=int(p[4]), start=int(p[5]), capacity=int(p[6]),
                          train_calls=[int(x) for x in z["t_calls"][co[i]:co[i + 1]]],
                          pushes=[int(x) for x in z["t_pushes"][lo:hi]], events=events))
    return cases


def round_up(x, r):
    return x + r - x % r


def schedule_model(case, epsilon_schedule, round_up_after_the_step=False, report_flag_per_call_only=False):
    """The event list of DQN.train in plain Python: per iteration (num_steps after the step, epsilon, optimized, reported,
    target_updated).  The replay's length after iteration k is min(capacity, pushes[0] + .. + pushes[k]).  The two keyword
    arguments are wrong readings: the three round_up evaluated on num_steps AFTER the step, and a report flag that is raised
    at the start of train() only."""
    B = case["num_envs"]
    num_steps, pushed, k = case["start"], 0, 0
    events = []
    for steps in case["train_calls"]:
        needs_report = True
        max_steps = num_steps + steps
        while num_steps < max_steps:
            next_opt = round_up(num_steps, case["optimize_interval"])
            next_update = round_up(num_steps, case["target_update_interval"])
            next_report = round_up(num_steps, case["report_interval"])
            epsilon = float(epsilon_schedule(num_steps))
            pushed += case["pushes"][k]
            k += 1
            num_steps += B
            if round_up_after_the_step:
                next_opt = round_up(num_steps, case["optimize_interval"])
                next_update = round_up(num_steps, case["target_update_interval"])
                next_report = round_up(num_steps, case["report_interval"])
            optimized = reported = updated = False
            if min(pushed, case["capacity"]) >= case["replay_initial"]:
                if num_steps >= next_report and not report_flag_per_call_only:
                    needs_report = True
                if num_steps >= next_opt:
                    optimized, reported, needs_report = True, needs_report, False
                if num_steps >= next_update:
                    updated = True
            events.append((num_steps, epsilon, optimized, reported, updated))
    return events
