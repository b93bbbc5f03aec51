"""
A numpy restatement of the multi-agent training-batch contract (include/safelife_hip.h, sl_rollout_multi): who is active
at which step, which rows form a trajectory, the trajectory's arithmetic with its float64 islands, ``traj_start``, the
order of the compacted rows and their ``agent_ids``.  It walks forwards, trajectory by trajectory, with numpy arrays whose
dtypes are chosen the way the reference's ``np.append`` chooses them; it shares nothing with the kernels (which walk the
columns backwards) nor with tests/gae_ref.py (which spells every rounding out as a scalar cast).

    window(R, D, V, fv, gamma, lmda, active0, resets0) -> Window

R: rewards [T,B,A] float32 / float64 as the env returned them; D: the ENV's done flags [T,B,A] (they stay 1 for an agent
that is gone); V: float32 [T,B,A] the model's values; fv: float32 [B,A], V(next_obs) of the window's last step; active0
[B,A] / resets0 [B]: the state carried in (None: everybody active, no resets yet).  Rows where ``active`` is 0 hold zeros.
The keyword arguments switch on one deliberate mistake each (WRONG_VARIANTS).
"""
import collections
import os

import numpy as np

f32, f64 = np.float32, np.float64

Window = collections.namedtuple("Window", "returns advantages traj_start active rows agent_ids active_end resets_end "
                                          "handed_done")


def bookkeeping(D, active0=None, resets0=None, *, reset_on_any=False):
    """-> active [T,B,A] bool, resets [T,B] (the env's reset count DURING step t), active_end [B,A], resets_end [B]."""
    D = np.asarray(D).astype(bool)
    T, B, A = D.shape
    now = np.ones((B, A), bool) if active0 is None else np.array(active0, bool)
    count = np.zeros(B, np.int64) if resets0 is None else np.array(resets0, np.int64)
    active, resets = np.zeros((T, B, A), bool), np.zeros((T, B), np.int64)
    for t in range(T):
        active[t], resets[t] = now, count
        now = now & ~D[t]
        over = now.sum(axis=1) < A if reset_on_any else ~now.any(axis=1)
        now[over] = True
        count = count + over
    return active, resets, now, count


def trajectory(r, v, final_value, gamma, lmda, *, closed_in_reward_dtype=False):
    """ppo.py:119-132 for one trajectory.  r: rewards (an array of the env's dtype), v: float32 values; final_value: None
    for the Python float 0.0 of a trajectory that nobody bootstrapped, else a float32 scalar."""
    n = len(r)
    with np.errstate(over="ignore", invalid="ignore"):
        if final_value is None and not closed_in_reward_dtype:
            tail = np.array([0.0], f64)                     # a Python float joins the array
        elif final_value is None:
            tail = np.array([0.0], f32)
        else:
            tail = np.array([final_value], f32)
        head = np.array(v[1:], f32) if n > 1 else np.array([], f64)     # np.append([], x) is float64
        val1 = np.concatenate([head, tail])                 # float64 as soon as one part is
        # (a Python float times a float32 ARRAY stays float32; numpy 2)
        g1 = val1.dtype.type(gamma)
        advantages = (r + g1 * val1) - np.array(v, f32)
        returns = np.array(r)
        returns[-1] = returns[-1] + (f32(gamma) * tail[0].astype(f32) if final_value is not None else 0.0)
        g_r, l_a = returns.dtype.type(gamma), advantages.dtype.type(lmda)
        for i in range(n - 2, -1, -1):
            returns[i] = returns[i] + g_r * returns[i + 1]
            advantages[i] = advantages[i] + l_a * advantages[i + 1]
    return returns.astype(f32), advantages.astype(f32)


def window(R, D, V, fv, gamma, lmda, active0=None, resets0=None, *, bootstrap_gone=False, gap_in_trajectory=False,
           no_carry=False, reset_on_any=False, closed_in_reward_dtype=False):
    R, V, fv = np.asarray(R), np.asarray(V, f32), np.asarray(fv, f32)
    D = np.asarray(D).astype(bool)
    assert R.dtype in (np.dtype(f32), np.dtype(f64)) and R.shape == D.shape == V.shape and R.ndim == 3
    T, B, A = R.shape
    if no_carry:
        active0 = None
    active, resets, active_end, resets_end = bookkeeping(D, active0, resets0, reset_on_any=reset_on_any)
    returns, advantages = np.zeros((T, B, A), f32), np.zeros((T, B, A), f32)
    start = np.zeros((T, B, A), np.uint8)
    for b in range(B):
        for a in range(A):
            act, done = active[:, b, a], D[:, b, a]
            # runs of rows that belong together
            runs, t0 = [], None
            for t in range(T):
                if t0 is None and (act[t] or gap_in_trajectory):
                    t0 = t
                if t0 is not None and act[t] and (done[t] or t == T - 1):
                    runs.append((t0, t))
                    t0 = None
            for t0, t1 in runs:
                rows = np.arange(t0, t1 + 1)
                r = np.where(act[rows], R[rows, b, a], R.dtype.type(0))
                v = np.where(act[rows], V[rows, b, a], f32(0))
                final = None if done[t1] else fv[b, a]      # t1 == T - 1 and the agent goes on
                ret, adv = trajectory(r, v, final, gamma, lmda, closed_in_reward_dtype=closed_in_reward_dtype)
                keep = act[rows]
                returns[rows[keep], b, a], advantages[rows[keep], b, a] = ret[keep], adv[keep]
                start[rows[keep][0], b, a] = 1
            if bootstrap_gone and runs and not act[T - 1] and runs[-1][1] < T - 1:
                t0, t1 = runs[-1]                           # the mistake: an agent that left earlier is bootstrapped
                rows = np.arange(t0, t1 + 1)
                ret, adv = trajectory(R[rows, b, a], V[rows, b, a], fv[b, a], gamma, lmda)
                returns[rows, b, a], advantages[rows, b, a] = ret, adv
    flat = np.flatnonzero(active.ravel())
    t_, rest = np.divmod(flat, B * A)
    b_, a_ = np.divmod(rest, A)
    agent_ids = np.stack([b_, resets[t_, b_], a_], axis=1)
    return Window(returns, advantages, start, active.astype(np.uint8), flat, agent_ids, active_end, resets_end,
                  (D & active).astype(np.uint8))


WRONG_VARIANTS = ("bootstrap_gone", "gap_in_trajectory", "no_carry", "reset_on_any", "closed_in_reward_dtype")


def two_windows(case, **variant):
    """Both windows of a fixture case, the second starting from what the first left."""
    out, active, resets = [], None, None
    for w in range(2):
        res = window(case["R"][w], case["D"][w], case["values"][w], case["V_boot"][w], case["gamma"], case["lmda"],
                     active, resets, **variant)
        out.append(res)
        active, resets = res.active_end, res.resets_end
    return out


_cases = None


def load_cases():
    """tests/golden/gae_multi_cases.npz (make_golden_gae_multi.py) as a list of dicts: T, B, A, gamma, lmda, R / D
    [2,T,B,A], V_boot [2,B,A], and the reference's returns / advantages / values / action_prob / valid [2,T,B,A].
    Loaded once; nobody writes into it."""
    global _cases
    if _cases is None:
        out = []
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gae_multi_cases.npz")) as d:
            z = {k: d[k] for k in d.files}
        for i in range(len(z["T"])):
            T, B, A = int(z["T"][i]), int(z["B"][i]), int(z["A"][i])
            n = 2 * T * B * A
            o, bo, ro = int(z["offsets"][i]), int(z["b_offsets"][i]), int(z["r_offsets"][i])
            c = dict(index=i, T=T, B=B, A=A, gamma=float(z["gamma"][i]), lmda=float(z["lmda"][i]),
                     R=z["R64" if z["reward_f64"][i] else "R32"][ro:ro + n].reshape(2, T, B, A),
                     V_boot=z["V_boot"][bo:bo + 2 * B * A].reshape(2, B, A), n_actions=int(z["n_actions"].ravel()[0]))
            for name in ("D", "valid", "returns", "advantages", "values", "action_prob"):
                c[name] = z[name][o:o + n].reshape(2, T, B, A)
            for a in c.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            c["id"] = "T%d-B%d-A%d-%s-g%g-l%g" % (T, B, A, c["R"].dtype.name, c["gamma"], c["lmda"])
            out.append(c)
        _cases = out
    return _cases


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)
