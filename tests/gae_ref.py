"""
A numpy restatement of the returns / GAE contract of slhip_training_batch (include/safelife_hip.h), written trajectory by
trajectory with every rounding spelled out as an explicit scalar cast -- it shares nothing with the kernel, which walks
columns backwards and decides a trajectory's width at its end.

    training_batch(R, D, V, fv, gamma, lmda) -> returns f32 [T,B], advantages f32 [T,B], traj_start u8 [T,B]

R: rewards [T,B] float32 or float64; D: done [T,B]; V: values float32 [T,B]; fv: float32 [B], V(next_obs) of the window's
last step.  The keyword arguments switch on one deliberate mistake each (tests/test_training_batch_host.py shows that the
reference's fixture tells every one of them from the contract).
"""
import numpy as np

f32, f64 = np.float32, np.float64


def trajectories(D):
    """(b, t0, t1): env b's steps t0 .. t1 inclusive form one trajectory -- it ends at a done step or at the window's end."""
    T, B = D.shape
    for b in range(B):
        t0 = 0
        for t in range(T):
            if D[t, b] or t == T - 1:
                yield b, t0, t
                t0 = t + 1


def one_trajectory(r, v, closed, final_value, gamma, lmda, *, all_float32=False, length1_narrow=False,
                   bootstrap_closed=False, wide_bootstrap_product=False):
    """r: the trajectory's rewards (float32 or float64), v: its float32 values; -> (returns, advantages) in float32."""
    n = len(r)
    rdt = r.dtype.type
    r64 = rdt is f64
    if closed and not bootstrap_closed:
        final_value = None                      # the Python float 0.0
    wide = closed or n == 1
    if length1_narrow and not closed:
        wide = False
    if all_float32:
        wide = False
    g32, l32, g_r = f32(gamma), f32(lmda), rdt(gamma)
    g64, l64 = f64(gamma), f64(lmda)

    ret = [None] * n
    if final_value is None:
        ret[n - 1] = rdt(r[n - 1] + rdt(0.0))
    elif wide_bootstrap_product and r64:
        ret[n - 1] = f64(r[n - 1] + g64 * f64(final_value))
    else:
        ret[n - 1] = rdt(r[n - 1] + rdt(f32(g32 * f32(final_value))))
    for i in range(n - 2, -1, -1):
        ret[i] = rdt(r[i] + rdt(g_r * ret[i + 1]))

    adv = [None] * n
    for i in range(n - 1, -1, -1):
        nxt = v[i + 1] if i + 1 < n else (f32(0.0) if final_value is None else f32(final_value))
        if wide:
            a = f64(f64(f64(r[i]) + f64(g64 * f64(nxt))) - f64(v[i]))
            if i + 1 < n:
                a = f64(a + f64(l64 * adv[i + 1]))
        elif r64 and not all_float32:
            prod = f64(g64 * f64(nxt)) if wide_bootstrap_product else f64(f32(g32 * f32(nxt)))
            a = f64(f64(r[i] + prod) - f64(v[i]))
            if i + 1 < n:
                a = f64(a + f64(l64 * adv[i + 1]))
        else:
            a = f32(f32(f32(r[i]) + f32(g32 * f32(nxt))) - f32(v[i]))
            if i + 1 < n:
                a = f32(a + f32(l32 * adv[i + 1]))
        adv[i] = a
    return np.array(ret).astype(f32), np.array(adv).astype(f32)


def training_batch(R, D, V, fv, gamma, lmda, **variant):
    R, V, fv = np.asarray(R), np.asarray(V, f32), np.asarray(fv, f32)
    D = np.asarray(D).astype(bool)
    assert R.dtype in (np.dtype(f32), np.dtype(f64)) and R.shape == D.shape == V.shape
    T, B = R.shape
    returns, advantages = np.zeros((T, B), f32), np.zeros((T, B), f32)
    start = np.zeros((T, B), np.uint8)
    with np.errstate(over="ignore", invalid="ignore"):
        for b, t0, t1 in trajectories(D):
            ret, adv = one_trajectory(R[t0:t1 + 1, b], V[t0:t1 + 1, b], bool(D[t1, b]), fv[b], gamma, lmda, **variant)
            returns[t0:t1 + 1, b], advantages[t0:t1 + 1, b] = ret, adv
            start[t0, b] = 1
    return returns, advantages, start


_cases = None


def load_cases():
    """tests/golden/gae_cases.npz (make_golden_gae.py) as a list of dicts: T, B, gamma, lmda, R, D, V [T+1,B] and the
    reference's returns / advantages / values / action_prob [T,B].  Loaded once; nobody writes into it."""
    global _cases
    if _cases is None:
        import os
        out = []
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gae_cases.npz")) as d:
            z = {k: d[k] for k in d.files}
        for i in range(len(z["T"])):
            T, B = int(z["T"][i]), int(z["B"][i])
            o, vo, ro = int(z["offsets"][i]), int(z["v_offsets"][i]), int(z["r_offsets"][i])
            c = dict(index=i, T=T, B=B, gamma=float(z["gamma"][i]), lmda=float(z["lmda"][i]),
                     R=z["R64" if z["reward_f64"][i] else "R32"][ro:ro + T * B].reshape(T, B),
                     V=z["V"][vo:vo + (T + 1) * B].reshape(T + 1, B), n_actions=int(z["n_actions"].ravel()[0]))
            for name in ("D", "returns", "advantages", "values", "action_prob"):
                c[name] = z[name][o:o + T * B].reshape(T, B)
            for a in c.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            c["id"] = "T%d-B%d-%s-g%g-l%g" % (T, B, c["R"].dtype.name, c["gamma"], c["lmda"])
            out.append(c)
        _cases = out
    return _cases


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


WRONG_VARIANTS = ("all_float32", "length1_narrow", "bootstrap_closed", "wide_bootstrap_product")
