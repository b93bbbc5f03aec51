"""Multi-agent PPO training batches on the device: slhip_training_batch_multi against what the reference's
PPO.gen_training_batch computed over two consecutive windows (tests/golden/gae_multi_cases.npz) and against
slhip_training_batch where there is one agent; slhip_rollout_record_multi against a torch restatement; the compaction and
the gather against numpy; the masked draw against tests/policy_ref.py; and MultiAgentRunner.gen_training_batch end to end
against tests/gae_multi_ref.py fed with the step stream of a second env stepped by hand."""
import ctypes as C

import numpy as np
import pytest

from safelife_amd import _hip
from tests import gae_multi_ref, gae_ref, policy_ref, util

pytestmark = pytest.mark.gpu

CASES = gae_multi_ref.load_cases()
SINGLE = gae_ref.load_cases()
SENTINEL = 12345.0
bits = gae_multi_ref.bits
_restated = {}


def _restatement(case):
    if case["index"] not in _restated:
        _restated[case["index"]] = gae_multi_ref.two_windows(case)
    return _restated[case["index"]]


def _device_counts(boards, goals):
    from safelife_amd.levels import _device_counts as f
    return f(boards, goals)


def _padded(torch, a, stride, dev, fill):
    """[T,N] numpy -> a device tensor [T,stride] whose first N columns hold it; the padding holds `fill`."""
    src = torch.from_numpy(np.array(a))
    t = torch.full((a.shape[0], stride), fill, dtype=src.dtype, device=dev)
    t[:, :a.shape[1]] = src.to(dev)
    return t


def _struct(T, N, A, f64, row_stride, out_stride, **tensors):
    m = _hip.RolloutMulti()
    m.w.T, m.w.B, m.w.row_stride, m.w.out_stride = T, N, row_stride, out_stride
    m.w.reward_dtype = _hip.REWARD_F64 if f64 else _hip.REWARD_F32
    m.n_agents = A
    for name, t in tensors.items():
        setattr(m if name == "active" else m.w, name, t.data_ptr())
    return m


def _training_batch_multi(R, D, V, active, fv, A, gamma, lmda, row_stride, out_stride, with_start):
    """R, D, V, active: numpy [T,N]; -> returns, advantages, traj_start [T,N] with SENTINEL / 77 where nothing was written
    (the padding is checked here)."""
    import torch
    dev, lib = _hip.device(), _hip.lib()
    T, N = R.shape
    Rd, Vd = _padded(torch, R, row_stride, dev, SENTINEL), _padded(torch, V, row_stride, dev, SENTINEL)
    Dd, Ad = _padded(torch, D, row_stride, dev, 1), _padded(torch, active, row_stride, dev, 1)
    fvd = torch.from_numpy(np.array(fv, np.float32).reshape(N)).to(dev)
    ret = torch.full((T, out_stride), SENTINEL, dtype=torch.float32, device=dev)
    adv = torch.full((T, out_stride), SENTINEL, dtype=torch.float32, device=dev)
    start = torch.full((T, out_stride), 77, dtype=torch.uint8, device=dev) if with_start else None
    m = _struct(T, N, A, R.dtype == np.float64, row_stride, out_stride, rewards=Rd, values=Vd, done=Dd, active=Ad)
    _hip.check(lib.slhip_training_batch_multi(C.byref(m), _hip.ptr(fvd), gamma, lmda, _hip.ptr(ret), _hip.ptr(adv),
                                              _hip.ptr(start), _hip.current_stream_ptr()))
    torch.cuda.synchronize()
    ret, adv = ret.cpu().numpy(), adv.cpu().numpy()
    assert np.all(ret[:, N:] == np.float32(SENTINEL)) and np.all(adv[:, N:] == np.float32(SENTINEL))
    if with_start:
        start = start.cpu().numpy()
        assert np.all(start[:, N:] == 77)
        start = start[:, :N]
    return ret[:, :N], adv[:, :N], start


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_training_batch_multi_equals_the_reference(case):
    """Both windows, bit for bit at the rows the reference's batch has; sentinels intact at the inactive rows and in the
    padding; dense and with padded rows, traj_start requested and null.  The inactive rows of the inputs hold what the
    record kernel leaves there (zeros) in the even cases, and a sentinel with the env's own done flag in the odd ones:
    nothing may depend on them."""
    T, B, A = case["T"], case["B"], case["A"]
    N = B * A
    for w, ref in enumerate(_restatement(case)):
        valid = case["valid"][w].reshape(T, N)
        on = valid != 0
        assert np.array_equal(ref.active.reshape(T, N), valid)
        R, V = case["R"][w].reshape(T, N).copy(), case["values"][w].reshape(T, N).copy()
        D = (case["D"][w].reshape(T, N) & valid).astype(np.uint8)
        if case["index"] % 2:
            R[~on], V[~on] = SENTINEL, SENTINEL
            D = case["D"][w].reshape(T, N).copy()
        want_ret, want_adv = case["returns"][w].reshape(T, N), case["advantages"][w].reshape(T, N)
        want_start = ref.traj_start.reshape(T, N)
        for row_stride, out_stride, with_start in ((N, N, True), (N, N, False), (N + 5, N + 3, True), (N + 64, N, False)):
            ret, adv, start = _training_batch_multi(R, D, V, valid, case["V_boot"][w], A, case["gamma"], case["lmda"],
                                                    row_stride, out_stride, with_start)
            where = (w, row_stride, out_stride, with_start)
            assert np.array_equal(bits(ret)[on], bits(want_ret)[on]), where
            assert np.array_equal(bits(adv)[on], bits(want_adv)[on]), where
            assert np.all(ret[~on] == np.float32(SENTINEL)) and np.all(adv[~on] == np.float32(SENTINEL)), where
            if with_start:
                assert np.array_equal(start[on], want_start[on]) and np.all(start[~on] == 77), where


@pytest.mark.parametrize("case", SINGLE, ids=[c["id"] for c in SINGLE])
def test_one_agent_all_active_equals_the_single_agent_kernel(case):
    """A = 1 and every row active on the single-agent fixture: the output of slhip_training_batch, bit for bit."""
    import torch
    dev, lib = _hip.device(), _hip.lib()
    T, B = case["T"], case["B"]
    ones = np.ones((T, B), np.uint8)
    ret, adv, start = _training_batch_multi(case["R"], case["D"], case["V"][:T], ones, case["V"][T], 1, case["gamma"],
                                            case["lmda"], B + 5, B + 3, True)
    R, V = _padded(torch, case["R"], B + 5, dev, SENTINEL), _padded(torch, case["V"][:T], B + 5, dev, SENTINEL)
    D = _padded(torch, case["D"], B + 5, dev, 1)
    fv = torch.from_numpy(np.array(case["V"][T])).to(dev)
    out = [torch.zeros((T, B + 3), dtype=dt, device=dev) for dt in (torch.float32, torch.float32, torch.uint8)]
    s = _hip.Rollout()
    s.T, s.B, s.row_stride, s.out_stride = T, B, B + 5, B + 3
    s.reward_dtype = _hip.REWARD_F64 if case["R"].dtype == np.float64 else _hip.REWARD_F32
    s.rewards, s.values, s.done = R.data_ptr(), V.data_ptr(), D.data_ptr()
    _hip.check(lib.slhip_training_batch(C.byref(s), _hip.ptr(fv), case["gamma"], case["lmda"], _hip.ptr(out[0]),
                                        _hip.ptr(out[1]), _hip.ptr(out[2]), _hip.current_stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(bits(ret), bits(out[0].cpu().numpy()[:, :B]))
    assert np.array_equal(bits(adv), bits(out[1].cpu().numpy()[:, :B]))
    assert np.array_equal(start, out[2].cpu().numpy()[:, :B])
    assert np.array_equal(bits(ret), bits(case["returns"])) and np.array_equal(bits(adv), bits(case["advantages"]))


@pytest.mark.parametrize("f64", [False, True], ids=["float32", "float64"])
@pytest.mark.parametrize("BA", [(1, 1), (21, 3), (8, 8), (13, 5), (257, 1)], ids=lambda x: "B%d-A%d" % x)
def test_rollout_record_multi_equals_torch(BA, f64):
    """Five steps into a padded window against torch: probs[row, action] gathered and the step copied where active_now is
    set, zeros elsewhere; active[t] = active_now; then active_now &= ~done, an env with nobody left gets everybody back
    and one more reset.  Inactive rows carry actions outside [0, n_actions) from the start (no status bit); the last
    step plants one on an active row (bit raised, probability 0, the action kept)."""
    import torch
    dev, lib = _hip.device(), _hip.lib()
    B, A = BA
    N, T, NA, stride = B * A, 5, 9, B * A + 7
    g = torch.Generator(device="cpu").manual_seed(1000 * N + f64)
    rdt = torch.float64 if f64 else torch.float32
    bufs = dict(actions=torch.full((T, stride), -5, dtype=torch.int32, device=dev),
                action_prob=torch.full((T, stride), SENTINEL, dtype=torch.float32, device=dev),
                rewards=torch.full((T, stride), SENTINEL, dtype=rdt, device=dev),
                values=torch.full((T, stride), SENTINEL, dtype=torch.float32, device=dev),
                done=torch.full((T, stride), 9, dtype=torch.uint8, device=dev),
                active=torch.full((T, stride), 9, dtype=torch.uint8, device=dev),
                status=torch.zeros(1, dtype=torch.int32, device=dev))
    m = _struct(T, N, A, f64, stride, stride, **bufs)
    want = {k: v.clone() for k, v in bufs.items()}
    now = (torch.rand((B, A), generator=g) < 0.7).to(torch.uint8)
    now[now.sum(dim=1) == 0] = 1                       # (the carried state never holds an env with nobody in it)
    now = now.to(dev)
    resets = torch.arange(B, dtype=torch.int64).to(dev) * 3
    for t in (1, 3, 0, 4, 2):
        plant = t == 2
        actions = torch.randint(0, NA, (N,), generator=g, dtype=torch.int32).to(dev)
        probs = torch.softmax(torch.randn((N, NA), generator=g), dim=1).to(dev)
        rewards = torch.randn(N, generator=g, dtype=rdt).to(dev)
        values = torch.randn(N, generator=g).to(dev)
        done = (torch.rand(N, generator=g) < 0.4).to(torch.uint8).to(dev)
        act = now.view(N).bool()
        actions[~act] = NA + 3                          # never looked at
        p = probs.gather(1, actions.clamp(0, NA - 1).to(torch.int64).view(N, 1)).view(N)
        if plant:
            where = int(torch.nonzero(act)[-1])
            actions[where] = NA if N % 2 else -1
            p[where] = 0.0
        zero = torch.zeros((), device=dev)
        want["actions"][t, :N] = torch.where(act, actions, torch.zeros_like(actions))
        want["action_prob"][t, :N] = torch.where(act, p, zero)
        want["rewards"][t, :N] = torch.where(act, rewards, torch.zeros_like(rewards))
        want["values"][t, :N] = torch.where(act, values, zero)
        want["done"][t, :N] = torch.where(act, done, torch.zeros_like(done))
        want["active"][t, :N] = now.view(N)
        want["status"][0] = _hip.ROLLOUT_BAD_ACTION if plant else 0
        left = (now.bool() & ~done.view(B, A).bool())
        over = ~left.any(dim=1)
        want_now = torch.where(over.view(B, 1), torch.ones_like(left), left).to(torch.uint8)
        want_resets = resets + over.to(torch.int64)
        _hip.check(lib.slhip_rollout_record_multi(C.byref(m), t, _hip.ptr(actions), _hip.ptr(probs), NA, _hip.ptr(rewards),
                                                  _hip.ptr(values), _hip.ptr(done), _hip.ptr(now), _hip.ptr(resets),
                                                  _hip.current_stream_ptr()))
        torch.cuda.synchronize()
        for name in bufs:
            assert torch.equal(bufs[name], want[name]), (t, name)
        assert torch.equal(now, want_now) and torch.equal(resets, want_resets), t


# ---------------------------------------------------------------------------------------------- compaction and gather

WINDOWS = [(1, 1, 1), (3, 7, 3), (2, 4, 8), (5, 13, 1), (3, 341, 1), (4, 32, 8), (5, 41, 5), (20, 257, 3)]
MASKS = ["ones", "zeros", "first", "last", 0.1, 0.5, 0.9]
OBS_BYTES = (16, 48, 4275)


def _mask(kind, total, rng):
    a = np.zeros(total, np.uint8)
    if kind == "ones":
        a[:] = 1
    elif kind == "first":
        a[0] = 1
    elif kind == "last":
        a[-1] = 1
    elif kind != "zeros":
        a = (rng.random(total) < kind).astype(np.uint8)
    return a


@pytest.mark.parametrize("kind", MASKS, ids=[str(k) for k in MASKS])
@pytest.mark.parametrize("shape", WINDOWS, ids=["x".join(map(str, s)) for s in WINDOWS])
def test_compact_and_gather_equal_numpy(shape, kind):
    """rows and N against np.flatnonzero(active) -- from a dense window and from one with padded rows -- with nothing
    written behind N; then the six gathered tensors against numpy fancy indexing, byte for byte (the observation rows of
    16, 48 or 4275 bytes: 16 bytes per lane, and the byte path an odd row size forces)."""
    import torch
    dev, lib = _hip.device(), _hip.lib()
    T, B, A = shape
    N = B * A
    total = T * N
    obs_bytes = OBS_BYTES[(WINDOWS.index(shape) + MASKS.index(kind)) % 3]
    rng = np.random.default_rng(total * 7 + MASKS.index(kind))
    active = _mask(kind, total, rng).reshape(T, N)
    want_rows = np.flatnonzero(active.ravel())
    n = len(want_rows)
    host = dict(actions=rng.integers(0, 9, (T, N)).astype(np.int32), action_prob=rng.random((T, N)).astype(np.float32),
                rewards=rng.normal(size=(T, N)).astype(np.float32), values=rng.normal(size=(T, N)).astype(np.float32),
                done=(rng.random((T, N)) < 0.3).astype(np.uint8), active=active)
    ret, adv = rng.normal(size=(T, N)).astype(np.float32), rng.normal(size=(T, N)).astype(np.float32)
    obs = rng.integers(0, 256, (total, obs_bytes), dtype=np.uint8)
    for row_stride, out_stride in ((N, N), (N + 5, N + 3)):
        tens = {k: _padded(torch, v, row_stride, dev, 1) for k, v in host.items()}
        tens["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
        m = _struct(T, N, A, False, row_stride, out_stride, **tens)
        chunks = lib.slhip_rollout_compact_chunks(C.byref(m))
        assert chunks == (total + _hip.ROLLOUT_SCAN_CHUNK - 1) // _hip.ROLLOUT_SCAN_CHUNK
        work = torch.full((chunks,), -1, dtype=torch.int32, device=dev)
        rows = torch.full((total,), -7, dtype=torch.int64, device=dev)
        count = torch.full((1,), -7, dtype=torch.int64, device=dev)
        _hip.check(lib.slhip_rollout_compact(C.byref(m), _hip.ptr(rows), _hip.ptr(count), _hip.ptr(work),
                                             _hip.current_stream_ptr()))
        torch.cuda.synchronize()
        assert int(count.item()) == n
        got_rows = rows.cpu().numpy()
        assert np.array_equal(got_rows[:n], want_rows) and np.all(got_rows[n:] == -7)
        retd, advd = _padded(torch, ret, out_stride, dev, SENTINEL), _padded(torch, adv, out_stride, dev, SENTINEL)
        obsd = torch.from_numpy(obs).to(dev)
        out = dict(obs=torch.full((max(n, 1), obs_bytes), 201, dtype=torch.uint8, device=dev),
                   actions=torch.full((max(n, 1),), -7, dtype=torch.int64, device=dev))
        for name in ("action_prob", "returns", "advantages", "values"):
            out[name] = torch.full((max(n, 1),), SENTINEL, dtype=torch.float32, device=dev)
        _hip.check(lib.slhip_rollout_gather(C.byref(m), _hip.ptr(rows), n, _hip.ptr(retd), _hip.ptr(advd), _hip.ptr(obsd),
                                            obs_bytes, _hip.ptr(out["obs"]), _hip.ptr(out["actions"]),
                                            _hip.ptr(out["action_prob"]), _hip.ptr(out["returns"]),
                                            _hip.ptr(out["advantages"]), _hip.ptr(out["values"]),
                                            _hip.current_stream_ptr()))
        torch.cuda.synchronize()
        assert int(tens["status"].item()) == 0
        got = {k: v.cpu().numpy() for k, v in out.items()}
        if n == 0:                                      # nothing written
            assert np.all(got["obs"] == 201) and np.all(got["actions"] == -7) and np.all(got["returns"] == np.float32(SENTINEL))
            continue
        assert np.array_equal(got["obs"], obs[want_rows])
        assert np.array_equal(got["actions"], host["actions"].ravel()[want_rows].astype(np.int64))
        assert np.array_equal(bits(got["action_prob"]), bits(host["action_prob"].ravel()[want_rows]))
        assert np.array_equal(bits(got["values"]), bits(host["values"].ravel()[want_rows]))
        assert np.array_equal(bits(got["returns"]), bits(ret.ravel()[want_rows]))
        assert np.array_equal(bits(got["advantages"]), bits(adv.ravel()[want_rows]))


@pytest.mark.parametrize("obs_bytes", OBS_BYTES)
def test_gather_skips_a_poisoned_index(obs_bytes):
    """Row ids outside [0, T * N): the status bit, and the output rows they would have filled keep what they held."""
    import torch
    dev, lib = _hip.device(), _hip.lib()
    T, N, A = 4, 66, 2
    total = T * N
    rng = np.random.default_rng(obs_bytes)
    host = dict(actions=rng.integers(0, 9, (T, N)).astype(np.int32), action_prob=rng.random((T, N)).astype(np.float32),
                rewards=rng.normal(size=(T, N)).astype(np.float32), values=rng.normal(size=(T, N)).astype(np.float32),
                done=np.zeros((T, N), np.uint8), active=np.ones((T, N), np.uint8))
    tens = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    tens["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
    m = _struct(T, N, A, False, N, N, **tens)
    ret = torch.from_numpy(rng.normal(size=(T, N)).astype(np.float32)).to(dev)
    obs = rng.integers(0, 256, (total, obs_bytes), dtype=np.uint8)
    obsd = torch.from_numpy(obs).to(dev)
    idx = rng.permutation(total)[:70].astype(np.int64)
    bad = {3: -1, 17: total, 40: 2 ** 40, 69: -2 ** 62}
    for k, v in bad.items():
        idx[k] = v
    rows = torch.from_numpy(idx).to(dev)
    n = len(idx)
    out_obs = torch.full((n, obs_bytes), 201, dtype=torch.uint8, device=dev)
    out_act = torch.full((n,), -7, dtype=torch.int64, device=dev)
    outs = [torch.full((n,), SENTINEL, dtype=torch.float32, device=dev) for _ in range(4)]
    _hip.check(lib.slhip_rollout_gather(C.byref(m), _hip.ptr(rows), n, _hip.ptr(ret), _hip.ptr(ret), _hip.ptr(obsd), obs_bytes,
                                        _hip.ptr(out_obs), _hip.ptr(out_act), *[_hip.ptr(o) for o in outs],
                                        _hip.current_stream_ptr()))
    torch.cuda.synchronize()
    assert int(tens["status"].item()) == _hip.ROLLOUT_BAD_INDEX
    good = np.array([k not in bad for k in range(n)])
    got_obs, got_act, got_val = out_obs.cpu().numpy(), out_act.cpu().numpy(), outs[3].cpu().numpy()
    assert np.array_equal(got_obs[good], obs[idx[good]]) and np.all(got_obs[~good] == 201)
    assert np.array_equal(got_act[good], host["actions"].ravel()[idx[good]]) and np.all(got_act[~good] == -7)
    assert np.array_equal(bits(got_val[good]), bits(host["values"].ravel()[idx[good]]))
    for o in outs:
        assert np.all(o.cpu().numpy()[~good] == np.float32(SENTINEL))


# -------------------------------------------------------------------------------------------------------- masked draw

@pytest.mark.parametrize("shape", [(21, 3, 5), (32, 2, 1), (13, 5, 7), (85, 3, 2), (128, 2, 3), (257, 1, 9)],
                         ids=lambda s: "B%d-A%d-offset%d" % s)
def test_masked_draw(shape):
    """Active rows: the model of tests/policy_ref.py for row (env_offset + e) * A + a, and what slhip_sample_actions itself
    draws; inactive rows: 0, also where the probabilities are NaN, inf or all zero."""
    import torch
    dev, lib = _hip.device(), _hip.lib()
    B, A, offset = shape
    N, NA, seed = B * A, 9, 0x1234567 + B
    rng = np.random.default_rng(N)
    p = rng.random((N, NA)).astype(np.float32) ** 3
    p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
    active = (rng.random(N) < 0.6).astype(np.uint8)
    active[:3] = (1, 0, 1)
    off = np.flatnonzero(active == 0)
    for k, row in enumerate(off):
        if k % 4 == 0:
            p[row] = np.nan
        elif k % 4 == 1:
            p[row] = np.inf
        elif k % 4 == 2:
            p[row] = 0.0
    probs, act = torch.from_numpy(p).to(dev), torch.from_numpy(active).to(dev)
    kernel_seed = (seed + policy_ref.G * offset * A) & policy_ref.MASK
    for counter in (0, 1, 77):
        out = torch.full((N,), -9, dtype=torch.int32, device=dev)
        plain = torch.full((N,), -9, dtype=torch.int32, device=dev)
        _hip.check(lib.slhip_sample_actions_masked(_hip.ptr(probs), _hip.ptr(act), N, NA, kernel_seed, counter,
                                                   _hip.ptr(out), _hip.current_stream_ptr()))
        _hip.check(lib.slhip_sample_actions(_hip.ptr(probs), N, NA, kernel_seed, counter, _hip.ptr(plain),
                                            _hip.current_stream_ptr()))
        torch.cuda.synchronize()
        got, plain = out.cpu().numpy(), plain.cpu().numpy()
        on = active != 0
        with np.errstate(invalid="ignore"):
            want = policy_ref.sample_model(p, seed, counter, first_env=offset * A)
        assert np.array_equal(got[on], want[on]) and np.array_equal(got[on], plain[on]), counter
        assert not got[~on].any(), counter
    # a null mask is the plain draw
    _hip.check(lib.slhip_sample_actions_masked(_hip.ptr(probs), None, N, NA, kernel_seed, 5, _hip.ptr(out),
                                               _hip.current_stream_ptr()))
    plain = torch.full((N,), -9, dtype=torch.int32, device=dev)
    _hip.check(lib.slhip_sample_actions(_hip.ptr(probs), N, NA, kernel_seed, 5, _hip.ptr(plain), _hip.current_stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(out, plain)


# --------------------------------------------------------------------------------------------------------- end to end

class ExactPolicy(object):
    """A small fixed policy whose arithmetic is exact in float32 and in integers -- integer weights on a 0 / 1 observation,
    sums far below 2^24, probabilities that are multiples of 1/32 -- so that it computes the same on any device and in any
    summation order: obs [n,C,W,H] -> (values [n], probabilities [n,9]).  An agent that sees an exit (channel 8 without
    the agent bit, channel 1; the env paints far exits on the view's rim) favours the move towards the nearest one with
    probability 3/4, so that some agents leave their level while the others stay; everybody else favours an action hashed
    from the observation."""

    def __init__(self, torch, obs_shape, device, seed=7):
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.torch = torch
        C, W, H = obs_shape
        self.w = torch.randint(-3, 4, (2, C * W * H), generator=g).to(torch.float32).to(device)
        x = torch.arange(W, dtype=torch.int64).view(W, 1).expand(W, H) - W // 2
        y = torch.arange(H, dtype=torch.int64).view(1, H).expand(W, H) - H // 2
        flat = torch.arange(W * H, dtype=torch.int64).view(W, H)
        self.key = ((x.abs() + y.abs()) * 4096 + flat).to(device)       # nearest first, no ties
        self.dx, self.dy = x.reshape(-1).to(device), y.reshape(-1).to(device)

    def __call__(self, obs):
        torch = self.torch
        n = obs.shape[0]
        x = obs.reshape(n, -1).to(torch.float32)
        h0, h1 = (x * self.w[0]).sum(dim=1), (x * self.w[1]).sum(dim=1)
        hashed = torch.remainder(h0, 9.0).to(torch.int64)
        exits = (obs[:, 8] != 0) & (obs[:, 1] == 0)
        far = 1 << 40
        key = torch.where(exits, self.key, torch.full_like(self.key, far)).view(n, -1).min(dim=1).values
        seen = key < far
        cell = torch.where(seen, key % 4096, torch.zeros_like(key))
        dx, dy = self.dx[cell], self.dy[cell]
        sideways = (dy == 0) | ((dx != 0) & (hashed % 2 == 0))
        move = torch.where(sideways, torch.where(dx > 0, 2, 4), torch.where(dy > 0, 3, 1))
        k = torch.where(seen, move, hashed)
        probs = torch.full((n, 9), 1.0 / 32, dtype=torch.float32, device=obs.device)
        probs[torch.arange(n, device=obs.device), k] = 1.0 - 8.0 / 32
        return h1 * 0.125, probs


TRAIN = dict(movement_bonus=0.1, movement_bonus_power=1e-100, movement_bonus_period=4, as_penalty=True, exit_bonus=0.5,
             penalty_coef=0.3, ignore_reward_cells=False)
# (min_performance_fraction 0: the exits are open from the start, so an agent that walks to one leaves before the time limit)
E2E = dict(B=21, T=20, time_limit=9, view_shape=(7, 11), seed=3, min_performance_fraction=0.0)


def spec_levels():
    levels = []
    for name in ("multi_asym1", "multi_build_coop", "multi_build_compete"):
        levels += util.levels_from_trace(util.load_trace(name))
    return levels


def _env(pool, n_levels, wrapped):
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    B = E2E["B"]
    kw = dict(wrappers=TRAIN) if wrapped else {}
    return SafeLifeMultiAgentVectorEnv(pool, B, first_level=np.arange(B) % n_levels, auto_reset=True,
                                       time_limit=E2E["time_limit"], view_shape=E2E["view_shape"],
                                       output_channels=tuple(range(12)) + (25, 26, 27), policy_layout="uint8",
                                       with_obs=False, **kw)


@pytest.mark.parametrize("wrapped", [False, True], ids=["game reward", "wrapped reward"])
def test_gen_training_batch_multi_end_to_end(wrapped):
    """Two consecutive windows of MultiAgentRunner.gen_training_batch(20) against gae_multi_ref fed with the step stream
    of a second env stepped by hand with the recorded actions: the rows and their agent ids, obs / actions / action_prob /
    values exactly, returns and advantages bit for bit; the actions handed to the env are 0 exactly where nobody was
    active; the env's all-done steps are the runner's reset increments; the agent-step count is the number of rows."""
    import torch
    from safelife_amd.levels import LevelPool
    from safelife_amd.runner import MultiAgentRunner
    B, T, A = E2E["B"], E2E["T"], 2
    levels = spec_levels()
    pool = LevelPool(levels, counts_fn=_device_counts, n_agents=A, min_performance_fraction=E2E["min_performance_fraction"])
    a, b = _env(pool, len(levels), wrapped), _env(pool, len(levels), wrapped)
    policy = ExactPolicy(torch, tuple(a.policy_tensor.shape[2:]), a.device)
    runner = MultiAgentRunner(a, policy, seed=E2E["seed"])
    handed, env_step = [], a.step

    def logging_step(actions):
        handed.append(actions.clone())
        return env_step(actions)

    a.step = logging_step
    b.reset()
    active0, resets0 = None, None
    rows_seen, gaps, reloads = 0, 0, 0
    for window in range(2):
        del handed[:]
        batch = runner.gen_training_batch(T, gamma=0.97, lmda=0.95)
        buf = runner.rollout
        buf.check_status()
        acts = torch.stack(handed)                                              # [T, B, A] as the env got them
        obs, R, D, V, P = [], [], [], [], []
        for t in range(T):
            o = b.policy_tensor.clone()
            v, p = policy(o.view((B * A,) + tuple(o.shape[2:])))
            b.step(acts[t])
            obs.append(o), V.append(v.view(B, A)), P.append(p.view(B, A, -1))
            R.append((b.shaped_reward if wrapped else b.reward).clone()), D.append(b.done.clone())
        fv = policy(b.policy_tensor.view((B * A,) + tuple(b.policy_tensor.shape[2:])))[0].view(B, A)
        R, D, V = (torch.stack(x).cpu().numpy() for x in (R, D, V))
        assert R.dtype == np.float32 and buf.rewards.dtype == torch.float32
        ref = gae_multi_ref.window(R, D, V, fv.cpu().numpy(), 0.97, 0.95, active0, resets0)
        active0, resets0 = ref.active_end, ref.resets_end
        act = ref.active != 0
        # the bookkeeping
        assert np.array_equal(buf.active.cpu().numpy().reshape(T, B, A), ref.active)
        assert np.array_equal(acts.cpu().numpy() != 0, (acts.cpu().numpy() != 0) & act)     # 0 wherever nobody is active
        assert np.array_equal(runner.active.cpu().numpy() != 0, ref.active_end)
        assert np.array_equal(runner.num_resets.cpu().numpy(), ref.resets_end)
        resets = np.concatenate([buf.resets_at.cpu().numpy(), ref.resets_end[None]])
        assert np.array_equal(np.diff(resets, axis=0) != 0, D.astype(bool).all(axis=2))      # a reload per all-done step
        assert np.array_equal(buf.done.cpu().numpy().reshape(T, B, A), ref.handed_done)
        rows_seen += int(act.sum())
        assert int(runner.num_agent_steps.item()) == rows_seen
        assert runner.num_steps == (window + 1) * T * B
        # the batch
        rows = ref.rows
        assert np.array_equal(buf.rows.cpu().numpy(), rows) and len(batch.actions) == len(rows)
        assert np.array_equal(buf.agent_ids.cpu().numpy(), ref.agent_ids)
        assert np.array_equal(buf.traj_start.cpu().numpy().reshape(T, B, A)[act], ref.traj_start[act])
        rows_t = torch.from_numpy(rows).to(a.device)
        assert batch.actions.dtype == torch.int64 and torch.equal(batch.actions, acts.reshape(-1)[rows_t].to(torch.int64))
        prob = torch.stack(P).gather(3, acts.to(torch.int64).unsqueeze(3)).reshape(-1)
        assert torch.equal(batch.action_prob, prob[rows_t])
        assert torch.equal(batch.values, torch.from_numpy(V).to(a.device).reshape(-1)[rows_t])
        all_obs = torch.stack(obs)
        assert torch.equal(batch.obs, all_obs.reshape((T * B * A,) + tuple(all_obs.shape[3:]))[rows_t])
        assert np.array_equal(bits(batch.returns.cpu().numpy()), bits(ref.returns.reshape(-1)[rows]))
        assert np.array_equal(bits(batch.advantages.cpu().numpy()), bits(ref.advantages.reshape(-1)[rows]))
        # dense: the same numbers in place, no host visit
        dense = buf.finish(fv, 0.97, 0.95, dense=True)
        assert torch.equal(dense.valid.view(T, B, A), buf.active.view(T, B, A)) and dense.returns.shape == (T * B * A,)
        assert torch.equal(dense.returns[rows_t], batch.returns) and torch.equal(dense.advantages[rows_t], batch.advantages)
        gaps += int((~act).sum())               # (an env with nobody left reloads at once: a gap is an env going on)
        reloads += int(D.astype(bool).all(axis=2).sum())
    # the run held what it is here for: agents away while their env went on, and envs reloading inside a window
    assert gaps > 0 and reloads > 0


# ------------------------------------------------------------------------- the carried state, windows and single steps

def _pair():
    """Two identical envs (game reward) on the spec levels with two agents, and the exact policy for them."""
    import torch
    from safelife_amd.levels import LevelPool
    levels = spec_levels()
    pool = LevelPool(levels, counts_fn=_device_counts, n_agents=2, min_performance_fraction=E2E["min_performance_fraction"])
    a, b = _env(pool, len(levels), False), _env(pool, len(levels), False)
    return a, b, ExactPolicy(torch, tuple(a.policy_tensor.shape[2:]), a.device)


def _log_actions(env):
    """-> the list that collects a clone of every action tensor ``env.step`` is handed from now on."""
    handed, env_step = [], env.step

    def logging_step(actions):
        handed.append(actions.clone())
        return env_step(actions)

    env.step = logging_step
    return handed


def _by_hand(env, policy, acts):
    """Step ``env`` with the actions ``acts`` [T,B,A]: -> numpy R, D, V [T,B,A] and V(next_obs) [B,A] of the last step."""
    import torch
    B, A = acts.shape[1:]
    rows = lambda o: o.view((B * A,) + tuple(o.shape[2:]))
    R, D, V = [], [], []
    for t in range(acts.shape[0]):
        V.append(policy(rows(env.policy_tensor))[0].view(B, A))
        env.step(acts[t])
        R.append(env.reward.clone()), D.append(env.done.clone())
    fv = policy(rows(env.policy_tensor))[0].view(B, A)
    return tuple(torch.stack(x).cpu().numpy() for x in (R, D, V)) + (fv.cpu().numpy(),)


def test_windows_and_single_steps_interleaved():
    """gen_training_batch(6), three take_one_step(), gen_training_batch(4) -- another length, so another window buffer --
    against gae_multi_ref fed with the step stream of a second env stepped by hand with the recorded actions, the state
    carried across the single steps by the reference's rule (gae_multi_ref.bookkeeping): both windows' rows and agent
    ids, returns and advantages bit for bit, and active / num_resets / num_agent_steps / num_steps after every phase."""
    import torch
    from safelife_amd.runner import MultiAgentRunner
    B, A = E2E["B"], 2
    a, b, policy = _pair()
    runner = MultiAgentRunner(a, policy, seed=E2E["seed"])
    handed = _log_actions(a)
    b.reset()
    now = dict(active=np.ones((B, A), bool), resets=np.zeros(B, np.int64), agent_steps=0, env_steps=0, gaps=0)

    def state_is_carried(where):
        assert np.array_equal(runner.active.cpu().numpy() != 0, now["active"]), where
        assert np.array_equal(runner.num_resets.cpu().numpy(), now["resets"]), where
        assert int(runner.num_agent_steps.item()) == now["agent_steps"], where
        assert runner.num_steps == now["env_steps"] * B, where

    def window(T):
        del handed[:]
        batch = runner.gen_training_batch(T, gamma=0.97, lmda=0.95)
        buf = runner.rollout
        buf.check_status()
        R, D, V, fv = _by_hand(b, policy, torch.stack(handed))
        ref = gae_multi_ref.window(R, D, V, fv, 0.97, 0.95, now["active"], now["resets"])
        assert buf.steps == T and np.array_equal(buf.rows.cpu().numpy(), ref.rows), T
        assert np.array_equal(buf.agent_ids.cpu().numpy(), ref.agent_ids), T
        assert np.array_equal(bits(batch.returns.cpu().numpy()), bits(ref.returns.reshape(-1)[ref.rows])), T
        assert np.array_equal(bits(batch.advantages.cpu().numpy()), bits(ref.advantages.reshape(-1)[ref.rows])), T
        now.update(active=ref.active_end, resets=ref.resets_end, agent_steps=now["agent_steps"] + len(ref.rows),
                   env_steps=now["env_steps"] + T, gaps=now["gaps"] + int((ref.active == 0).sum()))
        state_is_carried("window of %d" % T)
        return buf

    first = window(6)
    reloads = 0
    for k in range(3):
        del handed[:]
        step = runner.take_one_step()
        R, D, V, fv = _by_hand(b, policy, torch.stack(handed))
        assert np.array_equal(step.active.cpu().numpy() != 0, now["active"]), k
        assert np.array_equal(step.agent_ids[1].cpu().numpy(), now["resets"]), k
        assert np.array_equal(step.done.cpu().numpy(), D[0].astype(bool)), k
        took_part, _, active, resets = gae_multi_ref.bookkeeping(D, now["active"], now["resets"])
        reloads += int((resets != now["resets"]).sum())
        now.update(active=active, resets=resets, agent_steps=now["agent_steps"] + int(took_part.sum()),
                   env_steps=now["env_steps"] + 1, gaps=now["gaps"] + int((~took_part).sum()))
        state_is_carried("single step %d" % k)
    assert window(4) is not first
    # the run held what it is here for: an agent away while its env went on, and an env reloading between the windows
    print("gaps %d, reloads during the single steps %d" % (now["gaps"], reloads))
    assert now["gaps"] > 0 and reloads > 0


def test_a_finished_window_stays_whole():
    """The dense batch of a window hands out the window buffer's own tensors: single steps taken afterwards leave them,
    and the window's ``active``, as they were."""
    import torch
    from safelife_amd.runner import MultiAgentRunner
    a, _, policy = _pair()
    runner = MultiAgentRunner(a, policy, seed=E2E["seed"])
    dense = runner.gen_training_batch(6, dense=True)
    live = dict(dense._asdict(), window_active=runner.rollout.active)
    kept = {name: x.clone() for name, x in live.items()}
    for _ in range(2):
        runner.take_one_step()
    torch.cuda.synchronize()
    for name in live:
        assert torch.equal(live[name], kept[name]), name


def test_the_dqn_runner_moves_the_same_state():
    """MultiAgentRunner under a policy that puts probability 1 on the argmax of the Q-model's values, and
    MultiAgentDQNRunner with epsilon 0, on two identical envs: the same ``active`` and ``num_resets`` and the same ``done``
    after every one of 12 steps (time limit 9: every env reloads on the way)."""
    import torch
    from safelife_amd.runner import MultiAgentDQNRunner, MultiAgentRunner
    a, b, exact = _pair()

    def q_model(obs):
        return exact(obs)[1]                    # (one entry of 3/4 among entries of 1/32: the argmax is unique)

    def policy(obs):
        q = q_model(obs)
        probs = torch.zeros_like(q)
        probs[torch.arange(q.shape[0], device=q.device), q.argmax(dim=1)] = 1.0
        return q[:, 0], probs

    ppo, dqn = MultiAgentRunner(a, policy, seed=5), MultiAgentDQNRunner(b, q_model, seed=11)
    away = 0
    for t in range(12):
        s, d = ppo.take_one_step(), dqn.take_one_step(0.0)
        assert torch.equal(s.active, d.active) and torch.equal(s.done, d.done) and torch.equal(a.done, b.done), t
        assert torch.equal(ppo.active, dqn.active) and torch.equal(ppo.num_resets, dqn.num_resets), t
        away += int((ppo.active == 0).sum().item())
    print("agents away %d, reloads %d" % (away, int(ppo.num_resets.sum().item())))
    assert away > 0 and int(ppo.num_resets.min().item()) >= 1
