"""DQN replay on the device: slhip_replay_add against what the reference's DQN left in its replay buffer
(tests/golden/replay_cases.npz), the sampler and the epsilon-greedy draw against their exact host models
(tests/replay_ref.py), the gather against numpy indexing of the ring, and DQNRunner.collect end to end against the numpy
restatement fed the same step stream.  Everything is compared for equality."""
import collections
import ctypes as C

import numpy as np
import pytest

from safelife_amd import _hip
from tests import replay_ref as rr
from tests import util

pytestmark = pytest.mark.gpu

CASES = rr.load_cases()
ROW_BYTES = (16, 48, 6250, 6256)        # 16-byte lanes, 16-byte lanes with a tail wave, 2-byte lanes, 16-byte lanes
Step = collections.namedtuple("Step", "obs actions rewards done next_obs")


def _device_counts(boards, goals):
    from safelife_amd.levels import _device_counts as f
    return f(boards, goals)


def rows_of(b, t, nbytes):
    """The observation of env b at time t as a real row: uint8 [len(b), nbytes], every (b, t) a different row."""
    b, t = np.asarray(b, np.int64).reshape(-1, 1), np.asarray(t, np.int64).reshape(-1, 1)
    col = np.arange(nbytes, dtype=np.int64).reshape(1, -1)
    return ((b * 131 + t * 29 + col * 7 + (b * t + col // 251) % 13) % 251).astype(np.uint8)


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _buffer(case, nbytes):
    import torch
    from safelife_amd.replay import ReplayBuffer
    rdt = torch.float64 if case["R"].dtype == np.float64 else torch.float32
    return ReplayBuffer(case["capacity"], case["B"], multi_step=case["n"], gamma=case["gamma"], obs_shape=(nbytes,),
                        obs_dtype=torch.uint8, reward_dtype=rdt, device=_hip.device())


def _check_against_dump(buf, case, dump, steps, nbytes):
    n, B, cap = case["n"], case["B"], case["capacity"]
    size = len(dump["done"])
    assert int(buf.idx.item()) == dump["idx"] and len(buf) == size
    assert np.array_equal(buf.action.cpu().numpy()[:size], dump["action"])
    assert np.array_equal(bits64(buf.reward.cpu().numpy()[:size]), bits64(dump["reward"]))
    assert np.array_equal(buf.done.cpu().numpy()[:size], dump["done"])
    obs, nxt = buf.obs.cpu().numpy(), buf.next_obs.cpu().numpy()
    assert np.array_equal(obs[:size], rows_of(dump["obs_b"], dump["obs_t"], nbytes))
    assert np.array_equal(nxt[:size], rows_of(dump["next_b"], dump["next_t"], nbytes))
    assert not obs[size:].any() and not nxt[size:].any()           # slots never pushed stay as they were
    fill = buf.fill.cpu().numpy()
    assert np.array_equal(fill, dump["fill"])
    assert int(buf.head.item()) == steps % n
    # the device window is a ring over t mod n: the step k steps back sits in slot (steps - 1 - k) mod n
    wr, wa, wo = buf.win_reward.cpu().numpy(), buf.win_action.cpu().numpy(), buf.win_obs.cpu().numpy()
    for k in range(n):
        slot, live = (steps - 1 - k) % n, fill > k
        assert np.array_equal(bits64(wr[slot][live]), bits64(dump["w_reward"][k][live]))
        assert np.array_equal(wa[slot][live], dump["w_action"][k][live])
        assert np.array_equal(wo[slot][live], rows_of(np.arange(B)[live], dump["w_obs_t"][k][live], nbytes))
    assert int(buf.status.item()) == 0
    assert buf.min_len() <= size


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_add_equals_the_reference(case):
    """Ring, idx, fill and the windows equal the reference's at the three dumps, with real rows built from the tags: a
    small row size and a large one per case, all four sizes over the cases of every n."""
    import torch
    dev = _hip.device()
    B, T, i = case["B"], case["T"], case["index"]
    for nbytes in (ROW_BYTES[i % 2], ROW_BYTES[2 + (i // 2) % 2]):
        buf = _buffer(case, nbytes)
        envs = np.arange(B)
        for t in range(T):
            step = Step(torch.from_numpy(rows_of(envs, t, nbytes)).to(dev), torch.from_numpy(case["A"][t].copy()).to(dev),
                        torch.from_numpy(case["R"][t].copy()).to(dev), torch.from_numpy(case["D"][t].copy()).to(dev),
                        torch.from_numpy(rows_of(envs, t + 1, nbytes)).to(dev))
            buf.add(step)
            for j, s in enumerate(case["dump_steps"]):
                if s == t + 1:
                    _check_against_dump(buf, case, case["dumps"][j], t + 1, nbytes)
        assert buf.steps_added == T


def test_add_through_other_layouts_and_dtypes():
    """Padded and non-contiguous observations and rewards, bool done, int64 actions, host arrays: the same ring."""
    import torch
    dev = _hip.device()
    case = next(c for c in CASES if c["n"] == 5 and c["T"] == 17 and c["B"] == 65)
    B, T, nbytes = case["B"], case["T"], 48
    envs = np.arange(B)
    buf = _buffer(case, nbytes)
    for t in range(T):
        obs = torch.full((B, nbytes + 5), 255, dtype=torch.uint8, device=dev)
        obs[:, :nbytes] = torch.from_numpy(rows_of(envs, t, nbytes)).to(dev)
        nxt = torch.from_numpy(rows_of(envs, t + 1, nbytes)).to(dev).t().contiguous().t()       # column-major
        rewards = torch.zeros((B, 2), dtype=buf.reward_dtype, device=dev)
        rewards[:, 0] = torch.from_numpy(case["R"][t].copy()).to(dev)
        if t % 3 == 0:
            step = Step(obs[:, :nbytes], torch.from_numpy(case["A"][t].astype(np.int64)).to(dev), rewards[:, 0],
                        torch.from_numpy(case["D"][t] != 0).to(dev), nxt)
        elif t % 3 == 1:
            step = Step(obs[:, :nbytes].reshape(B, 4, 12), case["A"][t].astype(np.int64), rewards[:, 0],
                        case["D"][t].copy(), nxt.reshape(B, 4, 12))
        else:
            step = Step(obs[:, :nbytes].cpu(), torch.from_numpy(case["A"][t].astype(np.int64)), rewards[:, 0].cpu(),
                        torch.from_numpy(case["D"][t] != 0), nxt.cpu())
        buf.add(step)
    _check_against_dump(buf, case, case["dumps"][2], T, nbytes)
    with pytest.raises(ValueError):
        other = torch.float32 if buf.reward_dtype == torch.float64 else torch.float64
        buf.add(Step(step.obs, step.actions, torch.zeros(B, dtype=other, device=dev), step.done, step.next_obs))


def test_add_across_the_plan_kernels_chunk_boundary():
    """B = 1030 envs: the plan kernel scans them in chunks of 1024 and carries the pushes of the first chunk into the
    slots of the second.  n = 2, four steps, 16-byte rows, done flags on both sides of the boundary at every step; ring,
    idx and fill against the numpy restatement."""
    import torch
    from safelife_amd.replay import ReplayBuffer
    dev = _hip.device()
    B, n, T, nbytes, gamma = 1030, 2, 4, 16, 0.97
    cap = 2 * B * (n + 1)                               # no wrap: 4 steps push at most 4 * B rows
    envs = np.arange(B)
    rng = np.random.default_rng(1030)
    buf = ReplayBuffer(cap, B, multi_step=n, gamma=gamma, obs_shape=(nbytes,), obs_dtype=torch.uint8,
                       reward_dtype=torch.float32, device=dev)
    rep = rr.Replay(cap, B, n, gamma)
    for t in range(T):
        done = ((envs * 7 + t * 3) % 5 == 0).astype(np.uint8)
        assert done[:1024].any() and done[1024:].any() and not done[1024:].all()
        actions = rng.integers(0, 9, B).astype(np.int32)
        rewards = rng.normal(0, 3, B).astype(np.float32)
        obs, nxt = rows_of(envs, t, nbytes), rows_of(envs, t + 1, nbytes)
        before = rep.idx
        rep.add([r.tobytes() for r in obs], actions, rewards, done, [r.tobytes() for r in nxt])
        buf.add(Step(*(torch.from_numpy(x).to(dev) for x in (obs, actions, rewards, done, nxt))))
        assert int(buf.idx.item()) == rep.idx > before, t
    size = rep.idx
    assert size < cap and len(buf) == size
    assert np.array_equal(buf.fill.cpu().numpy(), rep.fill())
    obs, nxt = buf.obs.cpu().numpy(), buf.next_obs.cpu().numpy()
    act, rew, done = buf.action.cpu().numpy(), buf.reward.cpu().numpy(), buf.done.cpu().numpy()
    for s in range(size):
        o, a, r, no, d = rep.ring[s]
        assert obs[s].tobytes() == o and nxt[s].tobytes() == no and act[s] == a and done[s] == d, s
        assert bits64(rew[s]) == bits64(r), s
    assert not obs[size:].any() and not nxt[size:].any()
    assert int(buf.status.item()) == 0


# ---------------------------------------------------------------------------------------------------------- the sampler

def _sized_buffer(N, capacity=None):
    """A buffer that holds N rows: idx is set by hand (the sampler reads nothing else)."""
    import torch
    from safelife_amd.replay import ReplayBuffer
    buf = ReplayBuffer(max(capacity or N, 2), 1, multi_step=1, obs_shape=(16,), obs_dtype=torch.uint8, device=_hip.device())
    buf.idx.fill_(N)
    return buf


SEED_EDGES = ((0, 0), (5, 17), (2 ** 64 - 1, 2 ** 64 - 1), (2 ** 63, 2 ** 32), (1, 2 ** 64 - 1))


@pytest.mark.parametrize("N", [1, 95, 96, 97, 4096])
def test_sample_equals_the_model(N):
    buf = _sized_buffer(N)
    for k in sorted({k for k in (1, 64, 65, 96, N) if k <= N}):
        for seed, counter in SEED_EDGES if k != 4096 else SEED_EDGES[:2]:
            buf.seed, buf.draws = seed, counter
            got = buf.sample_indices(k).cpu().numpy()
            assert buf.draws == counter + 1
            assert np.array_equal(got, rr.sample_model(N, k, seed, counter)), (k, seed, counter)
    assert int(buf.status.item()) == 0


def test_sample_of_a_wrapped_ring_and_a_short_one():
    """N is min(idx, capacity); k > N raises the status bit and writes nothing."""
    import torch
    buf = _sized_buffer(1000, capacity=200)
    assert len(buf) == 200
    buf.seed, buf.draws = 9, 4
    assert np.array_equal(buf.sample_indices(96).cpu().numpy(), rr.sample_model(200, 96, 9, 4))
    buf = _sized_buffer(95, capacity=200)
    out = torch.full((96,), -7, dtype=torch.int64, device=buf.device)
    _hip.check(_hip.lib().slhip_replay_sample(C.byref(buf.struct), 96, 1, 2, _hip.ptr(out), _hip.current_stream_ptr()))
    assert int(buf.status.item()) == _hip.REPLAY_SHORT and (out.cpu().numpy() == -7).all()
    with pytest.raises(ValueError):
        buf.check_status()
    buf.status.zero_()
    _hip.check(_hip.lib().slhip_replay_sample(C.byref(buf.struct), 95, 1, 2, _hip.ptr(out), _hip.current_stream_ptr()))
    assert int(buf.status.item()) == 0
    assert np.array_equal(out.cpu().numpy()[:95], rr.sample_model(95, 95, 1, 2)) and int(out[95]) == -7
    with pytest.raises(ValueError):
        buf.sample_indices(201)


# ----------------------------------------------------------------------------------------------------------- the gather

@pytest.mark.parametrize("nbytes", ROW_BYTES)
def test_gather_equals_numpy_indexing(nbytes):
    import torch
    from safelife_amd.replay import ReplayBuffer
    dev, cap = _hip.device(), 300
    rng = np.random.default_rng(nbytes)
    buf = ReplayBuffer(cap, 3, multi_step=5, obs_shape=(nbytes,), obs_dtype=torch.uint8, device=dev)
    ring = dict(obs=rng.integers(0, 256, (cap, nbytes), dtype=np.uint8), next_obs=rng.integers(0, 256, (cap, nbytes), dtype=np.uint8),
                action=rng.integers(0, 9, cap).astype(np.int32), reward=rng.normal(0, 3, cap),
                done=(rng.random(cap) < 0.3).astype(np.uint8))
    ring["reward"][:4] = (1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, -(1.0 + 3 * 2.0 ** -24), 1e-50)   # ties and a tiny one
    for name, a in ring.items():
        getattr(buf, name).copy_(torch.from_numpy(a))
    index = np.concatenate([[0, cap - 1, 0, 1, 2, 3], rng.integers(0, cap, 91)]).astype(np.int64)
    for widen in (True, False):
        got = buf.gather(torch.from_numpy(index).to(dev), obs_float32=widen)
        assert got.obs.dtype == got.next_obs.dtype == (torch.float32 if widen else torch.uint8)
        assert got.action.dtype == torch.int64 and got.reward.dtype == got.done.dtype == torch.float32
        want_dtype = np.float32 if widen else np.uint8
        assert np.array_equal(got.obs.cpu().numpy(), ring["obs"][index].astype(want_dtype))
        assert np.array_equal(got.next_obs.cpu().numpy(), ring["next_obs"][index].astype(want_dtype))
        assert np.array_equal(got.action.cpu().numpy(), ring["action"][index].astype(np.int64))
        assert np.array_equal(got.reward.cpu().numpy().view(np.uint32), ring["reward"][index].astype(np.float32).view(np.uint32))
        assert np.array_equal(got.done.cpu().numpy(), ring["done"][index].astype(np.float32))
    assert int(buf.status.item()) == 0
    # an index outside the ring: its row is left alone, the status bit is raised
    bad = torch.tensor([5, cap, -1, 7], dtype=torch.int64, device=dev)
    got = buf.gather(bad, obs_float32=False)
    assert np.array_equal(got.obs.cpu().numpy()[[0, 3]], ring["obs"][[5, 7]]) and not got.obs.cpu().numpy()[[1, 2]].any()
    assert int(buf.status.item()) == _hip.REPLAY_BAD_INDEX


def test_gather_of_a_float_observation():
    """Rows of another dtype are opaque bytes: stored and returned as they are."""
    import torch
    from safelife_amd.replay import ReplayBuffer
    dev = _hip.device()
    buf = ReplayBuffer(20, 2, multi_step=1, obs_shape=(3, 5), obs_dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(3)
    steps = []
    for t in range(3):
        steps.append(Step(torch.randn((2, 3, 5), generator=g).to(dev), torch.tensor([t, 8 - t]), torch.randn(2, generator=g),
                          torch.tensor([t == 1, False]), torch.randn((2, 3, 5), generator=g).to(dev)))
        buf.add(steps[-1])
    # n = 1: step t pushes step t - 1 with step t's done flag; env 0 ends at t = 1 and flushes that step as well
    assert len(buf) == 4
    got = buf.gather(torch.tensor([0, 1, 2, 3], device=dev))
    assert got.obs.dtype == torch.float32
    assert torch.equal(got.obs, torch.stack([steps[0].obs[0], steps[1].obs[0], steps[0].obs[1], steps[1].obs[1]]))
    assert torch.equal(got.next_obs, torch.stack([steps[1].obs[0], steps[1].next_obs[0], steps[1].obs[1], steps[2].obs[1]]))
    assert got.action.tolist() == [0, 1, 8, 7] and got.done.tolist() == [1.0, 1.0, 0.0, 0.0]
    assert torch.equal(got.reward.cpu(), torch.stack([steps[0].rewards[0], steps[1].rewards[0], steps[0].rewards[1],
                                                      steps[1].rewards[1]]))


# ------------------------------------------------------------------------------------------------- the epsilon-greedy draw

def _q_rows(rng, B, A):
    q = rng.standard_normal((B, A)).astype(np.float32)
    if A > 1:
        q[0::7, :] = 0.0                                # all tied: the first
        q[1::7, A // 2] = q[1::7, A - 1] = 5.0          # two maxima
        q[2::7, A - 1] = np.nan                         # a NaN is the maximum
        q[3::7, A // 3] = q[3::7, A - 1] = np.nan       # the first NaN wins
        q[4::7, :] = -np.inf
        q[5::7, A // 2] = np.inf
    return q


@pytest.mark.parametrize("A", [1, 9, 64])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_eps_draw_equals_the_model(B, A):
    import torch
    dev, lib = _hip.device(), _hip.lib()
    q = _q_rows(np.random.default_rng(1000 * B + A), B, A)
    qd = torch.from_numpy(q).to(dev)

    def draw(rows, eps, seed, counter):
        out = torch.full((rows.shape[0] + 1,), -3, dtype=torch.int32, device=dev)
        _hip.check(lib.slhip_sample_actions_eps(_hip.ptr(rows), rows.shape[0], A, eps, seed % 2 ** 64, counter, _hip.ptr(out),
                                                _hip.current_stream_ptr()))
        out = out.cpu().numpy()
        assert out[-1] == -3
        return out[:-1]

    for eps in (0.0, 1.0, 0.03, 0.5):
        for seed, counter in SEED_EDGES:
            want, was_random = rr.eps_model(q, eps, seed, counter)
            assert np.array_equal(draw(qd, eps, seed, counter), want), (eps, seed, counter)
            assert was_random.all() if eps == 1.0 else (not was_random.any() if eps == 0.0 else True)
    if B > 1:       # the sub-batch rule: envs [lo, B) drawn on their own
        lo = B // 3
        whole = draw(qd, 0.5, 77, 3)
        assert np.array_equal(draw(qd[lo:].contiguous(), 0.5, 77 + rr.policy_ref.G * lo, 3), whole[lo:])


# ------------------------------------------------------------------------------------------------------------ end to end

class _QModel(object):
    """A small fixed network on the policy layout: obs [B,C,W,H] -> qvals [B,9]; remembers what it returned."""

    def __init__(self, torch, n_in, device):
        g = torch.Generator(device="cpu").manual_seed(7)
        self.torch, self.seen = torch, []
        self.w1 = (torch.randn((n_in, 16), generator=g) / n_in ** 0.5).to(device)
        self.w2 = torch.randn((16, 9), generator=g).to(device)

    def __call__(self, obs):
        torch = self.torch
        q = torch.tanh(obs.reshape(obs.shape[0], -1).to(torch.float32) @ self.w1) @ self.w2
        self.seen.append(q.cpu().numpy())
        return q


class _Recorder(object):
    """Hands every step on to the buffer and keeps a host copy."""

    def __init__(self, buf):
        self.buf, self.steps = buf, []

    def add(self, step):
        self.steps.append(Step(*(getattr(step, f).cpu().numpy().copy() for f in Step._fields)))
        self.buf.add(step)


def test_dqn_runner_end_to_end():
    """DQNRunner.collect on 65 envs with a time limit of 5 (episodes staggered by masked resets), n = 5, capacity 65 * 6:
    the ring, idx and fill equal the numpy restatement fed the recorded step stream, every action equals the draw's model
    on the Q-values the model returned, and a sample returns rows of the ring."""
    import torch
    from safelife_amd.replay import ReplayBuffer
    from safelife_amd.runner import DQNRunner
    from safelife_amd.vector_env import SafeLifeVectorEnv
    B, n, T, eps, seed = 65, 5, 24, 0.3, 12345
    pool, _ = util.pool_from_fixture("prune_still_25", _device_counts, n=8, min_performance_fraction=0.05)
    env = SafeLifeVectorEnv(pool, B, first_level=np.arange(B) % len(pool), auto_reset=True, time_limit=5,
                            view_shape=(9, 9), policy_layout="uint8", with_obs=False)
    model = _QModel(torch, int(np.prod(env.policy_tensor.shape[1:])), env.device)
    runner = DQNRunner(env, model, seed=seed)
    for k in range(3):          # stagger the episodes
        runner.take_one_step(1.0)
        env.reset((np.arange(B) % 4 == k).astype(np.uint8))
    model.seen.clear()
    draws0 = runner.draws
    buf = ReplayBuffer(B * (n + 1), B, multi_step=n, gamma=0.97, obs_shape=tuple(env.policy_tensor.shape[1:]),
                       obs_dtype=env.policy_tensor.dtype, reward_dtype=torch.float32, device=env.device, seed=3)
    rec = _Recorder(buf)
    last = runner.collect(T, eps, rec)
    assert runner.num_steps == T * B and buf.steps_added == T and len(rec.steps) == T
    assert last.rewards.dtype == torch.float32 and last.actions.dtype == torch.int32
    dones = np.stack([s.done for s in rec.steps])
    assert dones.any(axis=0).sum() > B // 2 and not dones.all()                 # episode ends were seen
    for t, s in enumerate(rec.steps):
        want, _ = rr.eps_model(model.seen[t], eps, seed, draws0 + t)
        assert np.array_equal(s.actions, want), t
        if t:
            assert np.array_equal(s.obs, rec.steps[t - 1].next_obs)
    rep = rr.Replay(B * (n + 1), B, n, 0.97)
    for s in rec.steps:
        flat, nxt = s.obs.reshape(B, -1), s.next_obs.reshape(B, -1)
        rep.add([r.tobytes() for r in flat], s.actions, s.rewards, s.done, [r.tobytes() for r in nxt])
    size = len(rep)
    assert int(buf.idx.item()) == rep.idx == T * B - rep.pending() and len(buf) == size == B * (n + 1)
    assert buf.min_len() <= size
    assert np.array_equal(buf.fill.cpu().numpy(), rep.fill())
    obs = buf.obs.cpu().numpy().reshape(size, -1)
    nxt = buf.next_obs.cpu().numpy().reshape(size, -1)
    act, rew, done = buf.action.cpu().numpy(), buf.reward.cpu().numpy(), buf.done.cpu().numpy()
    for s in range(size):
        o, a, r, no, d = rep.ring[s]
        assert obs[s].tobytes() == o and nxt[s].tobytes() == no and act[s] == a and done[s] == d, s
        assert bits64(rew[s]) == bits64(r), s
    batch = buf.sample(32)
    buf.check_status()
    assert batch.obs.dtype == torch.float32 and batch.obs.shape == (32,) + tuple(env.policy_tensor.shape[1:])
    rows = {(obs[s].tobytes(), int(act[s]), np.float32(rew[s]).tobytes(), nxt[s].tobytes(), float(done[s])) for s in range(size)}
    index = rr.sample_model(size, 32, 3, 0)
    for i in range(32):
        row = (batch.obs[i].cpu().numpy().astype(np.uint8).tobytes(), int(batch.action[i]),
               batch.reward[i].cpu().numpy().tobytes(), batch.next_obs[i].cpu().numpy().astype(np.uint8).tobytes(),
               float(batch.done[i]))
        assert row in rows, i
        assert row[0] == obs[index[i]].tobytes() and row[1] == int(act[index[i]])
