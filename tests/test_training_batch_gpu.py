"""PPO training batches on the device: slhip_training_batch against what the reference's PPO.gen_training_batch computed
(tests/golden/gae_cases.npz) and the numpy restatement (tests/gae_ref.py), slhip_rollout_record against torch's own
gather / copies, and VectorRunner.gen_training_batch end to end against a second runner stepped by hand."""
import ctypes as C

import numpy as np
import pytest

from safelife_amd import _hip
from tests import gae_ref, util

pytestmark = pytest.mark.gpu

CASES = gae_ref.load_cases()
SENTINEL = 12345.0


def _device_counts(boards, goals):
    from safelife_amd.levels import _device_counts as f
    return f(boards, goals)


def _padded(torch, a, stride, dev, fill):
    """[T,B] numpy -> a device tensor [T,stride] whose first B columns hold it; the padding holds `fill`."""
    src = torch.from_numpy(np.array(a))
    t = torch.full((a.shape[0], stride), fill, dtype=src.dtype, device=dev)
    t[:, :a.shape[1]] = src.to(dev)
    return t


def _training_batch(case, row_stride, out_stride, with_start):
    import torch
    dev, lib = _hip.device(), _hip.lib()
    T, B = case["T"], case["B"]
    R = _padded(torch, case["R"], row_stride, dev, SENTINEL)
    V = _padded(torch, case["V"][:T], row_stride, dev, SENTINEL)
    D = _padded(torch, case["D"], row_stride, dev, 1)
    fv = torch.from_numpy(np.array(case["V"][T])).to(dev)
    ret = torch.full((T, out_stride), SENTINEL, dtype=torch.float32, device=dev)
    adv = torch.full((T, out_stride), SENTINEL, dtype=torch.float32, device=dev)
    start = torch.full((T, out_stride), 77, dtype=torch.uint8, device=dev) if with_start else None
    s = _hip.Rollout()
    s.T, s.B, s.row_stride, s.out_stride = T, B, row_stride, out_stride
    s.reward_dtype = _hip.REWARD_F64 if case["R"].dtype == np.float64 else _hip.REWARD_F32
    s.rewards, s.values, s.done = R.data_ptr(), V.data_ptr(), D.data_ptr()
    _hip.check(lib.slhip_training_batch(C.byref(s), _hip.ptr(fv), case["gamma"], case["lmda"], _hip.ptr(ret), _hip.ptr(adv),
                                        _hip.ptr(start), _hip.current_stream_ptr()))
    torch.cuda.synchronize()
    ret, adv = ret.cpu().numpy(), adv.cpu().numpy()
    assert np.all(ret[:, B:] == np.float32(SENTINEL)) and np.all(adv[:, B:] == np.float32(SENTINEL))
    if with_start:
        start = start.cpu().numpy()
        assert np.all(start[:, B:] == 77)
        start = start[:, :B]
    return ret[:, :B], adv[:, :B], start


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_training_batch_equals_the_reference(case):
    """Bit for bit, dense and with padded rows (inputs and outputs padded differently), traj_start requested and null."""
    T, B = case["T"], case["B"]
    ref_ret, ref_adv, ref_start = gae_ref.training_batch(case["R"], case["D"], case["V"][:T], case["V"][T], case["gamma"],
                                                         case["lmda"])
    assert np.array_equal(gae_ref.bits(ref_ret), gae_ref.bits(case["returns"]))
    assert np.array_equal(gae_ref.bits(ref_adv), gae_ref.bits(case["advantages"]))
    for row_stride, out_stride, with_start in ((B, B, True), (B, B, False), (B + 5, B + 3, True), (B + 64, B, False)):
        ret, adv, start = _training_batch(case, row_stride, out_stride, with_start)
        where = (row_stride, out_stride, with_start)
        assert np.array_equal(gae_ref.bits(ret), gae_ref.bits(case["returns"])), where
        assert np.array_equal(gae_ref.bits(adv), gae_ref.bits(case["advantages"])), where
        if with_start:
            assert np.array_equal(start, ref_start), where


@pytest.mark.parametrize("f64", [False, True], ids=["float32", "float64"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_rollout_record_equals_torch(B, f64):
    """Row t of the five arrays against torch's gather and copies; the other rows and the padding stay as they were.  Then
    one planted action outside [0, A): probability 0, the status word raised, the action kept, nothing else touched."""
    import torch
    dev, lib = _hip.device(), _hip.lib()
    T, A, stride = 3, 9, B + 7
    g = torch.Generator(device="cpu").manual_seed(100 * B + f64)
    rdt = torch.float64 if f64 else torch.float32
    bufs = dict(actions=torch.full((T, stride), -5, dtype=torch.int32, device=dev),
                action_prob=torch.full((T, stride), SENTINEL, dtype=torch.float32, device=dev),
                rewards=torch.full((T, stride), SENTINEL, dtype=rdt, device=dev),
                values=torch.full((T, stride), SENTINEL, dtype=torch.float32, device=dev),
                done=torch.full((T, stride), 9, dtype=torch.uint8, device=dev),
                status=torch.zeros(1, dtype=torch.int32, device=dev))
    s = _hip.Rollout()
    s.T, s.B, s.row_stride, s.out_stride = T, B, stride, stride
    s.reward_dtype = _hip.REWARD_F64 if f64 else _hip.REWARD_F32
    for name, t in bufs.items():
        setattr(s, name, t.data_ptr())
    want = {k: v.clone() for k, v in bufs.items()}
    for t, plant in ((1, False), (2, False), (0, True)):
        actions = torch.randint(0, A, (B,), generator=g, dtype=torch.int32).to(dev)
        probs = torch.softmax(torch.randn((B, A), generator=g), dim=1).to(dev)
        rewards = torch.randn(B, generator=g, dtype=rdt).to(dev)
        values = torch.randn(B, generator=g).to(dev)
        done = (torch.rand(B, generator=g) < 0.4).to(torch.uint8).to(dev)
        p = probs.gather(1, actions.to(torch.int64).view(B, 1)).view(B)
        if plant:
            where = B // 2
            actions[where] = A if B % 2 else -1
            p[where] = 0.0
        _hip.check(lib.slhip_rollout_record(C.byref(s), t, _hip.ptr(actions), _hip.ptr(probs), A, _hip.ptr(rewards),
                                            _hip.ptr(values), _hip.ptr(done), _hip.current_stream_ptr()))
        want["actions"][t, :B], want["action_prob"][t, :B], want["rewards"][t, :B] = actions, p, rewards
        want["values"][t, :B], want["done"][t, :B] = values, done
        want["status"][0] = _hip.ROLLOUT_BAD_ACTION if plant else 0
        torch.cuda.synchronize()
        for name in bufs:
            assert torch.equal(bufs[name], want[name]), (t, name)


class _Policy(object):
    """A small fixed network on the policy layout: obs [B,C,W,H] -> (values [B], probabilities [B,9])."""

    def __init__(self, torch, n_in, device):
        g = torch.Generator(device="cpu").manual_seed(7)
        self.torch = torch
        self.w1 = (torch.randn((n_in, 16), generator=g) / n_in ** 0.5).to(device)
        self.w2 = torch.randn((16, 10), generator=g).to(device)

    def __call__(self, obs):
        torch = self.torch
        h = torch.tanh(obs.reshape(obs.shape[0], -1).to(torch.float32) @ self.w1) @ self.w2
        return h[:, 0].contiguous(), torch.softmax(h[:, 1:], dim=1)


WRAPPERS = dict(movement_bonus=0.1, movement_bonus_power=1e-100, movement_bonus_period=4, as_penalty=True, exit_bonus=0.5,
                penalty_coef=0.3, ignore_reward_cells=False)


def _runner(wrappers):
    """64 envs of the 25x25 pool with a time limit of 5, their episodes staggered by masked resets during three warm-up
    steps, so that an 8-step window holds closed trajectories, open tails of one step and of several, and windows that
    end on a done step."""
    import torch
    from safelife_amd.runner import VectorRunner
    from safelife_amd.vector_env import SafeLifeVectorEnv
    B = 64
    pool, _ = util.pool_from_fixture("prune_still_25", _device_counts, n=8, min_performance_fraction=0.05)
    kw = dict(wrappers=wrappers) if wrappers else {}
    env = SafeLifeVectorEnv(pool, B, first_level=np.arange(B) % len(pool), auto_reset=True, time_limit=5,
                            view_shape=(9, 9), policy_layout="uint8", with_obs=False, **kw)
    policy = _Policy(torch, int(np.prod(env.policy_tensor.shape[1:])), env.device)
    runner = VectorRunner(env, policy, generator=torch.Generator(device=env.device).manual_seed(11))
    for k in range(3):
        runner.take_one_step()
        env.reset((np.arange(B) % 4 == k).astype(np.uint8))
    return runner


@pytest.mark.parametrize("wrapped", [False, True], ids=["float32 reward", "float64 wrapped reward"])
def test_gen_training_batch_end_to_end(wrapped):
    """gen_training_batch(8) on one runner against gae_ref applied to the StepResults of an identically built second
    runner stepped by hand; obs, actions, action_prob and values exactly, returns and advantages bit for bit."""
    import torch
    T, B = 8, 64
    a, b = _runner(WRAPPERS if wrapped else None), _runner(WRAPPERS if wrapped else None)
    steps_before = a.num_steps
    batch = a.gen_training_batch(T, gamma=0.97, lmda=0.95)
    a.rollout.check_status()
    assert a.num_steps == steps_before + T * B
    steps = [b.take_one_step() for _ in range(T)]
    with torch.no_grad():
        fv = b.policy(steps[-1].next_obs.to(torch.float32))[0]
    rdt = torch.float64 if wrapped else torch.float32
    assert all(s.rewards.dtype == rdt for s in steps) and a.rollout.rewards.dtype == rdt
    R = torch.stack([s.rewards for s in steps]).cpu().numpy()
    D = torch.stack([s.done for s in steps]).cpu().numpy()
    V = torch.stack([s.values for s in steps]).cpu().numpy()
    acts = torch.stack([s.actions for s in steps])
    prob = torch.stack([s.policies.gather(1, s.actions.view(B, 1)).view(B) for s in steps])
    # the window is what the docstring of _runner promises
    assert D.sum(axis=0).max() >= 2 and D[T - 1].any() and (D[T - 2] & ~D[T - 1]).any() and not D[T - 1].all()
    ret, adv, start = gae_ref.training_batch(R, D, V, fv.cpu().numpy(), 0.97, 0.95)
    assert batch.actions.dtype == torch.int64 and batch.actions.shape == (T * B,)
    assert torch.equal(batch.actions, acts.reshape(-1))
    assert torch.equal(batch.action_prob, prob.reshape(-1))
    assert torch.equal(batch.values, torch.stack([s.values for s in steps]).reshape(-1))
    assert torch.equal(batch.obs, torch.stack([s.obs for s in steps]).reshape((T * B,) + tuple(steps[0].obs.shape[1:])))
    assert np.array_equal(a.rollout.done.cpu().numpy() != 0, D)
    assert np.array_equal(gae_ref.bits(batch.returns.cpu().numpy()), gae_ref.bits(ret.reshape(-1)))
    assert np.array_equal(gae_ref.bits(batch.advantages.cpu().numpy()), gae_ref.bits(adv.reshape(-1)))
    assert np.array_equal(a.rollout.traj_start.cpu().numpy(), start)
