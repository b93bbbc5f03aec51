"""The DQN update on the device (safelife_amd/dqn.py, sl_dqn.hip) against the reference's own results
(tests/golden/dqn_update_cases.npz) and the host models of tests/dqn_loss_ref.py.

td and d loss / d q_values are elementwise IEEE operations: they equal the reference's FLOAT32 run bit for bit (a NaN equals a
NaN whatever its payload).  The loss and the four report scalars are compared with the reference's FLOAT64 run; the bound is
twice the largest deviation the reference's own float32 run shows from its float64 run over the fixture's cases of the same
row count, computed from the fixture when the module loads, never from the kernel's output.  What is not finite must be the
same.  Every test prints its figures before asserting.

Measured on an MI355X: see DESIGN.md section 6f."""
import collections
import os
import types

import numpy as np
import pytest

from safelife_amd import _hip
from tests import dqn_loss_ref as ref
from tests import util

pytestmark = pytest.mark.gpu

HAVE = os.path.exists(os.path.join(util.GOLDEN, "dqn_update_cases.npz"))
CASES = ref.load_cases() if HAVE else []
IDS = [c["id"] for c in CASES]


def _bounds():
    """BOUNDS[n][k] = twice the largest |float32 run - float64 run| of scalar k over the fixture's cases of n rows."""
    b = collections.defaultdict(lambda: np.zeros(len(ref.SCALARS)))
    for c in CASES:
        with np.errstate(invalid="ignore"):
            d = np.abs(c["scalars32"] - c["scalars64"])
        b[c["n"]] = np.maximum(b[c["n"]], 2.0 * np.where(np.isfinite(d), d, 0.0))
    return b


BOUNDS = _bounds()


def _device_counts(boards, goals):
    from safelife_amd.levels import _device_counts as f
    return f(boards, goals)


def device_source(c, torch, dev, **replace):
    """The case's action, reward and done on the device in the storage types of its source form."""
    from safelife_amd.replay import ReplayBatch
    action, reward, done = ref.source_arrays(c)
    x = {k: torch.from_numpy(np.ascontiguousarray(replace.get(k, v))).to(dev)
         for k, v in (("action", action), ("reward", reward), ("done", done))}
    if c["ring"]:
        return types.SimpleNamespace(capacity=len(action), **x)
    return ReplayBatch(None, x["action"], x["reward"], None, x["done"])


def run(c, source=None, index=None, q_values=None, next_q_values=None, grad_loss=None, grad_td=None, status=None,
        loss_grad=True):
    """dqn_loss forward and backward on the device -> numpy results (sums included)."""
    import torch
    from safelife_amd import dqn
    dev = _hip.device()
    source = device_source(c, torch, dev) if source is None else source
    q = torch.from_numpy(np.ascontiguousarray(c["q_values"] if q_values is None else q_values)).to(dev).requires_grad_()
    nq = torch.from_numpy(np.ascontiguousarray(c["next_q_values"] if next_q_values is None else next_q_values)).to(dev)
    idx = None if index is None else torch.from_numpy(np.asarray(index, np.int64)).to(dev)
    kw = dict(gamma=c["gamma"], multi_step=c["multi_step"])
    if status is not None:
        kw["status"] = status
    td, loss = dqn.dqn_loss(q, nq.requires_grad_(), source, idx, **kw)      # a target output that requires grad is detached
    sums = dqn.dqn_loss.sums
    assert td.shape == (q.shape[0],) and loss.shape == () and loss.dtype == td.dtype == torch.float32
    total = None
    if loss_grad:
        total = loss if grad_loss is None else loss * grad_loss
    if grad_td is not None:
        extra = (td * torch.from_numpy(grad_td).to(dev)).sum()
        total = extra if total is None else total + extra
    total.backward()
    assert nq.grad is None
    s = sums.cpu().numpy().copy()
    return dict(td=td.detach().cpu().numpy(), loss=loss.detach().cpu().numpy(), sums=s,
                loss_f32_slot=s.view(np.float32)[2 * _hip.DQN_SUM_LOSS_F32], dq=q.grad.cpu().numpy())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_and_backward_against_the_reference(case):
    from safelife_amd import dqn
    out = run(case)
    print(case["id"])
    assert out["td"].dtype == out["dq"].dtype == np.float32
    assert ref.same_values(out["td"], case["td32"])
    assert ref.same_values(out["dq"], ref.full_gradient(case, "32"))
    s, want, bound = out["sums"], case["scalars64"], BOUNDS[case["n"]]
    ok = []
    for k, name in enumerate(ref.SCALARS):
        if np.isfinite(want[k]):
            dev = abs(s[k] - want[k])
            print("  %-14s deviation %.3e   the reference's float32 run %.3e   bound %.3e" % (
                name, dev, abs(case["scalars32"][k] - want[k]), bound[k]))
            ok.append(bool(dev <= bound[k]))
        else:
            print("  %-14s %r, the reference %r" % (name, s[k], want[k]))
            ok.append(ref.same_values(s[k:k + 1], want[k:k + 1]))
    assert all(ok), [n for n, o in zip(ref.SCALARS, ok) if not o]
    assert s[5] == case["n"] and s[6] == 0.0
    assert ref.same_values(np.float32(s[0]), out["loss"]) and ref.same_values(out["loss"], out["loss_f32_slot"])
    assert s.view(np.float32)[2 * _hip.DQN_SUM_LOSS_F32 + 1] == 0.0
    dqn.check_status()


def test_ring_through_an_index_equals_the_batch_of_the_gathered_rows():
    """A scrambled subset and a subset with repeated rows of a ring of 300 rows: every result equals the batch form on the
    rows gathered on the host, bit for bit; what the ring holds at rows not named (actions out of range, NaN rewards, a done
    byte of 255) is never read."""
    import torch
    dev = _hip.device()
    c = next(c for c in CASES if c["id"].startswith("n257-a9") and c["ring"])
    rng = np.random.default_rng(5)
    N, A = 300, c["n_actions"]
    action = rng.integers(0, A, N).astype(np.int32)
    reward = rng.normal(0, 1, N)
    done = (rng.random(N) < 0.3).astype(np.uint8)
    for name, index in (("scrambled", rng.permutation(N)[:100]), ("repeats", rng.integers(0, 40, 257)),
                        ("all", None)):
        n = N if index is None else len(index)
        pick = np.arange(N) if index is None else index
        q = rng.normal(0, 2, (n, A)).astype(np.float32)
        nq = rng.normal(0, 2, (n, A)).astype(np.float32)
        batch = dict(c, n=n, ring=False, action=action[pick].astype(np.int64),
                     reward=reward[pick].astype(np.float32).astype(np.float64), done=done[pick])
        want = run(batch, q_values=q, next_q_values=nq)
        ring = dict(action=action.copy(), reward=reward.copy(), done=done.copy())
        if index is not None:
            unnamed = np.setdiff1d(np.arange(N), index)
            ring["action"][unnamed], ring["reward"][unnamed], ring["done"][unnamed] = 1 << 30, np.nan, 255
        status = torch.zeros(1, dtype=torch.int64, device=dev)
        source = types.SimpleNamespace(capacity=N, **{k: torch.from_numpy(v).to(dev) for k, v in ring.items()})
        got = run(dict(c, n=n), source=source, index=index, q_values=q, next_q_values=nq, status=status)
        for k in ("td", "loss", "sums", "dq"):
            assert ref.same_values(got[k], want[k]), (name, k)
        assert int(status.item()) == 0 and np.isfinite(got["sums"]).all()
    with pytest.raises(ValueError):         # without an index the Q-values must cover the source
        run(dict(c, n=10), source=source, q_values=q[:10], next_q_values=nq[:10])
    with pytest.raises(ValueError):         # a batch takes no index
        run(batch, index=np.arange(n), q_values=q, next_q_values=nq)


def test_bad_indices_and_actions_are_flagged_and_contribute_nothing():
    """The comparison run holds, where the bad run has a bad index or a bad action, rows that add exactly zero to the loss
    and to q_target_max (q[a] = reward, done, a target row of zeros): the sums and every other row's results must then be
    equal bit for bit -- q_model_mean, q_model_max and q_target_mean count the bad rows as they count any row."""
    import torch
    from safelife_amd import dqn
    dev = _hip.device()
    c = next(c for c in CASES if c["id"].startswith("n257-a9") and c["ring"])
    N, A = c["n"], c["n_actions"]
    rng = np.random.default_rng(6)
    index = rng.permutation(N)[:150].astype(np.int64)
    at_index, at_action = (3, 77), (64, 149)                 # positions in the minibatch
    special = at_index + at_action
    q, nq = c["q_values"][index].copy(), c["next_q_values"][index].copy()
    action, reward, done = (x.copy() for x in ref.source_arrays(c))
    for i in special:
        r = index[i]
        action[r], reward[r], done[r] = 2, 0.5, 1
        q[i, 2] = 0.5
        nq[i] = 0.0

    def source(action):
        return device_source(c, torch, dev, action=action, reward=reward, done=done)

    clean_status = torch.zeros(1, dtype=torch.int64, device=dev)
    clean = run(c, source=source(action), index=index, q_values=q, next_q_values=nq, status=clean_status)
    assert int(clean_status.item()) == 0 and not clean["td"][list(special)].any()
    for which, bit in (("index", _hip.DQN_BAD_INDEX), ("action", _hip.DQN_BAD_ACTION), ("both", 3)):
        bad_index, bad_action, hit = index.copy(), action.copy(), []
        if which in ("index", "both"):
            bad_index[at_index[0]], bad_index[at_index[1]] = -1, N
            hit += at_index
        if which in ("action", "both"):
            bad_action[index[at_action[0]]], bad_action[index[at_action[1]]] = -1, A
            hit += at_action
        status = torch.zeros(1, dtype=torch.int64, device=dev)
        got = run(c, source=source(bad_action), index=bad_index, q_values=q, next_q_values=nq, status=status)
        assert int(status.item()) == bit, which
        with pytest.raises(ValueError):
            dqn.check_status(status)
        assert ref.same_values(got["sums"], clean["sums"]) and ref.same_values(got["loss"], clean["loss"]), which
        assert not got["td"][hit].any() and not got["dq"][hit].any()
        others = np.setdiff1d(np.arange(len(index)), hit)
        for k in ("td", "dq"):
            assert ref.same_values(got[k][others], clean[k][others]), (which, k)
    # a bad row's maximum is left out of q_target_max, whatever it is; the three other scalars count the row
    nq_inf = nq.copy()
    nq_inf[at_index[0]] = np.inf
    bad_index = index.copy()
    bad_index[at_index[0]] = N + 5
    got = run(c, source=source(action), index=bad_index, q_values=q, next_q_values=nq_inf,
              status=torch.zeros(1, dtype=torch.int64, device=dev))
    assert got["sums"][4] == clean["sums"][4] and got["sums"][0] == clean["sums"][0] and np.isinf(got["sums"][3])
    dqn.check_status()                      # the shared word was never touched


def test_two_calls_are_equal_bit_for_bit():
    for c in CASES:
        if c["n"] in (4099, 257) and c["ring"]:
            a, b = run(c), run(c)
            for k in ("td", "loss", "sums", "dq"):
                assert ref.same_values(a[k], b[k]), (c["id"], k)


def test_grad_loss_scales_and_grad_td_adds():
    """The hand-written gradient of tests/dqn_loss_ref.py in float32, bit for bit: (grad_loss / n) * (2 * td) + grad_td."""
    for name in ("n257-a9", "n65-a32"):
        c = next(c for c in CASES if c["id"].startswith(name))
        w = np.linspace(-1.0, 1.0, c["n"]).astype(np.float32)
        assert ref.same_values(run(c, grad_loss=0.5)["dq"], ref.restate(c, np.float32, grad_loss=0.5)["dq"])
        assert ref.same_values(run(c, grad_td=w)["dq"], ref.restate(c, np.float32, grad_td=w)["dq"])
        both = run(c, grad_loss=3.0, grad_td=w)
        assert ref.same_values(both["dq"], ref.restate(c, np.float32, grad_loss=3.0, grad_td=w)["dq"])
        alone = run(c, grad_td=w, loss_grad=False)          # td alone: no loss gradient at all
        want = np.zeros_like(alone["dq"])
        want[np.arange(c["n"]), c["action"]] = w
        assert np.array_equal(alone["dq"], want)


# ------------------------------------------------------------------------------------------------------------- optimize

Step = collections.namedtuple("Step", "obs actions rewards done next_obs")


def _filled_buffer(torch, dev, obs_bytes, seed):
    from safelife_amd.replay import ReplayBuffer
    B, n, T = 16, 5, 40
    rng = np.random.default_rng(seed)
    buf = ReplayBuffer(512, B, multi_step=n, gamma=0.97, obs_shape=(obs_bytes,), obs_dtype=torch.uint8,
                       reward_dtype=torch.float32, device=dev, seed=21)
    obs = rng.integers(0, 4, (T + 1, B, obs_bytes)).astype(np.uint8)
    for t in range(T):
        rewards = rng.normal(0, 1, B).astype(np.float32)
        rewards[rng.random(B) < 0.3] = 0.0
        buf.add(Step(torch.from_numpy(obs[t]).to(dev), torch.from_numpy(rng.integers(0, 9, B).astype(np.int32)).to(dev),
                     torch.from_numpy(rewards).to(dev), torch.from_numpy((rng.random(B) < 0.15)).to(dev),
                     torch.from_numpy(obs[t + 1]).to(dev)))
    assert len(buf) == 512
    return buf


@pytest.mark.parametrize("obs_bytes", (16, 6250))
def test_optimize_equals_the_torch_loop_bit_for_bit(obs_bytes):
    """Three `optimize` calls with a linear Q model and Adam end with parameters bit-equal to the same loop around the
    reference's torch expression (training/dqn.py:149-161) fed `replay.gather(index)` for the same draws."""
    import torch
    from safelife_amd import dqn
    dev = _hip.device()
    buf = _filled_buffer(torch, dev, obs_bytes, 31)
    gamma, n = buf.gamma, buf.multi_step
    torch.manual_seed(4)
    start = torch.nn.Linear(obs_bytes, 9).state_dict()
    target_start = torch.nn.Linear(obs_bytes, 9).state_dict()

    def fresh():
        model, target = torch.nn.Linear(obs_bytes, 9), torch.nn.Linear(obs_bytes, 9)
        model.load_state_dict(start), target.load_state_dict(target_start)
        model, target = model.to(dev), target.to(dev)
        return model, target, torch.optim.Adam(model.parameters(), lr=3e-4)

    draws0 = buf.draws
    model, target, opt = fresh()
    for k in range(3):
        sums = dqn.optimize(model, target, opt, buf, 96, gamma=gamma, multi_step=n, report=(k == 2))
    assert buf.draws == draws0 + 3
    s = sums.cpu().numpy()
    assert s[5] == 96 and np.isfinite(s).all() and s[0] > 0

    buf.draws = draws0                      # the same draws again
    model2, target2, opt2 = fresh()
    for k in range(3):
        index = buf.sample_indices(96)
        b = buf.gather(index)
        q_values = model2(b.obs)
        next_q_values = target2(b.next_obs).detach()
        q_value = q_values.gather(1, b.action.unsqueeze(1)).squeeze(1)
        next_q_value, _ = next_q_values.max(1)
        discount = gamma ** n * (1 - b.done)
        expected = b.reward + discount * next_q_value
        loss = torch.mean((q_value - expected) ** 2)
        opt2.zero_grad()
        loss.backward()
        opt2.step()
    print("loss of the third update: fused %.9g, torch %.9g" % (s[0], float(loss.detach())))
    moved = 0.0
    for (k, a), b in zip(model.state_dict().items(), model2.state_dict().values()):
        moved = max(moved, float((a.cpu() - start[k]).abs().max()))
        assert ref.same_values(a.cpu().numpy(), b.cpu().numpy()), k
    assert moved > 1e-4                     # three Adam steps of 3e-4 moved them
    for (k, a) in target.state_dict().items():
        assert torch.equal(a.cpu(), target_start[k])
    buf.check_status()
    dqn.check_status()


def test_sync_target_equals_load_state_dict_on_the_device():
    import torch
    from safelife_amd import dqn
    dev = _hip.device()

    def make(seed):
        torch.manual_seed(seed)
        m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                                torch.nn.Linear(36, 9)).to(dev)
        m(torch.randn(5, 3, 5, 5, device=dev))
        return m

    training, target, twin = make(1), make(2), make(2)
    training(torch.randn(7, 3, 5, 5, device=dev))
    before = {k: v.data_ptr() for k, v in target.state_dict().items()}
    dqn.sync_target(training, target)
    twin.load_state_dict(training.state_dict())
    got, want = target.state_dict(), twin.state_dict()
    assert list(got) == list(want) and any("running_mean" in k for k in got) and any("num_batches_tracked" in k for k in got)
    for k in got:
        assert got[k].is_cuda and got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
        assert got[k].data_ptr() == before[k] and got[k].data_ptr() != training.state_dict()[k].data_ptr()
    with pytest.raises(ValueError):
        dqn.sync_target(training, torch.nn.Linear(4, 3).to(dev))


# ----------------------------------------------------------------------------------------------------------- DQNTrainer

def _single_agent_env():
    from safelife_amd.levels import LevelPool
    from safelife_amd.vector_env import SafeLifeVectorEnv
    levels = []
    for name in ("worked_7x7_exit", "worked_7x7_noop"):
        levels += util.levels_from_trace(util.load_trace(name))
    assert all(lv.board.shape == (7, 7) for lv in levels)
    pool = LevelPool(levels, counts_fn=_device_counts)
    return SafeLifeVectorEnv(pool, 5, first_level=np.arange(5) % len(levels), auto_reset=True, time_limit=6,
                             view_shape=(5, 5), output_channels=tuple(range(12)) + (25, 26, 27), policy_layout="uint8",
                             with_obs=False)


def _multi_agent_env():
    from safelife_amd.levels import LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    levels = []
    for name in ("multi_asym1", "multi_build_coop", "multi_build_compete"):
        levels += util.levels_from_trace(util.load_trace(name))
    pool = LevelPool(levels, counts_fn=_device_counts, n_agents=2, min_performance_fraction=0.0)
    return SafeLifeMultiAgentVectorEnv(pool, 5, first_level=np.arange(5) % len(levels), auto_reset=True, time_limit=9,
                                       view_shape=(9, 9), output_channels=tuple(range(12)) + (25, 26, 27),
                                       policy_layout="uint8", with_obs=False)


def _trainer_parts(torch, multi, seed=77):
    from safelife_amd.replay import MultiAgentReplayBuffer, ReplayBuffer
    from safelife_amd.runner import DQNRunner, MultiAgentDQNRunner
    env = _multi_agent_env() if multi else _single_agent_env()
    obs_shape = tuple(env.policy_tensor.shape[2 if multi else 1:])
    torch.manual_seed(8)
    make = lambda: torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(int(np.prod(obs_shape)), 9)).to(env.device)  # noqa: E731
    model, target = make(), make()
    kw = dict(multi_step=2, gamma=0.97, obs_shape=obs_shape, obs_dtype=env.policy_tensor.dtype, reward_dtype=torch.float32,
              device=env.device, seed=5)
    if multi:
        runner = MultiAgentDQNRunner(env, model, seed=seed)
        replay = MultiAgentReplayBuffer(5 * 2 * 3 * 8, 5, 2, **kw)
    else:
        runner = DQNRunner(env, model, seed=seed)
        replay = ReplayBuffer(5 * 3 * 8, 5, **kw)
    return env, runner, replay, model, target


SCHEDULE = dict(training_batch_size=16, optimize_interval=10, target_update_interval=35, report_interval=25,
                replay_initial=60)


@pytest.mark.parametrize("multi", (False, True), ids=("5 envs of 7x7", "5 envs x 2 agents"))
def test_trainer_end_to_end(multi):
    """DQNTrainer.train for 40 steps of every env under the default epsilon schedule -- epsilon is 1 until 5e4 steps, so
    every action is the uniform draw, a function of (seed, step, row) alone, whatever the model has learnt: the ring must
    equal that of a plain `collect` with the same seeds and epsilons on a twin env.  The twin also says how many rows every
    step pushed, which is what the host model of the schedule needs to predict the event list."""
    import torch
    from safelife_amd import dqn
    B, T = 5, 40
    env, runner, replay, model, target = _trainer_parts(torch, multi)
    start = {k: v.clone() for k, v in model.state_dict().items()}
    target_start = {k: v.clone() for k, v in target.state_dict().items()}
    reports = []
    trainer = dqn.DQNTrainer(runner, replay, model, target, torch.optim.Adam(model.parameters(), lr=1e-3),
                             on_report=lambda *a: reports.append(a), record_events=True, **SCHEDULE)
    trainer.train(T * B)
    assert runner.num_steps == trainer.num_steps == T * B and len(trainer.events) == T

    _env2, runner2, replay2, _model2, _target2 = _trainer_parts(torch, multi)
    pushes, idx = [], 0
    for e in trainer.events:
        assert e[1] == trainer.epsilon_schedule(e[0] - B) and e[1] >= 1.0
        runner2.collect(1, e[1], replay2)
        now = int(replay2.idx.item())
        pushes.append(now - idx)
        idx = now
    for name in ("obs", "next_obs", "action", "reward", "done", "idx", "fill"):
        assert torch.equal(getattr(replay, name), getattr(replay2, name)), name
    assert int(replay.status.item()) == 0

    case = dict(num_envs=B, start=0, capacity=replay.capacity, train_calls=[T * B], pushes=pushes,
                optimize_interval=SCHEDULE["optimize_interval"], target_update_interval=SCHEDULE["target_update_interval"],
                report_interval=SCHEDULE["report_interval"], replay_initial=SCHEDULE["replay_initial"])
    want = ref.schedule_model(case, trainer.epsilon_schedule)
    print(trainer.events)
    assert trainer.events == want
    optimized = [e for e in want if e[2]]
    assert not want[0][2] and len(optimized) >= 5 and any(e[4] for e in want)          # replay_initial fell inside the run
    opened = next(k for k in range(T) if min(sum(pushes[:k + 1]), replay.capacity) >= SCHEDULE["replay_initial"])
    assert 0 < opened < T - 10
    # one exact len(replay) per step until the gate opened, no host visit afterwards
    assert trainer.host_visits == opened + 1
    assert [(r[0], r[1]) for r in reports] == [(e[0], e[1]) for e in want if e[3]]
    assert all(torch.is_tensor(r[2]) and r[2].is_cuda and r[2].shape == (8,) for r in reports)
    s = trainer.sums.cpu().numpy()
    assert s[5] == SCHEDULE["training_batch_size"] and np.isfinite(s).all()
    assert any(not torch.equal(v, start[k]) for k, v in model.state_dict().items())
    assert any(not torch.equal(v, target_start[k]) for k, v in target.state_dict().items())
    replay.check_status()
    dqn.check_status()
