"""The PPO train loop on the device (safelife_amd/ppo.py: ppo_report, PPOTrainer; runner.VectorRunner(seed=); the report
kernels of sl_ppo.hip) against the reference's own results (tests/golden/ppo_train_cases.npz) and the host models of
tests/ppo_train_ref.py and tests/policy_ref.py.

Bounds.  The four reported scalars are compared with the reference's FLOAT64 run.  The bound is that of
tests/test_ppo_loss_gpu.py: twice the largest deviation the reference's own float32 run shows from its float64 run over the
fixture's cases of the same row count, and never below one float32 ulp of the float64 value.  BOUNDS below is computed from
the fixture when the module loads; the test prints its figures before asserting.

Measured on an MI355X: see DESIGN.md section 6e."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

from safelife_amd import _hip
from tests import policy_ref
from tests import ppo_loss_ref
from tests import ppo_train_ref as ref
from tests import util

pytestmark = pytest.mark.gpu

HAVE = os.path.exists(ref.PATH)
REPORTS = ref.load_report_cases() if HAVE else []
BY_ID = {c["id"]: c for c in REPORTS}
Batch = collections.namedtuple("Batch", "obs actions action_prob returns advantages values")
POISON = float("nan")


def _bounds():
    """BOUNDS[n][k] = twice the largest |float32 run - float64 run| of scalar k over the fixture's cases of n rows."""
    b = collections.defaultdict(lambda: np.zeros(4))
    for c in REPORTS:
        b[c["n"]] = np.maximum(b[c["n"]], 2.0 * np.abs(c["scalars32"] - c["scalars64"]))
    return b


BOUNDS = _bounds()


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def device_batch(c, torch, dev, **replace):
    """The case's batch; `obs` holds every row's own number, which is how the stub model finds the row's stored outputs."""
    x = {k: torch.from_numpy(np.ascontiguousarray(replace.get(k, c[k]))).to(dev)
         for k in ("actions", "action_prob", "returns", "advantages", "old_values")}
    n = len(c["actions"])
    return Batch(torch.arange(n, dtype=torch.float32, device=dev), x["actions"], x["action_prob"], x["returns"],
                 x["advantages"], x["old_values"])


def stored_outputs(c, torch, dev, **replace):
    """-> (model, values, policy): the model hands back the stored outputs of the rows it is asked about."""
    values = torch.from_numpy(np.ascontiguousarray(replace.get("values", c["values"]))).to(dev)
    policy = torch.from_numpy(np.ascontiguousarray(replace.get("policy", c["policy"]))).to(dev)
    chunks = []

    def model(obs):
        assert obs.dtype == torch.float32 and not torch.is_grad_enabled()
        rows = obs.to(torch.int64)
        chunks.append(int(obs.shape[0]))
        return values[rows], policy[rows]

    model.chunks = chunks
    return model, values, policy


def hyper(c):
    return dict(zip(ppo_loss_ref.HYPER, c["hyper"]))


def raw_report(c, torch, dev, chunk_rows, batch, values, policy, status):
    """The two entry points themselves over a workspace poisoned with NaN -> (out, workspace)."""
    lib = _hip.lib()
    N, A = policy.shape
    s = _hip.PpoLoss()
    s.N, s.n_actions = N, A
    s.eps_policy, s.eps_value, s.vf_coef, s.entropy_reg, s.entropy_clip = c["hyper"]
    for name, t in (("actions", batch.actions), ("action_prob", batch.action_prob), ("old_values", batch.values),
                    ("returns", batch.returns), ("advantages", batch.advantages), ("status", status)):
        setattr(s, name, t.data_ptr())
    words = lib.slhip_ppo_report_workspace_bytes(N) // 8
    assert words == 5 * ((N + 255) // 256)
    work = torch.full((words + 5,), POISON, dtype=torch.float64, device=dev)       # five words of room behind it
    out = torch.full((_hip.PPO_REPORT_DOUBLES,), POISON, dtype=torch.float64, device=dev)
    for lo in range(0, N, chunk_rows):
        v, p = values[lo:lo + chunk_rows].contiguous(), policy[lo:lo + chunk_rows].contiguous()
        s.n, s.values, s.policy = v.shape[0], v.data_ptr(), p.data_ptr()
        _hip.check(lib.slhip_ppo_report_rows(C.byref(s), lo, _hip.ptr(work), _hip.current_stream_ptr()))
    _hip.check(lib.slhip_ppo_report_finish(C.byref(s), _hip.ptr(work), words // 5, _hip.ptr(out), _hip.current_stream_ptr()))
    torch.cuda.synchronize()
    return out, work


# ------------------------------------------------------------------------------------------------------ the report kernels

def test_report_scalars_against_the_reference():
    """Every fixture case in one test (28 small launches): the four float32 scalars against the float64 run."""
    import torch
    from safelife_amd import ppo
    dev = _hip.device()
    failed = []
    for c in REPORTS:
        model, _v, _p = stored_outputs(c, torch, dev)
        status = torch.zeros(1, dtype=torch.int64, device=dev)
        out = ppo.ppo_report(model, device_batch(c, torch, dev), status=status, **hyper(c))
        assert out.shape == (_hip.PPO_REPORT_DOUBLES,) and out.dtype == torch.float64 and int(status.item()) == 0
        assert model.chunks == [c["n"]]
        named = ppo.ppo_report.scalars(out)
        assert list(named) == list(ref.SCALARS) and all(isinstance(v, float) for v in named.values())
        got = np.array([named[k] for k in ref.SCALARS])
        o = out.cpu().numpy()
        wide = np.array([o[4], o[2], o[_hip.PPO_REPORT_VALUES], o[_hip.PPO_REPORT_ADVANTAGES]])
        assert same_bits(wide.astype(np.float32), got.astype(np.float32))          # the floats are the doubles, rounded once
        want = c["scalars64"]
        allowed = np.maximum(BOUNDS[c["n"]], ulp32(want))
        ratio, ratio_wide = np.abs(got - want) / allowed, np.abs(wide - want) / allowed
        print("%-24s ratios  float32 %s   float64 slots %s" % (c["id"], np.round(ratio, 3), np.round(ratio_wide, 3)))
        if not np.all(ratio <= 1.0):
            failed.append((c["id"], ratio))
        assert o[6] == c["n"] and o[5] == float(np.float32(o[2]) <= np.float32(c["hyper"][4]))
    assert not failed, failed


@pytest.mark.parametrize("name", ("n1-a9", "n255-a2", "n256-a32", "n257-a9", "n4099-a9", "n4099-a32"))
def test_report_does_not_depend_on_the_chunking(name):
    """chunk_rows 256, 512 and >= N over a poisoned workspace: the out tensors are byte-equal, their first seven slots are
    ppo_loss.sums of one dense ppo_loss call, the workspace holds five finite doubles per 256 rows and NaN behind them."""
    import torch
    from safelife_amd import ppo
    dev = _hip.device()
    c = BY_ID[name]
    N = c["n"]
    batch = device_batch(c, torch, dev)
    model, values, policy = stored_outputs(c, torch, dev)
    status = torch.zeros(1, dtype=torch.int64, device=dev)
    outs, works = [], []
    for chunk in (256, 512, 4352):
        out, work = raw_report(c, torch, dev, chunk, batch, values, policy, status)
        outs.append(out.cpu().numpy()), works.append(work.cpu().numpy())
        del model.chunks[:]
        wrapped = ppo.ppo_report(model, batch, chunk_rows=chunk, status=status, **hyper(c))
        assert model.chunks == [min(chunk, N - lo) for lo in range(0, N, chunk)]
        assert same_bits(wrapped.cpu().numpy(), outs[-1]), chunk
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2])
    assert same_bits(works[0], works[1]) and same_bits(works[0], works[2])
    assert np.isfinite(works[0][:-5]).all() and np.isnan(works[0][-5:]).all() and np.isfinite(outs[0][:9]).all()
    _entropy, loss = ppo.ppo_loss(values, policy, batch, status=status, **hyper(c))
    sums = ppo.ppo_loss.sums.cpu().numpy()
    assert same_bits(outs[0][:7], sums[:7])
    f32 = outs[0][_hip.PPO_REPORT_F32:].view(np.float32)
    assert same_bits(f32[0], loss.cpu().numpy()) and same_bits(f32[0], sums.view(np.float32)[2 * _hip.PPO_SUM_LOSS_F32])
    assert int(status.item()) == 0


def test_a_bad_action_is_flagged_and_adds_nothing():
    """The comparison run holds, where the bad run has a bad action, rows that add exactly zero to all five sums (advantage
    0, v = v_old = R = 0, a one-hot policy: float32 entropy 0)."""
    import torch
    from safelife_amd import ppo
    dev = _hip.device()
    c = BY_ID["n257-a9"]
    at = (3, 255, 256)
    fields = {k: c[k].copy() for k in ("actions", "action_prob", "old_values", "returns", "advantages", "values", "policy")}
    for i in at:
        fields["advantages"][i] = fields["old_values"][i] = fields["returns"][i] = fields["values"][i] = 0.0
        fields["policy"][i] = 0.0
        fields["policy"][i, 2] = 1.0
        fields["actions"][i] = 2
    model, _v, _p = stored_outputs(c, torch, dev, **fields)
    status = torch.zeros(1, dtype=torch.int64, device=dev)
    clean = ppo.ppo_report(model, device_batch(c, torch, dev, **fields), chunk_rows=256, status=status, **hyper(c))
    assert int(status.item()) == 0
    bad = {k: v.copy() for k, v in fields.items()}
    bad["actions"][list(at)] = (-1, 9, 1 << 40)
    for k in ("advantages", "old_values", "returns"):       # what the skipped rows hold is never added
        bad[k][list(at)] = 5.0
    got = ppo.ppo_report(model, device_batch(c, torch, dev, **bad), chunk_rows=256, status=status, **hyper(c))
    assert int(status.item()) == _hip.PPO_BAD_ACTION
    with pytest.raises(ValueError):
        ppo.check_status(status)
    assert same_bits(got.cpu().numpy(), clean.cpu().numpy())
    ppo.check_status()                          # the shared word was never touched


def test_refusals_leave_the_workspace_alone():
    import torch
    from safelife_amd import ppo
    dev = _hip.device()
    c = BY_ID["n257-a9"]
    batch = device_batch(c, torch, dev)
    model, values, policy = stored_outputs(c, torch, dev)
    with pytest.raises(ValueError, match="multiple of 256"):
        ppo.ppo_report(model, batch, chunk_rows=100)
    assert model.chunks == []
    lib = _hip.lib()
    s = _hip.PpoLoss()
    s.n, s.N, s.n_actions = 129, 257, 9
    s.eps_policy, s.eps_value, s.vf_coef, s.entropy_reg, s.entropy_clip = c["hyper"]
    status = torch.zeros(1, dtype=torch.int64, device=dev)
    for name, t in (("values", values), ("policy", policy), ("actions", batch.actions), ("action_prob", batch.action_prob),
                    ("old_values", batch.values), ("returns", batch.returns), ("advantages", batch.advantages),
                    ("status", status)):
        setattr(s, name, t.data_ptr())
    work = torch.full((10,), POISON, dtype=torch.float64, device=dev)
    assert lib.slhip_ppo_report_rows(C.byref(s), 128, _hip.ptr(work), _hip.current_stream_ptr()) == _hip.SL_E_ARG
    torch.cuda.synchronize()
    assert np.isnan(work.cpu().numpy()).all() and int(status.item()) == 0


# ------------------------------------------------------------------------------------------------------------ the trainer

CHANNELS = tuple(range(12)) + (25, 26, 27)
SINGLE_KW = dict(time_limit=6, view_shape=(5, 5), output_channels=CHANNELS, policy_layout="uint8", with_obs=False)
SCHEDULE = dict(steps_per_env=4, report_interval=40, test_interval=60, num_minibatches=4, epochs_per_batch=3, seed=9)


def _device_counts(boards, goals):
    from safelife_amd.levels import _device_counts as f
    return f(boards, goals)


def _single_pool():
    from safelife_amd.levels import LevelPool
    levels = []
    for name in ("worked_7x7_exit", "worked_7x7_noop"):
        levels += util.levels_from_trace(util.load_trace(name))
    return LevelPool(levels, counts_fn=_device_counts), len(levels)


class ConvPolicy(object):
    """Made inside a function (torch is imported late): a 3x3 convolution written as unfold + matmul, ReLU, one linear
    layer -> (values [n], softmax probabilities [n, 9])."""

    @staticmethod
    def make(torch, channels, width, height, device, seed):
        class Net(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.conv = torch.nn.Linear(channels * 9, 4)
                self.head = torch.nn.Linear(4 * (width - 2) * (height - 2), 10)

            def forward(self, x):
                patches = torch.nn.functional.unfold(x, 3).transpose(1, 2)          # [n, places, channels * 9]
                y = torch.relu(self.conv(patches)).flatten(1)
                y = self.head(y)
                return y[:, 0], torch.softmax(y[:, 1:], dim=-1)

        torch.manual_seed(seed)
        return Net().to(device)


def _single_parts(torch, with_test_runner):
    from safelife_amd import episode_run
    from safelife_amd.runner import VectorRunner
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool, n_levels = _single_pool()
    env = SafeLifeVectorEnv(pool, 5, first_level=np.arange(5) % n_levels, auto_reset=True, **SINGLE_KW)
    model = ConvPolicy.make(torch, len(CHANNELS), 5, 5, env.device, seed=8)
    runner = VectorRunner(env, model, seed=77)
    test_runner = None
    if with_test_runner:
        run = episode_run.EpisodeRun(pool, 5, 7)
        test_env = SafeLifeVectorEnv(pool, 5, episode_run=run, **SINGLE_KW, **run.env_arguments())
        test_runner = VectorRunner(test_env, model, seed=78)
    return env, runner, model, torch.optim.Adam(model.parameters(), lr=1e-3), test_runner


def _params(model):
    return [p.detach().clone() for p in model.parameters()]


def _watch_batches(runner, seen):
    make = runner.gen_training_batch

    def gen_training_batch(*a, **kw):
        seen.append(make(*a, **kw))
        return seen[-1]

    runner.gen_training_batch = gen_training_batch


def test_trainer_single_agent():
    """5 envs of 7x7, 4 steps per env: three batches of 20 steps -- nothing due, a report (num_steps lands ON the interval),
    a test run."""
    import torch
    from safelife_amd import ppo
    case = dict(num_envs=5, steps_per_env=4, report_interval=40, test_interval=60, start=0, has_logger=True, has_testing=True,
                train_calls=[60])
    want = ref.schedule_model(case)
    assert want == [(20, False, False), (40, True, False), (60, False, True)]

    env, runner, model, opt, test_runner = _single_parts(torch, True)
    start = _params(model)
    batches, reports, tests = [], [], []
    _watch_batches(runner, batches)

    def on_report(num_steps, report):
        direct = ppo.ppo_report(model, batches[-1], chunk_rows=256)
        reports.append((num_steps, same_bits(report.cpu().numpy(), direct.cpu().numpy()), ppo.ppo_report.scalars(report)))

    run_episodes = test_runner.run_episodes

    def counting_run_episodes():
        before = runner.num_steps
        results = run_episodes()
        tests.append((before, runner.num_steps, test_runner.num_steps, len(results)))
        return results

    test_runner.run_episodes = counting_run_episodes
    on_batch = []
    trainer = ppo.PPOTrainer(runner, model, opt, test_runner=test_runner, on_report=on_report, on_batch=on_batch.append,
                             record_events=True, **SCHEDULE)
    trainer.train(60)
    print(trainer.events, reports)
    assert trainer.events == want and trainer.host_visits == 0 and trainer.batches_done == 3 and on_batch == [20, 40, 60]
    assert [r[0] for r in reports] == [40] and reports[0][1] and all(np.isfinite(v) for v in reports[0][2].values())
    assert tests == [(60, 60, 0, 7)]            # run exactly then; neither runner's count moved across it
    assert len(batches) == 3 and all(b.actions.shape[0] == 20 for b in batches) and list(trainer._deals) == [20]
    got = _params(model)
    assert any(not torch.equal(a, b) for a, b in zip(got, start))
    s = trainer.sums.cpu().numpy()
    assert s[6] == 20 - ppo.split_points(20, 4)[-1] and np.isfinite(s[:5]).all()

    # the same calls made by hand, same seeds: the parameters are equal bit for bit
    env2, runner2, model2, opt2, _none = _single_parts(torch, False)
    deal = ppo.MinibatchDeal(20, 4, seed=9)
    for k in range(3):
        batch = runner2.gen_training_batch(4, 0.97, 0.95)
        ppo.train_batch(model2, opt2, batch, deal, k * 3, 3)
    assert all(torch.equal(a, b) for a, b in zip(got, _params(model2)))
    assert torch.equal(env.policy_tensor, env2.policy_tensor)

    # two train() calls are one call over the sum; a state_dict round trip
    env3, runner3, model3, opt3, test_runner3 = _single_parts(torch, True)
    twice = ppo.PPOTrainer(runner3, model3, opt3, test_runner=test_runner3, on_report=lambda *a: None, record_events=True,
                           **SCHEDULE)
    twice.train(35)
    assert twice.num_steps == 40 and twice.batches_done == 2
    state = twice.state_dict()
    assert state == dict(num_steps=40, batches_done=2, seed=9)
    fresh = ppo.PPOTrainer(runner3, model3, opt3, **dict(SCHEDULE, seed=0))
    fresh.load_state_dict(state)
    assert fresh.state_dict() == state
    twice.train(20)
    assert twice.events == want and twice.batches_done == 3
    assert all(torch.equal(a, b) for a, b in zip(got, _params(model3)))
    ppo.check_status()


MULTI_KW = dict(time_limit=9, view_shape=(7, 11), output_channels=CHANNELS, policy_layout="uint8", with_obs=False)


def _multi_parts(torch, own=0.0625, seed=7):
    from safelife_amd.levels import LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    from safelife_amd.runner import MultiAgentRunner
    from tests.test_training_batch_multi_gpu import ExactPolicy, spec_levels
    levels = spec_levels()
    pool = LevelPool(levels, counts_fn=_device_counts, n_agents=2, min_performance_fraction=0.0)
    env = SafeLifeMultiAgentVectorEnv(pool, 5, first_level=np.arange(5) % len(levels), auto_reset=True, **MULTI_KW)
    shape = tuple(env.policy_tensor.shape[2:])
    exact = ExactPolicy(torch, shape, env.device)

    class Net(torch.nn.Module):
        """A linear value and policy head; 15/16 of the probability stay with the exit-seeking exact policy, so that
        agents leave their levels before the time limit and the windows differ in their row counts (with a quarter of the
        probability of its own the head keeps every agent on its board for all six windows)."""

        def __init__(self):
            super().__init__()
            self.head = torch.nn.Linear(int(np.prod(shape)), 10)

        def forward(self, x):
            y = self.head(x.flatten(1))
            return y[:, 0], own * torch.softmax(y[:, 1:], dim=-1) + (1.0 - own) * exact(x)[1]

    torch.manual_seed(8)
    model = Net().to(env.device)
    return env, MultiAgentRunner(env, model, seed=seed), model, torch.optim.Adam(model.parameters(), lr=1e-3)


def test_trainer_multi_agent():
    """5 envs x 2 agents, 4 steps per env, six windows: the windows' row counts differ, each count gets its own deal and the
    epoch index runs on across them."""
    import torch
    from safelife_amd import ppo
    windows = 6
    case = dict(num_envs=5, steps_per_env=4, report_interval=50, test_interval=10 ** 9, start=0, has_logger=True,
                has_testing=False, train_calls=[20 * windows])
    env, runner, model, opt = _multi_parts(torch)
    batches, reports = [], []
    _watch_batches(runner, batches)
    trainer = ppo.PPOTrainer(runner, model, opt, steps_per_env=4, report_interval=50, seed=9,
                             on_report=lambda n, r: reports.append((n, r)), record_events=True)
    trainer.train(20 * windows)
    rows = [int(b.actions.shape[0]) for b in batches]
    print(trainer.events, rows)
    assert trainer.events == ref.schedule_model(case) and len(trainer.events) == windows
    assert trainer.host_visits == windows and trainer.batches_done == windows
    assert len(set(rows)) >= 2 and max(rows) <= 40 and sorted(trainer._deals) == sorted(set(rows))
    assert [n for n, _r in reports] == [e[0] for e in trainer.events if e[1]] and len(reports) >= 2
    for n, r in reports:
        o = r.cpu().numpy()
        assert o[6] == rows[n // 20 - 1] and np.isfinite(o[:9]).all()

    env2, runner2, model2, opt2 = _multi_parts(torch)
    deals = {}
    for k in range(windows):
        batch = runner2.gen_training_batch(4, 0.97, 0.95)
        N = int(batch.actions.shape[0])
        assert N == rows[k]
        deal = deals.setdefault(N, ppo.MinibatchDeal(N, 4, seed=9))
        ppo.train_batch(model2, opt2, batch, deal, k * 3, 3)
    assert all(torch.equal(a, b) for a, b in zip(_params(model), _params(model2)))
    ppo.check_status()


# ------------------------------------------------------------------------------------------------------------- the runner

class _TablePolicy(object):
    """Probabilities hashed from the observation and the call count; keeps what it returned."""

    def __init__(self, torch, n_actions=9):
        self.torch, self.n_actions, self.seen = torch, n_actions, []

    def __call__(self, obs):
        torch = self.torch
        n = obs.shape[0]
        g = torch.Generator(device="cpu").manual_seed(1000 + len(self.seen))
        probs = torch.softmax(3.0 * torch.randn(n, self.n_actions, generator=g), dim=-1).to(obs.device)
        self.seen.append(probs)
        return torch.zeros(n, device=obs.device), probs


def _runner_env(B, **kw):
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool, n_levels = _single_pool()
    return SafeLifeVectorEnv(pool, B, first_level=np.arange(B) % n_levels, auto_reset=True, **SINGLE_KW, **kw)


def test_vector_runner_with_a_seed_draws_as_the_host_model():
    import torch
    from safelife_amd.runner import VectorRunner
    B, offset, seed = 65, 11, 0xC0FFEE12345
    env = _runner_env(B, env_offset=offset)
    policy = _TablePolicy(torch)
    runner = VectorRunner(env, policy, seed=seed)
    for step in range(6):
        out = runner.take_one_step()
        want = policy_ref.sample_model(policy.seen[step].cpu().numpy(), seed, step, first_env=offset)
        assert out.actions.dtype == torch.int64 and np.array_equal(out.actions.cpu().numpy(), want), step
        assert out.actions.data_ptr() != runner.actions.data_ptr()
    assert runner.draws == 6 and runner.num_steps == 6 and len({tuple(p.cpu().numpy().argmax(1)) for p in policy.seen}) == 6
    batch = runner.gen_training_batch(3)
    assert runner.draws == 9 and batch.actions.shape == (3 * B,) and runner.num_steps == 6 + 3 * B
    want = np.concatenate([policy_ref.sample_model(policy.seen[6 + t].cpu().numpy(), seed, 6 + t, first_env=offset)
                           for t in range(3)])
    assert np.array_equal(batch.actions.cpu().numpy(), want)
    with pytest.raises(ValueError, match="probabilities"):
        VectorRunner(_runner_env(4), lambda obs: (None, torch.zeros(3, 9, device=obs.device)), seed=1).take_one_step()


def test_vector_runner_without_a_seed_draws_with_torch_as_before():
    import torch
    from safelife_amd.runner import VectorRunner
    B = 65
    env = _runner_env(B)
    policy = _TablePolicy(torch)
    runner = VectorRunner(env, policy, generator=torch.Generator(device=env.device).manual_seed(11))
    assert runner.seed is None and not hasattr(runner, "draws")
    twin = torch.Generator(device=env.device).manual_seed(11)
    for step in range(3):
        out = runner.take_one_step()
        want = torch.multinomial(policy.seen[step], 1, generator=twin).squeeze(1)
        assert out.actions.dtype == torch.int64 and torch.equal(out.actions, want), step
