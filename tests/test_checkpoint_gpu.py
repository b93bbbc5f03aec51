"""Checkpoints on the device (safelife_amd/checkpoint.py, sl_digest.hip): the state digest against the host model of
tests/checkpoint_ref.py bit for bit, and the feature's definition -- a run that is saved, rebuilt from nothing and resumed
ends in the same bits as the run that never stopped -- for four training stacks, tensor by tensor as well as by digest."""
import ctypes as C
import os

import numpy as np
import pytest

from safelife_amd import _hip
from tests import checkpoint_ref as ref
from tests import util

pytestmark = pytest.mark.gpu

SALT64 = 0xFEDCBA9876543210
SIZES = (0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, (1 << 20) + 3)
MIB = 1 << 20


# ------------------------------------------------------------------------------------------------------------- the digest

@pytest.fixture(scope="module")
def noise():
    """64 MiB + 64 of random bytes on the device, and the host's copy: computed once, never written."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(2026)
    host = torch.randint(0, 256, (64 * MIB + 64,), dtype=torch.uint8, generator=g)
    return host.to(_hip.device()), host.numpy()


def raw_digest(torch, segments, salt, room=0, poison=-1):
    """``slhip_state_digest`` itself over [(pointer, bytes)]: -> (digests, the `room` words behind out[n - 1])."""
    lib, dev, n = _hip.lib(), _hip.device(), len(segments)
    sizes = (C.c_ulonglong * max(n, 1))(*[b for _, b in segments])
    words = int(lib.slhip_state_digest_workspace_bytes(sizes, n)) // 8
    prefix = np.zeros(n + 1, np.uint64)
    assert lib.slhip_state_digest_prefix(sizes, n, prefix.ctypes.data_as(C.c_void_p)) == 0
    assert prefix[0] == 0 and words == n + 1 + int(prefix[n]) and (np.diff(prefix.astype(np.int64)) >= 1).all()
    table = torch.from_numpy(np.array([[p, b] for p, b in segments], np.uint64).reshape(n, 2).view(np.int64)).to(dev)
    work = torch.full((words,), poison, dtype=torch.int64, device=dev)
    work[:n + 1] = torch.from_numpy(prefix.view(np.int64)).to(dev)
    out = torch.full((n + room,), poison, dtype=torch.int64, device=dev)
    _hip.check(lib.slhip_state_digest(_hip.ptr(table), n, salt, _hip.ptr(out), _hip.ptr(work), _hip.current_stream_ptr()))
    got = out.cpu().numpy()
    return [int(v) for v in got[:n].view(np.uint64)], got[n:]


@pytest.mark.parametrize("salt", (0, SALT64), ids=("salt 0", "a 64-bit salt"))
def test_digest_of_every_size_equals_the_host_model(noise, salt):
    """Each size alone (a table of one segment) and all of them in one table, at a start that is 16-byte aligned."""
    import torch
    from safelife_amd import checkpoint
    dev_bytes, host = noise
    base = dev_bytes.data_ptr()
    assert base % 16 == 0
    want, segments, at = [], [], 0
    for n in SIZES:
        segments.append((base + at, n))
        want.append(ref.digest(host[at:at + n].tobytes(), salt))
        at += (n + 15) // 16 * 16
    for seg, w, n in zip(segments, want, SIZES):
        got, _ = raw_digest(torch, [seg], salt)
        assert got == [w], (n, hex(got[0]), hex(w))
    got, beyond = raw_digest(torch, segments, salt, room=3)
    assert got == want
    assert (beyond == -1).all()                                     # out slots beyond the table are untouched
    assert checkpoint.digest_segments(segments, salt) == want        # the package's own call
    if salt == 0:
        assert want[0] == ref.KNOWN[0][2]
        twenty = torch.arange(20, dtype=torch.uint8, device=dev_bytes.device)
        assert checkpoint.digest_segments([(twenty.data_ptr(), 20)], 0) == [ref.KNOWN[1][2]]
        assert checkpoint.digest_segments([(twenty.data_ptr(), 20)], 7) == [ref.KNOWN[2][2]]


def test_digest_at_every_pointer_offset_inside_poisoned_bytes(noise):
    """Offsets 0..15 (every byte alignment, both parities of the 8-byte word) and lengths around the word, the 16-byte
    pair and the 32 KiB chunk, cut out of a buffer whose other bytes are poison: the digest is that of the bytes inside
    and of nothing else."""
    import torch
    _dev_bytes, host = noise
    lengths = (0, 1, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 255, 4097, 32767, 32768, 32769, 65536 + 5)
    span = max(lengths) + 64
    segments, want, rows = [], [], []
    buf = torch.full((len(lengths) * 16, span), 0xA5, dtype=torch.uint8, device=_hip.device())
    row = 0
    for n in lengths:
        for off in range(16):
            rows.append((row, off, n))
            row += 1
    stage = np.full((row, span), 0xA5, np.uint8)
    for r, off, n in rows:
        stage[r, 16 + off:16 + off + n] = host[1000 + r:1000 + r + n]
        want.append(ref.digest(stage[r, 16 + off:16 + off + n].tobytes(), 5))
    buf.copy_(torch.from_numpy(stage))
    assert buf.data_ptr() % 16 == 0 and span % 16 != 0              # the rows themselves start at every alignment too
    segments = [(buf.data_ptr() + r * span + 16 + off, n) for r, off, n in rows]
    got, _ = raw_digest(torch, segments, 5)
    bad = [(rows[i], hex(got[i]), hex(want[i])) for i in range(len(rows)) if got[i] != want[i]]
    assert not bad, bad[:5]
    assert torch.equal(buf.cpu(), torch.from_numpy(stage))          # the inputs are only read


@pytest.mark.parametrize("count", (1, 63, 64, 65, 1000))
def test_tables_mixing_counters_and_large_segments(noise, count):
    """4-byte counters next to multi-MiB segments in one table; two calls are bit-equal."""
    import torch
    dev_bytes, host = noise
    base = dev_bytes.data_ptr()
    rng = np.random.default_rng(count)
    segments, want = [], []
    big = {0, count // 2, count - 1}
    for i in range(count):
        if i in big:
            n = int(rng.integers(2 * MIB, 5 * MIB)) + int(rng.integers(0, 8))
            at = int(rng.integers(0, 32 * MIB))
        else:
            n, at = 4, 4 * int(rng.integers(0, 8 * MIB))
        segments.append((base + at, n))
        want.append(ref.digest(host[at:at + n].tobytes(), SALT64))
    got, _ = raw_digest(torch, segments, SALT64)
    assert got == want
    again, _ = raw_digest(torch, segments, SALT64, poison=0x5A5A5A5A)
    assert again == got


def test_one_segment_spans_the_capped_grid_several_times():
    """ONE segment of 256 MiB + 3 bytes from an odd address: 8193 chunks of 32 KiB over the grid of 2048 workgroups, four
    sweeps and a chunk, so most chunk indices lie far above the grid -- against the host model.  Both sides fill the same
    pattern (word k = k * G mod 2^64), so nothing of this size crosses to the device."""
    import torch
    words = 32 * MIB + 2
    with np.errstate(over="ignore"):
        host = (np.arange(words, dtype=np.uint64) * np.uint64(ref.G)).view(np.uint8)
    dev = torch.arange(words, dtype=torch.int64, device=_hip.device()) * (ref.G - (1 << 64))     # (the same bits: it wraps)
    probe = [0, 1, 12345, words - 1]
    assert dev[probe].cpu().numpy().view(np.uint64).tolist() == host.view(np.uint64)[probe].tolist()
    n = 256 * MIB + 3
    got, _ = raw_digest(torch, [(dev.data_ptr() + 5, n), (dev.data_ptr() + 8, 4)], SALT64)
    assert got == [ref.digest(host[5:5 + n].tobytes(), SALT64), ref.digest(host[8:12].tobytes(), SALT64)]


def test_segments_of_one_sweep_and_a_chunk_side_by_side(noise):
    """64 MiB + 61 bytes (2049 chunks: one sweep of the grid and one chunk) four times over in one table, from four
    alignments, next to a counter."""
    import torch
    dev_bytes, host = noise
    base = dev_bytes.data_ptr()
    n = 64 * MIB + 61
    segments = [(base + 3, n), (base + 8, 4), (base + 1, n), (base, n + 3), (base + 2, n - 7)]
    want = [ref.digest(host[p - base:p - base + b].tobytes(), 1) for p, b in segments]
    got, _ = raw_digest(torch, segments, 1)
    assert got == want
    assert len(set(got)) == len(got)


def test_digest_refusals():
    import torch
    lib = _hip.lib()
    dev = _hip.device()
    x = torch.zeros(16, dtype=torch.int64, device=dev)
    assert lib.slhip_state_digest(None, 0, 0, None, None, None) == 0                    # an empty table: nothing to do
    assert lib.slhip_state_digest(_hip.ptr(x), -1, 0, _hip.ptr(x), _hip.ptr(x), None) == _hip.SL_E_ARG
    assert lib.slhip_state_digest(None, 1, 0, _hip.ptr(x), _hip.ptr(x), None) == _hip.SL_E_ARG
    assert lib.slhip_state_digest(_hip.ptr(x), 1, 0, C.c_void_p(x.data_ptr() + 4), _hip.ptr(x), None) == _hip.SL_E_ARG
    assert lib.slhip_state_digest_workspace_bytes(None, 0) == 0
    torch.cuda.synchronize()
    assert int(x.abs().sum().item()) == 0


# ------------------------------------------------------------------------------------------------- resume equals straight

def _bits(t):
    return t.detach().contiguous().view(-1).view(__import__("torch").uint8)


def assert_same_state(a, c, where):
    """Two roots agree in everything `checkpoint` calls state: by digest AND tensor by tensor, and in their scalars."""
    import torch
    from safelife_amd import checkpoint
    da, dc = checkpoint.state_digest(a), checkpoint.state_digest(c)
    assert sorted(da) == sorted(dc)
    differ = [k for k in da if da[k] != dc[k]]
    ca, cc = checkpoint.capture(a), checkpoint.capture(c)
    assert sorted(ca) == sorted(cc)
    unequal = []
    for name in ca:
        assert ca[name]["class"] == cc[name]["class"] and ca[name]["config"] == cc[name]["config"]
        assert ca[name]["scalars"] == cc[name]["scalars"], (where, name, ca[name]["scalars"], cc[name]["scalars"])
        for k, t in ca[name]["tensors"].items():
            if not torch.equal(_bits(t), _bits(cc[name]["tensors"][k])):
                unequal.append("%s/%s" % (name, k))
    assert sorted(differ) == sorted(unequal), (where, differ, unequal)     # the digest sees exactly what a comparison sees
    assert not unequal, (where, unequal)
    assert len(da) == sum(len(x["tensors"]) for x in ca.values())


def assert_same_models(pairs, opt_a, opt_c):
    import torch
    for ma, mc in pairs:
        sa, sc = ma.state_dict(), mc.state_dict()
        assert list(sa) == list(sc) and all(torch.equal(_bits(sa[k]), _bits(sc[k])) for k in sa)
    sa, sc = opt_a.state_dict(), opt_c.state_dict()
    assert sa["param_groups"] == sc["param_groups"] and sorted(sa["state"]) == sorted(sc["state"]) and sa["state"]
    for k in sa["state"]:
        for name, v in sa["state"][k].items():
            w = sc["state"][k][name]
            assert torch.equal(_bits(v.cpu()), _bits(w.cpu())) if torch.is_tensor(v) else v == w, (k, name)


def pointers(root):
    from safelife_amd import checkpoint
    return {"%s/%s" % (name, k): t.data_ptr() for name, rec in checkpoint.capture(root).items()
            for k, t in rec["tensors"].items()}


def _fixture_levels():
    levels = []
    for name in ("worked_7x7_exit", "worked_7x7_noop"):
        levels += util.levels_from_trace(util.load_trace(name))
    return levels


def _ppo_single(torch):
    """5 envs on the 7x7 fixture levels with the training wrappers, a finished-episode queue, a curriculum schedule whose
    exit difficulty moves with the training step, an episode log and a history; a test runner over an EpisodeRun."""
    from safelife_amd import episode_history, episode_log, episode_run, ppo, schedule
    from safelife_amd.levels import LevelPool
    from safelife_amd.runner import VectorRunner
    from safelife_amd.vector_env import SafeLifeVectorEnv
    from tests.step_matrix_cases import TRAINING_WRAPPERS
    from tests.test_ppo_train_gpu import CHANNELS, ConvPolicy, _device_counts
    pool = LevelPool(_fixture_levels(), counts_fn=_device_counts)
    kw = dict(time_limit=6, view_shape=(5, 5), output_channels=CHANNELS, policy_layout="uint8", with_obs=False)
    sched = schedule.LevelSchedule(pool, [(0, 1), (1, 1)], mode="curriculum", seed=12, lookback=5,
                                   min_performance_fraction=schedule.LinearSchedule([0, 200], [0.25, 1.0]))
    log = episode_log.EpisodeLog(pool, 5, 64, side_effect_weights={"life-green": 1.0, "spawner-yellow": 2.0})
    hist = episode_history.EpisodeHistory(pool, 5, [0, 2, 4], 12, interval=2)
    env = SafeLifeVectorEnv(pool, 5, auto_reset=True, wrappers=dict(TRAINING_WRAPPERS), level_schedule=sched, episode_log=log,
                            episode_history=hist, side_effects=dict(capacity=128, num_samples=4), **kw)
    model = ConvPolicy.make(torch, len(CHANNELS), 5, 5, env.device, seed=8)
    runner = VectorRunner(env, model, seed=77)
    run = episode_run.EpisodeRun(pool, 5, 7)
    test_env = SafeLifeVectorEnv(pool, 5, episode_run=run, **kw, **run.env_arguments())
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    trainer = ppo.PPOTrainer(runner, model, opt, test_runner=VectorRunner(test_env, model, seed=78), steps_per_env=7,
                             report_interval=70, test_interval=140, num_minibatches=4, epochs_per_batch=3, seed=9,
                             on_report=lambda *a: None, record_events=True)
    return trainer, {"model": model}, opt


def _ppo_multi(torch):
    from safelife_amd import ppo
    from tests.test_ppo_train_gpu import _multi_parts
    env, runner, model, opt = _multi_parts(torch)
    trainer = ppo.PPOTrainer(runner, model, opt, steps_per_env=7, report_interval=50, seed=9, on_report=lambda *a: None,
                             record_events=True)
    return trainer, {"model": model}, opt


def _dqn(torch, multi, capacity, replay_initial, tests=True):
    from safelife_amd import dqn, episode_run
    from safelife_amd.levels import LevelPool
    from safelife_amd.replay import MultiAgentReplayBuffer, ReplayBuffer
    from safelife_amd.runner import DQNRunner, MultiAgentDQNRunner
    from safelife_amd.vector_env import SafeLifeVectorEnv
    from tests.step_matrix_cases import TRAINING_WRAPPERS
    from tests.test_ppo_train_gpu import CHANNELS, _device_counts
    test_runner = None
    if multi:
        from tests.test_dqn_update_gpu import _multi_agent_env
        env = _multi_agent_env()
    else:
        pool = LevelPool(_fixture_levels(), counts_fn=_device_counts)
        kw = dict(time_limit=6, view_shape=(5, 5), output_channels=CHANNELS, policy_layout="uint8", with_obs=False)
        env = SafeLifeVectorEnv(pool, 5, first_level=np.arange(5) % 2, auto_reset=True, wrappers=dict(TRAINING_WRAPPERS), **kw)
    obs_shape = tuple(env.policy_tensor.shape[2 if multi else 1:])
    torch.manual_seed(8)
    make = lambda: torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(int(np.prod(obs_shape)), 9)).to(env.device)  # noqa: E731
    model, target = make(), make()
    reward_dtype = env.shaped_reward.dtype if env.shaped_reward is not None else torch.float32
    kw = dict(multi_step=2, gamma=0.97, obs_shape=obs_shape, obs_dtype=env.policy_tensor.dtype, reward_dtype=reward_dtype,
              device=env.device, seed=5)
    if multi:
        runner = MultiAgentDQNRunner(env, model, seed=77)
        replay = MultiAgentReplayBuffer(capacity, 5, 2, **kw)
    else:
        assert reward_dtype == torch.float64                        # the wrappers' shaped reward
        runner = DQNRunner(env, model, seed=77)
        replay = ReplayBuffer(capacity, 5, **kw)
        if tests:
            run = episode_run.EpisodeRun(pool, 5, 7)
            test_env = SafeLifeVectorEnv(pool, 5, episode_run=run, time_limit=6, view_shape=(5, 5), output_channels=CHANNELS,
                                         policy_layout="uint8", with_obs=False, **run.env_arguments())
            test_runner = DQNRunner(test_env, model, seed=78)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    trainer = dqn.DQNTrainer(runner, replay, model, target, opt, training_batch_size=16, optimize_interval=10,
                             target_update_interval=35, report_interval=25, replay_initial=replay_initial,
                             epsilon_schedule=lambda n: 0.6 - n / 1000.0, on_report=lambda *a: None, record_events=True,
                             test_runner=test_runner, test_interval=50, epsilon_testing=0.01)
    return trainer, {"training_model": model, "target_model": target}, opt


def resume_equals_straight(build, half, tmp_path, between=lambda trainer: None):
    """A: 2N iterations (two train() calls, as C makes two: DQN raises its report flag at every call).  B: N and save.  C:
    built from nothing, load, N.  -> (A, C) with their models and optimisers, compared in everything.

    ``between`` runs on A and B behind the first half and on A and C behind the second, in front of the comparison.  The
    stack with a finished-episode queue flushes it there: the step kernels take a queue slot with an atomic add, so the ORDER
    of a queue's entries is the one thing in this library that two identical runs do not share (every consumer matches
    entries by env and episode); behind a flush the queue is empty and everything made of its entries -- the log's joined
    rows, the histories' last frames -- is in place, so nothing escapes the comparison."""
    import torch
    from safelife_amd import checkpoint
    a, models_a, opt_a = build(torch)
    b, models_b, opt_b = build(torch)
    a.train(half), between(a)
    a.train(half)
    b.train(half), between(b)
    path = tmp_path / "half.data"
    saved = checkpoint.save(path, b, model=models_b, optimizer=opt_b)
    assert saved == checkpoint.state_digest(b)
    c, models_c, opt_c = build(torch)
    before = pointers(c)
    checkpoint.load(path, c, model=models_c, optimizer=opt_c)
    assert pointers(c) == before                                    # every state tensor keeps its data_ptr()
    assert_same_state(b, c, "behind the load")
    assert c.num_steps == b.num_steps == half and c.events == b.events
    c.train(half)
    between(a), between(c)
    torch.cuda.synchronize()
    assert a.num_steps == c.num_steps == 2 * half
    assert a.events == c.events and len(a.events) == 2 * len(b.events)
    assert_same_state(a, c, "at the end")
    assert_same_models([(models_a[k], models_c[k]) for k in models_a], opt_a, opt_c)
    kept = lambda ptrs: {k: v for k, v in ptrs.items() if "/queue_" not in k}          # noqa: E731 (a flush hands the queue's
    assert kept(pointers(c)) == kept(before)                                            #  buffers to its batch: by design)
    return a, b, c


def test_resume_ppo_single_agent(tmp_path):
    """N = 3 windows of 7 steps of 5 envs; the log's flush (the side-effect queue's) before the save; the test run at 140
    steps, in the second half."""
    flush = lambda trainer: trainer.runner.env.episode_log.flush()                     # noqa: E731
    a, b, c = resume_equals_straight(_ppo_single, 105, tmp_path, between=flush)
    assert [e[0] for e in a.events] == [35, 70, 105, 140, 175, 210]
    assert [e[2] for e in a.events] == [False, False, False, True, False, False] and any(e[1] for e in a.events)
    ea, ec = a.runner.env, c.runner.env
    rows_a, rows_c = ea.episode_log.rows(), ec.episode_log.rows()
    assert len(rows_a) >= 10 and rows_a.tobytes() == rows_c.tobytes()
    assert (rows_a["flags"] & _hip.LOG_JOINED).all()
    assert ea.episode_log.summary() == ec.episode_log.summary() and ea.episode_log.counters() == ec.episode_log.counters()
    ha, hc = ea.episode_history, ec.episode_history
    assert len(ha.entries()) >= 3 and ha.entries().tobytes() == hc.entries().tobytes() and ha.counters() == hc.counters()
    for i in range(len(ha.entries())):
        x, y = ha.history(i), hc.history(i)
        assert np.array_equal(x["board"], y["board"]) and np.array_equal(x["goals"], y["goals"])
    sa, sc = ea.level_schedule.stats(), ec.level_schedule.stats()
    assert all(np.array_equal(sa[k], sc[k]) for k in sa) and sa["episodes"].sum() >= 10
    ra, rc = a.test_runner.env.episode_run.results(), c.test_runner.env.episode_run.results()
    assert len(ra) == 7 and (ra["flags"] & _hip.RUN_WRITTEN).all() and ra.tobytes() == rc.tobytes()
    assert b.runner.env.level_schedule._fraction_sent not in (None, ea.level_schedule._fraction_sent)


def test_resume_ppo_multi_agent(tmp_path):
    a, b, c = resume_equals_straight(_ppo_multi, 105, tmp_path)
    assert a.host_visits == c.host_visits == 6 and int(a.runner.num_agent_steps.item()) == int(c.runner.num_agent_steps.item())


@pytest.mark.parametrize("capacity,replay_initial", ((40, 20), (120, 80)),
                         ids=("the ring wraps and the gate opens before the save", "the gate opens after the save"))
def test_resume_dqn_single_agent(tmp_path, capacity, replay_initial):
    """N = 12 steps of 5 envs under float64 shaped rewards and an epsilon that lets the model act; target updates at 35, 70
    and 105 steps, test runs at 50 and 100."""
    build = lambda torch: _dqn(torch, False, capacity, replay_initial)                 # noqa: E731
    a, b, c = resume_equals_straight(build, 60, tmp_path)
    pushed_at_save, opened_at_save = int(b.replay.idx.item()), b._gate_open
    print("pushes at the save", pushed_at_save, "gate", opened_at_save, "events", a.events, "tests", a.tests_run)
    if capacity == 40:
        assert pushed_at_save > capacity and opened_at_save         # the ring has wrapped, the gate is open
        assert a.tests_run == c.tests_run == [50, 100]
    else:
        assert not opened_at_save and a._gate_open and c._gate_open
        assert a.tests_run == c.tests_run == [100]
    second = [e for e in a.events if e[0] > 60]
    assert any(e[4] for e in second) and any(e[2] for e in second)  # a target update and an optimise in the second half
    assert a.host_visits == c.host_visits
    assert int(a.replay.status.item()) == 0


def test_resume_dqn_multi_agent(tmp_path):
    build = lambda torch: _dqn(torch, True, 60, 30)                                    # noqa: E731
    a, b, c = resume_equals_straight(build, 60, tmp_path)
    assert int(b.replay.idx.item()) > 60 and b._gate_open
    assert any(e[4] for e in a.events if e[0] > 60)


def _multi_env_stack(torch):
    """5 envs x 2 agents with everything a multi-agent env can carry: the training wrappers, a finished-episode queue, a
    switching schedule whose per-agent exit difficulty moves, the multi-agent log and history; driven by a
    MultiAgentDQNRunner with a fixed linear Q-model."""
    from safelife_amd import episode_history, episode_log, schedule
    from safelife_amd.levels import LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    from safelife_amd.runner import MultiAgentDQNRunner
    from tests.test_multi_wrap import TRAIN
    from tests.test_ppo_train_gpu import CHANNELS, _device_counts
    levels = []
    for name in ("multi_asym1", "multi_build_coop", "multi_build_compete"):
        levels += util.levels_from_trace(util.load_trace(name))
    pool = LevelPool(levels, counts_fn=_device_counts, n_agents=2, min_performance_fraction=0.0)
    sched = schedule.LevelSchedule(pool, [(0, 3), (3, len(levels) - 3)], mode="switching", p_switch=0.4, seed=21,
                                   min_performance_fraction=schedule.LinearSchedule([0, 150], [0.1, 1.0]))
    log = episode_log.MultiAgentEpisodeLog(pool, 5, 64, side_effect_weights={"life-green": 1.0})
    hist = episode_history.MultiAgentEpisodeHistory(pool, 5, [0, 3], 6)
    env = SafeLifeMultiAgentVectorEnv(pool, 5, auto_reset=True, time_limit=9, view_shape=(9, 9), output_channels=CHANNELS,
                                      policy_layout="uint8", with_obs=False, wrappers=dict(TRAIN),
                                      side_effects=dict(capacity=64, num_samples=4), level_schedule=sched, episode_log=log,
                                      episode_history=hist)
    torch.manual_seed(3)
    q = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(int(np.prod(env.policy_tensor.shape[2:])), 9)).to(env.device)
    return MultiAgentDQNRunner(env, q, seed=31)


def _drive(runner, steps):
    for _ in range(steps):
        runner.take_one_step(0.5)
        runner.num_steps += runner.env.num_envs     # (what collect() counts: the schedule reads it as the training step)
    runner.env.episode_log.flush()


def test_resume_multi_agent_env_with_schedule_log_history_and_wrappers(tmp_path):
    """The multi-agent env's own state (agents, per-agent level records under a schedule, wrapper state, the agents' queue
    records) and the multi-agent log's and history's, under a runner: 2 x 20 steps straight against 20, save, rebuild, load,
    20.  Compared behind the log's flush, as the single-agent stack is."""
    import torch
    from safelife_amd import checkpoint
    a, b = _multi_env_stack(torch), _multi_env_stack(torch)
    _drive(a, 20), _drive(a, 20), _drive(b, 20)
    checkpoint.save(tmp_path / "multi.data", b)
    c = _multi_env_stack(torch)
    before = pointers(c)
    checkpoint.load(tmp_path / "multi.data", c)
    assert pointers(c) == before and sorted(checkpoint.capture(c)) == [
        "root", "root.env", "root.env.base", "root.env.episode_history", "root.env.episode_log", "root.env.level_schedule"]
    assert_same_state(b, c, "behind the load")
    _drive(c, 20)
    torch.cuda.synchronize()
    assert_same_state(a, c, "at the end")
    la, lc = a.env.episode_log, c.env.episode_log
    assert len(la.rows()) >= 5 and la.rows().tobytes() == lc.rows().tobytes() and la.summary() == lc.summary()
    ha, hc = a.env.episode_history, c.env.episode_history
    assert len(ha.entries()) >= 1 and ha.entries().tobytes() == hc.entries().tobytes()
    assert a.env.level_schedule._fraction_sent == c.env.level_schedule._fraction_sent != b.env.level_schedule._fraction_sent
    assert not torch.equal(a.env.t["pool_agents"], _multi_env_stack(torch).env.t["pool_agents"])   # the schedule moved them


# ---------------------------------------------------------------------------------------------------------- load's edges

def _plain_env(B=64, pool=None, **kw):
    from safelife_amd.vector_env import SafeLifeVectorEnv
    from tests.test_ppo_train_gpu import _device_counts
    if pool is None:
        pool = util.pool_from_fixture("prune_still_25", _device_counts, n=8)[0]
    return SafeLifeVectorEnv(pool, B, auto_reset=True, view_shape=(15, 15), with_obs=False, time_limit=13, level_stride=3, **kw)


def _walk_env(env, steps, seed):
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        env.step(rng.integers(0, 9, env.num_envs).astype(np.int32))


def test_load_invalidates_the_goal_cache_and_the_env_steps_on(tmp_path):
    import torch
    from safelife_amd import checkpoint
    a, b, c = _plain_env(), _plain_env(), _plain_env()
    assert a.goal_cache_group > 0
    for env in (a, b, c):
        env.reset()
    _walk_env(a, 10, 3), _walk_env(b, 10, 3), _walk_env(c, 10, 99)
    assert c.goal_cache_flags().max() == 1                          # C runs on cached goal words of ITS boards
    checkpoint.save(tmp_path / "env.data", b)
    checkpoint.load(tmp_path / "env.data", c)
    assert c.goal_cache_flags().max() == 0 and c.steps_dispatched == 10
    _walk_env(a, 10, 4), _walk_env(c, 10, 4)
    torch.cuda.synchronize()
    assert_same_state(a, c, "plain envs")
    assert np.array_equal(a.numpy("reward"), c.numpy("reward")) and c.goal_cache_flags().max() == 1


def test_loading_into_other_objects_names_what_differs(tmp_path):
    import torch
    from safelife_amd import checkpoint
    from safelife_amd.levels import LevelPool
    from safelife_amd.replay import MultiAgentReplayBuffer, ReplayBuffer
    from tests.test_ppo_train_gpu import _device_counts
    env = _plain_env(8)
    env.reset()
    path = tmp_path / "env.data"
    checkpoint.save(path, env)
    with pytest.raises(ValueError, match="root: num_envs is 9 here and 8 in the file"):
        checkpoint.load(path, _plain_env(9))
    with pytest.raises(ValueError, match="root: env_offset is 8 here and 0 in the file"):
        checkpoint.load(path, _plain_env(8, env_offset=8))
    levels = list(env.pool.levels)
    with pytest.raises(ValueError, match="root: pool is '[0-9a-f]{40}' here and '[0-9a-f]{40}' in the file"):
        checkpoint.load(path, _plain_env(8, pool=LevelPool(levels[::-1], counts_fn=_device_counts)))
    kw = dict(multi_step=2, obs_shape=(3,), obs_dtype=torch.uint8, device=env.device)
    checkpoint.save(path, ReplayBuffer(40, 5, **kw))
    with pytest.raises(ValueError, match="root: capacity is 48 here and 40 in the file"):
        checkpoint.load(path, ReplayBuffer(48, 5, **kw))
    checkpoint.save(path, MultiAgentReplayBuffer(48, 4, 2, **kw))
    with pytest.raises(ValueError, match="root: n_agents is 1 here and 2 in the file"):
        checkpoint.load(path, MultiAgentReplayBuffer(48, 8, 1, **kw))


def test_a_tensor_altered_in_the_file_is_named(tmp_path):
    import torch
    from safelife_amd import checkpoint
    env = _plain_env(8)
    env.reset()
    _walk_env(env, 3, 1)
    path = tmp_path / "env.data"
    checkpoint.save(path, env)
    blob = torch.load(path, weights_only=True)
    blob["objects"]["root"]["tensors"]["rng"][5, 2] ^= 1 << 40
    torch.save(blob, path)
    with pytest.raises(ValueError, match="root/rng does not match its digest"):
        checkpoint.load(path, _plain_env(8))


def test_refusals_on_live_objects(tmp_path):
    import torch
    from safelife_amd import checkpoint, episode_run
    from safelife_amd.levels import LevelPool
    from safelife_amd.runner import PipelinedRunner, VectorRunner
    from safelife_amd.vector_env import SafeLifeVectorEnv
    from tests.test_ppo_train_gpu import CHANNELS, _device_counts
    policy = lambda obs: (torch.zeros(obs.shape[0], device=obs.device),                 # noqa: E731
                          torch.full((obs.shape[0], 9), 1.0 / 9, device=obs.device))
    kw = dict(output_channels=CHANNELS, policy_layout="uint8")
    with pytest.raises(ValueError, match=r"VectorRunner\(seed=None\).*build it with seed="):
        checkpoint.capture(VectorRunner(_plain_env(8, **kw), policy))

    pool = util.pool_from_fixture("prune_still_25", _device_counts, n=4)[0]
    run = episode_run.EpisodeRun(pool, 5, 7)
    test_env = SafeLifeVectorEnv(pool, 5, episode_run=run, view_shape=(15, 15), with_obs=False, time_limit=5, **kw,
                                 **run.env_arguments())
    runner = VectorRunner(test_env, policy, seed=3)
    checkpoint.capture(runner)
    run.start()
    with pytest.raises(ValueError, match=r"EpisodeRun is live \(mid test\)"):
        checkpoint.save(tmp_path / "x.data", runner)
    assert not os.path.exists(tmp_path / "x.data")
    assert len(runner.run_episodes()) == 7
    checkpoint.save(tmp_path / "x.data", runner)                    # between tests it is fine

    queued = _plain_env(8, side_effects=dict(capacity=64, num_samples=4))
    queued.reset()
    _walk_env(queued, 14, 2)
    batch = queued.side_effects_flush(overlap=True)
    with pytest.raises(ValueError, match=r"not joined: call env.side_effects_join\(\) first"):
        checkpoint.state_digest(queued)
    queued.side_effects_join()
    assert len(checkpoint.state_digest(queued)) >= 9 and len(batch) >= 1

    fresh = LevelPool(list(pool.levels), counts_fn=_device_counts, refreshable=True)
    refreshed = _plain_env(8, pool=fresh)
    refreshed.reset()
    refreshed.pool_stage([0, 2], [pool.levels[1], pool.levels[3]])
    with pytest.raises(ValueError, match=r"a pool write is staged: call env.pool_commit\(\) first"):
        checkpoint.capture(refreshed)
    assert refreshed.pool_commit()
    with pytest.raises(ValueError, match=r"LevelPool\(refreshable=True\) is not checkpointed"):
        checkpoint.capture(refreshed)

    sliced = _plain_env(128, slices=2, **kw)
    with pytest.raises(ValueError, match="PipelinedRunner is not checkpointed"):
        checkpoint.capture(PipelinedRunner(sliced, policy))


# ------------------------------------------------------------------------------------------------- Checkpointer end to end

def _model_case(kind, interval, keep, calls, **more):
    return dict(dict(kind=kind, num_envs=5, steps_per_env=7, interval=interval, keep=keep, reload_after=0, replay_initial=0,
                     test_interval=0, calls=calls, before=[], eps_testing=0.01), **more)


def test_checkpointer_with_a_ppo_trainer(tmp_path):
    """Interval 60 over batches of 35 steps: the saves and the files are the host model's, and load_latest() in fresh
    objects goes on to the straight run's bits."""
    import torch
    from safelife_amd import checkpoint, ppo
    from tests.test_ppo_train_gpu import SCHEDULE, _single_parts
    schedule = dict(SCHEDULE, steps_per_env=7)

    def build(directory):
        env, runner, model, opt, _none = _single_parts(torch, False)
        ck = checkpoint.Checkpointer(directory, interval=60, keep=2)
        return ppo.PPOTrainer(runner, model, opt, checkpointer=ck, record_events=True, **schedule), ck, model, opt

    case = _model_case("ppo", 60, 2, [140, 105])
    want_saves, want_left, _s, _e = ref.schedule_model(case, replay_restored=True)
    a, ck_a, model_a, opt_a = build(tmp_path / "a")
    a.train(140), a.train(105)
    assert ck_a.saved == want_saves == [35, 105, 140, 210, 245] and sorted(os.listdir(tmp_path / "a")) == want_left
    assert ck_a.root is a and ck_a.model is model_a and ck_a.optimizer is opt_a
    b, ck_b, _m, _o = build(tmp_path / "b")
    b.train(140)
    c, ck_c, model_c, opt_c = build(tmp_path / "b")
    assert ck_c.load_latest() == 140 and ck_c.last == 140 and c.num_steps == 140 and c.batches_done == 4
    c.train(105)
    assert ck_b.saved + ck_c.saved == want_saves and sorted(os.listdir(tmp_path / "b")) == want_left
    assert a.events == c.events
    assert_same_state(a, c, "ppo with a checkpointer")
    assert_same_models([(model_a, model_c)], opt_a, opt_c)


def test_checkpointer_with_a_dqn_trainer(tmp_path):
    """Interval 20, the replay gate in mid-run: nothing is saved in front of the gate; the pushes per step, which the host
    model needs, are read from the straight run's ring."""
    import torch
    from safelife_amd import checkpoint

    def build(directory):
        trainer, models, opt = _dqn(torch, False, 120, 30, tests=False)
        trainer.checkpointer = ck = checkpoint.Checkpointer(directory, interval=20, keep=3, root=trainer, model=models,
                                                            optimizer=opt)
        return trainer, ck, models, opt

    a, ck_a, models_a, opt_a = build(tmp_path / "a")
    pushes, collect = [], a.runner.collect

    def counting_collect(*args):
        step = collect(*args)
        pushes.append(int(a.replay.idx.item()) - sum(pushes))
        return step

    a.runner.collect = counting_collect
    a.train(60), a.train(60)
    case = _model_case("dqn", 20, 3, [60, 60], replay_initial=30, pushes=pushes, capacity=120)
    want_saves, want_left, _s, _e = ref.schedule_model(case, replay_restored=True)
    print(pushes, want_saves)
    assert ck_a.saved == want_saves and sorted(os.listdir(tmp_path / "a")) == want_left
    assert min(want_saves) >= 30 and len(want_saves) >= 5
    b, ck_b, _m, _o = build(tmp_path / "b")
    b.train(60)
    c, ck_c, models_c, opt_c = build(tmp_path / "b")
    assert ck_c.load_latest() == 60 and c.num_steps == 60 and c._gate_open
    c.train(60)
    assert ck_b.saved + ck_c.saved == want_saves and sorted(os.listdir(tmp_path / "b")) == want_left
    assert a.events == c.events
    assert_same_state(a, c, "dqn with a checkpointer")
    assert_same_models([(models_a[k], models_c[k]) for k in models_a], opt_a, opt_c)


# --------------------------------------------------------------------- files written in the middle of a train() call

def test_resume_from_a_file_written_inside_train_ppo(tmp_path):
    """The files an interrupted run actually has.  35-step batches, checkpoint interval 60, report interval 50, test interval
    100: checkpoint-105 is written by the loop (not by the end of train()) in the iteration in which a report AND a test
    run are due.  It holds the whole iteration -- the event, the test run's results -- and a fresh stack that loads it and
    trains on ends in the straight run's bits."""
    import torch
    from safelife_amd import checkpoint

    def build(directory):
        trainer, models, opt = _ppo_single(torch)
        trainer.report_interval, trainer.test_interval = 50, 100
        trainer.checkpointer = ck = checkpoint.Checkpointer(directory, interval=60, keep=10, root=trainer, model=models,
                                                            optimizer=opt)
        return trainer, ck, models, opt

    a, ck_a, models_a, opt_a = build(tmp_path / "a")
    a.train(210)
    case = _model_case("ppo", 60, 10, [210], reload_after=-1)
    want_saves, want_left, _s, _e = ref.schedule_model(case)
    assert ck_a.saved == want_saves == [35, 105, 175, 210] and sorted(os.listdir(tmp_path / "a")) == want_left
    assert a.events[2] == (105, True, True) and [e[0] for e in a.events if e[2]] == [105, 210]
    b, ck_b, _m, _o = build(tmp_path / "b")
    b.train(210)
    c, ck_c, models_c, opt_c = build(tmp_path / "b")
    assert ck_c.load("checkpoint-105.data") == 105 and ck_c.last == 105
    assert c.num_steps == 105 and c.batches_done == 3 and c.events == a.events[:3]
    played = c.test_runner.env.episode_run.results()
    assert len(played) == 7 and (played["flags"] & _hip.RUN_WRITTEN).all()      # the file is from BEHIND the test run
    c.train(105)
    assert ck_c.saved == [175, 210]
    for t in (a, c):
        t.runner.env.episode_log.flush()
    torch.cuda.synchronize()
    assert c.events == a.events and len(a.events) == 6
    assert_same_state(a, c, "ppo, resumed from a file written inside train()")
    assert_same_models([(models_a["model"], models_c["model"])], opt_a, opt_c)
    assert a.runner.env.episode_log.rows().tobytes() == c.runner.env.episode_log.rows().tobytes()


def test_resume_from_a_file_written_inside_train_dqn(tmp_path):
    """DQN on 5 envs, checkpoint interval 20, test interval 55: checkpoint-55 is written by the loop in the iteration in
    which a test run is due.  The file carries the loop's report flag, so the resumed train() call goes on where the
    interrupted one stood: events, test steps and every bit of state equal the straight run's."""
    import torch
    from safelife_amd import checkpoint

    def build(directory):
        trainer, models, opt = _dqn(torch, False, 120, 30)
        trainer.test_interval = 55
        trainer.checkpointer = ck = checkpoint.Checkpointer(directory, interval=20, keep=10, root=trainer, model=models,
                                                            optimizer=opt)
        return trainer, ck, models, opt

    a, ck_a, models_a, opt_a = build(tmp_path / "a")
    pushes, collect = [], a.runner.collect

    def counting_collect(*args):
        step = collect(*args)
        pushes.append(int(a.replay.idx.item()) - sum(pushes))
        return step

    a.runner.collect = counting_collect
    a.train(120)
    case = _model_case("dqn", 20, 10, [120], reload_after=-1, replay_initial=30, pushes=pushes, capacity=120,
                       test_interval=55)
    want_saves, want_left, want_tests, _e = ref.schedule_model(case)
    print(pushes, want_saves, want_tests, a.events)
    assert ck_a.saved == want_saves and sorted(os.listdir(tmp_path / "a")) == want_left and a.tests_run == want_tests
    assert 55 in want_saves[:-1] and 55 in want_tests
    b, ck_b, _m, _o = build(tmp_path / "b")
    b.train(120)
    c, ck_c, models_c, opt_c = build(tmp_path / "b")
    assert ck_c.load("checkpoint-55.data") == 55 and c.num_steps == 55 and c._in_train
    assert c.events == a.events[:11] and c.tests_run == [55] and c.epsilon == 0.01
    c.train(65)
    assert c.events == a.events and c.tests_run == a.tests_run and not c._in_train
    assert ck_c.saved == [s for s in want_saves if s > 55]
    assert_same_state(a, c, "dqn, resumed from a file written inside train()")
    assert_same_models([(models_a[k], models_c[k]) for k in models_a], opt_a, opt_c)
