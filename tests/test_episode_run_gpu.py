"""
Evaluation runs on the device (safelife_amd/episode_run.py, csrc/sl_episode_run.hip) against the numpy restatement
(tests/episode_run_ref.py), bit for bit: the harvest kernels on synthetic record streams, the tickets kernel on a scrambled
queue, and whole runs of a ``SafeLifeVectorEnv`` and a ``SafeLifeMultiAgentVectorEnv`` against a plain auto-reset env dealt the
same levels and given the same actions.
"""
import ctypes as C

import numpy as np
import pytest

from safelife_amd import _hip, episode_log, episode_run
from tests import episode_log_ref as er
from tests import episode_run_ref as rr
from tests import util

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


class DeviceRun(object):
    """The run's device state without an env: what ``EpisodeRun._attach`` allocates, and the entry points."""

    def __init__(self, B, G, env_offset, N, L, A=1, base_episode=None):
        torch = _torch()
        dev = self.dev = _hip.device()
        self.B, self.A, self.N = B, A, N
        t = self.t = dict(active=torch.zeros(B, dtype=torch.uint8, device=dev),
                          played=torch.zeros(B, dtype=torch.int32, device=dev),
                          base_episode=torch.zeros(B, dtype=torch.int32, device=dev),
                          counters=torch.full((4,), -77, dtype=torch.int32, device=dev),
                          results=torch.full((N, 8), 0x5a5a5a5a, dtype=torch.int32, device=dev),
                          agent_results=torch.full((N, A, 4), 0x5a5a5a5a, dtype=torch.int32, device=dev),
                          side_effects=torch.full((N, 2), 3.5, dtype=torch.float64, device=dev))
        s = self.struct = _hip.EpisodeRun()
        s.B, s.G, s.env_offset, s.N, s.L, s.n_agents = B, G, env_offset, N, L, A
        for name in t:
            setattr(s, name, t[name].data_ptr())
        self.lib = _hip.lib()
        scalars = np.zeros((B, 16), np.int32)
        if base_episode is not None:
            scalars[:, _hip.SCALAR_COLS["episode_idx"]] = base_episode
        self.scalars = torch.from_numpy(scalars).to(dev)
        _hip.check(self.lib.slhip_episode_run_start(C.byref(s), _hip.ptr(self.scalars), _hip.current_stream_ptr()))
        self.steps = 0

    def harvest(self, records):
        """records: ``rr.STEP_OUT`` [B, A] -> the masked records as the kernel left them."""
        torch = _torch()
        out = torch.from_numpy(np.ascontiguousarray(records).view(np.int32).reshape(self.B, self.A, 4).copy()).to(self.dev)
        self.steps += 1
        entry = self.lib.slhip_episode_run_harvest_multi if self.A > 1 else self.lib.slhip_episode_run_harvest
        _hip.check(entry(C.byref(self.struct), _hip.ptr(out), self.steps, _hip.current_stream_ptr()))
        return out.cpu().numpy().view(rr.STEP_OUT).reshape(self.B, self.A)

    def state(self):
        t = self.t
        c = t["counters"].cpu().numpy()
        return dict(active=t["active"].cpu().numpy(), played=t["played"].cpu().numpy(),
                    counters=dict(completed=int(c[0]), in_progress=int(c[1]), env_steps=int(c[2])),
                    results=t["results"].cpu().numpy().view(rr.ROW).reshape(-1),
                    agent_results=t["agent_results"].cpu().numpy().view(rr.AGENT).reshape(self.N, self.A))


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_state_equals_model(d, m, where):
    s = d.state()
    assert np.array_equal(s["active"], m.active), where
    assert np.array_equal(s["played"], m.played), where
    assert s["counters"] == m.counters(), where
    assert _same_bytes(s["results"], m.results), where
    assert _same_bytes(s["agent_results"], m.agent_results), where


def _record_stream(rng, B, A, steps, sure_from):
    """Per-agent records the way the envs write them: an agent that is done stays done (with its accumulators) until all
    agents of its env are, and the env starts over on the next step.  From step `sure_from` on every agent finishes at once."""
    gone = np.zeros((B, A), bool)
    length = np.zeros((B, A), np.int32)
    total = np.zeros((B, A), np.float32)
    for t in range(steps):
        out = np.zeros((B, A), rr.STEP_OUT)
        p = 1.0 if t >= sure_from else 0.35
        for e in range(B):
            if gone[e].all():
                gone[e], length[e], total[e] = False, 0, 0
            for a in range(A):
                if not gone[e, a]:
                    r = np.float32(rng.integers(-8, 9) * 0.25)
                    length[e, a] += 1
                    total[e, a] += r
                    out[e, a]["reward"] = r
                    if rng.random() < p:
                        gone[e, a] = True
                        out[e, a]["success"], out[e, a]["times_up"] = rng.integers(0, 2), rng.integers(0, 2)
                out[e, a]["done"] = gone[e, a]
                out[e, a]["episode_reward"], out[e, a]["episode_length"] = total[e, a], length[e, a]
        yield out


STEPS, SURE_FROM = 40, 24


def _harvest_case(B, A, N, G=None, env_offset=0, L=7):
    G = B if G is None else G
    rng = np.random.default_rng(1000 * B + 10 * A + N % 7)
    base = rng.integers(0, 50, B).astype(np.int32)
    d, m = DeviceRun(B, G, env_offset, N, L, A, base), rr.RunModel(B, G, env_offset, N, L, A, base)
    _assert_state_equals_model(d, m, "start")
    frozen, some = None, set()
    for t, out in enumerate(_record_stream(rng, B, A, STEPS, SURE_FROM)):
        n_done = out["done"].astype(bool).sum(axis=1)
        some |= {"none" if n == 0 else "all" if n == A else "some" for n in n_done.tolist()}
        # the records of the envs that are retired, or were never active, hold garbage before the launch
        out[m.active == 0] = np.frombuffer(b"\x7f" * 16, rr.STEP_OUT)[0]
        got = d.harvest(out)
        want = m.step(out)
        assert _same_bytes(got, want), t
        _assert_state_equals_model(d, m, t)
        if t == STEPS - 11:
            assert m.finished(), "the stream was meant to end the run by now"
            frozen = (d.state(), m.counters())
    assert some >= ({"none", "all", "some"} if A > 1 else {"none", "all"})
    # a finished run stepped ten more times changes nothing but the records, which all come out zero
    end = d.state()
    assert _same_bytes(end["results"], frozen[0]["results"]) and _same_bytes(end["agent_results"], frozen[0]["agent_results"])
    assert end["counters"] == frozen[0]["counters"] == frozen[1] and not end["active"].any()
    assert (got.view(np.uint8) == 0).all()
    mine = np.array([env_offset <= t % G < env_offset + B for t in range(N)])
    assert np.array_equal(m.writes, mine.astype(np.int64)) and m.completed == mine.sum()   # every ticket filed once
    return d, m


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("which", ["N<B", "N==B", "N==3B-1"])
def test_harvest_equals_the_restatement(B, which):
    N = {"N<B": max(1, B - 3), "N==B": B, "N==3B-1": 3 * B - 1}[which]
    _harvest_case(B, 1, N)


@pytest.mark.parametrize("B,A", [(1, 1), (63, 2), (65, 3), (64, 8)])
@pytest.mark.parametrize("which", ["N<B", "N==B", "N==3B-1"])
def test_harvest_multi_equals_the_restatement(B, A, which):
    N = {"N<B": max(1, B - 3), "N==B": B, "N==3B-1": 3 * B - 1}[which]
    _harvest_case(B, A, N)


def test_harvest_of_a_shard():
    """envs 70..134 of 200: the shard files only its own tickets."""
    d, m = _harvest_case(65, 1, 3 * 200 - 1, G=200, env_offset=70, L=11)
    rows = d.state()["results"]
    mine = (rows["flags"] & 1) != 0
    assert mine.sum() == 65 * 3 and set((np.nonzero(mine)[0] % 200).tolist()) == set(range(70, 135))


def test_tickets_of_a_scrambled_queue():
    torch = _torch()
    B, G, off, N, L = 65, 200, 70, 530, 11
    rng = np.random.default_rng(8)
    base = rng.integers(0, 90, B).astype(np.int32)
    d, m = DeviceRun(B, G, off, N, L, 1, base), rr.RunModel(B, G, off, N, L, 1, base)
    # every (env, episode) once: from two episodes before the run to phantom episodes past the env's last ticket, and envs
    # that are none of the batch's
    entries = [(e, int(base[e]) + k) for e in range(B) for k in range(-2, 6)] + [(-1, 3), (B, 4), (B + 7, 0)]
    entries = [entries[i] for i in rng.permutation(len(entries))]
    cap = len(entries) + 9
    rec = np.zeros((cap, 8), np.int32)
    rec[:len(entries), 0], rec[:len(entries), 3] = np.array(entries).T
    rec[len(entries):, 0], rec[len(entries):, 3] = 3, base[3]          # (stale slots past the count: a real ticket's entry)
    want = np.array([m.ticket(e, ep) for e, ep in entries] + [-1] * 9, np.int32)
    assert (want >= 0).sum() == sum(len(rr.tickets_of_env(off + e, G, N)) for e in range(B)) and (want < 0).sum() > 2 * B
    K = _hip.SL_SE_MAX_KEYS
    keys = rng.choice(np.array([0xFFFF, 1, 2, 3, 40, 41], np.uint16), (cap, K))
    scores = rng.random((cap, K, 2))
    scores[rng.random((cap, K, 2)) < 0.1] = np.nan
    n_cells = rng.integers(0, 30, (cap, K)).astype(np.int32)
    n_cells[::17, 0] = -1
    weights = [(1, 1.0), (3, 0.5), (40, 2.0), (1, 0.25)]
    w = _hip.LogWeights()
    w.n = len(weights)
    for j, (cell, weight) in enumerate(weights):
        w.cell[j], w.weight[j] = cell, weight
    dev = d.dev
    q = _hip.EpisodeQueue()
    count = torch.tensor([len(entries)], dtype=torch.int32, device=dev)
    records = torch.from_numpy(rec).to(dev)
    q.capacity, q.env_base, q.count, q.records = cap, 0, count.data_ptr(), records.data_ptr()
    tk = torch.full((cap,), 12345, dtype=torch.int32, device=dev)
    # tickets alone
    _hip.check(d.lib.slhip_episode_run_tickets(C.byref(d.struct), C.byref(q), _hip.ptr(tk), None, None, None, None,
                                               _hip.current_stream_ptr()))
    assert np.array_equal(tk.cpu().numpy(), want)
    assert (d.t["side_effects"].cpu().numpy() == 0).all()
    # ... and with the scores: the totals of slhip_episode_log_join, by ticket
    ds, dk, dn = torch.from_numpy(scores).to(dev), torch.from_numpy(keys.view(np.int16)).to(dev), torch.from_numpy(n_cells).to(dev)
    _hip.check(d.lib.slhip_episode_run_tickets(C.byref(d.struct), C.byref(q), _hip.ptr(tk), _hip.ptr(ds), _hip.ptr(dk),
                                               _hip.ptr(dn), C.byref(w), _hip.current_stream_ptr()))
    assert np.array_equal(tk.cpu().numpy(), want)
    got = d.t["side_effects"].cpu().numpy()
    expect, scored = np.zeros((N, 2)), np.zeros(N, bool)
    for i, t in enumerate(want):
        if t >= 0:
            expect[t], scored[t] = er.entry_totals(weights, keys[i], scores[i], n_cells[i]), True
    assert er.same_floats(got, expect)
    flags = d.state()["results"]["flags"]
    assert np.array_equal((flags & _hip.RUN_SCORED) != 0, scored) and np.isnan(got).any()
    # a count beyond the capacity reads the capacity
    count.fill_(cap + 100)
    _hip.check(d.lib.slhip_episode_run_tickets(C.byref(d.struct), C.byref(q), _hip.ptr(tk), None, None, None, None,
                                               _hip.current_stream_ptr()))
    assert np.array_equal(tk.cpu().numpy()[:len(entries)], want[:len(entries)]) and (tk.cpu().numpy()[len(entries):] == 3 + off).all()


# ------------------------------------------------------------------------------------------------------------- end to end

B_E2E, L_E2E, LIMIT = 65, 12, 12
N_E2E = 3 * B_E2E - 1
WEIGHTS = {"life-green": 1.0, "life-red": 0.5, "crate-gray": 2.0, "life-yellow": 1.0}
ENV_KW = dict(time_limit=LIMIT, view_shape=(15, 15))


def _single(with_log=False, **kw):
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=L_E2E)[0]
    run = episode_run.EpisodeRun(pool, B_E2E, N_E2E)
    extra = dict(kw)
    if with_log:
        extra["episode_log"] = episode_log.EpisodeLog(pool, B_E2E, 1024, episode_type="benchmark",
                                                      side_effect_weights=WEIGHTS)
        extra["side_effects"] = dict(capacity=N_E2E + B_E2E, num_samples=8)
    env = SafeLifeVectorEnv(pool, B_E2E, episode_run=run, **ENV_KW, **extra, **run.env_arguments())
    plain = SafeLifeVectorEnv(pool, B_E2E, **ENV_KW, **run.env_arguments())
    return pool, run, env, plain


MB, MA, MLIMIT = 21, 2, 9
MN = 3 * MB - 1
MULTI_KW = dict(time_limit=MLIMIT, view_shape=(7, 11), output_channels=tuple(range(12)) + (25, 26, 27),
                policy_layout="uint8", with_obs=False)


def _multi_pool():
    from safelife_amd import levels
    from tests.test_level_schedule_multi_gpu import _counts, _families
    return levels.LevelPool([lv for fam in _families() for lv in fam], counts_fn=_counts, n_agents=MA,
                            min_performance_fraction=0.0)


def _multi(with_log=False):
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    pool = _multi_pool()
    run = episode_run.EpisodeRun(pool, MB, MN, n_agents=MA)
    extra = {}
    if with_log:
        extra["episode_log"] = episode_log.MultiAgentEpisodeLog(pool, MB, 256, episode_type="benchmark",
                                                                side_effect_weights=WEIGHTS)
        extra["side_effects"] = dict(capacity=MN + MB, num_samples=8)
    env = SafeLifeMultiAgentVectorEnv(pool, MB, episode_run=run, **MULTI_KW, **extra, **run.env_arguments())
    plain = SafeLifeMultiAgentVectorEnv(pool, MB, **MULTI_KW, **run.env_arguments())
    return pool, run, env, plain


def _out(env, B, A):
    return env.t["out"].cpu().numpy().view(rr.STEP_OUT).reshape(B, A).copy()


def _view(env):
    t = env.obs if env.obs is not None else env.policy_tensor
    return t.cpu().numpy()


def _against_a_plain_env(run, env, plain, B, A, N, limit, actions):
    """Steps both envs with the same actions: the run's active envs report what the plain env does at every step, the retired
    ones nothing; the result table is what the plain env's records imply under the deal."""
    base = getattr(env, "base", env)
    pbase = getattr(plain, "base", plain)
    L = run.n_slots
    assert run.finished()                               # (nothing started yet)
    run.start()
    plain.reset()
    assert np.array_equal(base.numpy("level_idx"), np.arange(B) % L)
    assert np.array_equal(_view(env), _view(plain))
    m = rr.RunModel(B, B, 0, N, L, A, base.numpy("episode_idx"))
    for t in range(len(actions)):
        active = run.active.cpu().numpy().astype(bool)
        assert np.array_equal(active, m.active.astype(bool)), t
        slot_before, episode_before = pbase.numpy("level_idx").copy(), pbase.numpy("episode_idx").copy()
        env.step(actions[t])
        plain.step(actions[t])
        got, want = _out(env, B, A), _out(plain, B, A)
        assert _same_bytes(got[active], want[active]), t
        assert (got[~active].view(np.uint8) == 0).all(), t
        assert np.array_equal(_view(env)[active], _view(plain)[active]), t
        for name in ("board", "level_idx", "episode_idx", "rng"):
            assert np.array_equal(base.numpy(name), pbase.numpy(name)), (t, name)       # (the step itself is untouched)
        masked = m.step(want)
        assert _same_bytes(got, masked), t
        ended = active & want["done"].astype(bool).all(axis=1)
        for e in np.nonzero(ended)[0]:
            row = m.results[e + B * (m.played[e] - 1)]
            assert (row["slot"], row["episode_idx"]) == (slot_before[e], episode_before[e]), (t, e)
        assert run.finished() == m.finished(), t
        assert run.counters() == m.counters(), t
    assert m.finished() and m.results["step"].max() <= 3 * limit < m.steps and (m.writes == 1).all()
    res = run.results()
    for name in rr.ROW.names:
        assert np.array_equal(res[name], m.results[name]), name
    assert _same_bytes(np.ascontiguousarray(res["agents"]), m.agent_results)
    assert (res["flags"] == _hip.RUN_WRITTEN).all() and res["step"].max() <= 3 * limit
    assert np.array_equal(res["slot"], np.arange(N) % L) and np.array_equal(res["env"], np.arange(N) % B)
    dev = run.results_device()
    assert tuple(dev["results"].shape) == (N, 8) and tuple(dev["agent_results"].shape) == (N, A, 4)
    return m


def test_a_run_equals_a_plain_env_dealt_the_same_levels():
    pool, run, env, plain = _single()
    actions = np.random.default_rng(31).integers(0, 9, (3 * LIMIT + 3, B_E2E)).astype(np.int32)
    _against_a_plain_env(run, env, plain, B_E2E, 1, N_E2E, LIMIT, actions)


def test_a_multi_agent_run_equals_a_plain_env_dealt_the_same_levels():
    from tests.test_training_batch_multi_gpu import ExactPolicy
    torch = _torch()
    pool, run, env, plain = _multi()
    # two agents in three take the policy's favourite, towards an exit they see, so that agents leave one ahead of the other
    policy = ExactPolicy(torch, tuple(plain.policy_tensor.shape[2:]), plain.device)
    rng = np.random.default_rng(17)
    probe = _multi()[3]
    probe.reset()
    actions = []
    for t in range(3 * MLIMIT + 3):
        o = probe.policy_tensor
        fav = policy(o.view((-1,) + tuple(o.shape[2:])))[1].argmax(dim=1).view(MB, MA).cpu().numpy().astype(np.int32)
        a = np.where(rng.random((MB, MA)) < 0.67, fav, rng.integers(0, 9, (MB, MA)).astype(np.int32)).astype(np.int32)
        probe.step(a)
        actions.append(a)
    _against_a_plain_env(run, env, plain, MB, MA, MN, MLIMIT, np.array(actions))


def _logged_run(run, env, B, A, N, limit, seed):
    """One whole run with actions masked by the run, three steps past its end, the flush -> batch."""
    rng = np.random.default_rng(seed)
    run.start()
    steps = 0
    while not run.finished():
        a = rng.integers(0, 9, (B, A) if A > 1 or hasattr(env, "base") else (B,)).astype(np.int32)
        act = run.active.cpu().numpy().astype(np.int32)
        env.step(a * (act[:, None] if a.ndim == 2 else act))
        steps += 1
        assert steps <= 3 * limit
    for _ in range(3):
        env.step(np.zeros_like(a))
    return env.episode_log.flush()


def _check_logged(run, env, B, A, N, limit):
    log = env.episode_log
    base = getattr(env, "base", env)
    batch = _logged_run(run, env, B, A, N, limit, 3)
    L = run.n_slots
    c = log.counters()
    assert c["n_rows"] == c["episodes"] == c["summarised"] == N and batch.dropped() == 0
    rows = log.rows()
    tickets = rows["env"] + B * rows["episode_idx"]                 # (the envs' episode counters started at 0)
    assert sorted(tickets.tolist()) == list(range(N))               # exactly the N tickets: none from a phantom episode
    assert (rows["flags"] & _hip.LOG_JOINED).all() and np.array_equal(rows["level"], tickets % L)
    se = run.side_effects(batch).cpu().numpy()
    assert er.same_floats(se[tickets], rows["side_effects"])        # the log's joined totals, row for row
    res = run.results()
    assert (res["flags"] == _hip.RUN_WRITTEN | _hip.RUN_SCORED).all()
    tk = run.tickets(batch).cpu().numpy()
    n = len(batch)
    assert n >= N and sorted(tk[tk >= 0].tolist()) == list(range(N)) and (tk[n:] == -1).all()
    key = "benchmark/length" if A == 1 and not hasattr(env, "base") else "benchmark/agent0-length"
    first = log.summary()
    assert key in first and (log._state()[1] > 0).any()
    # validation does this every test_interval: the summaries start over, the same slots are replayed
    log.reset_summary()
    assert not log._state()[1].any() and not log._state()[2].any() and not log._state()[3].any()
    assert log.counters() == c
    batch2 = _logged_run(run, env, B, A, N, limit, 3)
    rows2 = log.rows(first=N)
    base_episode = run.t["base_episode"].cpu().numpy()
    assert (base_episode > 0).all() and len(rows2) == N and batch2.dropped() == 0
    t2 = rows2["env"] + B * (rows2["episode_idx"] - base_episode[rows2["env"]])
    assert sorted(t2.tolist()) == list(range(N)) and np.array_equal(rows2["level"], t2 % L)
    counts = log._state()[1]
    assert counts.max() == N                                        # every row of the second run, none of the first
    assert np.array_equal(run.results()["slot"], np.arange(N) % L)
    assert base.numpy("episode_idx").min() > base_episode.min()


def test_a_run_with_a_log_and_side_effects():
    pool, run, env, plain = _single(with_log=True)
    _check_logged(run, env, B_E2E, 1, N_E2E, LIMIT)


def test_a_multi_agent_run_with_a_log_and_side_effects():
    pool, run, env, plain = _multi(with_log=True)
    _check_logged(run, env, MB, MA, MN, MLIMIT)


# ------------------------------------------------------------------------------------------------------------- the runners

def _uniform_policy(torch):
    def policy(obs):
        n = obs.shape[0]
        return torch.zeros(n, device=obs.device), torch.full((n, 9), 1.0 / 9.0, device=obs.device)
    return policy


def _vector_runner(N=N_E2E):
    from safelife_amd.runner import VectorRunner
    from safelife_amd.vector_env import SafeLifeVectorEnv
    torch = _torch()
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=L_E2E)[0]
    run = episode_run.EpisodeRun(pool, B_E2E, N)
    env = SafeLifeVectorEnv(pool, B_E2E, episode_run=run, policy_layout="uint8", with_obs=False, **ENV_KW,
                            **run.env_arguments())
    gen = torch.Generator(device=env.device).manual_seed(11)
    return run, env, VectorRunner(env, _uniform_policy(torch), generator=gen)


def _same_tables(a, b):
    return all(np.array_equal(a[name], b[name]) for name in a.dtype.names if name != "step") and np.array_equal(
        a["step"], b["step"])


def test_vector_runner_run_episodes():
    tables = []
    for poll in (1, 16):
        run, env, runner = _vector_runner()
        runner.num_steps = 1234
        res = runner.run_episodes(poll_every=poll)
        assert runner.num_steps == 1234 and run.finished() and (res["flags"] & 1).all()
        assert run.steps % poll == 0 and run.steps <= 3 * LIMIT + 15
        step = runner.take_one_step()                               # every env is retired: action 0, nothing reported
        assert not step.actions.cpu().numpy().any() and not step.done.cpu().numpy().any()
        tables.append(res)
    assert _same_tables(*tables)
    with pytest.raises(ValueError, match="built for %d episodes" % N_E2E):
        runner.run_episodes(num_episodes=5)
    # envs that never become active carry action 0 from the first step on
    run, env, runner = _vector_runner(N=B_E2E - 5)
    run.start()
    runner._started = True
    acts = np.array([runner.take_one_step().actions.cpu().numpy() for _ in range(4)])
    assert not acts[:, B_E2E - 5:].any() and acts[:, :B_E2E - 5].any()


def _multi_runner(N=MN):
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    from safelife_amd.runner import MultiAgentRunner
    from tests.test_training_batch_multi_gpu import ExactPolicy
    torch = _torch()
    pool = _multi_pool()
    run = episode_run.EpisodeRun(pool, MB, N, n_agents=MA)
    env = SafeLifeMultiAgentVectorEnv(pool, MB, episode_run=run, **MULTI_KW, **run.env_arguments())
    policy = ExactPolicy(torch, tuple(env.policy_tensor.shape[2:]), env.device)
    return run, env, MultiAgentRunner(env, policy, seed=3)


def test_multi_agent_runner_run_episodes():
    tables = []
    for poll in (1, 16):
        run, env, runner = _multi_runner()
        runner.num_steps = 77
        res = runner.run_episodes(poll_every=poll)
        assert runner.num_steps == 77 and run.finished() and (res["flags"] & 1).all()
        step = runner.take_one_step()
        assert not step.actions.cpu().numpy().any() and not step.active.cpu().numpy().any()
        tables.append(res)
    assert _same_tables(*tables)
    # no rollout row for an env that is not active in the run
    run, env, runner = _multi_runner(N=MB - 4)
    run.start()
    runner._started = True
    runner._run_begins()
    batch = runner.gen_training_batch(4)
    active = runner.rollout.active.cpu().numpy().reshape(4, MB, MA)
    assert not active[:, MB - 4:].any() and active[:, :MB - 4].any()
    assert len(batch.actions) == int(active.sum())


def test_dqn_runner_with_epsilon_zero_is_the_argmax_run():
    from safelife_amd.runner import DQNRunner
    from safelife_amd.vector_env import SafeLifeVectorEnv
    torch = _torch()
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=L_E2E)[0]
    tables = []
    for how in ("runner", "argmax"):
        run = episode_run.EpisodeRun(pool, B_E2E, N_E2E)
        env = SafeLifeVectorEnv(pool, B_E2E, episode_run=run, policy_layout="uint8", with_obs=False, **ENV_KW,
                                **run.env_arguments())
        g = torch.Generator(device="cpu").manual_seed(5)
        w = torch.randint(-3, 4, (int(np.prod(env.policy_tensor.shape[1:])), 9), generator=g).to(torch.float32).to(env.device)
        q_model = lambda obs: obs.reshape(obs.shape[0], -1).to(torch.float32) @ w  # noqa: E731  (integers: exact in float32)
        if how == "runner":
            tables.append(DQNRunner(env, q_model, seed=9).run_episodes(epsilon=0.0, poll_every=4))
        else:
            run.start()
            while not run.finished():
                a = q_model(env.policy_tensor).argmax(dim=1).to(torch.int32) * run.active
                env.step(a)
            tables.append(run.results())
    assert _same_tables(tables[0], tables[1]) and (tables[0]["flags"] & 1).all()
