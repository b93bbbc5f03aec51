"""
The multi-agent episode log without a GPU: the ABI of the four slhip_episode_log_*_multi entry points, the host restatement
(tests/episode_log_multi_ref.py) against what the reference's SafeLifeLogger logged for episodes of 1, 2, 3 and 8 agents
(tests/golden/episode_log_multi_cases.npz, written by tests/golden/make_golden_episode_log_multi.py), and the argument checks
of safelife_amd.episode_log.MultiAgentEpisodeLog and of SafeLifeMultiAgentVectorEnv(episode_log=...).

Per-episode fields (training_steps, reward_possible, reward_needed and per-agent reward_frac and score, the row's
side_effects_frac) equal the fixture BIT FOR BIT.  The running summaries and the run summary equal it within a measured
tolerance, for the reasons tests/test_episode_log_host.py gives for the single-agent log:

* SUMMARY_MEASURED = 1.1368683772161603e-12: the largest |restatement - reference| over every summary_stats value after every
  episode of every case (1506 episodes, up to 16 names x 4 keys): the reference's weight p (1 - p**n) / (1 - p) against the
  recurrence w <- p (1 + w).  With polyak 1 and 0 the weights are exact and the deviation is 0, which the test asserts.
* RUN_MEASURED = 1.7053025658242404e-13: the same for the twelve run-summary numbers, where they are finite: one chain in
  (row, agent) order here against numpy's pairwise sums over the [N, A] arrays.

The bounds of the tests are twice the measured values, on the host here and on the device in
tests/test_episode_log_multi_gpu.py (where the kernels must equal the restatement bit for bit, so the same bound holds).

The fixture also records that a multi-agent run never summarises side_effects: combined_score() returns a shape-(1,)
fraction, which fails np.isscalar, so the key reaches neither summary_stats nor wandb (c_se_isscalar, c_se_in_wandb,
c_se_summarised are all False, and wandb saw exactly four keys per distinct agent name of the level beside
reward_frac_needed and the two counters).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from safelife_amd import _hip, episode_log, levels
from tests import episode_log_multi_ref as emr
from tests import episode_log_ref as er
from tests import util
from tests.test_episode_log_host import deviation

SUMMARY_MEASURED = 1.1368683772161603e-12
RUN_MEASURED = 1.7053025658242404e-13
SUMMARY_BOUND, RUN_BOUND = 2 * SUMMARY_MEASURED, 2 * RUN_MEASURED

NAMES = ("slhip_episode_log_harvest_multi", "slhip_episode_log_join_multi", "slhip_episode_log_summaries_multi",
         "slhip_episode_log_run_summary_multi")
CASES = ["a1_polyak1", "a2_nosuccess", "a2_polyak099", "a3_polyak0", "a8_polyak099"]


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "episode_log_multi_cases.npz")) as d:
        return {k: d[k] for k in d.files}


# ------------------------------------------------------------------------------------------------------------- the ABI

def test_symbols_and_version():
    lib = _hip.lib()
    header = open(os.path.join(util.REPO, "include", "safelife_hip.h")).read()
    for name in NAMES:
        assert name in _hip.EXPORTS and hasattr(lib, name) and name + "(" in header
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13


def test_layouts_match_the_header(tmp_path):
    """The ctypes mirror of sl_episode_log_multi and numpy's row dtypes against gcc's offsetof / sizeof; the single-agent
    structs keep their sizes."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "safelife_hip.h"', 'int main(void) {',
             'printf("consts %d %d %d %d %d %d\\n", SL_LOG_MAX_NAMES, SL_LOG_NO_NAME, SL_LOG_MULTI_KEYS, SL_MAX_AGENTS, '
             'SL_LOG_ROW_MULTI_BYTES(1), SL_LOG_ROW_MULTI_BYTES(8));',
             'printf("sizes %zu %zu %zu %zu %zu\\n", sizeof(sl_episode_log_multi), sizeof(sl_episode_log_row_multi), '
             'sizeof(sl_episode_log_agent), sizeof(sl_episode_log), sizeof(sl_episode_log_row));']
    want = ["consts %d %d %d %d %d %d" % (_hip.LOG_MAX_NAMES, _hip.LOG_NO_NAME, len(_hip.LOG_MULTI_KEYS), _hip.SL_MAX_AGENTS,
                                          _hip.log_row_multi_bytes(1), _hip.log_row_multi_bytes(8)),
            "sizes %d 64 40 104 96" % C.sizeof(_hip.EpisodeLogMulti)]
    for name, ctype in _hip.EpisodeLogMulti._fields_:
        lines.append('printf("%s %%zu %%zu\\n", offsetof(sl_episode_log_multi, %s), sizeof(((sl_episode_log_multi *)0)->%s));'
                     % (name, name, name))
        want.append("%s %d %d" % (name, getattr(_hip.EpisodeLogMulti, name).offset, C.sizeof(ctype)))
    dt = emr.row_dtype(3)
    for cname, sub in (("sl_episode_log_row_multi", dt), ("sl_episode_log_agent", dt["agents"].base)):
        for name in sub.names:
            if name == "agents":
                continue
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, name, cname, name))
            want.append("%s.%s %d" % (cname, name, sub.fields[name][1]))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(util.REPO, "include"), str(src), "-o", exe])
    got = [g for g in subprocess.check_output([exe]).decode().split("\n") if g]
    assert got == want
    assert C.sizeof(_hip.EpisodeLogMulti) == 120
    for A in range(1, _hip.SL_MAX_AGENTS + 1):
        assert emr.row_dtype(A) == episode_log.multi_row_dtype(A)
        assert emr.row_dtype(A).itemsize == _hip.log_row_multi_bytes(A) == 64 + 40 * A
        assert emr.row_dtype(A).fields["agents"][1] == 64
    assert (emr.MAX_NAMES, emr.NO_NAME, emr.QUANTITIES, emr.MAX_AGENTS) == (_hip.LOG_MAX_NAMES, _hip.LOG_NO_NAME,
                                                                            _hip.LOG_MULTI_KEYS, _hip.SL_MAX_AGENTS)


def _log(**kw):
    """A description whose pointers are non-null but never dereferenced: every call below is refused first."""
    s = _hip.EpisodeLogMulti()
    s.capacity, s.B, s.L, s.n_agents, s.n_names, s.polyak = 64, 8, 4, 2, 3, 0.99
    for name, ctype in _hip.EpisodeLogMulti._fields_:
        if ctype is C.c_void_p:
            setattr(s, name, 0x1000)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_bad_descriptions_are_refused_before_any_launch():
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    q = _hip.EpisodeQueue()
    q.capacity, q.count, q.records = 4, 0x1000, 0x1000
    w = _hip.LogWeights()

    def every(s, B=8):
        return (lib.slhip_episode_log_harvest_multi(s, p, p, p, B, None),
                lib.slhip_episode_log_join_multi(s, C.byref(q), p, p, p, C.byref(w), None),
                lib.slhip_episode_log_summaries_multi(s, None), lib.slhip_episode_log_run_summary_multi(s, 0, p, None))

    for bad in (dict(B=0), dict(L=0), dict(capacity=7), dict(polyak=-0.5), dict(polyak=float("nan")), dict(polyak=float("inf")),
                dict(n_agents=0), dict(n_agents=9), dict(n_names=0), dict(n_names=17)):
        assert every(C.byref(_log(**bad))) == (_hip.SL_E_SHAPE,) * 4, bad
        assert b"episode_log" in lib.slhip_last_error()
    for name, ctype in _hip.EpisodeLogMulti._fields_:
        if ctype is C.c_void_p:
            assert every(C.byref(_log(**{name: None}))) == (_hip.SL_E_ARG,) * 4, name
    assert every(None) == (_hip.SL_E_ARG,) * 4
    ok = C.byref(_log())
    assert lib.slhip_episode_log_harvest_multi(ok, p, p, p, 9, None) == _hip.SL_E_SHAPE      # not the log's B
    for k in range(1, 4):
        args = [ok, p, p, p, 8, None]
        args[k] = None
        assert lib.slhip_episode_log_harvest_multi(*args) == _hip.SL_E_ARG
    assert lib.slhip_episode_log_run_summary_multi(ok, 0, None, None) == _hip.SL_E_ARG
    for k in (1, 2, 3, 4, 5):
        args = [ok, C.byref(q), p, p, p, C.byref(w), None]
        args[k] = None
        assert lib.slhip_episode_log_join_multi(*args) == _hip.SL_E_ARG
    w.n = 25
    assert lib.slhip_episode_log_join_multi(ok, C.byref(q), p, p, p, C.byref(w), None) == _hip.SL_E_SHAPE
    w.n, q.capacity = 0, 0
    assert lib.slhip_episode_log_join_multi(ok, C.byref(q), p, p, p, C.byref(w), None) == _hip.SL_E_SHAPE


# ------------------------------------------------------------------------------------- the restatement against the reference

def replay_case(g, c, capacity=None, join=True):
    """The restatement driven as the fixture's run was: one harvest per step over B envs of A agents, every episode on a
    pool slot of its own (slot n: episode n), an agent's record saying done from the step it finished on, the episode's
    totals applied to its row at once.  -> the model and the rows in log order (copies, taken when each was complete)."""
    B, T, A = int(g[c + "_B"]), int(g[c + "_T"]), int(g[c + "_A"])
    N = len(g[c + "_env"])
    possible = g[c + "_available"].astype(np.int64) + g[c + "_exit_points"][:, None]
    m = emr.MultiLogModel(B, A, capacity or max(N, B), float(g[c + "_polyak"]), possible, g[c + "_name_id"], len(g[c + "_names"]))
    per_env = [[n for n in range(N) if g[c + "_env"][n] == e] for e in range(B)]
    at = [0] * B                                    # the env's current episode: per_env[e][at[e]]

    def current():
        return [per_env[e][at[e]] if at[e] < len(per_env[e]) else 0 for e in range(B)]

    def scalars():
        cur = current()
        return dict(level_idx=np.array(cur, np.int32), required_points=g[c + "_required"][cur].astype(np.int32),
                    episode_idx=np.array(at, np.int32))

    m.rewind(scalars())
    rows, n, partial = [], 0, 0
    for t in range(T):
        out = dict(done=np.zeros((B, A), np.uint8), success=np.full((B, A), 7, np.uint8), times_up=np.full((B, A), 7, np.uint8),
                   episode_reward=np.full((B, A), np.float32(np.nan)), episode_length=np.full((B, A), -99, np.int32))
        for e in range(B):                          # agents that are done, of an episode still under way or ending now
            if at[e] < len(per_env[e]):
                k = per_env[e][at[e]]
                out["done"][e] = g[c + "_done_step"][k] <= t
                partial += int(0 < out["done"][e].sum() < A)
        ended = []
        while n < N and g[c + "_step"][n] == t:
            e = int(g[c + "_env"][n])
            assert per_env[e][at[e]] == n and out["done"][e].all()
            out["success"][e], out["times_up"][e] = g[c + "_success"][n], 0
            out["episode_reward"][e], out["episode_length"][e] = g[c + "_reward"][n], g[c + "_length"][n]
            at[e] += 1
            ended.append(n)
            n += 1
        m.harvest(out, scalars())
        for k in ended:
            pos = m.find(int(g[c + "_env"][k]), int(m.rows[k % m.capacity]["episode_idx"]))
            assert pos == k % m.capacity
            if join:
                m.apply(pos, g[c + "_total"][k].tolist())
            rows.append(m.rows[pos].copy())
    assert n == N and m.n_rows == N and m.unmatched == 0
    assert A == 1 or partial > 0                    # (envs with only some agents done filed nothing)
    return m, np.array(rows, emr.row_dtype(A))


def test_golden_inputs_are_what_the_issue_asks_for(golden):
    g = golden
    assert [str(c) for c in g["cases"]] == CASES
    assert sorted(int(g[c + "_A"]) for c in CASES) == [1, 2, 2, 3, 8]
    assert {float(g[c + "_polyak"]) for c in CASES} == {0.0, 0.99, 1.0}
    c = "a2_polyak099"
    possible = g[c + "_available"] + g[c + "_exit_points"][:, None]
    assert {0, 1} <= set(possible.ravel().tolist()) and (g[c + "_reward"] < 0).any()
    tot = g[c + "_total"]
    assert ((tot[:, 1] < 1) & (tot[:, 1] > 0)).any() and (tot[:, 1] == 0).any()
    assert {0, 1000, 1001} <= set(g[c + "_length"].ravel().tolist())
    mid = slice(10, len(tot) - 10)
    assert np.isnan(tot[mid]).any() and np.isinf(tot[mid]).any()
    assert not g["a2_nosuccess_success"].any() and np.isnan(g["a2_nosuccess_run"][9])
    for c in CASES:
        ids, A = g[c + "_name_id"], int(g[c + "_A"])
        if A > 1:
            assert (g[c + "_done_step"] < g[c + "_step"][:, None]).any()          # agents that finish on different steps
        if c != "a2_nosuccess":
            assert not g[c + "_present"].all(axis=0).all()                       # a key that skips episodes
            if A > 1:
                assert any(len(set(row)) < A for row in ids.tolist())            # two agents of one name
    assert len(g["a8_polyak099_names"]) == _hip.LOG_MAX_NAMES
    size = os.path.getsize(os.path.join(util.REPO, "tests", "golden", "episode_log_multi_cases.npz"))
    assert size <= os.path.getsize(os.path.join(util.REPO, "tests", "golden", "episode_log_cases.npz"))


def test_the_reference_never_summarises_side_effects_of_a_multi_agent_run(golden):
    """Recorded data, not an assumption: the shape-(1,) fraction fails np.isscalar, so neither summary_stats nor wandb ever
    hold <type>/side_effects, and wandb saw four keys per distinct name of the level, reward_frac_needed and two counters."""
    for c in CASES:
        g = golden
        assert not g[c + "_se_isscalar"].any() and not g[c + "_se_in_wandb"].any() and not bool(g[c + "_se_summarised"])
        assert np.array_equal(g[c + "_n_keys"], 4 * g[c + "_present"].sum(axis=1) + 3)
        distinct = np.array([len(set(row)) for row in g[c + "_name_id"].tolist()])
        assert np.array_equal(g[c + "_present"].sum(axis=1), distinct)


@pytest.mark.parametrize("c", CASES)
def test_rows_equal_the_reference_bit_for_bit(golden, c):
    g = golden
    m, rows = replay_case(g, c)
    A, ag = int(g[c + "_A"]), rows["agents"]
    assert np.array_equal(rows["training_steps"], g[c + "_training_steps"])
    assert np.array_equal(ag["reward_possible"], g[c + "_reward_possible"])
    assert np.array_equal(ag["reward_needed"], g[c + "_reward_needed"])
    assert np.array_equal(ag["name"], g[c + "_name_id"]) and (rows["n_agents"] == A).all()
    assert er.same_floats(rows["side_effects_frac"], g[c + "_side_effects_frac"])
    assert er.same_floats(ag["score"], g[c + "_score"])
    # what wandb saw under each name: the LAST agent of that name, and nothing for a name the level does not have
    sc, present = g[c + "_scalars"], g[c + "_present"]
    for n in range(len(rows)):
        ids = ag["name"][n].tolist()
        for name in range(sc.shape[1]):
            assert bool(present[n, name]) == (name in ids)
            if name in ids:
                a = A - 1 - ids[::-1].index(name)
                want = [float(ag["length"][n, a]), ag["reward_frac"][n, a], float(ag["success"][n, a]), ag["score"][n, a]]
                assert er.same_floats(want, sc[n, name]), (n, name)
    assert (m.steps, m.episodes) == (int(g[c + "_B"]) * int(g[c + "_T"]), len(rows))


def summaries_after_every_row(g, c):
    """The restatement's summary_stats after every episode, [N,M,4] (NaN: no value yet), and the counts."""
    m, rows = replay_case(g, c)
    M = len(g[c + "_names"])
    fresh = emr.MultiLogModel(m.B, m.A, m.capacity, m.polyak, m.reward_possible, m.name_id, M)
    fresh.rows[:len(rows)] = rows
    stats, counts = [], []
    for n in range(len(rows)):
        fresh.n_rows = n + 1
        fresh.summarise()
        stats.append([v if k else er.NAN for v, k in zip(fresh.value[:4 * M], fresh.count[:4 * M])])
        counts.append(list(fresh.count[:4 * M]))
    assert not any(fresh.count[4 * M:])
    return np.array(stats).reshape(-1, M, 4), np.array(counts).reshape(-1, M, 4), m


def test_summaries_within_the_measured_bound(golden):
    """log_scalars() after every episode of every case; see the module docstring for the two numbers."""
    worst, run_worst = 0.0, 0.0
    for c in CASES:
        stats, counts, m = summaries_after_every_row(golden, c)
        assert np.array_equal(counts, golden[c + "_counts"])
        d = deviation(stats, golden[c + "_stats"])
        if float(golden[c + "_polyak"]) in (0.0, 1.0):
            assert d == 0.0, c                      # the weights are exact there
        worst = max(worst, d)
        run = m.run_summary(0)
        assert run[0] == golden[c + "_run"][0] and run[11] == golden[c + "_run"][11]
        run_worst = max(run_worst, deviation(run, golden[c + "_run"]))
    print("largest |restatement - reference|: summaries %r, run summary %r" % (worst, run_worst))
    assert worst <= SUMMARY_BOUND and run_worst <= RUN_BOUND
    assert worst >= SUMMARY_MEASURED / 2 and run_worst >= RUN_MEASURED / 2      # (the docstring's numbers are this run's)


def test_one_call_equals_many_calls_and_the_ring_loses_its_oldest_rows(golden):
    g, c = golden, "a2_polyak099"
    full, rows = replay_case(g, c)
    full.summarise()
    stats, _, _ = summaries_after_every_row(g, c)
    M = len(g[c + "_names"])
    assert er.same_floats(np.array(full.value[:4 * M]).reshape(M, 4), stats[-1])
    names = [str(n) for n in g[c + "_names"]]
    s = full.summary(names)
    assert s["training/episodes"] == len(rows) and set(s) == ({"training/%s-%s" % (n, q) for n in names for q in emr.QUANTITIES}
                                                               | {"training/steps", "training/episodes"})
    m, _ = replay_case(g, c, capacity=16)
    N = len(rows)
    assert er.same_floats(m.run_summary(0), m.run_summary(N - 16))
    tail = emr.MultiLogModel(m.B, m.A, N, m.polyak, m.reward_possible, m.name_id, M)
    tail.rows[:N], tail.n_rows = rows, N
    assert er.same_floats(m.run_summary(0), tail.run_summary(N - 16))
    assert m.find(int(rows["env"][0]), int(rows["episode_idx"][0])) is None         # overwritten
    assert m.find(int(rows["env"][N - 1]), int(rows["episode_idx"][N - 1])) == (N - 1) % 16
    assert m.find(-1, 0) is None and m.find(m.B, 0) is None


# --------------------------------------------------------------------------------------------------------- the Python class

@pytest.fixture(scope="module")
def pool2():
    lvls = []
    for name in ("multi_asym1", "multi_build_coop", "multi_build_compete"):
        lvls += util.levels_from_trace(util.load_trace(name))
    return levels.LevelPool(lvls, counts_fn=util.oracle_counts, n_agents=2)


def test_constructor_errors_and_defaults(pool2):
    from safelife_amd import schedule
    ML, L = episode_log.MultiAgentEpisodeLog, len(pool2)
    log = ML(pool2, 8, 8)
    assert log.summary_polyak == 0.99 and ML(pool2, 8, 64, episode_type="validation").summary_polyak == 1.0
    assert log.n_agents == 2 and log.names == ["agent0", "agent1"] and np.array_equal(log.name_id, [[0, 1]] * L)
    sched = schedule.LevelSchedule(pool2, [(0, L)], mode="uniform", seed=0)
    assert np.array_equal(log.available, sched.available) and log.available.shape == (L, 2)
    assert np.array_equal(log.reward_possible(3), sched.reward_possible(3))
    assert log.row_dtype.itemsize == 144
    with pytest.raises(ValueError, match="capacity"):
        ML(pool2, 8, 7)
    with pytest.raises(ValueError):
        ML(pool2, 0, 8)
    with pytest.raises(TypeError):
        ML(None, 8, 8)
    for p in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="polyak"):
            ML(pool2, 8, 8, summary_polyak=p)
    with pytest.raises(ValueError, match="weights"):
        ML(pool2, 8, 8, side_effect_weights={"life-%d" % k: 1.0 for k in range(25)})
    w = ML(pool2, 8, 8, side_effect_weights={"life-green": 1.0, "spawner-yellow": 0.5})._weights
    assert (w.n, w.cell[0], w.cell[1], w.weight[0], w.weight[1]) == (2, 0x409, 152 | 0x600, 1.0, 0.5)
    # names: one list of A per slot; duplicates share an id; more than 16 distinct ones are refused
    names = [["red", "red"]] + [["red", "blue"]] * (L - 1)
    named = ML(pool2, 8, 8, agent_names=names)
    assert named.names == ["red", "blue"] and named.name_id.tolist() == [[0, 0]] + [[0, 1]] * (L - 1)
    with pytest.raises(ValueError, match="agent_names"):
        ML(pool2, 8, 8, agent_names=names[:-1])
    with pytest.raises(ValueError, match="agent_names"):
        ML(pool2, 8, 8, agent_names=[["a"]] * L)
    big = levels.LevelPool(list(pool2.levels) * 2, counts_fn=util.oracle_counts, n_agents=2)
    sixteen = [["n%d" % (2 * k), "n%d" % (2 * k + 1)] for k in range(8)]
    assert len(big) >= 9 and len(ML(big, 8, 8, agent_names=sixteen + [["n0", "n15"]] * (len(big) - 8)).names) == 16
    with pytest.raises(ValueError, match="16 distinct"):
        ML(big, 8, 8, agent_names=sixteen + [["n0", "n16"]] * (len(big) - 8))
    for call in (log.summary, log.rows, log.counters):
        with pytest.raises(ValueError, match="no device state"):
            call()
    with pytest.raises(ValueError, match="not attached"):
        log.flush()


def test_the_single_agent_log_still_refuses_a_multi_agent_pool(pool2):
    with pytest.raises(ValueError, match="single-agent"):
        episode_log.EpisodeLog(pool2, 8, 8)
    with pytest.raises(ValueError, match="MultiAgentEpisodeLog"):
        episode_log.EpisodeLog(pool2, 8, 8)


def test_the_multi_env_refuses_a_log_without_auto_reset(pool2):
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    log = episode_log.MultiAgentEpisodeLog(pool2, 4, 8)
    with pytest.raises(ValueError, match="auto_reset=True"):
        SafeLifeMultiAgentVectorEnv(pool2, 4, auto_reset=False, episode_log=log)
    assert log.env is None and log.t is None            # nothing was attached or allocated


def test_stepping_modes_refuse_an_episode_log():
    """The multi-agent env hands its log to the base env, whose slice, queue and rollout() stepping refuse it before they
    touch anything, in the schedule's wording."""
    import inspect
    from safelife_amd import multi_env
    from safelife_amd.vector_env import SafeLifeVectorEnv
    assert "base.episode_log = episode_log" in inspect.getsource(multi_env.SafeLifeMultiAgentVectorEnv.__init__)
    base = object.__new__(SafeLifeVectorEnv)
    base.level_schedule, base.episode_log, base._queues = None, object.__new__(episode_log.MultiAgentEpisodeLog), None
    for call in (lambda: base.rollout(None), lambda: base.step_async(0), lambda: base.step_slice(0, 0),
                 lambda: base.step_queues(0), lambda: base.step_queues_many(0), lambda: base.queues_open(),
                 lambda: base.set_step_outputs(1)):
        with pytest.raises(ValueError, match="cannot drive an episode log: .* \\(use step\\(\\)\\)"):
            call()


def test_records_against_the_fixtures_log_data(golden):
    g, c = golden, "a3_polyak0"
    _, rows = replay_case(g, c)
    names = [str(n) for n in g[c + "_names"]]
    titles = ["level-%d" % n for n in range(len(rows))]
    recs = episode_log.multi_rows_to_records(rows, titles, names)
    assert len(recs) == len(rows)
    for n, d in enumerate(recs):
        assert list(d) == ["length", "reward", "success", "side_effects", "agents", "level_name", "reward_possible",
                           "reward_needed"]
        assert d["level_name"] == "level-%d" % n and d["length"] == g[c + "_length"][n].tolist()
        assert d["reward"] == g[c + "_reward"][n].astype(np.float64).tolist()
        assert d["success"] == g[c + "_success"][n].astype(bool).tolist() and all(type(v) is bool for v in d["success"])
        assert d["agents"] == [names[k] for k in g[c + "_name_id"][n]]
        assert d["reward_possible"] == g[c + "_reward_possible"][n].tolist()
        assert d["reward_needed"] == g[c + "_reward_needed"][n].tolist()
        assert er.same_floats(d["side_effects"]["total"], g[c + "_total"][n])
    _, bare = replay_case(g, c, join=False)
    assert all("side_effects" not in d for d in episode_log.multi_rows_to_records(bare, titles, names))
