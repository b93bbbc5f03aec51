"""
Evaluation runs without a GPU: the ABI of the slhip_episode_run_* entry points, the numpy restatement
(tests/episode_run_ref.py) against what the reference's ``BaseAlgo.run_episodes`` played and logged
(tests/golden/episode_run_cases.npz, written by tests/golden/make_golden_episode_run.py), the model's edges, and the
argument checks of safelife_amd.episode_run and of the env classes.

The reference deals levels to whichever env finishes first; the run deals ticket t to slot t % L and env t % G.  For every
parity case (no more envs than episodes) the MULTISET of levels played is the same: the iterator's first N levels.  The
summaries of the episode log over the restatement's rows equal the reference's ``summary_stats`` within

* SUMMARY_MEASURED = 4.973799150320701e-14: the largest |restatement - reference| over the five benchmark summaries of
  every parity case.  With ``summary_polyak`` 1 the recurrence value <- (v + n value) / (1 + n) has exact weights on both
  sides; the only difference is the ORDER of the rows -- the run's rows arrive in (step, env) order of the static deal, the
  reference's in its finishing order -- and a running mean of up to 192 values around 10 (lengths) or 60 (scores) moves by a
  few ulp of those, 1e-14, when its terms are permuted.

The bound of the test is twice the measured value, as elsewhere in this suite.
"""
import collections
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from safelife_amd import _hip, episode_run
from tests import episode_log_ref as er
from tests import episode_run_ref as rr
from tests import util

SUMMARY_MEASURED = 4.973799150320701e-14
SUMMARY_BOUND = 2 * SUMMARY_MEASURED

NAMES = ("slhip_episode_run_start", "slhip_episode_run_harvest", "slhip_episode_run_harvest_multi",
         "slhip_episode_run_tickets")


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "episode_run_cases.npz")) as d:
        return {k: d[k] for k in d.files}


def parity_cases(g):
    return [str(c) for c in g["cases"] if int(g[str(c) + "_parity"])]


# ------------------------------------------------------------------------------------------------------------- the ABI

def test_symbols_and_version():
    lib = _hip.lib()
    for name in NAMES:
        assert name in _hip.EXPORTS and hasattr(lib, name)
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13


def test_layouts_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "safelife_hip.h"', 'int main(void) {',
             'printf("consts %d %d %d\\n", SL_RUN_WRITTEN, SL_RUN_SCORED, SL_RUN_COUNTERS);',
             'printf("sizes %zu %zu %zu\\n", sizeof(sl_episode_run), sizeof(sl_episode_run_row), sizeof(sl_episode_run_agent));']
    want = ["consts %d %d %d" % (_hip.RUN_WRITTEN, _hip.RUN_SCORED, len(_hip.RUN_COUNTERS)),
            "sizes %d %d %d" % (C.sizeof(_hip.EpisodeRun), episode_run.ROW_DTYPE.itemsize, episode_run.AGENT_DTYPE.itemsize)]
    for name, ctype in _hip.EpisodeRun._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(sl_episode_run, %s));' % (name, name))
        want.append("%s %d" % (name, getattr(_hip.EpisodeRun, name).offset))
    for cname, dt in (("sl_episode_run_row", episode_run.ROW_DTYPE), ("sl_episode_run_agent", episode_run.AGENT_DTYPE)):
        for name in dt.names:
            lines.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (name, cname, name))
            want.append("%s %d" % (name, dt.fields[name][1]))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(util.REPO, "include"), str(src), "-o", exe])
    got = [g for g in subprocess.check_output([exe]).decode().split("\n") if g]
    assert got == want
    assert (C.sizeof(_hip.EpisodeRun), episode_run.ROW_DTYPE.itemsize, episode_run.AGENT_DTYPE.itemsize) == (80, 32, 16)
    assert episode_run.ROW_DTYPE == rr.ROW and episode_run.AGENT_DTYPE == rr.AGENT and rr.STEP_OUT.itemsize == 16
    assert rr.WRITTEN == _hip.RUN_WRITTEN


def _run(**kw):
    """A description whose pointers are non-null but never dereferenced: every call below is refused first."""
    s = _hip.EpisodeRun()
    s.B, s.G, s.env_offset, s.N, s.L, s.n_agents = 8, 8, 0, 20, 4, 1
    for name, ctype in _hip.EpisodeRun._fields_:
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

    def every(s):
        return (lib.slhip_episode_run_start(s, p, None), lib.slhip_episode_run_harvest(s, p, 1, None),
                lib.slhip_episode_run_harvest_multi(s, p, 1, None),
                lib.slhip_episode_run_tickets(s, C.byref(q), p, None, None, None, None, None))

    for bad in (dict(B=0), dict(L=0), dict(N=0), dict(G=7), dict(env_offset=-1), dict(env_offset=1), dict(n_agents=0),
                dict(n_agents=9)):
        assert every(C.byref(_run(**bad))) == (_hip.SL_E_SHAPE,) * 4, bad
        assert b"episode_run" in lib.slhip_last_error()
    for name, ctype in _hip.EpisodeRun._fields_:
        if ctype is C.c_void_p:
            assert every(C.byref(_run(**{name: None}))) == (_hip.SL_E_ARG,) * 4, name
    assert every(None) == (_hip.SL_E_ARG,) * 4
    ok = C.byref(_run())
    assert lib.slhip_episode_run_start(ok, None, None) == _hip.SL_E_ARG
    assert lib.slhip_episode_run_harvest(ok, None, 1, None) == _hip.SL_E_ARG
    assert lib.slhip_episode_run_harvest_multi(ok, None, 1, None) == _hip.SL_E_ARG
    assert lib.slhip_episode_run_harvest(C.byref(_run(n_agents=2)), p, 1, None) == _hip.SL_E_SHAPE   # records [B] have one agent
    assert lib.slhip_episode_run_tickets(ok, None, p, None, None, None, None, None) == _hip.SL_E_ARG
    assert lib.slhip_episode_run_tickets(ok, C.byref(q), None, None, None, None, None, None) == _hip.SL_E_ARG
    for k in (4, 5, 6):                                 # scores without keys / n_cells / weights
        args = [ok, C.byref(q), p, p, p, p, C.byref(w), None]
        args[k] = None
        assert lib.slhip_episode_run_tickets(*args) == _hip.SL_E_ARG
    w.n = 25
    assert lib.slhip_episode_run_tickets(ok, C.byref(q), p, p, p, p, C.byref(w), None) == _hip.SL_E_SHAPE
    q.capacity = 0
    assert lib.slhip_episode_run_tickets(ok, C.byref(q), p, None, None, None, None, None) == _hip.SL_E_SHAPE


# ------------------------------------------------------------------------------------- the restatement against the reference

def _episode(g):
    return lambda s: (int(g["level_length"][s]), float(g["level_reward"][s]), int(g["level_success"][s]))


def _play_logged(g, B, N, L):
    """The restatement's run over the fixture's stub levels with the episode log's restatement behind it, as the env files
    them: run harvest, then log harvest, per step.  -> run model, log model, steps."""
    possible = g["level_available"].astype(np.int64) + 1
    log = er.LogModel(B, max(N, B), 1.0, possible)
    first = dict(level_idx=(np.arange(B) % L).astype(np.int32), required_points=np.zeros(B, np.int32),
                 episode_idx=np.zeros(B, np.int32))
    log.rewind(first)
    m = None
    for m, out, sc in rr.play(B, B, 0, N, L, _episode(g), extra_steps=3):
        log.harvest({k: out[k] for k in ("done", "success", "times_up", "episode_reward", "episode_length")},
                    dict(sc, required_points=np.zeros(B, np.int32)))
    for r in range(log.n_rows):
        log.apply(r, g["level_total"][int(log.rows[r]["level"])].tolist())
    log.summarise()
    return m, log


def test_the_golden_cases_are_what_the_issue_asks_for(golden):
    g = golden
    cases = parity_cases(g)
    assert {int(g[c + "_B"]) for c in cases} == {1, 5, 20, 64}
    for B in (5, 20, 64):
        ns = {int(g[c + "_N"]) for c in cases if int(g[c + "_B"]) == B}
        assert ns == {B, B + 1, 3 * B, 3 * B - 1, -1}
    assert any(int(g[c + "_L"]) < max(int(g[c + "_N"]), 1) for c in cases)
    assert any(int(g[c + "_L"]) > int(g[c + "_N"]) > 0 for c in cases)
    assert all(int(g[c + "_B"]) <= (int(g[c + "_N"]) if int(g[c + "_N"]) > 0 else int(g[c + "_B"])) for c in cases)
    c = "more_envs_than_episodes"
    assert int(g[c + "_parity"]) == 0 and int(g[c + "_B"]) > int(g[c + "_N"])
    assert os.path.getsize(os.path.join(util.REPO, "tests", "golden", "episode_run_cases.npz")) < 1 << 20


def test_the_same_episodes_as_the_reference(golden):
    g = golden
    worst = 0.0
    for c in parity_cases(g):
        B, L = int(g[c + "_B"]), int(g[c + "_L"])
        N = int(g[c + "_N"]) if int(g[c + "_N"]) > 0 else B            # (None: the reference takes the env count)
        m, log = _play_logged(g, B, N, L)
        # exactly N episodes, every ticket once, and the multiset of levels the reference logged: the iterator's first N
        assert m.completed == N and (m.writes == 1).all() and log.n_rows == N, c
        played = collections.Counter(m.results["slot"].tolist())
        assert played == collections.Counter(g[c + "_levels"].tolist()), c
        assert played == collections.Counter(t % L for t in range(N)), c
        assert np.array_equal(log.rows[:N]["level"][np.argsort(log.rows[:N]["env"] + B * log.rows[:N]["episode_idx"])],
                              m.results["slot"]), c
        # the reference hands out one more level per env than it plays: our phantom episodes
        assert int(g[c + "_handed"]) == N + B, c
        assert list(log.count) == g[c + "_counts"].tolist(), c
        dev = np.abs(np.array(log.value) - g[c + "_stats"])
        assert np.isfinite(dev).all(), c
        worst = max(worst, float(dev.max()))
    print("largest |restatement - reference| of the benchmark summaries: %r" % worst)
    assert worst <= SUMMARY_BOUND


def test_more_envs_than_episodes_is_where_the_run_differs(golden):
    """The reference steps all 20 envs for 7 episodes and logs whichever finish first; the run never starts envs 7..19 and
    plays the iterator's first 7 levels."""
    g, c = golden, "more_envs_than_episodes"
    B, N, L = int(g[c + "_B"]), int(g[c + "_N"]), int(g[c + "_L"])
    m, log = _play_logged(g, B, N, L)
    assert m.results["slot"].tolist() == list(range(N)) and m.env_steps < B * m.steps
    assert sorted(g[c + "_levels"].tolist()) != list(range(N)) and int(g[c + "_handed"]) == N + B


# ------------------------------------------------------------------------------------------------------------- the model

def _lengths(s):
    return 1 + (s * 7) % 5, float(s), s % 2


@pytest.mark.parametrize("B,N,L", [(8, 5, 3), (8, 8, 3), (8, 9, 3), (8, 23, 3), (8, 23, 1), (8, 23, 40), (1, 1, 1), (1, 4, 3)])
def test_model_edges(B, N, L):
    m = None
    retired_at = {}
    for m, out, sc in rr.play(B, B, 0, N, L, _lengths, extra_steps=5):
        for e in range(B):
            if not m.active[e]:
                retired_at.setdefault(e, m.steps)
            if m.steps > retired_at.get(e, 10 ** 9):
                assert out[e].tobytes() == bytes(16), (e, m.steps)      # retired before this step: nothing is reported
    assert m.completed == N and (m.writes == 1).all() and m.in_progress == 0 and not m.active.any()
    for t in range(N):
        row = m.results[t]
        assert (row["slot"], row["env"], row["episode_idx"]) == rr.deal(t, L, B) == (t % L, t % B, t // B)
        assert (row["length"], row["reward"], row["success"]) == _lengths(t % L)
        assert m.ticket(t % B, t // B) == t
    assert m.played.tolist() == [len(rr.tickets_of_env(g, B, N)) for g in range(B)]
    assert [m.ticket(e, int(m.played[e])) for e in range(B)] == [-1] * B           # the phantom episode that follows
    assert m.ticket(0, -1) == m.ticket(-1, 0) == m.ticket(B, 0) == -1
    if N < B:
        assert set(range(N, B)) <= {e for e, s in retired_at.items() if s == 1}    # envs >= N never start


def test_two_shards_merge_into_the_one_process_table():
    G, N, L = 13, 30, 4
    whole = None
    for whole, _, _ in rr.play(G, G, 0, N, L, _lengths):
        pass
    parts = []
    for off, B in ((0, 6), (6, 7)):
        m = None
        for m, _, _ in rr.play(B, G, off, N, L, _lengths):
            pass
        parts.append(m)
        mine = np.array([off <= t % G < off + B for t in range(N)])
        assert np.array_equal(m.writes, mine.astype(np.int64)) and m.completed == mine.sum()
    assert not (parts[0].writes & parts[1].writes).any()
    merged = np.where(parts[0].writes.astype(bool), parts[0].results, parts[1].results)
    for name in ("slot", "env", "episode_idx", "length", "reward", "success", "times_up", "flags"):
        assert np.array_equal(merged[name], whole.results[name]), name
    assert parts[0].completed + parts[1].completed == whole.completed == N


# ------------------------------------------------------------------------------------------------------------- the checks

@pytest.fixture(scope="module")
def pool():
    return util.pool_from_fixture("prune_still_25", util.oracle_counts, n=6)[0]


def test_env_arguments(pool):
    run = episode_run.EpisodeRun(pool, 4, 30, env_offset=8, global_envs=20)
    kw = run.env_arguments()
    assert sorted(kw) == ["auto_reset", "first_level", "level_stride"] and kw["auto_reset"] is True
    assert kw["first_level"].tolist() == [2, 3, 4, 5] and kw["level_stride"] == 20 % 6
    assert run.num_tickets == 6 and run.global_envs == 20          # envs 8..11 of 20: tickets 8..11 and 28, 29
    assert episode_run.EpisodeRun(pool, 7, 3).global_envs == 7
    assert episode_run.deal(29, 6, 20) == (5, 9, 1) and episode_run.ticket_of(9, 1, 20) == 29
    for bad in (dict(num_envs=0, num_episodes=3), dict(num_envs=3, num_episodes=0),
                dict(num_envs=3, num_episodes=3, env_offset=2, global_envs=4),
                dict(num_envs=3, num_episodes=3, env_offset=-1), dict(num_envs=3, num_episodes=3, n_agents=2)):
        with pytest.raises(ValueError):
            episode_run.EpisodeRun(pool, bad.pop("num_envs"), bad.pop("num_episodes"), **bad)
    with pytest.raises(TypeError):
        episode_run.EpisodeRun(object(), 3, 3)
    with pytest.raises(ValueError, match="no device state"):
        run.finished()


def test_an_env_built_otherwise_is_refused(pool):
    """Every refusal comes before anything is allocated: no device is needed to meet it."""
    from safelife_amd.levels import LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    from safelife_amd.vector_env import SafeLifeVectorEnv
    run = episode_run.EpisodeRun(pool, 8, 20)
    good = run.env_arguments()
    for cls in (SafeLifeVectorEnv, SafeLifeMultiAgentVectorEnv):
        for bad in (dict(auto_reset=False), dict(first_level=None), dict(first_level=0), dict(level_stride=1),
                    dict(env_offset=3)):
            with pytest.raises(ValueError, match=r"run\.env_arguments\(\)"):
                cls(pool, 8, episode_run=run, **dict(good, **bad))
        with pytest.raises(ValueError, match="reference's evaluation envs carry none"):
            cls(pool, 8, episode_run=run, wrappers=dict(movement_bonus=0.1), **good)
        with pytest.raises(ValueError, match="both own the successor rule"):
            cls(pool, 8, episode_run=run, level_schedule=object(), **good)
        with pytest.raises(ValueError, match="built for 8 envs"):
            cls(pool, 9, episode_run=run, **good)
        other = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=6)[0]
        with pytest.raises(ValueError, match="another pool"):
            cls(other, 8, episode_run=run, **good)
    levels = list(pool.levels)
    with pytest.raises(ValueError, match="both own the successor rule"):
        episode_run.EpisodeRun(LevelPool(levels, counts_fn=util.oracle_counts, refreshable=True), 8, 20)
    # the sliced and queue steppers and rollout(): nothing would file the episode ends or mask the retired envs
    stub = types.SimpleNamespace(level_schedule=None, episode_log=None, episode_run=run)
    for what in ("step_async()", "step_slice()", "step_queues()", "queues_open()", "rollout()", "set_step_outputs()"):
        with pytest.raises(ValueError, match="cannot drive an episode run.*nothing would file the episode ends"):
            SafeLifeVectorEnv._no_schedule(stub, what, "why", "why")
    SafeLifeVectorEnv._no_schedule(types.SimpleNamespace(level_schedule=None, episode_log=None), "rollout()", "why", "why")


def test_reset_summary_is_a_new_method_of_both_logs():
    from safelife_amd import episode_log
    for cls in (episode_log.EpisodeLog, episode_log.MultiAgentEpisodeLog):
        assert callable(getattr(cls, "reset_summary"))
    log = episode_log.EpisodeLog(util.pool_from_fixture("prune_still_25", util.oracle_counts, n=3)[0], 4, 8,
                                 episode_type="benchmark")
    with pytest.raises(ValueError, match="no device state"):
        log.reset_summary()
