"""
The episode log without a GPU: the ABI of the four slhip_episode_log_* entry points, the host restatement
(tests/episode_log_ref.py) against what the reference's SafeLifeLogger logged (tests/golden/episode_log_cases.npz, written
by tests/golden/make_golden_episode_log.py), and the argument checks of safelife_amd.episode_log.

Per-episode fields (reward_frac, side_effects_frac, score, training_steps, reward_possible, reward_needed) equal the
fixture BIT FOR BIT.  The running summaries and the run summary equal it within a measured tolerance:

* SUMMARY_MEASURED = 1.5916157281026244e-12: the largest |restatement - reference| over every summary_stats value after
  every episode of every case (3549 episodes, 5 keys).  It is not zero because the reference computes the weight as
  p (1 - p**n) / (1 - p) -- a pow and a subtraction that cancels while p**n is close to 1: for n = 1 and p = 0.99 the
  difference 1 - p**n keeps an absolute error of half an ulp of 1, a relative error of 1e-14 -- where the kernel and the
  restatement run the recurrence w <- p (1 + w), two roundings per step.  Both weights are close to the exact one, not
  equal to each other; (v + w old) / (1 + w) inherits a relative difference of a few 1e-15, which on `length` (values
  around 500) is 1e-12.  With polyak 1 and 0 the weights are exact and the deviation is 0, which the test asserts.
* RUN_MEASURED = 1.1368683772161603e-13: the same for the twelve run-summary numbers, where they are finite.  The kernel and
  the restatement add every column up as one chain in row order; numpy's np.average / np.std add pairwise (eight
  accumulators over blocks of 128).  Both are exact sums of the same terms up to rounding: over 3102 rows of lengths around
  500 and scores around 100 the running sums reach 1e6 (1e9 for the squared deviations), an ulp of those is 1e-10 (1e-7),
  and divided by n -- and, for a deviation, through the square root -- a few ulp of difference come to 1e-13.

The bounds of the tests are twice the measured values, on the host here and on the device in tests/test_episode_log_gpu.py
(where the kernels must equal the restatement bit for bit, so the same bound holds).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from safelife_amd import _hip, episode_log
from tests import episode_log_ref as er
from tests import util

SUMMARY_MEASURED = 1.5916157281026244e-12
RUN_MEASURED = 1.1368683772161603e-13
SUMMARY_BOUND, RUN_BOUND = 2 * SUMMARY_MEASURED, 2 * RUN_MEASURED

NAMES = ("slhip_episode_log_harvest", "slhip_episode_log_join", "slhip_episode_log_summaries",
         "slhip_episode_log_run_summary")


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "episode_log_cases.npz")) as d:
        return {k: d[k] for k in d.files}


def case_names(golden):
    return [str(c) for c in golden["cases"]]


# ------------------------------------------------------------------------------------------------------------- the ABI

def test_symbols_and_version():
    lib = _hip.lib()
    for name in NAMES:
        assert name in _hip.EXPORTS and hasattr(lib, name)
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13


def test_layouts_match_the_header(tmp_path):
    """ctypes mirrors of sl_episode_log, sl_episode_log_row and sl_log_weights, and numpy's row dtype, against gcc's
    offsetof / sizeof, and the constants."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "safelife_hip.h"', 'int main(void) {',
             'printf("consts %d %d %d %d %d %d\\n", SL_LOG_JOINED, SL_LOG_KEYS, SL_LOG_COUNTERS, SL_LOG_MAX_HOPS, '
             'SL_LOG_RUN_SUMMARY, SL_SE_MAX_KEYS);']
    want = ["consts %d %d %d %d %d %d" % (_hip.LOG_JOINED, len(_hip.LOG_KEYS), len(_hip.LOG_COUNTERS), _hip.LOG_MAX_HOPS,
                                          _hip.LOG_RUN_SUMMARY, _hip.SL_SE_MAX_KEYS)]
    for cname, st in (("sl_episode_log", _hip.EpisodeLog), ("sl_episode_log_row", _hip.EpisodeLogRow),
                      ("sl_log_weights", _hip.LogWeights)):
        lines.append('printf("size %%zu\\n", sizeof(%s));' % cname)
        want.append("size %d" % C.sizeof(st))
        for name, ctype in st._fields_:
            lines.append('printf("%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));'
                         % (name, cname, name, cname, name))
            want.append("%s %d %d" % (name, getattr(st, name).offset, C.sizeof(ctype)))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(util.REPO, "include"), str(src), "-o", exe])
    got = [g for g in subprocess.check_output([exe]).decode().split("\n") if g]
    assert got == want
    assert (C.sizeof(_hip.EpisodeLog), C.sizeof(_hip.EpisodeLogRow), C.sizeof(_hip.LogWeights)) == (104, 96, 248)
    for dt in (episode_log.ROW_DTYPE, er.ROW_DTYPE):
        assert dt.itemsize == 96
        for name, _ in _hip.EpisodeLogRow._fields_:
            assert dt.fields[name][1] == getattr(_hip.EpisodeLogRow, name).offset, name
    assert episode_log.ROW_DTYPE == er.ROW_DTYPE
    assert (er.JOINED, er.MAX_HOPS, er.MAX_KEYS, er.KEYS) == (_hip.LOG_JOINED, _hip.LOG_MAX_HOPS, _hip.SL_SE_MAX_KEYS,
                                                              _hip.LOG_KEYS)


def _log(**kw):
    """A description whose pointers are non-null but never dereferenced: every call below is refused first."""
    s = _hip.EpisodeLog()
    s.capacity, s.B, s.L, s.polyak = 64, 8, 4, 0.99
    for name, ctype in _hip.EpisodeLog._fields_:
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
        return (lib.slhip_episode_log_harvest(s, p, p, B, None), lib.slhip_episode_log_join(s, C.byref(q), p, p, p, C.byref(w), None),
                lib.slhip_episode_log_summaries(s, None), lib.slhip_episode_log_run_summary(s, 0, p, None))

    for bad in (dict(B=0), dict(L=0), dict(capacity=7), dict(polyak=-0.5), dict(polyak=float("nan")),
                dict(polyak=float("inf"))):
        assert every(C.byref(_log(**bad))) == (_hip.SL_E_SHAPE,) * 4, bad
        assert b"episode_log" in lib.slhip_last_error()
    for name, ctype in _hip.EpisodeLog._fields_:
        if ctype is C.c_void_p:
            assert every(C.byref(_log(**{name: None}))) == (_hip.SL_E_ARG,) * 4, name
    assert every(None) == (_hip.SL_E_ARG,) * 4
    ok = C.byref(_log())
    assert lib.slhip_episode_log_harvest(ok, p, p, 9, None) == _hip.SL_E_SHAPE           # not the log's B
    assert lib.slhip_episode_log_harvest(ok, None, p, 8, None) == _hip.SL_E_ARG
    assert lib.slhip_episode_log_harvest(ok, p, None, 8, None) == _hip.SL_E_ARG
    assert lib.slhip_episode_log_run_summary(ok, 0, None, None) == _hip.SL_E_ARG
    assert lib.slhip_episode_log_join(ok, None, p, p, p, C.byref(w), None) == _hip.SL_E_ARG
    assert lib.slhip_episode_log_join(ok, C.byref(q), p, p, p, None, None) == _hip.SL_E_ARG
    for k in range(2, 5):
        args = [ok, C.byref(q), p, p, p, C.byref(w), None]
        args[k] = None
        assert lib.slhip_episode_log_join(*args) == _hip.SL_E_ARG
    w.n = 25
    assert lib.slhip_episode_log_join(ok, C.byref(q), p, p, p, C.byref(w), None) == _hip.SL_E_SHAPE
    w.n, q.capacity = 0, 0
    assert lib.slhip_episode_log_join(ok, C.byref(q), p, p, p, C.byref(w), None) == _hip.SL_E_SHAPE


# ------------------------------------------------------------------------------------- the restatement against the reference

def replay_case(g, c, capacity=None, join=True):
    """The restatement driven as the fixture's run was: one harvest per step over B envs, every episode on a pool slot of
    its own (slot n: episode n), the episode's totals applied to its row at once.  -> the model and the rows in log
    order (copies, taken when each was complete)."""
    B, T = int(g[c + "_B"]), int(g[c + "_T"])
    N = len(g[c + "_env"])
    possible = g[c + "_available"].astype(np.int64) + g[c + "_exit_points"]
    m = er.LogModel(B, capacity or max(N, B), float(g[c + "_polyak"]), possible)
    per_env = [[n for n in range(N) if g[c + "_env"][n] == e] for e in range(B)]
    at = [0] * B                                    # the env's current episode: per_env[e][at[e]]

    def scalars():
        cur = [per_env[e][at[e]] if at[e] < len(per_env[e]) else 0 for e in range(B)]
        return dict(level_idx=np.array(cur, np.int32), required_points=g[c + "_required"][cur].astype(np.int32),
                    episode_idx=np.array(at, np.int32))

    m.rewind(scalars())
    rows, stats, n = [], [], 0
    for t in range(T):
        out = dict(done=np.zeros(B, np.uint8), success=np.full(B, 7, np.uint8), times_up=np.full(B, 7, np.uint8),
                   episode_reward=np.full(B, np.float32(np.nan)), episode_length=np.full(B, -99, np.int32))
        ended = []
        while n < N and g[c + "_step"][n] == t:
            e = int(g[c + "_env"][n])
            assert per_env[e][at[e]] == n
            out["done"][e], out["success"][e], out["times_up"][e] = 1, g[c + "_success"][n], 0
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
    return m, np.array(rows, er.ROW_DTYPE)


def test_golden_inputs_are_what_the_issue_asks_for(golden):
    g = golden
    assert sorted(float(g[c + "_polyak"]) for c in case_names(g)) == [0.0, 0.99, 1.0, 1.0]
    assert max(len(g[c + "_env"]) for c in case_names(g)) >= 3000
    c = "polyak099"
    possible = g[c + "_available"] + g[c + "_exit_points"]
    assert {0, 1} <= set(possible.tolist()) and (g[c + "_reward"] < 0).any()
    tot = g[c + "_total"]
    assert ((tot[:, 1] < 1) & (tot[:, 1] > 0)).any() and (tot[:, 1] == 0).any()
    assert {0, 1000, 1001} <= set(g[c + "_length"].tolist())
    mid = slice(10, len(tot) - 10)
    assert np.isnan(tot[mid]).any() and np.isinf(tot[mid]).any()
    assert not g["nosuccess_success"].any() and np.isnan(g["nosuccess_run"][9])
    assert os.path.getsize(os.path.join(util.REPO, "tests", "golden", "episode_log_cases.npz")) < 1 << 20


@pytest.mark.parametrize("c", ["nosuccess", "polyak0", "polyak099", "polyak1"])
def test_rows_equal_the_reference_bit_for_bit(golden, c):
    g = golden
    m, rows = replay_case(g, c)
    assert np.array_equal(rows["training_steps"], g[c + "_training_steps"])
    assert np.array_equal(rows["reward_possible"], g[c + "_reward_possible"])
    assert np.array_equal(rows["reward_needed"], g[c + "_reward_needed"])
    sc = g[c + "_scalars"]                          # side_effects, length, reward, success, score as wandb saw them
    assert er.same_floats(rows["side_effects_frac"], sc[:, 0])
    assert er.same_floats(rows["length"].astype(np.float64), sc[:, 1])
    assert er.same_floats(rows["reward_frac"], sc[:, 2])
    assert er.same_floats(rows["success"].astype(np.float64), sc[:, 3])
    assert er.same_floats(rows["score"], sc[:, 4])
    assert (m.steps, m.episodes) == (int(g[c + "_B"]) * int(g[c + "_T"]), len(rows))


def summaries_after_every_row(g, c):
    """The restatement's summary_stats after every episode, [N,5] (NaN: no value yet), and the counts."""
    m, rows = replay_case(g, c)
    fresh = er.LogModel(m.B, m.capacity, m.polyak, m.reward_possible)
    fresh.rows[:len(rows)] = rows
    stats, counts = [], []
    for n in range(len(rows)):
        fresh.n_rows = n + 1
        fresh.summarise()
        stats.append([v if k else er.NAN for v, k in zip(fresh.value, fresh.count)])
        counts.append(list(fresh.count))
    return np.array(stats), np.array(counts), m


def deviation(got, want):
    """Largest |got - want| over the finite entries; the others must be of the same kind."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
    return float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0


def test_summaries_within_the_measured_bound(golden):
    """log_scalars() after every episode of every case; see the module docstring for the two numbers."""
    worst, run_worst = 0.0, 0.0
    for c in case_names(golden):
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


def test_one_call_equals_many_calls(golden):
    m, rows = replay_case(golden, "polyak1")
    m.summarise()
    stats, _, _ = summaries_after_every_row(golden, "polyak1")
    assert er.same_floats(m.value, stats[-1])
    assert m.summary()["training/episodes"] == len(rows) and m.summarised == len(rows)


def test_ring_and_chain_of_the_restatement(golden):
    """A ring shorter than the run: old rows go, the run summary covers what is left, and an entry of an overwritten or a
    never-logged episode finds nothing."""
    g, c = golden, "polyak1"
    full, rows = replay_case(g, c)
    m, _ = replay_case(g, c, capacity=16)
    assert er.same_floats(m.run_summary(0), m.run_summary(len(rows) - 16))
    tail = er.LogModel(m.B, len(rows), m.polyak, m.reward_possible)
    tail.rows[:len(rows)], tail.n_rows = rows, len(rows)
    assert er.same_floats(m.run_summary(0), tail.run_summary(len(rows) - 16))
    first_env, first_idx = int(rows["env"][0]), int(rows["episode_idx"][0])
    N = len(rows)
    assert full.find(int(rows["env"][N - 1]), int(rows["episode_idx"][N - 1])) == N - 1
    assert m.find(int(rows["env"][N - 1]), int(rows["episode_idx"][N - 1])) == (N - 1) % 16
    assert m.find(first_env, first_idx) is None                         # overwritten
    assert (rows["env"] == first_env).sum() > er.MAX_HOPS and full.find(first_env, first_idx) is None   # too far back
    nth = np.flatnonzero(rows["env"] == first_env)[-er.MAX_HOPS:]        # the last MAX_HOPS rows of the env are in reach
    assert full.find(first_env, int(rows["episode_idx"][nth[0]])) == nth[0]
    assert full.find(first_env, int(rows["episode_idx"][nth[0]]) - 1) is None
    assert m.find(first_env, 10 ** 6) is None and m.find(-1, 0) is None and m.find(m.B, 0) is None


def test_entry_totals():
    w = [(9, 1.0), (0x209, 0.5), (9, 0.25)]
    keys = np.full(24, 0xFFFF, np.uint16)
    keys[[0, 3, 5]] = [9, 0x209, 0x409]
    scores = np.full((24, 2), np.nan)
    scores[0], scores[3], scores[5] = [0.3, 2.0], [np.nan, 4.0], [7.0, 7.0]
    n_cells = np.zeros(24, np.int32)
    assert er.entry_totals(w, keys, scores, n_cells) == [0.0 + 1.25 * 0.3 + 0.0 * 7.0, 0.0 + 1.25 * 2.0 + 0.5 * 4.0 + 0.0 * 7.0]
    n_cells[0] = -1
    assert all(np.isnan(er.entry_totals(w, keys, scores, n_cells)))
    assert er.entry_totals([], keys, scores, np.zeros(24, np.int32)) == [0.0, 0.0]


# --------------------------------------------------------------------------------------------------------- the Python class

@pytest.fixture(scope="module")
def pool():
    return util.pool_from_fixture("prune_still_25", util.oracle_counts, n=12)


def test_constructor_errors_and_defaults(pool):
    pool, ref = pool
    EL = episode_log.EpisodeLog
    log = EL(pool, 8, 8)
    assert log.summary_polyak == 0.99 and EL(pool, 8, 64, episode_type="validation").summary_polyak == 1.0
    assert EL(pool, 8, 64, episode_type="benchmark").summary_polyak == 1.0
    assert EL(pool, 8, 64, episode_type="validation", summary_polyak=0.5).summary_polyak == 0.5
    assert np.array_equal(log.available, ref["initial_available_points"][:12].reshape(12, -1)[:, 0])
    assert np.array_equal(log.reward_possible(3), log.available + 3)
    with pytest.raises(ValueError, match="capacity"):
        EL(pool, 8, 7)
    with pytest.raises(ValueError):
        EL(pool, 0, 8)
    with pytest.raises(TypeError):
        EL(None, 8, 8)
    for p in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="polyak"):
            EL(pool, 8, 8, summary_polyak=p)
    with pytest.raises(ValueError, match="weights"):
        EL(pool, 8, 8, side_effect_weights={"life-%d" % k: 1.0 for k in range(25)})
    w = EL(pool, 8, 8, side_effect_weights={"life-green": 1.0, "spawner-yellow": 0.5})._weights
    assert (w.n, w.cell[0], w.cell[1], w.weight[0], w.weight[1]) == (2, 0x409, 152 | 0x600, 1.0, 0.5)
    for call in (log.summary, log.rows, log.counters):
        with pytest.raises(ValueError, match="no device state"):
            call()
    with pytest.raises(ValueError, match="not attached"):
        log.flush()


def test_multi_agent_pools_are_refused():
    from safelife_amd import levels
    multi = object.__new__(levels.LevelPool)        # (refused on n_agents alone, before anything of the pool is read)
    multi.n_agents = 2
    with pytest.raises(ValueError, match="single-agent"):
        episode_log.EpisodeLog(multi, 8, 8)


def test_stepping_modes_refuse_an_episode_log():
    """Slice, queue and rollout() stepping refuse a log before they touch anything, in the schedule's wording."""
    from safelife_amd.vector_env import SafeLifeVectorEnv
    env = object.__new__(SafeLifeVectorEnv)
    env.level_schedule, env.episode_log, env._queues = None, object(), None
    for call in (lambda: env.rollout(None), lambda: env.step_async(0), lambda: env.step_slice(0, 0),
                 lambda: env.step_queues(0), lambda: env.step_queues_many(0), lambda: env.queues_open(),
                 lambda: env.set_step_outputs(1)):
        with pytest.raises(ValueError, match="cannot drive an episode log: .* \\(use step\\(\\)\\)"):
            call()


def test_records_against_the_fixtures_log_data(golden):
    g, c = golden, "polyak1"
    _, rows = replay_case(g, c)
    names = ["level-%d" % n for n in range(len(rows))]
    recs = episode_log.rows_to_records(rows, names)
    assert len(recs) == len(rows)
    for n, d in enumerate(recs):
        assert list(d) == ["length", "reward", "success", "side_effects", "level_name", "reward_possible", "reward_needed"]
        assert d["level_name"] == "level-%d" % n and d["length"] == int(g[c + "_length"][n])
        assert d["reward"] == float(g[c + "_reward"][n]) and d["success"] is bool(g[c + "_success"][n])
        assert d["reward_possible"] == int(g[c + "_reward_possible"][n]) and d["reward_needed"] == int(g[c + "_reward_needed"][n])
        assert er.same_floats(d["side_effects"]["total"], g[c + "_total"][n])
    _, bare = replay_case(g, c, join=False)
    assert all("side_effects" not in d for d in episode_log.rows_to_records(bare, names))
