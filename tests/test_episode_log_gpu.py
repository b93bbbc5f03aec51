"""
The episode log on the device (csrc/sl_episode_log.hip, safelife_amd/episode_log.py): every kernel against the host
restatement of tests/episode_log_ref.py BIT FOR BIT, fed what the device was fed, and a SafeLifeVectorEnv with a log against
the restatement fed the run's own step records and side-effect batches.  Against the reference's logger the summaries hold
the bounds measured in tests/test_episode_log_host.py (the restatement meets them on the host; the kernels equal the
restatement).
"""
import ctypes as C

import numpy as np
import pytest

from safelife_amd import _hip, episode_log, schedule
from tests import episode_log_ref as er
from tests import util
from tests.test_episode_log_host import RUN_BOUND, SUMMARY_BOUND, deviation, golden, replay_case  # noqa: F401

pytestmark = pytest.mark.gpu

HARVEST_TILE = 256 * 64
COLS = _hip.SCALAR_COLS


def _torch():
    import torch
    return torch


class DeviceLog(object):
    """A struct sl_episode_log with its device arrays, fresh."""

    def __init__(self, B, capacity, polyak, reward_possible, weights=()):
        torch, dev = _torch(), _hip.device()
        self.B, self.capacity = B, capacity
        t = self.t = {}
        t["rows"] = torch.zeros((capacity, 12), dtype=torch.int64, device=dev)
        t["rows"][:, 0] = -1
        t["counters"] = torch.zeros(5, dtype=torch.int64, device=dev)
        for name in ("cur_slot", "cur_required", "cur_episode"):
            t[name] = torch.zeros(B, dtype=torch.int32, device=dev)
        t["last_row"] = torch.full((B,), -1, dtype=torch.int64, device=dev)
        t["reward_possible"] = torch.from_numpy(np.asarray(reward_possible, np.int32)).to(dev)
        t["value"] = torch.zeros(5, dtype=torch.float64, device=dev)
        t["count"] = torch.zeros(5, dtype=torch.int64, device=dev)
        t["weight"] = torch.zeros(5, dtype=torch.float64, device=dev)
        t["run"] = torch.full((_hip.LOG_RUN_SUMMARY,), -1.0, dtype=torch.float64, device=dev)
        s = self.struct = _hip.EpisodeLog()
        s.capacity, s.B, s.L, s.polyak = capacity, B, len(reward_possible), polyak
        for name, ctype in _hip.EpisodeLog._fields_:
            if ctype is C.c_void_p:
                setattr(s, name, t[name].data_ptr())
        self.ref, self.lib = C.byref(s), _hip.lib()
        w = self.weights = _hip.LogWeights()
        w.n = len(weights)
        for j, (cell, weight) in enumerate(weights):
            w.cell[j], w.weight[j] = cell, weight

    def host(self, name):
        a = self.t[name].cpu().numpy()
        return a.view(er.ROW_DTYPE).reshape(-1) if name == "rows" else a

    def put_rows(self, rows, n_rows):
        """Rows (global indices n_rows - len(rows) .. n_rows - 1) into their ring places; n_rows into the counter."""
        torch = _torch()
        ring = self.host("rows").copy()
        ring[np.arange(n_rows - len(rows), n_rows) % self.capacity] = rows
        self.t["rows"].copy_(torch.from_numpy(ring.view(np.int64).reshape(self.capacity, 12)))
        self.t["counters"][0] = n_rows

    def rewind(self, scalars, mask=None):
        torch = _torch()
        sel = torch.ones(self.B, dtype=torch.bool, device=scalars.device) if mask is None else torch.from_numpy(mask != 0).to(scalars.device)
        for name, col in (("cur_slot", "level_idx"), ("cur_required", "required_points"), ("cur_episode", "episode_idx")):
            self.t[name][sel] = scalars[:, COLS[col]][sel]
        self.t["last_row"][sel] = -1

    def harvest(self, out, scalars):
        _hip.check(self.lib.slhip_episode_log_harvest(self.ref, _hip.ptr(out), _hip.ptr(scalars), self.B,
                                                      _hip.current_stream_ptr()))

    def join(self, count, records, scores, keys, n_cells):
        q = _hip.EpisodeQueue()
        q.capacity, q.count, q.records = records.shape[0], count.data_ptr(), records.data_ptr()
        _hip.check(self.lib.slhip_episode_log_join(self.ref, C.byref(q), _hip.ptr(scores), _hip.ptr(keys), _hip.ptr(n_cells),
                                                   C.byref(self.weights), _hip.current_stream_ptr()))

    def summarise(self):
        _hip.check(self.lib.slhip_episode_log_summaries(self.ref, _hip.current_stream_ptr()))

    def run_summary(self, first):
        _hip.check(self.lib.slhip_episode_log_run_summary(self.ref, first, _hip.ptr(self.t["run"]), _hip.current_stream_ptr()))
        return self.host("run")


def assert_state_equal(d, m, where):
    er.assert_rows_equal(d.host("rows"), m.rows)
    assert d.host("counters").tolist() == [m.n_rows, m.steps, m.episodes, m.summarised, m.unmatched], where
    for name in ("cur_slot", "cur_required", "cur_episode", "last_row"):
        assert np.array_equal(d.host(name), getattr(m, name)), (where, name)


def assert_summaries_equal(d, m):
    assert er.same_floats(d.host("value"), m.value) and er.same_floats(d.host("weight"), m.weight)
    assert d.host("count").tolist() == m.count


def scalars_dict(sc):
    return {k: sc[:, COLS[k]].copy() for k in ("level_idx", "required_points", "episode_idx")}


def out_dict(raw):
    """int32 [B,4] struct sl_step_out rows -> the restatement's arrays."""
    flags = raw[:, 1:2].copy().view(np.uint8)
    return dict(done=flags[:, 0], success=flags[:, 1], times_up=flags[:, 2],
                episode_reward=raw[:, 2].copy().view(np.float32), episode_length=raw[:, 3].copy())


# ----------------------------------------------------------------------------------------------------------------- harvest

def _random_step(rng, B, L, done):
    """Step records [B,4] with the records of the envs that are not done poisoned, and scalars [B,16] after the step."""
    raw = np.zeros((B, 4), np.int32)
    flags = np.zeros((B, 4), np.uint8)
    flags[:, 0] = done
    flags[:, 1], flags[:, 2] = rng.integers(0, 2, B), rng.integers(0, 2, B)
    reward = (rng.integers(-40, 200, B) * 0.25).astype(np.float32)
    length = rng.integers(0, 1002, B).astype(np.int32)
    poison = done == 0
    flags[poison, 1:] = 0xA5
    reward[poison], length[poison] = np.float32(np.nan), -99
    raw[:, 0] = np.float32(1.5).view(np.int32)
    raw[:, 1] = flags.view(np.int32)[:, 0]
    raw[:, 2], raw[:, 3] = reward.view(np.int32), length
    sc = rng.integers(0, 1000, (B, 16)).astype(np.int32)
    sc[:, COLS["level_idx"]] = rng.integers(0, L, B)
    sc[rng.random(B) < 0.02, COLS["level_idx"]] = rng.choice([-1, L, L + 7])        # (no such slot: reward_possible 0)
    return raw, sc


@pytest.mark.parametrize("B", [1, 63, 64, 65, HARVEST_TILE + 1])
def test_harvest_equals_the_model(B):
    """No env done, every env done, random halves; capacity = B, so the ring wraps (at least 3 B episodes); the records of the
    envs that are not done are poisoned; the stamps are steps + e + 1; a rewind of some envs in the middle."""
    torch, dev = _torch(), _hip.device()
    rng = np.random.default_rng(B)
    L = 37
    possible = rng.integers(0, 90, L).astype(np.int32)
    possible[:2] = [0, 1]
    d, m = DeviceLog(B, B, 0.99, possible), er.LogModel(B, B, 0.99, possible)
    _, sc = _random_step(rng, B, L, np.zeros(B, np.uint8))
    d.rewind(torch.from_numpy(sc).to(dev)), m.rewind(scalars_dict(sc))
    plans = ["none", "all", "half", "half", "rewind", "half", "all", "all"]
    for t, plan in enumerate(plans):
        if plan == "rewind":
            mask = (rng.random(B) < 0.4).astype(np.uint8)
            _, sc = _random_step(rng, B, L, np.zeros(B, np.uint8))
            d.rewind(torch.from_numpy(sc).to(dev), mask), m.rewind(scalars_dict(sc), mask)
            assert_state_equal(d, m, (t, plan))
            continue
        done = {"none": np.zeros(B), "all": np.ones(B), "half": rng.random(B) < 0.5}[plan].astype(np.uint8)
        raw, sc = _random_step(rng, B, L, done)
        d.harvest(torch.from_numpy(raw).to(dev), torch.from_numpy(sc).to(dev))
        m.harvest(out_dict(raw), scalars_dict(sc))
        assert_state_equal(d, m, (t, plan))
    assert m.n_rows >= 3 * B and m.steps == 7 * B
    rows = d.host("rows")
    live = rows[np.arange(m.n_rows - B, m.n_rows) % B]
    assert np.array_equal(live["index"], np.arange(m.n_rows - B, m.n_rows))
    assert np.array_equal(live["training_steps"], 6 * B + live["env"] + 1)       # the last call: every env, in env order
    assert np.isnan(live["score"]).all() and not live["flags"].any()


# -------------------------------------------------------------------------------------------------------------------- join

CELLS = [9, 0x209, 0x409, 0x609, 152 | 0x600, 48, 16]


def test_join_equals_the_model_and_counts_what_it_cannot_place():
    """4 envs, a ring of 12 rows, 5 steps that end every episode: 20 episodes, the last three of every env in the ring.  The
    queue holds all 20 in scrambled order (three episodes of one env in one queue), entries of episodes that never got a
    row and of envs outside the batch; key lists empty, cut short, with NaN and infinite scores."""
    torch, dev = _torch(), _hip.device()
    rng = np.random.default_rng(7)
    B, cap, L, K, Cq = 4, 12, 5, _hip.SL_SE_MAX_KEYS, 40
    possible = np.array([0, 1, 10, 25, 60], np.int32)
    weights = [(9, 1.0), (0x409, 0.5), (9, 0.25), (48, -2.0)]
    d, m = DeviceLog(B, cap, 1.0, possible, weights), er.LogModel(B, cap, 1.0, possible, weights)
    _, sc = _random_step(rng, B, L, np.zeros(B, np.uint8))
    sc[:, COLS["episode_idx"]] = 0
    d.rewind(torch.from_numpy(sc).to(dev)), m.rewind(scalars_dict(sc))
    for t in range(5):
        raw, sc = _random_step(rng, B, L, np.ones(B, np.uint8))
        sc[:, COLS["episode_idx"]] = t + 1
        d.harvest(torch.from_numpy(raw).to(dev), torch.from_numpy(sc).to(dev))
        m.harvest(out_dict(raw), scalars_dict(sc))
    entries = [(e, k) for e in range(B) for k in range(5)]              # (env, episode_idx): k < 2 has been overwritten
    entries += [(0, 10 ** 6), (3, 5), (-1, 0), (B, 0), (2, -1)]           # never logged; no such env
    want_unmatched = 2 * B + 5
    rng.shuffle(entries)
    n = len(entries)
    rec = np.zeros((Cq, 8), np.int32)
    rec[:n, 0], rec[:n, 3] = [e for e, _ in entries], [k for _, k in entries]
    rec[n:, 0], rec[n:, 3] = 1, 10 ** 6 + np.arange(Cq - n)             # (past the count: not read by the first join)
    keys = np.full((Cq, K), 0xFFFF, np.uint16)
    scores = np.full((Cq, K, 2), np.nan)
    n_cells = np.zeros((Cq, K), np.int32)
    for i in range(Cq):
        kind = i % 5
        if kind == 0:
            continue                                                    # an empty key list: totals 0, 0
        slots = rng.choice(K, rng.integers(1, 9), replace=False)
        keys[i, slots] = rng.choice(CELLS, len(slots))
        scores[i, slots] = rng.random((len(slots), 2)) * 4
        if kind == 1:
            scores[i, slots[0], rng.integers(0, 2)] = np.nan            # a NaN score contributes nothing
        if kind == 2:
            n_cells[i, 0] = -1                                          # cut short: NaN totals
        if kind == 3 and i % 2:
            scores[i, slots[0], 0] = np.inf
        n_cells[i, 1:] = rng.integers(0, 600, K - 1)
    dev_args = [torch.from_numpy(a).to(dev) for a in (np.array([n], np.int32), rec, scores, keys.view(np.int16), n_cells)]
    d.join(*dev_args)
    m.join(n, dict(env=rec[:, 0], episode_idx=rec[:, 3]), scores, keys, n_cells)
    assert m.unmatched == want_unmatched
    assert_state_equal(d, m, "join")
    rows = d.host("rows")
    assert (rows["flags"] & 1).sum() == n - want_unmatched == 3 * B
    # a count past the capacity is the capacity; the same entries joined again change nothing but `unmatched`
    d.t["counters"][4] = 0
    m.unmatched = 0
    dev_args[0] = torch.from_numpy(np.array([Cq + 5], np.int32)).to(dev)
    d.join(*dev_args)
    m.join(Cq + 5, dict(env=rec[:, 0], episode_idx=rec[:, 3]), scores, keys, n_cells)
    assert m.unmatched == want_unmatched + Cq - n
    assert_state_equal(d, m, "join again")
    d.summarise(), m.summarise()
    assert_summaries_equal(d, m)


# --------------------------------------------------------------------------------------------- summaries and the run summary

@pytest.fixture(scope="module")
def cases(golden):  # noqa: F811
    """Per fixture case: the restatement's rows in log order and the fixture."""
    return {str(c): replay_case(golden, str(c))[1] for c in golden["cases"]}


@pytest.mark.parametrize("c", ["nosuccess", "polyak0", "polyak099", "polyak1"])
def test_summaries_over_the_fixture(golden, cases, c):  # noqa: F811
    """The fixture's rows uploaded: one call over all of them, and many calls over the same rows (cuts at the staging
    batch's edges), equal the restatement bit for bit and each other; and the reference within the measured bound."""
    rows, polyak = cases[c], float(golden[c + "_polyak"])
    N = len(rows)
    one, many, m = DeviceLog(2, N, polyak, [1]), DeviceLog(2, N, polyak, [1]), er.LogModel(2, N, polyak, [1])
    m.rows[:], m.n_rows = rows, N
    m.summarise()
    one.put_rows(rows, N)
    one.summarise()
    assert_summaries_equal(one, m)
    assert one.host("counters")[3] == N
    many.put_rows(rows, N)
    worst = 0.0
    for cut in sorted({1, 2, min(N, 255), min(N, 256), min(N, 257), min(N, 513), N // 2, N}):
        many.t["counters"][0] = cut
        many.summarise()
        got = np.where(many.host("count") > 0, many.host("value"), np.nan)
        worst = max(worst, deviation(got, golden[c + "_stats"][cut - 1]))
        assert np.array_equal(many.host("count"), golden[c + "_counts"][cut - 1])
    assert_summaries_equal(many, m)
    print("%s: largest |device - reference| of the summaries at the cuts: %r" % (c, worst))
    assert worst <= SUMMARY_BOUND
    one.summarise()                                                      # nothing new: nothing moves
    assert_summaries_equal(one, m)


@pytest.mark.parametrize("c", ["nosuccess", "polyak0", "polyak099", "polyak1"])
def test_run_summary_over_the_fixture(golden, cases, c):  # noqa: F811
    rows = cases[c]
    N = len(rows)
    d, m = DeviceLog(2, N, 1.0, [1]), er.LogModel(2, N, 1.0, [1])
    m.rows[:], m.n_rows = rows, N
    d.put_rows(rows, N)
    for first in (0, -7, 5, N - 1, N, N + 3):
        assert er.same_floats(d.run_summary(first), m.run_summary(first)), first
    worst = deviation(d.run_summary(0), golden[c + "_run"])
    print("%s: largest |device - reference| of the run summary: %r" % (c, worst))
    assert worst <= RUN_BOUND
    # a ring that has lost its oldest rows: ranges that begin before the ring's oldest row start there
    cap = max(2, min(300, N // 2))
    ring, rm = DeviceLog(2, cap, 1.0, [1]), er.LogModel(2, cap, 1.0, [1])
    rm.rows[np.arange(N - cap, N) % cap], rm.n_rows = rows[N - cap:], N
    ring.put_rows(rows[N - cap:], N)
    for first in (0, N - cap - 1, N - cap, N - cap + 1, N - 3):
        got = ring.run_summary(first)
        assert er.same_floats(got, rm.run_summary(first)), first
        assert er.same_floats(got, m.run_summary(max(first, N - cap))), first


# ------------------------------------------------------------------------------------------------------------- end to end

B_E2E, T_E2E, N_LEVELS = 65, 60, 12
WEIGHTS = {"life-green": 1.0, "life-red": 0.5, "crate-gray": 2.0, "life-yellow": 1.0}
ENV_KW = dict(time_limit=5, view_shape=(15, 15), auto_reset=True)


def _run_logged(queue_capacity, sched=None, flushes=(19, 39, 59)):
    """60 steps of 65 envs with a log; the restatement is fed the per-step records read back and, at every flush, the
    batch's own records, keys and scores.  -> env, log, model, per-flush (ended, batch records, joined rows)."""
    from safelife_amd.vector_env import SafeLifeVectorEnv
    from safelife_amd.side_effects import name_to_cell
    pool = sched.pool if sched is not None else util.pool_from_fixture("prune_still_25", util.oracle_counts, n=N_LEVELS)[0]
    log = episode_log.EpisodeLog(pool, B_E2E, 1024, side_effect_weights=WEIGHTS)
    env = SafeLifeVectorEnv(pool, B_E2E, episode_log=log, level_schedule=sched,
                            side_effects=dict(capacity=queue_capacity, num_samples=8), **ENV_KW)
    env.reset()
    m = er.LogModel(B_E2E, 1024, 0.99, log.reward_possible(1), [(name_to_cell(k), w) for k, w in WEIGHTS.items()])
    m.rewind(scalars_dict(env.t["scalars"].cpu().numpy()))
    actions = np.random.default_rng(21).integers(0, 9, (T_E2E, B_E2E)).astype(np.int32)
    per_flush, ended = [], 0
    for t in range(T_E2E):
        if sched is not None:
            sched.training_steps = t
        env.step(actions[t])
        raw = env.t["out"].cpu().numpy()
        m.harvest(out_dict(raw), scalars_dict(env.t["scalars"].cpu().numpy()))
        ended += int(out_dict(raw)["done"].astype(bool).sum())
        if t in flushes:
            before = log.rows()["flags"] & 1
            batch = log.flush()
            emd = batch.scores_all()
            rec = batch.records()
            count = int(batch.count.item())
            m.join(count, dict(env=batch.rec_tensor[:, 0].cpu().numpy(), episode_idx=batch.rec_tensor[:, 3].cpu().numpy()),
                   emd["scores"].cpu().numpy(), batch.keys.cpu().numpy().view(np.uint16), emd["n_cells"].cpu().numpy())
            m.summarise()
            after = log.rows()["flags"] & 1
            per_flush.append(dict(ended=ended, count=count, dropped=batch.dropped(), rec=rec,
                                  newly_joined=int(after.sum() - before.sum()), batch=batch, emd=emd))
            ended = 0
    return env, log, m, per_flush


def _assert_log_equals_model(log, m):
    er.assert_rows_equal(log.rows(0), m.row_range(0))
    assert log.counters() == m.counters()
    got, want = log.summary(), m.summary()
    assert list(got) == list(want)
    assert er.same_floats([got[k] for k in got], [want[k] for k in want])
    assert er.same_floats(np.array([log.run_summary(0)[k] for k in episode_log.RUN_SUMMARY_FIELDS], np.float64),
                          m.run_summary(0))


def test_end_to_end_equals_the_model():
    env, log, m, per_flush = _run_logged(1024)
    assert all(f["dropped"] == 0 and f["count"] == f["ended"] == f["newly_joined"] for f in per_flush)
    c = log.counters()
    assert c["unmatched"] == 0 and c["steps"] == T_E2E * B_E2E and c["episodes"] == c["n_rows"] >= 10 * B_E2E
    assert c["summarised"] == c["n_rows"]
    _assert_log_equals_model(log, m)
    rows = log.rows()
    assert (rows["flags"] & 1).all() and np.isfinite(rows["score"]).all()
    assert np.array_equal(rows["reward_possible"], log.reward_possible(1)[rows["level"]])
    assert set(log.summary()) == {"training/" + k for k in _hip.LOG_KEYS + ("steps", "episodes")}
    recs = log.records()
    assert len(recs) == len(rows) and recs[0]["side_effects"]["total"] == rows["side_effects"][0].tolist()


def test_end_to_end_under_a_level_schedule():
    """reward_needed follows min_performance_fraction: the rows carry the required points of the episode they describe."""
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=N_LEVELS)[0]
    sched = schedule.LevelSchedule(pool, [(0, 6), (6, 6)], mode="uniform", seed=5,
                                   min_performance_fraction=lambda t: 0.001 if t < 20 else 1.0)
    env, log, m, per_flush = _run_logged(1024, sched=sched)
    assert all(f["dropped"] == 0 and f["count"] == f["ended"] for f in per_flush) and log.counters()["unmatched"] == 0
    _assert_log_equals_model(log, m)
    rows = log.rows()
    assert len(set(zip(rows["level"].tolist(), rows["reward_needed"].tolist()))) > len(set(rows["level"].tolist()))
    assert sched.stats()["episodes"].sum() == len(rows)


def test_end_to_end_with_a_queue_that_overflows():
    """A queue of 2: which episodes it keeps is the arrival order of an atomic, so exactly min(ended, 2) rows per flush carry
    the joined flag, each joined row is right for its entry, and the summaries are the restatement's fed the same entries."""
    env, log, m, per_flush = _run_logged(2)
    rows = log.rows()
    by_episode = {(int(r["env"]), int(r["episode_idx"])): r for r in rows}
    weights = m.weights
    for f in per_flush:
        kept = min(f["ended"], 2)
        assert f["count"] == f["ended"] and f["dropped"] == f["ended"] - kept and f["newly_joined"] == kept
        keys = f["batch"].keys.cpu().numpy().view(np.uint16)
        scores, n_cells = f["emd"]["scores"].cpu().numpy(), f["emd"]["n_cells"].cpu().numpy()
        for i in range(kept):
            r = by_episode[(int(f["rec"]["env"][i]), int(f["rec"]["episode_idx"][i]))]
            total = er.entry_totals(weights, keys[i], scores[i], n_cells[i])
            frac, score = er.combined(total[0], total[1], float(r["reward_frac"]), r["length"])
            assert r["flags"] & 1 and er.same_floats(r["side_effects"], total)
            assert er.same_floats([r["side_effects_frac"], r["score"]], [frac, score])
            assert (r["level"], r["length"]) == (f["rec"]["level"][i], f["rec"]["episode_length"][i])
    assert (rows["flags"] & 1).sum() == sum(min(f["ended"], 2) for f in per_flush) and log.counters()["unmatched"] == 0
    _assert_log_equals_model(log, m)
    s = log.summary()
    assert s["training/episodes"] == len(rows) and "training/score" in s


def test_without_a_log_nothing_changes():
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=N_LEVELS)[0]
    actions = np.random.default_rng(5).integers(0, 9, (20, B_E2E)).astype(np.int32)
    one = SafeLifeVectorEnv(pool, B_E2E, episode_log=None, **ENV_KW)
    two = SafeLifeVectorEnv(pool, B_E2E, **ENV_KW)
    logged = SafeLifeVectorEnv(pool, B_E2E, episode_log=episode_log.EpisodeLog(pool, B_E2E, 128), **ENV_KW)
    assert one.episode_log is None and two.episode_log is None and sorted(one.t) == sorted(two.t)
    envs = (one, two, logged)
    obs = [e.reset().cpu().numpy() for e in envs]
    assert np.array_equal(obs[0], obs[1]) and np.array_equal(obs[0], obs[2])
    for t in range(len(actions)):
        for e in envs:
            e.step(actions[t])
        for name in ("reward", "done", "obs", "board", "level_idx", "success", "rng"):
            assert np.array_equal(one.numpy(name), two.numpy(name)), (t, name)
            assert np.array_equal(one.numpy(name), logged.numpy(name)), (t, name)
    assert one.steps_dispatched == two.steps_dispatched == logged.steps_dispatched == len(actions)
    c = logged.episode_log.counters()
    assert c["steps"] == len(actions) * B_E2E and c["episodes"] >= 4 * B_E2E       # time_limit 5: at least four ends in 20 steps
    with pytest.raises(ValueError, match="already serves"):
        SafeLifeVectorEnv(pool, B_E2E, episode_log=logged.episode_log, **ENV_KW)
    with pytest.raises(ValueError, match="built for 8 envs"):
        SafeLifeVectorEnv(pool, B_E2E, episode_log=episode_log.EpisodeLog(pool, 8, 128), **ENV_KW)
    logged.episode_log.flush()                          # no queue: only length, reward and success ever count
    s = logged.episode_log.summary()
    assert "training/length" in s and "training/score" not in s and "training/side_effects" not in s
