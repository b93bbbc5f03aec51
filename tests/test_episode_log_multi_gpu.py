"""
The multi-agent episode log on the device (csrc/sl_episode_log.hip, safelife_amd.episode_log.MultiAgentEpisodeLog): every
kernel against the host restatement of tests/episode_log_multi_ref.py BIT FOR BIT, fed what the device was fed, and a
SafeLifeMultiAgentVectorEnv with a log against the restatement fed the run's own step records and side-effect batches.
Against the reference's logger the summaries hold the bounds measured in tests/test_episode_log_multi_host.py (the
restatement meets them on the host; the kernels equal the restatement).
"""
import ctypes as C

import numpy as np
import pytest

from safelife_amd import _hip, episode_log, schedule
from tests import episode_log_multi_ref as emr
from tests import episode_log_ref as er
from tests.test_episode_log_host import deviation
from tests.test_episode_log_multi_host import CASES, RUN_BOUND, SUMMARY_BOUND, golden, replay_case  # noqa: F401

pytestmark = pytest.mark.gpu

HARVEST_TILE = 256 * 64
COLS, ACOLS = _hip.SCALAR_COLS, _hip.AGENT_COLS
NQ = _hip.LOG_MAX_NAMES * len(_hip.LOG_MULTI_KEYS)


def _torch():
    import torch
    return torch


class DeviceLog(object):
    """A struct sl_episode_log_multi with its device arrays, fresh."""

    def __init__(self, B, A, capacity, polyak, reward_possible, name_id, n_names, weights=()):
        torch, dev = _torch(), _hip.device()
        self.B, self.A, self.capacity, self.dtype = B, A, capacity, emr.row_dtype(A)
        self.words = self.dtype.itemsize // 8
        reward_possible = np.asarray(reward_possible, np.int32).reshape(-1, A)
        t = self.t = {}
        t["rows"] = torch.zeros((capacity, self.words), dtype=torch.int64, device=dev)
        t["rows"][:, 0] = -1
        t["counters"] = torch.zeros(5, dtype=torch.int64, device=dev)
        t["cur_slot"], t["cur_episode"] = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
        t["cur_required"] = torch.zeros((B, A), dtype=torch.int32, device=dev)
        t["last_row"] = torch.full((B,), -1, dtype=torch.int64, device=dev)
        t["reward_possible"] = torch.from_numpy(reward_possible).to(dev)
        t["name_id"] = torch.from_numpy(np.asarray(name_id, np.uint8).reshape(-1, A)).to(dev)
        t["value"] = torch.zeros(NQ, dtype=torch.float64, device=dev)
        t["count"] = torch.zeros(NQ, dtype=torch.int64, device=dev)
        t["weight"] = torch.zeros(NQ, dtype=torch.float64, device=dev)
        t["run"] = torch.full((_hip.LOG_RUN_SUMMARY,), -1.0, dtype=torch.float64, device=dev)
        s = self.struct = _hip.EpisodeLogMulti()
        s.capacity, s.B, s.L, s.n_agents, s.n_names, s.polyak = capacity, B, len(reward_possible), A, n_names, polyak
        for name, ctype in _hip.EpisodeLogMulti._fields_:
            if ctype is C.c_void_p:
                setattr(s, name, t[name].data_ptr())
        self.ref, self.lib = C.byref(s), _hip.lib()
        w = self.weights = _hip.LogWeights()
        w.n = len(weights)
        for j, (cell, weight) in enumerate(weights):
            w.cell[j], w.weight[j] = cell, weight

    def host(self, name):
        a = self.t[name].cpu().numpy()
        return a.view(self.dtype).reshape(-1) if name == "rows" else a

    def put_rows(self, rows, n_rows):
        """Rows (global indices n_rows - len(rows) .. n_rows - 1) into their ring places; n_rows into the counter."""
        torch = _torch()
        ring = self.host("rows").copy()
        ring[np.arange(n_rows - len(rows), n_rows) % self.capacity] = rows
        self.t["rows"].copy_(torch.from_numpy(ring.view(np.int64).reshape(self.capacity, self.words)))
        self.t["counters"][0] = n_rows

    def rewind(self, agents, scalars, mask=None):
        torch = _torch()
        sel = torch.ones(self.B, dtype=torch.bool, device=scalars.device) if mask is None else torch.from_numpy(mask != 0).to(scalars.device)
        self.t["cur_slot"][sel] = scalars[:, COLS["level_idx"]][sel]
        self.t["cur_episode"][sel] = scalars[:, COLS["episode_idx"]][sel]
        self.t["cur_required"][sel] = agents[:, :, ACOLS["required_points"]][sel]
        self.t["last_row"][sel] = -1

    def harvest(self, out, agents, scalars):
        _hip.check(self.lib.slhip_episode_log_harvest_multi(self.ref, _hip.ptr(out), _hip.ptr(agents), _hip.ptr(scalars),
                                                            self.B, _hip.current_stream_ptr()))

    def join(self, count, records, scores, keys, n_cells):
        q = _hip.EpisodeQueue()
        q.capacity, q.count, q.records = records.shape[0], count.data_ptr(), records.data_ptr()
        _hip.check(self.lib.slhip_episode_log_join_multi(self.ref, C.byref(q), _hip.ptr(scores), _hip.ptr(keys),
                                                         _hip.ptr(n_cells), C.byref(self.weights), _hip.current_stream_ptr()))

    def summarise(self):
        _hip.check(self.lib.slhip_episode_log_summaries_multi(self.ref, _hip.current_stream_ptr()))

    def run_summary(self, first):
        _hip.check(self.lib.slhip_episode_log_run_summary_multi(self.ref, first, _hip.ptr(self.t["run"]),
                                                                _hip.current_stream_ptr()))
        return self.host("run")


def assert_state_equal(d, m, where):
    emr.assert_rows_equal(d.host("rows"), m.rows)
    assert d.host("counters").tolist() == [m.n_rows, m.steps, m.episodes, m.summarised, m.unmatched], where
    for name in ("cur_slot", "cur_required", "cur_episode", "last_row"):
        assert np.array_equal(d.host(name), getattr(m, name)), (where, name)


def assert_summaries_equal(d, m):
    assert er.same_floats(d.host("value"), m.value) and er.same_floats(d.host("weight"), m.weight)
    assert d.host("count").tolist() == m.count


def scalars_dict(sc, agents):
    return dict(level_idx=sc[:, COLS["level_idx"]].copy(), episode_idx=sc[:, COLS["episode_idx"]].copy(),
                required_points=agents[:, :, ACOLS["required_points"]].copy())


def out_dict(raw):
    """int32 [B,A,4] struct sl_step_out records -> the restatement's arrays [B,A]."""
    flags = raw[:, :, 1:2].copy().view(np.uint8)
    return dict(done=flags[:, :, 0], success=flags[:, :, 1], times_up=flags[:, :, 2],
                episode_reward=raw[:, :, 2].copy().view(np.float32), episode_length=raw[:, :, 3].copy())


# ----------------------------------------------------------------------------------------------------------------- harvest

def _random_step(rng, B, A, L, done):
    """Step records [B,A,4] for done flags [B,A] -- of an env that has NOT finished everything but the done bytes is
    poisoned, its done agents' records included -- and agent states [B,A,12] and scalars [B,16] after the step."""
    raw = np.zeros((B, A, 4), np.int32)
    flags = np.zeros((B, A, 4), np.uint8)
    flags[:, :, 0] = done
    flags[:, :, 1], flags[:, :, 2] = rng.integers(0, 2, (B, A)), rng.integers(0, 2, (B, A))
    reward = (rng.integers(-40, 200, (B, A)) * 0.25).astype(np.float32)
    length = rng.integers(0, 1002, (B, A)).astype(np.int32)
    poison = ~(done != 0).all(axis=1)
    flags[poison, :, 1:] = 0xA5
    reward[poison], length[poison] = np.float32(np.nan), -99
    raw[:, :, 0] = np.float32(1.5).view(np.int32)
    raw[:, :, 1] = flags.view(np.int32)[:, :, 0]
    raw[:, :, 2], raw[:, :, 3] = reward.view(np.int32), length
    sc = rng.integers(0, 1000, (B, 16)).astype(np.int32)
    sc[:, COLS["level_idx"]] = rng.integers(0, L, B)
    sc[rng.random(B) < 0.02, COLS["level_idx"]] = rng.choice([-1, L, L + 7])        # (no such slot: reward_possible 0, no name)
    if B > 1:
        sc[B // 2, COLS["level_idx"]] = rng.choice([-1, L, L + 7])
    agents = rng.integers(0, 1000, (B, A, 12)).astype(np.int32)
    return raw, agents, sc


def _done_plan(rng, plan, B, A):
    if plan == "none":
        return np.zeros((B, A), np.uint8)
    if plan == "all":
        return np.ones((B, A), np.uint8)
    done = (rng.random((B, A)) < 0.6).astype(np.uint8)         # some agents of an env, few envs whole
    done[rng.random(B) < 0.4] = 1
    return done


@pytest.mark.parametrize("B,A", [(1, 1), (63, 2), (64, 3), (65, 8), (HARVEST_TILE + 1, 2)])
def test_harvest_equals_the_model(B, A):
    """No agent done, every agent done, and steps where some envs have some, all or none of their agents done; capacity = B,
    so the ring wraps; the records of the envs that have not finished are poisoned; slots outside 0 .. L-1; a rewind of
    some envs in the middle."""
    torch, dev = _torch(), _hip.device()
    rng = np.random.default_rng(B * 10 + A)
    L, M = 37, 5
    possible = rng.integers(0, 90, (L, A)).astype(np.int32)
    possible[0, 0], possible[1, A - 1] = 0, 1
    name_id = rng.integers(0, M, (L, A)).astype(np.uint8)
    d, m = DeviceLog(B, A, B, 0.99, possible, name_id, M), emr.MultiLogModel(B, A, B, 0.99, possible, name_id, M)
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    _, ag, sc = _random_step(rng, B, A, L, np.zeros((B, A), np.uint8))
    d.rewind(up(ag), up(sc)), m.rewind(scalars_dict(sc, ag))
    plans = ["none", "all", "some", "some", "rewind", "some", "all", "all"]
    partial = 0
    for t, plan in enumerate(plans):
        if plan == "rewind":
            mask = (rng.random(B) < 0.4).astype(np.uint8)
            _, ag, sc = _random_step(rng, B, A, L, np.zeros((B, A), np.uint8))
            d.rewind(up(ag), up(sc), mask), m.rewind(scalars_dict(sc, ag), mask)
            assert_state_equal(d, m, (t, plan))
            continue
        done = _done_plan(rng, plan, B, A)
        partial += int(((done.sum(axis=1) > 0) & (done.sum(axis=1) < A)).sum())
        raw, ag, sc = _random_step(rng, B, A, L, done)
        d.harvest(up(raw), up(ag), up(sc))
        m.harvest(out_dict(raw), scalars_dict(sc, ag))
        assert_state_equal(d, m, (t, plan))
    assert m.n_rows >= 3 * B and m.steps == 7 * B and (partial > 0 or A == 1 or B == 1)
    rows = d.host("rows")
    live = rows[np.arange(m.n_rows - B, m.n_rows) % B]
    assert np.array_equal(live["index"], np.arange(m.n_rows - B, m.n_rows))
    assert np.array_equal(live["training_steps"], 6 * B + live["env"] + 1)       # the last call: every env, in env order
    assert np.isnan(live["agents"]["score"]).all() and np.isnan(live["side_effects_frac"]).all() and not live["flags"].any()
    if B > 1:
        outside = live[live["env"] == B // 2][0]                         # (its slot was outside 0 .. L-1)
        assert (outside["agents"]["name"] == _hip.LOG_NO_NAME).all() and not outside["agents"]["reward_possible"].any()


# -------------------------------------------------------------------------------------------------------------------- join

CELLS = [9, 0x209, 0x409, 0x609, 152 | 0x600, 48, 16]


def test_join_equals_the_model_and_counts_what_it_cannot_place():
    """Envs of 3 agents.  Part one: 4 envs, a ring of 12 rows, 5 steps that end every episode; the queue holds all 20 entries
    in scrambled order, entries of episodes that never got a row and of envs outside the batch; key lists empty, cut short,
    with NaN and infinite scores.  Part two: one env with 70 rows in a ring of 128 -- the chain is longer than the hop
    limit, so the entry of its oldest row finds nothing and the one 64 rows back does."""
    torch, dev = _torch(), _hip.device()
    rng = np.random.default_rng(7)
    B, A, cap, L, K, Cq = 4, 3, 12, 5, _hip.SL_SE_MAX_KEYS, 40
    possible = np.array([[0, 1, 10], [1, 10, 25], [10, 25, 60], [25, 60, 0], [60, 0, 1]], np.int32)
    name_id = np.array([[0, 1, 2]] * 3 + [[0, 0, 1], [2, 2, 2]], np.uint8)
    weights = [(9, 1.0), (0x409, 0.5), (9, 0.25), (48, -2.0)]
    d = DeviceLog(B, A, cap, 1.0, possible, name_id, 3, weights)
    m = emr.MultiLogModel(B, A, cap, 1.0, possible, name_id, 3, weights)
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    _, ag, sc = _random_step(rng, B, A, L, np.zeros((B, A), np.uint8))
    sc[:, COLS["episode_idx"]] = 0
    d.rewind(up(ag), up(sc)), m.rewind(scalars_dict(sc, ag))
    for t in range(5):
        raw, ag, sc = _random_step(rng, B, A, L, np.ones((B, A), np.uint8))
        sc[:, COLS["episode_idx"]] = t + 1
        d.harvest(up(raw), up(ag), up(sc))
        m.harvest(out_dict(raw), scalars_dict(sc, ag))
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
    dev_args = [up(a) for a in (np.array([n], np.int32), rec, scores, keys.view(np.int16), n_cells)]
    d.join(*dev_args)
    m.join(n, dict(env=rec[:, 0], episode_idx=rec[:, 3]), scores, keys, n_cells)
    assert m.unmatched == want_unmatched
    assert_state_equal(d, m, "join")
    rows = d.host("rows")
    assert (rows["flags"] & 1).sum() == n - want_unmatched == 3 * B
    joined = rows[(rows["flags"] & 1) != 0]
    assert np.array_equal(np.isnan(joined["agents"]["score"]), np.isnan(joined["side_effects_frac"])[:, None].repeat(A, 1))
    # a count past the capacity is the capacity; the same entries joined again change nothing but `unmatched`
    d.t["counters"][4] = 0
    m.unmatched = 0
    dev_args[0] = up(np.array([Cq + 5], np.int32))
    d.join(*dev_args)
    m.join(Cq + 5, dict(env=rec[:, 0], episode_idx=rec[:, 3]), scores, keys, n_cells)
    assert m.unmatched == want_unmatched + Cq - n
    assert_state_equal(d, m, "join again")
    d.summarise(), m.summarise()
    assert_summaries_equal(d, m)
    # part two: the hop limit
    d1, m1 = DeviceLog(1, A, 128, 1.0, possible, name_id, 3, weights), emr.MultiLogModel(1, A, 128, 1.0, possible, name_id, 3, weights)
    _, ag, sc = _random_step(rng, 1, A, L, np.zeros((1, A), np.uint8))
    sc[:, COLS["episode_idx"]] = 0
    d1.rewind(up(ag), up(sc)), m1.rewind(scalars_dict(sc, ag))
    for t in range(70):
        raw, ag, sc = _random_step(rng, 1, A, L, np.ones((1, A), np.uint8))
        sc[:, COLS["episode_idx"]] = t + 1
        d1.harvest(up(raw), up(ag), up(sc))
        m1.harvest(out_dict(raw), scalars_dict(sc, ag))
    rec1 = np.zeros((4, 8), np.int32)
    rec1[:, 3] = [0, 70 - er.MAX_HOPS - 1, 70 - er.MAX_HOPS, 69]          # out of reach twice, the farthest in reach, the newest
    args1 = [up(a) for a in (np.array([4], np.int32), rec1, scores[1:5].copy(), keys[1:5].view(np.int16).copy(), n_cells[1:5].copy())]
    d1.join(*args1)
    m1.join(4, dict(env=rec1[:, 0], episode_idx=rec1[:, 3]), scores[1:5], keys[1:5], n_cells[1:5])
    assert m1.unmatched == 2 and (m1.rows["flags"] & 1).sum() == 2
    assert_state_equal(d1, m1, "hops")


# --------------------------------------------------------------------------------------------- summaries and the run summary

@pytest.fixture(scope="module")
def cases(golden):  # noqa: F811
    """Per fixture case: the restatement's model and its rows in log order."""
    return {c: replay_case(golden, c) for c in CASES}


def _pair(golden, c, m0, capacity):  # noqa: F811
    M = len(golden[c + "_names"])
    polyak = float(golden[c + "_polyak"])
    return (DeviceLog(2, m0.A, capacity, polyak, m0.reward_possible, m0.name_id, M),
            emr.MultiLogModel(2, m0.A, capacity, polyak, m0.reward_possible, m0.name_id, M), M)


@pytest.mark.parametrize("c", CASES)
def test_summaries_over_the_fixture(golden, cases, c):  # noqa: F811
    """The fixture's rows uploaded -- levels with two agents of one name and levels without some names among them: one call
    over all of them, and many calls over the same rows (cuts at the staging batch's edges), equal the restatement bit for
    bit and each other; and the reference within the measured bound."""
    m0, rows = cases[c]
    N = len(rows)
    one, m, M = _pair(golden, c, m0, N)
    many = _pair(golden, c, m0, N)[0]
    m.rows[:], m.n_rows = rows, N
    m.summarise()
    one.put_rows(rows, N)
    one.summarise()
    assert_summaries_equal(one, m)
    assert one.host("counters")[3] == N
    many.put_rows(rows, N)
    worst = 0.0
    for cut in sorted({1, 2, min(N, 63), min(N, 64), min(N, 65), min(N, 129), N // 2, N}):
        many.t["counters"][0] = cut
        many.summarise()
        got = np.where(many.host("count") > 0, many.host("value"), np.nan)[:4 * M].reshape(M, 4)
        worst = max(worst, deviation(got, golden[c + "_stats"][cut - 1]))
        assert np.array_equal(many.host("count")[:4 * M].reshape(M, 4), golden[c + "_counts"][cut - 1])
    assert_summaries_equal(many, m)
    assert not many.host("count")[4 * M:].any()
    print("%s: largest |device - reference| of the summaries at the cuts: %r" % (c, worst))
    assert worst <= SUMMARY_BOUND
    one.summarise()                                                      # nothing new: nothing moves
    assert_summaries_equal(one, m)


@pytest.mark.parametrize("c", CASES)
def test_run_summary_over_the_fixture(golden, cases, c):  # noqa: F811
    m0, rows = cases[c]
    N = len(rows)
    d, m, _ = _pair(golden, c, m0, N)
    m.rows[:], m.n_rows = rows, N
    d.put_rows(rows, N)
    for first in (0, -7, 5, N - 1, N, N + 3):
        assert er.same_floats(d.run_summary(first), m.run_summary(first)), first
    worst = deviation(d.run_summary(0), golden[c + "_run"])
    print("%s: largest |device - reference| of the run summary: %r" % (c, worst))
    assert worst <= RUN_BOUND
    # a ring that has lost its oldest rows: ranges that begin before the ring's oldest row start there
    cap = max(2, min(150, N // 2))
    ring, rm, _ = _pair(golden, c, m0, cap)
    rm.rows[np.arange(N - cap, N) % cap], rm.n_rows = rows[N - cap:], N
    ring.put_rows(rows[N - cap:], N)
    for first in (0, N - cap - 1, N - cap, N - cap + 1, N - 3):
        got = ring.run_summary(first)
        assert er.same_floats(got, rm.run_summary(first)), first
        assert er.same_floats(got, m.run_summary(max(first, N - cap))), first


# ------------------------------------------------------------------------------------------------------------- end to end

from tests.test_level_schedule_multi_gpu import A_E2E, B_E2E, T_E2E, _actions, _counts, _env, _families, _schedule  # noqa: E402

WEIGHTS = {"life-green": 1.0, "life-red": 0.5, "crate-gray": 2.0, "life-yellow": 1.0}
FLUSHES = (16, 33, 49)


def _plain_pool():
    """The three families end to end; no points required, so the exits are open and agents leave ahead of the time limit,
    one of an env ahead of the other."""
    from safelife_amd import levels
    return levels.LevelPool([lv for fam in _families() for lv in fam], counts_fn=_counts, n_agents=A_E2E,
                            min_performance_fraction=0.0)


def _run_logged(queue_capacity, sched=None, agent_names=None):
    """50 steps of 21 envs x 2 agents (time_limit 9, the training wrappers, a side-effect queue) with a log; the restatement
    is fed the per-step records read back and, at every flush, the batch's own records, keys and scores."""
    from safelife_amd.side_effects import name_to_cell
    from tests.test_training_batch_multi_gpu import ExactPolicy
    torch = _torch()
    pool = sched.pool if sched is not None else _plain_pool()
    log = episode_log.MultiAgentEpisodeLog(pool, B_E2E, 256, side_effect_weights=WEIGHTS, agent_names=agent_names)
    env = _env(pool, True, episode_log=log, level_schedule=sched, side_effects=dict(capacity=queue_capacity, num_samples=8))
    assert env.episode_log is log and env.base.episode_log is log
    if sched is not None:
        sched.training_steps = 0
    env.reset()
    m = emr.MultiLogModel(B_E2E, A_E2E, 256, 0.99, log.reward_possible(1), log.name_id, len(log.names),
                          [(name_to_cell(k), w) for k, w in WEIGHTS.items()])
    state = lambda: scalars_dict(env.base.t["scalars"].cpu().numpy(), env.t["agents"].cpu().numpy())  # noqa: E731
    m.rewind(state())
    policy = ExactPolicy(torch, tuple(env.policy_tensor.shape[2:]), env.device)
    rng = np.random.default_rng(17)
    per_flush, ended, partial, required = [], 0, 0, []
    for t in range(T_E2E):
        if sched is not None:
            sched.training_steps = t
        required.append(env.numpy("required_points").copy())
        env.step(_actions(env, policy, rng))
        out = out_dict(env.t["out"].cpu().numpy())
        m.harvest(out, state())
        n_done = out["done"].astype(bool).sum(axis=1)
        ended += int((n_done == A_E2E).sum())
        partial += int(((n_done > 0) & (n_done < A_E2E)).sum())
        if t in FLUSHES:
            before = log.rows()["flags"] & 1
            batch = log.flush()
            emd = batch.scores_all()
            count = int(batch.count.item())
            scores, keys = emd["scores"].cpu().numpy(), batch.keys.cpu().numpy().view(np.uint16)
            n_cells = emd["n_cells"].cpu().numpy()
            m.join(count, dict(env=batch.rec_tensor[:, 0].cpu().numpy(), episode_idx=batch.rec_tensor[:, 3].cpu().numpy()),
                   scores, keys, n_cells)
            m.summarise()
            after = log.rows()["flags"] & 1
            # (host copies, taken now: the queue's buffers come round again a few flushes later)
            per_flush.append(dict(ended=ended, count=count, dropped=batch.dropped(), rec=batch.records(),
                                  newly_joined=int(after.sum() - before.sum()), scores=scores.copy(), keys=keys.copy(),
                                  n_cells=n_cells.copy()))
            ended = 0
    assert partial > 0                                  # (agents of one env did finish on different steps)
    return env, log, m, per_flush, required


def _assert_log_equals_model(log, m):
    emr.assert_rows_equal(log.rows(0), m.row_range(0))
    assert log.counters() == m.counters()
    got, want = log.summary(), m.summary(log.names)
    assert list(got) == list(want)
    assert er.same_floats([got[k] for k in got], [want[k] for k in want])
    assert er.same_floats(np.array([log.run_summary(0)[k] for k in episode_log.RUN_SUMMARY_FIELDS], np.float64),
                          m.run_summary(0))


def test_end_to_end_equals_the_model():
    env, log, m, per_flush, _ = _run_logged(1024)
    assert all(f["dropped"] == 0 and f["count"] == f["ended"] == f["newly_joined"] for f in per_flush)
    c = log.counters()
    assert c["unmatched"] == 0 and c["steps"] == T_E2E * B_E2E and c["episodes"] == c["n_rows"] >= 4 * B_E2E
    assert c["summarised"] == c["n_rows"]
    _assert_log_equals_model(log, m)
    rows = log.rows()
    assert (rows["flags"] & 1).all() and np.isfinite(rows["agents"]["score"]).all()
    assert np.array_equal(rows["agents"]["reward_possible"], log.reward_possible(1)[rows["level"]])
    assert (rows["agents"]["length"] <= 9).all() and (rows["agents"]["length"].min(axis=1) < rows["agents"]["length"].max(axis=1)).any()
    assert set(log.summary()) == ({"training/agent%d-%s" % (a, q) for a in range(2) for q in _hip.LOG_MULTI_KEYS}
                                  | {"training/steps", "training/episodes"})
    recs = log.records()
    assert len(recs) == len(rows) and recs[0]["side_effects"]["total"] == rows["side_effects"][0].tolist()
    assert recs[0]["agents"] == ["agent0", "agent1"] and recs[0]["length"] == rows["agents"]["length"][0].tolist()
    rs = log.run_summary()
    assert rs["rows"] == len(rows) and rs["successes"] == int(rows["agents"]["success"].sum())


def test_end_to_end_with_shared_and_differing_names():
    """Every level of the first family has two agents of one name, the last family names its agents differently: keys skip
    episodes, and of the two agents of one name the second one counts."""
    sizes = [len(f) for f in _families()]
    names = [["red", "red"]] * sizes[0] + [["red", "blue"]] * sizes[1] + [["green", "blue"]] * sizes[2]
    env, log, m, per_flush, _ = _run_logged(1024, agent_names=names)
    assert log.names == ["red", "blue", "green"]
    _assert_log_equals_model(log, m)
    state = log._state()
    count = state[1][:12].reshape(3, 4)
    rows = log.rows()
    has = np.array([[(r["agents"]["name"] == n).any() for n in range(3)] for r in rows])
    assert np.array_equal(count[:, 0], has.sum(axis=0)) and 0 < count[2, 0] < len(rows)
    assert (count[:, 3] == count[:, 0]).all() and not state[1][12:].any()


def test_end_to_end_under_a_level_schedule():
    """reward_needed follows min_performance_fraction per agent: every row carries the required points its agents played
    under, which the env showed before the step that ended the episode."""
    sched = _schedule("uniform")
    env, log, m, per_flush, required = _run_logged(1024, sched=sched)
    assert all(f["dropped"] == 0 and f["count"] == f["ended"] for f in per_flush) and log.counters()["unmatched"] == 0
    _assert_log_equals_model(log, m)
    rows = log.rows()
    step = (rows["training_steps"] - rows["env"] - 1) // B_E2E
    for r, t in zip(rows, step):
        assert np.array_equal(r["agents"]["reward_needed"], required[t][r["env"]])
    seen = set(zip(rows["level"].tolist(), map(tuple, rows["agents"]["reward_needed"].tolist())))
    assert len(seen) > len(set(rows["level"].tolist()))                  # one level, several fractions
    assert sched.stats()["episodes"].sum() == len(rows)


def test_end_to_end_with_a_queue_that_overflows():
    """A queue of 2: exactly min(ended, 2) rows per flush carry the joined flag, each joined row is right for its entry, and
    the summaries are the restatement's fed the same entries."""
    env, log, m, per_flush, _ = _run_logged(2)
    rows = log.rows()
    by_episode = {(int(r["env"]), int(r["episode_idx"])): r for r in rows}
    for f in per_flush:
        kept = min(f["ended"], 2)
        assert f["count"] == f["ended"] and f["dropped"] == f["ended"] - kept and f["newly_joined"] == kept
        keys, scores, n_cells = f["keys"], f["scores"], f["n_cells"]
        for i in range(kept):
            r = by_episode[(int(f["rec"]["env"][i]), int(f["rec"]["episode_idx"][i]))]
            total = er.entry_totals(m.weights, keys[i], scores[i], n_cells[i])
            frac = total[0] / er.at_least_one(total[1])
            assert r["flags"] & 1 and er.same_floats(r["side_effects"], total) and er.same_floats(r["side_effects_frac"], frac)
            for g in r["agents"]:
                assert er.same_floats(g["score"], emr.agent_score(float(g["reward_frac"]), g["length"], frac))
    assert (rows["flags"] & 1).sum() == sum(min(f["ended"], 2) for f in per_flush) and log.counters()["unmatched"] == 0
    _assert_log_equals_model(log, m)
    s = log.summary()
    assert s["training/episodes"] == len(rows) and "training/agent1-score" in s


def test_a_one_agent_pool_logs_agent0_keys():
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    from tests import util
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=6)[0]
    assert pool.n_agents == 1
    B = 9
    log = episode_log.MultiAgentEpisodeLog(pool, B, 64)
    env = SafeLifeMultiAgentVectorEnv(pool, B, time_limit=4, episode_log=log)
    env.reset()
    actions = np.random.default_rng(3).integers(0, 9, (12, B, 1)).astype(np.int32)
    for a in actions:
        env.step(a)
    log.flush()
    s = log.summary()
    assert set(s) == {"training/agent0-length", "training/agent0-reward", "training/agent0-success", "training/steps",
                      "training/episodes"}                             # (no queue: the score never counts)
    assert s["training/steps"] == 12 * B and s["training/episodes"] >= 3 * B
    rows = log.rows()
    assert rows["agents"].shape == (len(rows), 1) and (rows["n_agents"] == 1).all()
    recs = log.records()
    assert recs[0]["agents"] == ["agent0"] and isinstance(recs[0]["length"], list) and "side_effects" not in recs[0]


@pytest.mark.parametrize("B", [1, 65])
def test_a_one_agent_log_equals_the_single_agent_log(B):
    """The harvest and the join are one body under both logs: an ``EpisodeLog`` and a one-agent ``MultiAgentEpisodeLog`` on
    the same pool, allocated by hand and fed the same 6 steps (the records of the envs that go on poisoned, a slot outside
    the pool) and one join of a scrambled queue with an entry that has no row, hold the same counters and the same rows, bit
    for bit -- NaNs included.  B = 1: a lone lane; B = 65: a lane past a wave's edge."""
    from safelife_amd.side_effects import name_to_cell
    from tests import util
    torch, dev = _torch(), _hip.device()
    rng = np.random.default_rng(40 + B)
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=6)[0]
    assert pool.n_agents == 1
    L, K, weights = pool.n_slots, _hip.SL_SE_MAX_KEYS, {"life-green": 1.0, "life-red": 0.5, "crate-gray": -2.0}
    one = episode_log.EpisodeLog(pool, B, 6 * B, side_effect_weights=weights)
    many = episode_log.MultiAgentEpisodeLog(pool, B, 6 * B, side_effect_weights=weights)
    one.allocate(torch, dev), many.allocate(torch, dev)
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    for t, plan in enumerate(["none", "all", "some", "some", "all", "some"]):
        raw, ag, sc = _random_step(rng, B, 1, L, _done_plan(rng, plan, B, 1))
        sc[:, COLS["episode_idx"]] = t + 1
        ag[:, 0, ACOLS["required_points"]] = sc[:, COLS["required_points"]]
        out, agents, scalars = up(raw), up(ag), up(sc)
        one.harvest(out.view(B, 4), scalars)
        many.harvest(out, agents, scalars)
    filed = one.rows()
    entries = [(int(r["env"]), int(r["episode_idx"])) for r in filed] + [(0, 10 ** 6)]      # the last one: never logged
    rng.shuffle(entries)
    n = len(entries)
    rec = np.zeros((n, 8), np.int32)
    rec[:, 0], rec[:, 3] = [e for e, _ in entries], [k for _, k in entries]
    cells = [name_to_cell(name) for name in weights] + [48, 16]
    keys = np.full((n, K), 0xFFFF, np.uint16)
    scores = np.full((n, K, 2), np.nan)
    n_cells = np.zeros((n, K), np.int32)
    for i in range(n):
        if i % 5 == 0:
            continue                                                    # an empty key list: totals 0, 0
        slots = rng.choice(K, rng.integers(1, 9), replace=False)
        keys[i, slots] = rng.choice(cells, len(slots))
        scores[i, slots] = rng.random((len(slots), 2)) * 4
        if i % 5 == 1:
            scores[i, slots[0], rng.integers(0, 2)] = np.nan            # a NaN score contributes nothing
        if i % 5 == 2:
            n_cells[i, 0] = -1                                          # cut short: NaN totals
    args = [up(a) for a in (np.array([n], np.int32), rec, scores, keys.view(np.int16), n_cells)]
    one.join(*args), many.join(*args)
    c = one.counters()
    assert c == many.counters()
    assert c["unmatched"] == 1 and c["steps"] == 6 * B and c["n_rows"] == c["episodes"] == len(filed) >= 2 * B
    r1, rm = one.rows(), many.rows()
    bits = lambda a: np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}.get(a.dtype.itemsize, a.dtype))  # noqa: E731
    assert len(r1) == len(rm) == c["n_rows"] and (rm["n_agents"] == 1).all()
    for name in ("index", "training_steps", "prev", "env", "level", "episode_idx", "flags", "side_effects",
                 "side_effects_frac"):
        assert np.array_equal(bits(r1[name]), bits(rm[name])), name
    for name in ("length", "reward", "reward_possible", "reward_needed", "success", "times_up", "reward_frac", "score"):
        assert np.array_equal(bits(r1[name]), bits(rm["agents"][name][:, 0])), name
    assert (r1["flags"] & _hip.LOG_JOINED).all()
    assert B == 1 or (np.isnan(r1["score"]).any() and np.isfinite(r1["score"]).any())


def test_without_a_log_nothing_changes():
    pool = _plain_pool()
    rng = np.random.default_rng(5)
    actions = rng.integers(0, 9, (20, B_E2E, A_E2E)).astype(np.int32)
    one, two = _env(pool, True, episode_log=None), _env(pool, True)
    logged = _env(pool, True, episode_log=episode_log.MultiAgentEpisodeLog(pool, B_E2E, 64))
    assert one.episode_log is None and two.episode_log is None and sorted(one.t) == sorted(two.t)
    assert one.base.episode_log is None
    envs = (one, two, logged)
    for e in envs:
        e.reset()
    for t in range(len(actions)):
        for e in envs:
            e.step(actions[t])
        for name in ("reward", "done", "shaped_reward", "board", "level_idx", "success", "rng", "episode_reward"):
            assert np.array_equal(one.numpy(name), two.numpy(name), equal_nan=True), (t, name)
            assert np.array_equal(one.numpy(name), logged.numpy(name), equal_nan=True), (t, name)
        assert np.array_equal(one.policy_tensor.cpu().numpy(), logged.policy_tensor.cpu().numpy())
    c = logged.episode_log.counters()
    assert c["steps"] == len(actions) * B_E2E and c["episodes"] >= 2 * B_E2E       # time_limit 9: two ends in 20 steps
    with pytest.raises(ValueError, match="already serves"):
        _env(pool, True, episode_log=logged.episode_log)
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    with pytest.raises(ValueError, match="built for 8 envs"):
        SafeLifeMultiAgentVectorEnv(pool, B_E2E, episode_log=episode_log.MultiAgentEpisodeLog(pool, 8, 64))
    with pytest.raises(ValueError, match="another pool"):
        SafeLifeMultiAgentVectorEnv(_plain_pool(), B_E2E, episode_log=episode_log.MultiAgentEpisodeLog(pool, B_E2E, 64))
    with pytest.raises(ValueError, match="cannot drive an episode log"):
        logged.base.step_async(0)
    # a partial reset rewinds the reset envs: their chains start over and their next rows describe the new episode
    mask = np.zeros(B_E2E, np.uint8)
    mask[::2] = 1
    logged.reset(mask)
    last = logged.episode_log.t["last_row"].cpu().numpy()
    assert (last[::2] == -1).all() and (last[1::2] >= 0).all()
    assert np.array_equal(logged.episode_log.t["cur_required"].cpu().numpy()[::2], logged.numpy("required_points")[::2])


def test_the_runner_advances_the_log():
    from safelife_amd.runner import MultiAgentRunner
    from tests.test_training_batch_multi_gpu import ExactPolicy
    torch = _torch()
    pool = _plain_pool()
    log = episode_log.MultiAgentEpisodeLog(pool, B_E2E, 256)
    env = _env(pool, True, episode_log=log)
    policy = ExactPolicy(torch, tuple(env.policy_tensor.shape[2:]), env.device)
    runner = MultiAgentRunner(env, policy, seed=3)
    T = 12
    batch = runner.gen_training_batch(T)
    assert len(batch.actions) > 0
    c = log.counters()
    assert c["steps"] == T * B_E2E == runner.num_steps
    assert c["episodes"] == c["n_rows"] == int(runner.num_resets.cpu().numpy().sum()) >= B_E2E
    log.flush()
    assert log.counters()["summarised"] == c["n_rows"] and "training/agent0-length" in log.summary()
