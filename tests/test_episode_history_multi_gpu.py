"""
Episode histories of multi-agent envs on the device (csrc/sl_history.hip: k_history_book on the reader of A records per env;
safelife_amd/episode_history.MultiAgentEpisodeHistory): slhip_history_capture_multi against the numpy restatement of
tests/episode_history_multi_ref.py BIT FOR BIT on synthetic record streams -- slots, entries, ownership, the free order, the
cursor and the counters after every call --, at one agent against slhip_history_capture itself, and
SafeLifeMultiAgentVectorEnv with a recorder against the restatement driven by the oracle's env, against the reference's
saved arrays (tests/golden/episode_history_multi_cases.npz) and against an env without a recorder.  Integer copies and
integer bookkeeping: no tolerance anywhere.
"""
import ctypes as C

import numpy as np
import pytest

from safelife_amd import _hip, episode_history, episode_log, episode_run, render
from tests import episode_history_multi_ref as mr
from tests import episode_history_ref as hr
from tests import multi_step_cases as msc
from tests import util
from tests.test_episode_history_gpu import COLS, T_SYN, DeviceHistory, Synthetic, _dev, _torch, assert_state_equal, watch_sets
from tests.test_episode_history_multi_host import RUNS, B_FIX, fixture_pool, golden_multi  # noqa: F401

pytestmark = pytest.mark.gpu


class DeviceMultiHistory(DeviceHistory):
    def capture_multi(self, board, goals, scalars, out, A, queue, active=None):
        _hip.check(self.lib.slhip_history_capture_multi(self.ref, _hip.ptr(board), _hip.ptr(goals), _hip.ptr(scalars),
                                                        _hip.ptr(out), A, queue, _hip.ptr(active), _hip.current_stream_ptr()))


class MultiSynthetic(Synthetic):
    """The single-agent stream's boards, goals and queue with records [B, A]: an agent leaves with probability p_leave a
    step, an env's episode ends once all have (or at T_SYN steps, when all that are left finish at once).  While an env's
    episode goes on EVERY non-done byte of its records is poison -- those of the agents that have left too --, and so is
    scalars.episode_length, which the multi-agent kernels do not keep."""

    def __init__(self, rng, B, A, H, W, watch):
        super().__init__(rng, B, H, W, watch)
        self.A = A
        self.gone = np.zeros((B, A), bool)
        self.left_at = np.zeros((B, A), np.int32)

    def scalars(self):
        sc = self.rng.integers(0, 1000, (self.B, 16)).astype(np.int32)
        sc[:, COLS["level_idx"]], sc[:, COLS["episode_idx"]], sc[:, COLS["num_steps"]] = self.level, self.episode, self.length
        sc[:, COLS["episode_length"]] = -77
        return sc

    def step(self, p_leave, drop=0, active=None):
        rng, B, A = self.rng, self.B, self.A
        self.t += 1
        self.length += 1
        leaves = ~self.gone & ((rng.random((B, A)) < p_leave) | (self.length >= T_SYN)[:, None])
        self.left_at[leaves] = np.broadcast_to(self.length[:, None], (B, A))[leaves]
        self.gone |= leaves
        done = self.gone.all(axis=1)
        board = np.full((B, self.H, self.W), 0x0BAD, np.uint16)
        for e in self.watch:
            board[e] = self.cells(e)
        flags = np.zeros((B, A, 4), np.uint8)
        flags[:, :, 0] = self.gone
        flags[:, :, 1], flags[:, :, 2] = rng.integers(0, 2, (B, A)), rng.integers(0, 2, (B, A))
        length = self.left_at.copy()
        flags[~done, :, 1:] = 0xA5
        length[~done] = -99
        raw = np.zeros((B, A, 4), np.int32)
        raw[:, :, 0], raw[:, :, 1], raw[:, :, 2], raw[:, :, 3] = 7, flags.view(np.int32)[:, :, 0], 9, length
        ended = rng.permutation(np.flatnonzero(done))
        on = np.ones(B, bool) if active is None else active != 0
        lost = set(ended[on[ended]][:drop].tolist())
        for e in ended:
            if int(e) not in lost:
                self.push(int(e), int(self.episode[e]), self.cells(e, final=True))
        self.level[done] = rng.integers(0, 9, int(done.sum()))
        self.episode[done] += 1
        self.length[done] = 0
        self.goal_tag[done] += 1000
        out = dict(done=flags[:, :, 0].copy(), success=flags[:, :, 1].copy(), times_up=flags[:, :, 2].copy(),
                   episode_length=length)
        self.partial = int((self.gone.any(axis=1) & ~done).sum())
        self.gone[done], self.left_at[done] = False, 0
        return board, self.goals(), self.scalars(), raw, out


def multi_watch_sets(B):
    sets = watch_sets(B)
    if B == 257:
        sets.append(list(range(B)))                     # 257 watched envs: the second chunk of the per-env passes
    return sets


SHAPES = {1: (3, 3), 63: (25, 25), 64: (7, 7), 65: (3, 3), 257: (7, 7)}


@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("B,A", [(1, 1), (63, 2), (64, 3), (65, 8), (257, 2)])
def test_the_kernel_equals_the_model(B, A, interval):
    """Per watch set: a rewind at attach, then steps with no agent done, many done, a masked rewind, a step that loses queue
    entries, a release, a fresh queue, a step that ends EVERY episode (more than 256 new queue entries at 257 envs) and -- for
    the last watch set -- an active mask; the state after every call."""
    H, W = SHAPES[B] if interval == 1 else {(3, 3): (25, 25), (25, 25): (7, 7), (7, 7): (3, 3)}[SHAPES[B]]
    rng = np.random.default_rng(1000 * B + 10 * A + interval)
    kept = partial = chunk2_partial = 0
    sets = multi_watch_sets(B)
    for w, watch in enumerate(sets):
        n = len(watch)
        K = max(1, n - 1) if interval == 1 else min(n + 3, 1024)
        syn = MultiSynthetic(rng, B, A, H, W, watch)
        d, m = DeviceMultiHistory(B, watch, K, T_SYN, H, W, interval), mr.MultiHistoryModel(B, A, watch, K, T_SYN, H, W, interval)
        d.rewind(_dev(syn.goals()), _dev(syn.scalars()))
        m.rewind(syn.goals(), syn.level, syn.episode)
        assert_state_equal(d, m, (watch, "attach"))
        masked = w == len(sets) - 1 and B != 257
        plans = [0.0, 0.4, 0.3, "rewind", 0.4, "drop", "release", 0.5, "fresh", 0.5, 0.3, 1.0]
        for step, plan in enumerate(plans):
            where = (watch[:4], step, plan)
            if plan == "rewind":
                mask = (rng.random(B) < 0.5).astype(np.uint8)
                sel = mask != 0
                syn.level[sel], syn.length[sel] = rng.integers(0, 9, int(sel.sum())), 0
                syn.gone[sel], syn.left_at[sel] = False, 0
                syn.episode[sel] += 1
                syn.goal_tag[sel] += 1000
                d.rewind(_dev(syn.goals()), _dev(syn.scalars()), _dev(mask))
                m.rewind(syn.goals(), syn.level, syn.episode, mask)
            elif plan == "release":
                live = m.listing()["slot"][::2].tolist()
                d.release(live), m.release(live)
            elif plan == "fresh":
                syn.fresh_queue()
                d.t["counters"][4] = 0
                m.cursor = 0
            else:
                active = (rng.random(B) < 0.7).astype(np.uint8) if masked else None
                board, goals, sc, raw, out = syn.step(0.5 if plan == "drop" else plan, drop=2 if plan == "drop" else 0,
                                                      active=active)
                partial += syn.partial
                if n > 256:
                    chunk2_partial += int((syn.gone[256:].any(axis=1) & ~syn.gone[256:].all(axis=1)).sum())
                d.capture_multi(_dev(board), _dev(goals), _dev(sc), _dev(raw), A, C.byref(syn.device_queue()),
                                None if active is None else _dev(active))
                m.capture_multi(board, goals, syn.level, syn.episode, syn.length, out, syn.model_queue(), active)
            assert_state_equal(d, m, where)
        kept += m.kept
        if not masked:
            assert m.episodes >= B
            if interval == 1 and n > 1:
                assert m.missed >= 1                             # the slots did run out
    assert kept >= 1 and (A == 1 or partial >= 1)
    if B == 257:
        assert chunk2_partial >= 1          # an env beyond the first 256 watched ones with some but not all agents done


def test_across_the_tile_of_the_done_scan():
    """16385 envs of 2 agents on 3x3 boards: the second tile of the done scan holds one env, watched, and the numbering of
    its episode counts every env of the first tile."""
    B, A, H, W = 16385, 2, 3, 3
    rng = np.random.default_rng(5)
    watch = [0, 16383, 16384]
    syn = MultiSynthetic(rng, B, A, H, W, watch)
    d, m = DeviceMultiHistory(B, watch, 8, T_SYN, H, W, 1), mr.MultiHistoryModel(B, A, watch, 8, T_SYN, H, W, 1)
    d.rewind(_dev(syn.goals()), _dev(syn.scalars()))
    m.rewind(syn.goals(), syn.level, syn.episode)
    for step, p in enumerate((0.5, 0.6, 1.0)):
        board, goals, sc, raw, out = syn.step(p)
        d.capture_multi(_dev(board), _dev(goals), _dev(sc), _dev(raw), A, C.byref(syn.device_queue()))
        m.capture_multi(board, goals, syn.level, syn.episode, syn.length, out, syn.model_queue())
        assert_state_equal(d, m, step)
    assert m.episodes >= B and m.listing()["row"].max() >= 16384 and m.listing()["env"].tolist().count(16384) >= 1


@pytest.mark.parametrize("B,shape", [(65, (25, 25)), (257, (3, 3))])
def test_at_one_agent_it_is_the_single_agent_capture(B, shape):
    """The same stream of inputs into both entry points: every state tensor byte for byte, but for the entry's `reserved`,
    which carries A = 1 from the one and 0 from the other."""
    H, W = shape
    rng = np.random.default_rng(B)
    watch = watch_sets(B)[-1]
    syn = Synthetic(rng, B, H, W, watch)
    one, multi = DeviceHistory(B, watch, 6, T_SYN, H, W, 3), DeviceMultiHistory(B, watch, 6, T_SYN, H, W, 3)
    sc = syn.scalars()
    for d in (one, multi):
        d.rewind(_dev(syn.goals()), _dev(sc))
    for step, p in enumerate((0.0, 0.5, 0.3, 0.5, 1.0, 0.4)):
        active = (rng.random(B) < 0.8).astype(np.uint8) if step >= 3 else None
        board, goals, sc, raw, out = syn.step(p, drop=1 if step == 3 else 0, active=active)
        sc[:, COLS["num_steps"]] = sc[:, COLS["episode_length"]]        # (each reads its own column)
        act = None if active is None else _dev(active)
        one.capture(_dev(board), _dev(goals), _dev(sc), _dev(raw), C.byref(syn.device_queue()), act)
        multi.capture_multi(_dev(board), _dev(goals), _dev(sc), _dev(raw), 1, C.byref(syn.device_queue()), act)
        for name in ("owner", "cur_level", "cur_episode", "slot_state", "counters", "goals", "frames", "orders"):
            assert np.array_equal(one.host(name), multi.host(name)), (step, name)
        a, b = one.host("entries"), multi.host("entries")
        for name in hr.ENTRY_DTYPE.names:
            if name != "reserved":
                assert np.array_equal(a[name], b[name]), (step, name)
        live = (b["flags"] & hr.LIVE) != 0
        assert not a["reserved"].any() and (b["reserved"][live] == 1).all() and not b["reserved"][~live].any()
    assert live.sum() >= 2


# ------------------------------------------------------------------------------------------------------------ whole envs

def assert_history_equals_model(h, m, where=""):
    got, want = h.entries(), m.listing()
    for name in hr.ENTRY_DTYPE.names:
        assert np.array_equal(got[name], want[name]), (where, name)
    c = h.counters()
    assert (c["episodes"], c["kept"], c["missed"], c["incomplete"]) == (m.episodes, m.kept, m.missed, m.incomplete), where
    for i, en in enumerate(want):
        a, b = h.history(i), m.history(en)
        assert np.array_equal(a["board"], b["board"]) and np.array_equal(a["goals"], b["goals"]), (where, i)
    return len(want)


def _trace_pool(A):
    from safelife_amd.levels import LevelPool
    if A == 2:
        levels = [lv for name in ("multi_asym1", "multi_build_coop", "multi_build_compete")
                  for lv in util.levels_from_trace(util.load_trace(name))]
    else:
        levels = msc.levels_of(msc.case("dense/3x5x5"))
    return LevelPool(levels, counts_fn=util.oracle_counts, n_agents=A, min_performance_fraction=0.0)


@pytest.mark.parametrize("B,A,watch", [(21, 2, [0, 5, 11, 20]), (9, 3, [0, 3, 4, 8])])
def test_whole_envs_equal_the_restatement_and_an_env_without_a_history(B, A, watch):
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    pool = _trace_pool(A)
    T, limit, slots, interval = 36, 9, 12, 2
    kw = dict(time_limit=limit, view_shape=(5, 5), auto_reset=True, episode_streams=False)
    se = dict(capacity=128, num_samples=4)
    h = episode_history.MultiAgentEpisodeHistory(pool, B, watch, slots, interval=interval)
    log = episode_log.MultiAgentEpisodeLog(pool, B, 512)
    env = SafeLifeMultiAgentVectorEnv(pool, B, episode_history=h, episode_log=log, side_effects=se, **kw)
    plain = SafeLifeMultiAgentVectorEnv(pool, B, side_effects=se, **kw)
    assert env.episode_history is h and env.base.episode_history is h and plain.episode_history is None
    assert sorted(plain.t) == sorted(env.t)
    d = mr.MultiOracleDrive(pool, B, limit, watch, slots, interval, episode_streams=False)
    assert np.array_equal(env.reset().cpu().numpy(), plain.reset().cpu().numpy())
    rng = np.random.default_rng(17)
    idle = np.zeros((B, A), bool)
    seen = partial = 0
    for t in range(T):
        acts = msc.steered_actions(rng, d.A["board"], d.ma["agent_loc"], np.ones(B, bool))
        acts[idle] = 0                                  # an agent that is done takes 0
        env.step(acts), plain.step(acts)
        out = d.step(acts)
        gone = out["done"] != 0
        idle = gone & ~gone.all(axis=1)[:, None]
        partial += int(idle.any(axis=1).sum())
        for name in ("reward", "done", "success", "times_up", "obs", "board", "goals", "level_idx", "episode_idx",
                     "episode_length", "episode_reward"):
            assert np.array_equal(env.numpy(name), plain.numpy(name)), (t, name)
        assert np.array_equal(env.numpy("board"), d.A["board"]) and np.array_equal(env.numpy("done"), out["done"]), t
        if t in (11, 23):
            seen += assert_history_equals_model(h, d.model, t)
            rows = log.rows()
            for en in h.entries():
                row = rows[int(en["row"])]
                assert (row["env"], row["episode_idx"], row["level"]) == (en["env"], en["episode_idx"], en["level"])
                assert row["agents"]["length"].max() == en["length"] and en["reserved"] == A
                assert h.success(en).tolist() == (row["agents"]["success"] != 0).tolist()
            slots_now = h.entries()["slot"].tolist()
            assert h.release() == len(slots_now)
            d.model.release(slots_now)
            env.side_effects_flush(), plain.side_effects_flush(), d.flush()
    seen += assert_history_equals_model(h, d.model, "end")
    # (on the 26x26 trace levels two steered agents do not reach an exit within the limit: there every episode ends for both
    # at once, and agents that finish apart are the 5x5 family's part -- and the fixture's, below)
    assert seen >= 4 and (A == 2 or partial >= 20) and h.counters()["incomplete"] == 0
    assert h.counters()["episodes"] == log.counters()["episodes"]


@pytest.mark.parametrize("r", RUNS)
def test_the_fixture_s_runs_on_the_device_equal_what_the_reference_saved(golden_multi, r):  # noqa: F811
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    g = golden_multi
    A, acts = int(g[r + "_agents"]), g[r + "_actions"]
    pool = fixture_pool(g, r)
    h = episode_history.MultiAgentEpisodeHistory(pool, B_FIX, range(B_FIX), 40, interval=int(g[r + "_interval"]))
    env = SafeLifeMultiAgentVectorEnv(pool, B_FIX, episode_history=h, side_effects=dict(capacity=64, num_samples=4),
                                      time_limit=int(g[r + "_time_limit"]), view_shape=(5, 5), episode_streams=False)
    env.reset()
    ended, locs = {}, []
    for t in range(len(acts)):
        env.step(acts[t])
        locs.append(env.numpy("agent_locs").copy())
        for e in np.flatnonzero(env.numpy("done").all(axis=1)):
            ended[(int(e), int(env.numpy("episode_idx")[e]) - 1)] = t
    n = len(g[r + "_env"])
    listing = h.entries()
    listing = listing[listing["row"] < n]
    assert listing["row"].tolist() == g[r + "_kept"].tolist() and not (listing["flags"] & _hip.HIST_NO_FINAL).any()
    for i, en in enumerate(listing):
        k, length, e = int(en["row"]), int(en["length"]), int(en["env"])
        assert (e, en["level"], length, en["reserved"]) == (g[r + "_env"][k], g[r + "_level"][k], g[r + "_num_steps"][k], A)
        assert h.success(en).tolist() == g[r + "_success"][k].tolist() and bool(en["times_up"]) == bool(g[r + "_times_up"][k])
        first = ended[(e, int(en["episode_idx"]))] - length + 1
        hist = h.history(i)
        want = g["%s_board_%d" % (r, k)]
        assert np.array_equal(hist["goals"], g["%s_goals_%d" % (r, k)])
        assert np.array_equal(hist["board"][-1], want[-1])
        bridge = ([locs[first + f][e] for f in range(length - 1)], [acts[first + 1 + f][e] for f in range(length - 1)])
        assert np.array_equal(mr.as_the_reference_saved(hist["board"], *bridge), want), (r, k)


def test_an_episode_run_a_log_and_the_frames():
    """7 tickets on 5 envs of 2 agents, every env watched, interval 1: exactly 7 histories, none of a phantom episode; every
    entry's row is the log's row of the same (env, episode_idx); frames(i) is render_board of the device history."""
    torch = _torch()
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    pool = _trace_pool(3)
    B, N, limit, A = 5, 7, 6, 3
    run = episode_run.EpisodeRun(pool, B, N, n_agents=A)
    h = episode_history.MultiAgentEpisodeHistory(pool, B, range(B), 16)
    log = episode_log.MultiAgentEpisodeLog(pool, B, 64)
    env = SafeLifeMultiAgentVectorEnv(pool, B, episode_run=run, episode_history=h, episode_log=log, view_shape=(5, 5),
                                      side_effects=dict(capacity=64, num_samples=4), time_limit=limit, **run.env_arguments())
    run.start()
    rng = np.random.default_rng(8)
    for _ in range(4 * limit):
        done = env.numpy("done") != 0
        acts = rng.integers(0, 9, (B, A)).astype(np.int32)
        acts[done & ~done.all(axis=1)[:, None]] = 0
        env.step(acts)
    assert run.finished() and h.counters() == dict(episodes=N, kept=N, missed=0, incomplete=0)
    listing, results, rows = h.entries(), run.results(), log.rows()
    assert listing["row"].tolist() == list(range(N)) and len(rows) == N
    assert sorted(zip(listing["env"], listing["level"])) == sorted((int(r["env"]), int(r["slot"])) for r in results)
    for i, en in enumerate(listing):
        row = rows[int(en["row"])]
        assert (row["index"], row["env"], row["episode_idx"]) == (en["row"], en["env"], en["episode_idx"])
        assert row["agents"]["length"].max() == en["length"]
        dev = h.history(i, device=True)
        want = render.render_board(dev["board"], dev["goals"][0])
        assert torch.equal(h.frames(i), want) and tuple(want.shape[:1]) == (int(en["length"]),)


def test_refusals_that_need_the_device():
    from safelife_amd.levels import Level, LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    pool = _trace_pool(3)
    se = dict(capacity=32, num_samples=4)
    h = episode_history.MultiAgentEpisodeHistory(pool, 4, [0], 2)
    env = SafeLifeMultiAgentVectorEnv(pool, 4, episode_history=h, side_effects=se, time_limit=5, view_shape=(5, 5))
    # the base env's other steppers would step without the recorder
    acts = np.zeros(4, np.int32)
    for call in (lambda: env.base.step_async(acts), lambda: env.base.step_queues(acts), lambda: env.base.queues_open(),
                 lambda: env.base.rollout(np.zeros((2, 4), np.int32))):
        with pytest.raises(ValueError, match="cannot drive an episode history"):
            call()
    with pytest.raises(ValueError, match="already serves"):
        env = SafeLifeMultiAgentVectorEnv(pool, 4, episode_history=h, side_effects=se, time_limit=5, view_shape=(5, 5))
    # the base env's other steppers would step without the recorder
    acts = np.zeros(4, np.int32)
    for call in (lambda: env.base.step_async(acts), lambda: env.base.step_queues(acts), lambda: env.base.queues_open(),
                 lambda: env.base.rollout(np.zeros((2, 4), np.int32))):
        with pytest.raises(ValueError, match="cannot drive an episode history"):
            call()
    lv = pool.levels[0]
    goals = np.zeros_like(lv.goals)
    goals[2, 1:4] = 9 | (2 << 9)                        # three live green cells in a row: one CA step changes them
    moving = Level(lv.board, goals, lv.agent_locs, spawn_prob=lv.spawn_prob, min_performance=lv.min_performance,
                   points_table=lv.points_table, rng_words=lv.rng_words, seed=lv.seed)
    bad = LevelPool([pool.levels[1], moving], counts_fn=util.oracle_counts, n_agents=3)
    with pytest.raises(ValueError, match=r"need static goals.*pool slot\(s\) \[1\]"):
        SafeLifeMultiAgentVectorEnv(bad, 4, episode_history=episode_history.MultiAgentEpisodeHistory(bad, 4, [0], 2),
                                    side_effects=se, time_limit=5, view_shape=(5, 5))
