"""
Episode histories on the device (csrc/sl_history.hip, safelife_amd/episode_history.py): the two kernels against the numpy
restatement of tests/episode_history_ref.py BIT FOR BIT on synthetic inputs -- slots, entries, ownership, the free order, the
cursor and the counters after every call -- and SafeLifeVectorEnv with a recorder against the restatement driven by the
oracle's env, against the reference's saved arrays (tests/golden/episode_history_cases.npz; what stands between the
recorder's frames and the reference's saved bytes is said in tests/test_episode_history_host.py) and against an env without
a recorder.  Integer copies and integer bookkeeping: no tolerance anywhere.
"""
import ctypes as C

import numpy as np
import pytest

from safelife_amd import _hip, episode_history, episode_log, episode_run, render, schedule
from tests import episode_history_ref as hr
from tests import util
from tests.test_episode_history_host import fixture_pool, golden  # noqa: F401

pytestmark = pytest.mark.gpu

COLS = _hip.SCALAR_COLS
T_SYN = 5


def _torch():
    import torch
    return torch


def _dev(a):
    torch = _torch()
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint16): np.int16}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view is not None else a).to(_hip.device())


class DeviceHistory(object):
    """A struct sl_episode_history with its device arrays, slots poisoned."""

    def __init__(self, B, watch, slots, T, H, W, interval):
        torch, dev = _torch(), _hip.device()
        watch = np.asarray(watch, np.int32)
        n = len(watch)
        t = self.t = {}
        t["watch"] = _dev(watch)
        t["owner"] = torch.full((n,), -1, dtype=torch.int32, device=dev)
        t["cur_level"] = torch.zeros(n, dtype=torch.int32, device=dev)
        t["cur_episode"] = torch.zeros(n, dtype=torch.int32, device=dev)
        t["slot_state"] = torch.zeros(slots, dtype=torch.int32, device=dev)
        t["entries"] = torch.zeros((slots, 4), dtype=torch.int64, device=dev)
        t["counters"] = torch.zeros(len(_hip.HIST_COUNTERS), dtype=torch.int64, device=dev)
        t["goals"] = _dev(np.full((slots, H, W), hr.POISON, np.uint16))
        t["frames"] = _dev(np.full((slots, T, H, W), hr.POISON, np.uint16))
        t["orders"] = torch.full((n, _hip.HIST_ORDER_WORDS), -7, dtype=torch.int32, device=dev)
        s = self.struct = _hip.EpisodeHistory()
        s.B, s.n_watch, s.n_slots, s.T, s.H, s.W, s.interval = B, n, slots, T, H, W, interval
        for name, ctype in _hip.EpisodeHistory._fields_:
            if ctype is C.c_void_p:
                setattr(s, name, t[name].data_ptr())
        self.ref, self.lib = C.byref(s), _hip.lib()

    def host(self, name):
        a = self.t[name].cpu().numpy()
        if name == "entries":
            return a.view(hr.ENTRY_DTYPE).reshape(-1)
        return a.view(np.uint16) if name in ("goals", "frames") else a

    def capture(self, board, goals, scalars, out, queue, active=None):
        _hip.check(self.lib.slhip_history_capture(self.ref, _hip.ptr(board), _hip.ptr(goals), _hip.ptr(scalars), _hip.ptr(out),
                                                  queue, _hip.ptr(active), _hip.current_stream_ptr()))

    def rewind(self, goals, scalars, mask=None):
        _hip.check(self.lib.slhip_history_rewind(self.ref, _hip.ptr(goals), _hip.ptr(scalars), _hip.ptr(mask),
                                                 _hip.current_stream_ptr()))

    def release(self, slots):
        idx = _dev(np.asarray(slots, np.int64))
        self.t["slot_state"][idx] = 0
        self.t["entries"][idx] = 0


def assert_state_equal(d, m, where):
    for name in ("owner", "cur_level", "cur_episode", "slot_state"):
        assert np.array_equal(d.host(name), getattr(m, name)), (where, name)
    c = d.host("counters")
    assert c[:5].tolist() == [m.episodes, m.kept, m.missed, m.incomplete, m.cursor] and not c[5:].any(), where
    got = d.host("entries")
    for name in hr.ENTRY_DTYPE.names:
        assert np.array_equal(got[name], m.entries[name]), (where, name)
    assert np.array_equal(d.host("goals"), m.goals), (where, "goals")
    assert np.array_equal(d.host("frames"), m.frames), (where, "frames")


def watch_sets(B):
    sets = [[0], [B - 1]]
    if B <= 65:
        sets.append(list(range(B)))
    edge = [e for e in (62, 63, 64, 65, 255, 256) if e < B] or [B // 2]
    sets.append(edge[-4:] if B < 257 else [63, 64, 255, 256])
    out = []
    for s in sets:
        if sorted(set(s)) not in out:
            out.append(sorted(set(s)))
    return out


class Synthetic(object):
    """Scripted step outputs and scalars; env e's board after step t holds ((e * 64 + t) << 4) + cell index, the board as the
    agent left it the same with bit 15 set; the boards of unwatched envs, and the records of envs that are not done, are
    poison.  The queue is scrambled within a step and holds phantom entries in front."""

    def __init__(self, rng, B, H, W, watch):
        self.rng, self.B, self.H, self.W, self.watch = rng, B, H, W, np.asarray(watch)
        self.level = rng.integers(0, 9, B).astype(np.int32)
        self.episode = rng.integers(0, 5, B).astype(np.int32)
        self.length = np.zeros(B, np.int32)
        self.goal_tag = np.arange(B, dtype=np.int64) * 3 + 1
        self.t = 0
        self.cap = 16 * B + 16
        self.q_env, self.q_episode = np.zeros(self.cap, np.int32), np.zeros(self.cap, np.int32)
        self.q_boards = np.full((self.cap, H, W), 0x0BAD, np.uint16)
        self.count = 0
        # phantoms: no such env, an unwatched env, a watched env's NEXT episode (an earlier entry when that one is played)
        for e, k in [(-1, 0), (B, 0), (int(watch[0]), int(self.episode[watch[0]]) + 1), (int(watch[-1]), -3)]:
            self.push(e, k, np.full((H, W), 0x0BAD, np.uint16))

    def push(self, e, k, board):
        if self.count < self.cap:
            self.q_env[self.count], self.q_episode[self.count], self.q_boards[self.count] = e, k, board
        self.count += 1

    def cells(self, e, final=False):
        v = (((e * 64 + self.t) << 4) + np.arange(self.H * self.W)) & 0x7FFF
        return (v | (0x8000 if final else 0)).astype(np.uint16).reshape(self.H, self.W)

    def goals(self):
        g = np.zeros((self.B, self.H, self.W), np.uint16)
        g[:] = (self.goal_tag & 0xFFFF).astype(np.uint16)[:, None, None]
        g[:, 0, 0] = np.arange(self.B) & 0xFFFF
        return g

    def scalars(self):
        sc = self.rng.integers(0, 1000, (self.B, 16)).astype(np.int32)
        sc[:, COLS["level_idx"]], sc[:, COLS["episode_idx"]], sc[:, COLS["episode_length"]] = self.level, self.episode, self.length
        return sc

    def step(self, p_done, drop=0, active=None):
        """-> board, goals, scalars (after the step), raw out [B,4], the model's out dict.  `drop`: that many of the done
        envs' queue entries are lost."""
        rng, B = self.rng, self.B
        self.t += 1
        self.length += 1
        done = ((rng.random(B) < p_done) | (self.length >= T_SYN)).astype(np.uint8)
        board = np.full((B, self.H, self.W), 0x0BAD, np.uint16)
        for e in self.watch:
            board[e] = self.cells(e)
        flags = np.zeros((B, 4), np.uint8)
        flags[:, 0], flags[:, 1], flags[:, 2] = done, rng.integers(0, 2, B), rng.integers(0, 2, B)
        length = self.length.copy()
        flags[done == 0, 1:] = 0xA5
        length[done == 0] = -99
        raw = np.zeros((B, 4), np.int32)
        raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3] = 7, flags.view(np.int32)[:, 0], 9, length
        ended = rng.permutation(np.flatnonzero(done))
        on = np.ones(B, bool) if active is None else active != 0
        lost = set(ended[on[ended]][:drop].tolist())
        for e in ended:
            if int(e) not in lost:
                self.push(int(e), int(self.episode[e]), self.cells(e, final=True))
        self.level[done != 0] = rng.integers(0, 9, int(done.sum()))
        self.episode[done != 0] += 1
        self.length[done != 0] = 0
        self.goal_tag[done != 0] += 1000
        out = dict(done=done, success=flags[:, 1], times_up=flags[:, 2], episode_length=length)
        return board, self.goals(), self.scalars(), raw, out

    def device_queue(self):
        q = _hip.EpisodeQueue()
        rec = np.zeros((self.cap, 8), np.int32)
        rec[:, 0], rec[:, 3] = self.q_env, self.q_episode
        self.keep = [_dev(np.array([self.count], np.int32)), _dev(rec), _dev(self.q_boards)]
        q.capacity, q.env_base = self.cap, 0
        q.count, q.records, q.boards = (k.data_ptr() for k in self.keep)
        return q

    def model_queue(self):
        return (self.count, self.q_env, self.q_episode, self.q_boards)

    def fresh_queue(self):
        self.count = 0


@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("shape", [(3, 3), (25, 25), (64, 64)])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_the_kernels_equal_the_model(B, shape, interval):
    """Per watch set: a rewind at attach, then steps with no env done, many done, a masked rewind, a step that loses queue
    entries, a release, a fresh queue and -- for the last watch set -- an active mask; the state after every call."""
    H, W = shape
    rng = np.random.default_rng(1000 * B + 10 * H + interval)
    kept = 0
    for w, watch in enumerate(watch_sets(B)):
        n = len(watch)
        K = max(1, n - 1) if interval == 1 else n + 3           # interval 1: the slots run out
        syn = Synthetic(rng, B, H, W, watch)
        d, m = DeviceHistory(B, watch, K, T_SYN, H, W, interval), hr.HistoryModel(B, watch, K, T_SYN, H, W, interval)
        sc = syn.scalars()
        d.rewind(_dev(syn.goals()), _dev(sc))
        m.rewind(syn.goals(), syn.level, syn.episode)
        assert_state_equal(d, m, (watch, "attach"))
        masked = w == len(watch_sets(B)) - 1
        plans = [0.0, 0.5, 0.3, "rewind", 0.4, "drop", "release", 0.5, "fresh", 0.6, 0.3, 1.0]
        for step, plan in enumerate(plans):
            where = (watch, step, plan)
            if plan == "rewind":
                mask = (rng.random(B) < 0.5).astype(np.uint8)
                sel = mask != 0
                syn.level[sel], syn.length[sel] = rng.integers(0, 9, int(sel.sum())), 0
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
                d.capture(_dev(board), _dev(goals), _dev(sc), _dev(raw), C.byref(syn.device_queue()),
                          None if active is None else _dev(active))
                m.capture(board, goals, syn.level, syn.episode, syn.length, out, syn.model_queue(), active)
            assert_state_equal(d, m, where)
        kept += m.kept
        if not masked:
            assert m.episodes >= B
            if interval == 1 and n > 1:
                assert m.missed >= 1                             # the slots did run out
    assert kept >= 1


def test_no_queue_means_no_final_frame():
    B, H, W = 5, 3, 3
    rng = np.random.default_rng(3)
    syn = Synthetic(rng, B, H, W, [1, 3])
    d, m = DeviceHistory(B, [1, 3], 6, T_SYN, H, W, 1), hr.HistoryModel(B, [1, 3], 6, T_SYN, H, W, 1)
    d.rewind(_dev(syn.goals()), _dev(syn.scalars())), m.rewind(syn.goals(), syn.level, syn.episode)
    for p in (0.0, 1.0):
        board, goals, sc, raw, out = syn.step(p)
        d.capture(_dev(board), _dev(goals), _dev(sc), _dev(raw), None)
        m.capture(board, goals, syn.level, syn.episode, syn.length, out, None)
        assert_state_equal(d, m, p)
    assert m.incomplete == m.kept == 2 and m.cursor == 0


# ------------------------------------------------------------------------------------------------------------ whole envs

B_E2E, T_E2E, LIMIT = 65, 40, 12
WATCH = [0, 7, 31, 32, 63, 64]
ENV_KW = dict(time_limit=LIMIT, view_shape=(15, 15), auto_reset=True)


def assert_history_equals_model(h, m, where=""):
    got, want = h.entries(), m.listing()
    for name in hr.ENTRY_DTYPE.names:
        assert np.array_equal(got[name], want[name]), (where, name)
    c = h.counters()
    assert (c["episodes"], c["kept"], c["missed"], c["incomplete"]) == (m.episodes, m.kept, m.missed, m.incomplete), where
    for i, en in enumerate(want):
        a, b = h.history(i), m.history(en)
        assert a["board"].dtype == a["goals"].dtype == np.uint16
        assert np.array_equal(a["board"], b["board"]) and np.array_equal(a["goals"], b["goals"]), (where, i)
    return len(want)


@pytest.mark.parametrize("family", ["prune_still_25", "append_spawn_25"])
def test_whole_envs_equal_the_restatement_and_an_env_without_a_history(family):
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool = util.pool_from_fixture(family, util.oracle_counts, n=8)[0]
    h = episode_history.EpisodeHistory(pool, B_E2E, WATCH, 10, interval=3)
    log = episode_log.EpisodeLog(pool, B_E2E, 1024)
    se = dict(capacity=256, num_samples=4)
    env = SafeLifeVectorEnv(pool, B_E2E, episode_history=h, episode_log=log, side_effects=se, **ENV_KW)
    plain = SafeLifeVectorEnv(pool, B_E2E, side_effects=se, **ENV_KW)
    assert plain.episode_history is None and sorted(plain.t) == sorted(env.t)
    d = hr.OracleDrive(pool, B_E2E, LIMIT, WATCH, 10, 3)
    assert np.array_equal(env.reset().cpu().numpy(), plain.reset().cpu().numpy())
    actions = np.random.default_rng(17).integers(0, 9, (T_E2E, B_E2E)).astype(np.int32)
    seen = 0
    for t in range(T_E2E):
        env.step(actions[t]), plain.step(actions[t]), d.step(actions[t])
        for name in ("reward", "done", "obs", "board", "goals", "level_idx", "episode_idx", "success", "rng"):
            assert np.array_equal(env.numpy(name), plain.numpy(name)), (t, name)
        assert np.array_equal(env.numpy("board"), d.A["board"]), t
        if t in (13, 27):
            seen += assert_history_equals_model(h, d.model, t)
            rows = log.rows()
            for en in h.entries():
                row = rows[int(en["row"])]
                assert (row["env"], row["episode_idx"], row["level"], row["length"]) == (en["env"], en["episode_idx"],
                                                                                         en["level"], en["length"])
            slots = h.entries()["slot"].tolist()
            assert h.release() == len(slots)
            d.model.release(slots)
            env.side_effects_flush(), plain.side_effects_flush(), d.flush()
    seen += assert_history_equals_model(h, d.model, "end")
    assert seen >= 6 and h.counters()["incomplete"] == 0 and h.counters()["episodes"] == log.counters()["episodes"]


def test_the_fixture_s_runs_on_the_device_equal_what_the_reference_saved(golden):  # noqa: F811
    from safelife_amd.vector_env import SafeLifeVectorEnv
    g = golden
    pool = fixture_pool(g)
    for r in map(str, g["runs"]):
        T, acts = int(g[r + "_time_limit"]), g[r + "_actions"]
        h = episode_history.EpisodeHistory(pool, 5, range(5), 40, interval=int(g[r + "_interval"]))
        env = SafeLifeVectorEnv(pool, 5, episode_history=h, side_effects=dict(capacity=64, num_samples=4), time_limit=T,
                                episode_streams=False)
        env.reset()
        ended = {}
        for t in range(len(acts)):
            env.step(acts[t])
            for e in np.flatnonzero(env.numpy("done")):
                ended[(int(e), int(env.numpy("episode_idx")[e]) - 1)] = t
        listing = h.entries()
        assert listing["row"].tolist() == g[r + "_kept"].tolist() and not (listing["flags"] & _hip.HIST_NO_FINAL).any()
        for i, en in enumerate(listing):
            k, n, e = int(en["row"]), int(en["length"]), int(en["env"])
            assert (e, n, en["level"]) == (g[r + "_env"][k], g[r + "_length"][k], g[r + "_level"][k])
            end = ended[(e, int(en["episode_idx"]))]
            hist = h.history(i)
            want = g["%s_board_%d" % (r, k)]
            assert np.array_equal(hist["goals"], g["%s_goals_%d" % (r, k)])
            assert np.array_equal(hist["board"][-1], want[-1])
            nxt = [int(acts[end - n + 2 + f][e]) for f in range(n - 1)]
            assert np.array_equal(hr.as_the_reference_saved(hist["board"], nxt), want), (r, k)


def test_under_a_level_schedule_the_entry_names_the_level_that_was_played():
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=8)[0]
    sched = schedule.LevelSchedule(pool, [(0, 4), (4, 4)], mode="uniform", seed=5)
    B = 16
    h = episode_history.EpisodeHistory(pool, B, [2, 9, 15], 24)
    env = SafeLifeVectorEnv(pool, B, episode_history=h, level_schedule=sched, side_effects=dict(capacity=128, num_samples=4),
                            time_limit=4, first_level=None)
    env.reset()
    actions = np.random.default_rng(2).integers(0, 9, (20, B)).astype(np.int32)
    played = {}
    for t in range(len(actions)):
        before = (env.numpy("level_idx").copy(), env.numpy("episode_idx").copy())
        env.step(actions[t])
        for e in np.flatnonzero(env.numpy("done")):
            played[(int(e), int(before[1][e]))] = int(before[0][e])
    listing = h.entries()
    assert len(listing) >= 9 and len(set(listing["level"].tolist())) >= 3
    for en in listing:
        assert en["level"] == played[(int(en["env"]), int(en["episode_idx"]))]


def test_an_episode_run_gives_exactly_its_tickets_histories():
    """7 tickets on 5 envs, every env watched, interval 1: 7 histories, none of a phantom episode, each what a plain env
    plays on that level under the same actions (prune-still has no spawners: no generator takes part)."""
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=4)[0]
    B, N, limit = 5, 7, 6
    run = episode_run.EpisodeRun(pool, B, N)
    h = episode_history.EpisodeHistory(pool, B, range(B), 16)
    env = SafeLifeVectorEnv(pool, B, episode_run=run, episode_history=h, side_effects=dict(capacity=64, num_samples=4),
                            time_limit=limit, **run.env_arguments())
    run.start()
    rng = np.random.default_rng(8)
    actions = []
    for _ in range(4 * limit):
        actions.append(rng.integers(0, 9, B).astype(np.int32))
        env.step(actions[-1])
    assert run.finished() and h.counters() == dict(episodes=N, kept=N, missed=0, incomplete=0)
    listing, results = h.entries(), run.results()
    assert listing["row"].tolist() == list(range(N)) and sorted(zip(listing["env"], listing["level"])) == sorted(
        (int(r["env"]), int(r["slot"])) for r in results)
    for i, en in enumerate(listing):
        res = results[[int(r["env"]) == en["env"] and int(r["episode_idx"]) == en["episode_idx"] for r in results]]
        assert len(res) == 1 and res[0]["length"] == en["length"] and res[0]["flags"] & _hip.RUN_WRITTEN
        end, n, e = int(res[0]["step"]), int(en["length"]), int(en["env"])
        one = SafeLifeVectorEnv(pool, 1, first_level=int(en["level"]), auto_reset=False, time_limit=limit)
        one.reset()
        want = []
        for t in range(end - n, end):
            one.step(actions[t][e:e + 1])
            want.append(one.numpy("board")[0])
        assert np.array_equal(h.history(i)["board"], np.array(want)), i
        assert np.array_equal(h.history(i)["goals"][0], one.numpy("goals")[0])


def test_without_auto_reset_the_final_frame_still_comes_from_the_queue():
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=4)[0]
    B, limit = 6, 5
    h = episode_history.EpisodeHistory(pool, B, [1, 4], 12)
    env = SafeLifeVectorEnv(pool, B, episode_history=h, side_effects=dict(capacity=64, num_samples=4), time_limit=limit,
                            auto_reset=False)
    d = hr.OracleDrive(pool, B, limit, [1, 4], 12)
    env.reset()
    actions = np.random.default_rng(4).integers(0, 9, (13, B)).astype(np.int32)
    for t in range(len(actions)):
        env.step(actions[t]), d.step(actions[t])
        done = env.numpy("done")
        if done.any():
            env.reset(done)
        assert np.array_equal(env.numpy("board"), d.A["board"]), t
    assert assert_history_equals_model(h, d.model) >= 4 and h.counters()["incomplete"] == 0


def test_frames_save_and_the_runner(tmp_path):
    torch = _torch()
    from safelife_amd.runner import VectorRunner
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=4)[0]
    B = 4
    h = episode_history.EpisodeHistory(pool, B, [0, 3], 6)
    env = SafeLifeVectorEnv(pool, B, episode_history=h, side_effects=dict(capacity=32, num_samples=4), time_limit=3,
                            policy_layout="uint8", with_obs=False, view_shape=(9, 9))

    def uniform(obs):
        return torch.zeros(obs.shape[0], device=obs.device), torch.full((obs.shape[0], 9), 1.0 / 9, device=obs.device)
    runner = VectorRunner(env, uniform, generator=torch.Generator(device=env.device).manual_seed(3))
    for _ in runner.run_steps(7):
        pass
    assert runner.env.episode_history is h and h.counters()["kept"] >= 4          # two episodes of each watched env
    hist = h.history(1)
    assert hist["board"].shape == hist["goals"].shape == (3, 25, 25)
    on_device = h.history(1, device=True)
    assert on_device["board"].is_cuda and np.array_equal(on_device["board"].cpu().numpy().view(np.uint16), hist["board"])
    assert np.array_equal(on_device["goals"].cpu().numpy().view(np.uint16), hist["goals"])
    frames = h.frames(1)
    assert frames.is_cuda and tuple(frames.shape) == (3, 25 * 14, 25 * 14, 3)
    assert np.array_equal(frames.cpu().numpy(), render.render_board_host(hist["board"], hist["goals"]))
    path = str(tmp_path / "episode.npz")
    h.save(1, path)
    with np.load(path) as f:
        assert sorted(f.files) == ["board", "goals"]
        assert np.array_equal(f["board"], hist["board"]) and np.array_equal(f["goals"], hist["goals"])
    rows = h.entries()["row"]
    assert h.release([0, 2]) == 2 and h.entries()["row"].tolist() == np.delete(rows, [0, 2]).tolist()


def test_refusals():
    from safelife_amd.levels import Level, LevelPool
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=4)[0]
    se = dict(capacity=32, num_samples=4)
    with pytest.raises(ValueError, match="finished-episode queue"):
        SafeLifeVectorEnv(pool, 4, episode_history=episode_history.EpisodeHistory(pool, 4, [0], 2), time_limit=5)
    with pytest.raises(ValueError, match=r"max_bytes allows 1000"):
        SafeLifeVectorEnv(pool, 4, episode_history=episode_history.EpisodeHistory(pool, 4, [0], 2, max_bytes=1000),
                          side_effects=se, time_limit=5)
    h = episode_history.EpisodeHistory(pool, 4, [0], 2)
    env = SafeLifeVectorEnv(pool, 4, episode_history=h, side_effects=se, time_limit=5, slices=2)
    with pytest.raises(ValueError, match="already serves"):
        SafeLifeVectorEnv(pool, 4, episode_history=h, side_effects=se, time_limit=5)
    acts = np.zeros(4, np.int32)
    for call in (lambda: env.step_async(acts), lambda: env.step_slice(0, acts), lambda: env.step_queues(acts),
                 lambda: env.queues_open(), lambda: env.rollout(np.zeros((2, 4), np.int32))):
        with pytest.raises(ValueError, match="cannot drive an episode history"):
            call()
    # a level with a blinker in its goals: one CA step changes them
    lv = pool.levels[0]
    goals = np.zeros_like(lv.goals)
    goals[10, 9:12] = 9 | (2 << 9)                      # three live green cells in a row
    moving = Level(lv.board, goals, lv.agent_locs, spawn_prob=lv.spawn_prob, min_performance=lv.min_performance,
                   points_table=lv.points_table, rng_words=lv.rng_words)
    bad = LevelPool([pool.levels[1], moving], counts_fn=util.oracle_counts)
    with pytest.raises(ValueError, match=r"need static goals.*pool slot\(s\) \[1\]"):
        SafeLifeVectorEnv(bad, 4, episode_history=episode_history.EpisodeHistory(bad, 4, [0], 2), side_effects=se,
                          time_limit=5)
