"""
Level schedules on the device (csrc/sl_schedule.hip, safelife_amd/schedule.py): every kernel against the host restatement
of tests/schedule_ref.py, and a scheduled SafeLifeVectorEnv against the plain one -- which is itself held to the oracle --
replaying the levels the schedule chose.
"""
import ctypes as C
import os

import numpy as np
import pytest

from safelife_amd import _hip, levels, schedule
from tests import schedule_ref as sr
from tests import util
from tests.test_level_schedule_host import CURRICULUM_BOUND

pytestmark = pytest.mark.gpu

M64 = 2 ** 64 - 1


def _torch():
    import torch
    return torch


class DeviceSchedule(object):
    """A struct sl_level_schedule with its device arrays, fresh (ring[g][0] = 0.0, count = pos = 1)."""

    def __init__(self, groups, L, lookback=100, B=1, cur_slot=None, reward_possible=None, min_performance=None,
                 available=None):
        torch = _torch()
        dev = _hip.device()
        G = len(groups)
        t = self.t = {}
        t["min_performance"] = torch.from_numpy(np.zeros(L) if min_performance is None else np.asarray(min_performance, np.float64)).to(dev)
        t["available"] = torch.from_numpy(np.zeros(L, np.int32) if available is None else np.asarray(available, np.int32)).to(dev)
        t["reward_possible"] = torch.from_numpy(np.ones(L, np.int32) if reward_possible is None
                                                else np.asarray(reward_possible, np.int32)).to(dev)
        t["cur_slot"] = torch.from_numpy(np.zeros(B, np.int32) if cur_slot is None else np.asarray(cur_slot, np.int32)).to(dev)
        t["ring"] = torch.zeros((G, lookback), dtype=torch.float64, device=dev)
        t["count"] = torch.ones(G, dtype=torch.int64, device=dev)
        t["episodes"] = torch.zeros(G, dtype=torch.int64, device=dev)
        t["pos"] = torch.ones(G, dtype=torch.int32, device=dev)
        t["best"] = torch.zeros(G, dtype=torch.float64, device=dev)
        t["mean"] = torch.zeros(G, dtype=torch.float64, device=dev)
        t["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
        s = self.struct = _hip.LevelSchedule()
        s.G, s.lookback, s.L = G, lookback, L
        for g, (a, n) in enumerate(groups):
            s.start[g], s.len[g] = a, n
        for name in t:
            setattr(s, name, t[name].data_ptr())
        self.ref = C.byref(s)

    def host(self, name):
        return self.t[name].cpu().numpy()


def _group_sets(L):
    """Group layouts for a pool of L slots: G in {1, 2, 3, 8} where they fit, with groups of length 1, slots outside
    every group and zero-probability groups."""
    sets = [([(0, L)], [1.0]), ([(L - 1, 1)], [0.25])]
    if L >= 2:
        sets.append(([(0, 1), (1, L - 1)], [0.3, 0.7]))
        sets.append(([(1, L - 1), (0, 1)], [0.0, 2.0]))                     # (not sorted; the first never drawn)
    if L >= 63:
        sets.append(([(2, 20), (30, 1), (L - 7, 6)], [0.2, 0.0, 0.8]))      # slots 0, 1, 22..29, ... L-1 in no group
        sets.append(([(3, 1), (5, 1), (40, 17)], [1e-3, 1.0, 1e3]))
        w = [1, 7, 2, 9, 1, 4, 8, 5]
        at, eight = 1, []
        for n in w:
            eight.append((at, n))
            at += n + 1                                                     # a gap behind every group
        sets.append((eight, [0.05, 0.1, 0.0, 0.2, 0.15, 0.0, 0.3, 0.2]))
        sets.append((eight, [1.0] * 8))
    return sets


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 1000, 4097])
def test_draw_equals_the_model(L):
    """slhip_schedule_draw element for element: probabilities by value and from the device array, seed and counter at 0
    and 2^64 - 1, into the middle of a canary buffer."""
    torch = _torch()
    lib, st = _hip.lib(), _hip.current_stream_ptr()
    PAD = 64
    for groups, probs in _group_sets(L):
        d = DeviceSchedule(groups, L)
        dprobs = torch.tensor(probs, dtype=torch.float64, device=_hip.device())
        for seed, counter in ((0, 0), (M64, M64), (0, M64), (0x1234567890ABCDEF, 41)):
            want = sr.draw(groups, probs, seed, counter, L)
            for by_value in (True, False):
                buf = torch.full((L + 2 * PAD,), -7, dtype=torch.int32, device=_hip.device())
                hp = (C.c_double * len(probs))(*probs) if by_value else None
                _hip.check(lib.slhip_schedule_draw(d.ref, hp, _hip.ptr(dprobs), seed, counter, buf.data_ptr() + 4 * PAD, L, st))
                got = buf.cpu().numpy()
                assert (got[:PAD] == -7).all() and (got[PAD + L:] == -7).all()
                assert np.array_equal(got[PAD:PAD + L], want), (groups, probs, seed, counter, by_value)
        member = np.zeros(L, bool)
        for (a, n), p in zip(groups, probs):
            if p > 0:
                member[a:a + n] = True
        assert member[want].all()                       # every successor lies in a group that can be drawn
        assert d.host("status")[0] == 0


def test_draw_falls_back_on_bad_device_probabilities():
    torch = _torch()
    lib, st, L = _hip.lib(), _hip.current_stream_ptr(), 300
    groups = [(0, 100), (150, 1), (200, 100)]
    out = torch.zeros(L, dtype=torch.int32, device=_hip.device())
    for bad in ([0.0, 0.0, 0.0], [float("nan"), 0.5, 0.5], [0.5, float("inf"), 0.5], [0.5, -0.25, 0.75],
                [1e308, 1e308, 0.0]):
        d = DeviceSchedule(groups, L)
        p = torch.tensor(bad, dtype=torch.float64, device=_hip.device())
        _hip.check(lib.slhip_schedule_draw(d.ref, None, _hip.ptr(p), 5, 9, _hip.ptr(out), L, st))
        probs, status = sr.device_probs(bad)
        assert status == sr.BAD_PROBS and d.host("status")[0] == _hip.SCHEDULE_BAD_PROBS
        assert np.array_equal(out.cpu().numpy(), sr.draw(groups, probs, 5, 9, L)), bad
        # a good array afterwards draws from it; the bit stays up (only ever raised)
        p.copy_(torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
        _hip.check(lib.slhip_schedule_draw(d.ref, None, _hip.ptr(p), 5, 10, _hip.ptr(out), L, st))
        assert (out.cpu().numpy() >= 200).all() and d.host("status")[0] == _hip.SCHEDULE_BAD_PROBS


def _ulp_neighbours(x):
    return [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]


@pytest.mark.parametrize("L", [1, 65, 1000])
def test_required_points_bit_for_bit(L):
    """slhip_schedule_required against levels.required_points(np.float64(mp) * fraction, available) on every slot, the
    other seven words of every record untouched.  Fractions: 0, 0.001, 0.5, 1, 1 - 2^-53, and fractions that put
    mp * fraction * available on an integer for the slots built for it (mp 0.5, 24 points: 0.75 -> 9 exactly; mp 0.3,
    50 points: 0.2 -> about 3) with one ulp to either side."""
    torch = _torch()
    lib, st = _hip.lib(), _hip.current_stream_ptr()
    rng = np.random.default_rng(L)
    mp = rng.choice([-1.0, 0.0, 0.5, 0.3, 1.0 / 3.0, 1.0, 0.001, 0.999], L)
    avail = rng.integers(-40, 200, L).astype(np.int32)
    special = [(0.5, 24), (0.3, 50), (-1.0, 30), (-1.0, -30), (1.0, 2 ** 31 - 1), (0.5, -2 ** 31), (1.0, 0), (0.5, 26)]
    for k, (m, a) in enumerate(special[:L]):
        mp[k], avail[k] = m, a
    d = DeviceSchedule([(0, L)], L, min_performance=mp, available=avail)
    records = rng.integers(-2 ** 31, 2 ** 31 - 1, (L, 8)).astype(np.int32)
    fractions = [0.0, 0.001, 0.5, 1.0, 1.0 - 2.0 ** -53] + _ulp_neighbours(0.75) + _ulp_neighbours(0.2)
    on_integer = 0
    for f in fractions:
        ps = torch.from_numpy(records).to(_hip.device())
        _hip.check(lib.slhip_schedule_required(d.ref, float(f), _hip.ptr(ps), L, st))
        got = ps.cpu().numpy()
        want = np.array([levels.required_points(np.float64(mp[l]) * f, int(avail[l])) for l in range(L)])
        assert np.array_equal(got[:, 3], want), f
        assert np.array_equal(got[:, 3], [sr.required_points(mp[l], f, avail[l]) for l in range(L)])
        keep = [0, 1, 2, 4, 5, 6, 7]
        assert np.array_equal(got[:, keep], records[:, keep]), f
        v = (mp * f) * avail.astype(np.float64)
        on_integer += int(((v == np.round(v)) & (v > 0)).sum())
    assert on_integer > 0


def _out_records(reward, done, episode_reward):
    """struct sl_step_out rows as int32 [B, 4]."""
    B = len(done)
    rec = np.zeros((B, 4), np.int32)
    rec[:, 0] = np.asarray(reward, np.float32).view(np.int32)
    flags = np.zeros((B, 4), np.uint8)
    flags[:, 0] = done
    rec[:, 1] = flags.view(np.int32)[:, 0]
    rec[:, 2] = np.asarray(episode_reward, np.float32).view(np.int32)
    rec[:, 3] = 1
    return rec


def _assert_state(d, m, where):
    for name in ("ring", "count", "episodes", "pos", "best", "mean", "cur_slot"):
        got, want = d.host(name), getattr(m, name)
        if got.dtype.kind == "f":       # bit for bit
            assert np.array_equal(got.view(np.int64), np.asarray(want, np.float64).view(np.int64)), (where, name, got, want)
        else:
            assert np.array_equal(got, want), (where, name, got, want)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1025, 16449])      # (16449: past the harvest's tile of 16384 envs)
def test_harvest_and_curriculum_equal_the_model(B):
    """Scripted `out` / `level_idx` streams: rings and counters bit for bit after every step, the curriculum's probabilities
    within the measured bound.  Steps with no env done, with every env done (the order of the appends is then what the
    ring holds), and random ones; lookback 4, so the rings wrap many times; slots outside every group and slots whose
    reward_possible is 0."""
    torch = _torch()
    lib, st, dev = _hip.lib(), _hip.current_stream_ptr(), _hip.device()
    rng = np.random.default_rng(B)
    L, lookback = 40, 4
    groups = [(2, 10), (13, 1), (20, 15)]                          # 0, 1, 12, 14..19, 35..39 in no group
    possible = rng.integers(5, 60, L).astype(np.int32)
    possible[[4, 25]] = 0
    def slots():                                                    # (one in five on the group of a single slot)
        return np.where(rng.random(B) < 0.2, 13, rng.integers(0, L, B)).astype(np.int32)
    cur = slots()
    d = DeviceSchedule(groups, L, lookback=lookback, B=B, cur_slot=cur, reward_possible=possible)
    m = sr.ScheduleModel(groups, lookback, possible, cur)
    probs = torch.zeros(3, dtype=torch.float64, device=dev)
    patterns = ["none", "all", "random", "random", "all", "none", "random", "one", "random", "all", "random", "random"]
    worst = 0.0
    for t, pattern in enumerate(patterns):
        done = {"none": np.zeros(B, bool), "all": np.ones(B, bool), "random": rng.random(B) < 0.3,
                "one": np.arange(B) == B - 1}[pattern]
        ep = np.round(rng.normal(10.0 + 2.0 * t, 8.0, B)).astype(np.float32)
        ep[rng.random(B) < 0.1] = 0.0
        level_idx = slots()
        scal = np.zeros((B, 16), np.int32)
        scal[:, _hip.SCALAR_COLS["level_idx"]] = level_idx
        out = torch.from_numpy(_out_records(rng.normal(0, 1, B), done, ep)).to(dev)
        scalars = torch.from_numpy(scal).to(dev)
        _hip.check(lib.slhip_schedule_harvest(d.ref, _hip.ptr(out), _hip.ptr(scalars), B, st))
        _hip.check(lib.slhip_schedule_curriculum(d.ref, _hip.ptr(probs), st))
        m.harvest(done.astype(np.uint8), ep, level_idx)
        _assert_state(d, m, (t, pattern))
        diff = np.abs(probs.cpu().numpy() - m.curriculum()).max()
        worst = max(worst, diff)
        assert diff <= CURRICULUM_BOUND, (t, pattern, diff)
    print("B=%d: largest |device - model| of the probabilities %r" % (B, worst))
    if B >= 63:
        assert (m.count > 2 * lookback).all()


@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_golden_episodes_one_per_step(case, golden_dir):
    """The golden curricula (the reference's CurricularLevelIterator fed scripted episodes) through the two kernels, one
    episode per harvest: every logged probability within the measured bound, best_perf_lvl* exact."""
    torch = _torch()
    lib, st, dev = _hip.lib(), _hip.current_stream_ptr(), _hip.device()
    with np.load(os.path.join(golden_dir, "schedule_cases.npz")) as z:
        g = {k: z[k] for k in z.files}
    G, lookback = int(g["cur_groups"][case]), int(g["cur_lookback"][case])
    lo, hi = int(g["cur_offsets"][case]), int(g["cur_offsets"][case + 1])
    N, K = hi - lo, 91                                  # group k = slots [k * 91, (k + 1) * 91): one per reward_possible
    assert g["cur_possible"][lo:hi].max() < K
    slot = g["cur_group"][lo:hi].astype(np.int64) * K + g["cur_possible"][lo:hi]
    possible = np.tile(np.arange(K, dtype=np.int32), G)
    d = DeviceSchedule([(k * K, K) for k in range(G)], G * K, lookback=lookback, B=1, cur_slot=slot[:1],
                       reward_possible=possible)
    out = torch.from_numpy(_out_records(np.zeros(N), np.ones(N, np.uint8), g["cur_reward"][lo:hi])).to(dev)
    scal = np.zeros((N, 16), np.int32)
    scal[:-1, _hip.SCALAR_COLS["level_idx"]] = slot[1:]                 # after episode e the env stands on episode e+1's slot
    scalars = torch.from_numpy(scal).to(dev)
    probs = torch.zeros((N, 8), dtype=torch.float64, device=dev)
    best = torch.zeros((N, G), dtype=torch.float64, device=dev)
    for e in range(N):
        _hip.check(lib.slhip_schedule_harvest(d.ref, out.data_ptr() + 16 * e, scalars.data_ptr() + 64 * e, 1, st))
        _hip.check(lib.slhip_schedule_curriculum(d.ref, probs.data_ptr() + 64 * e, st))
        best[e].copy_(d.t["best"])
    got = probs.cpu().numpy()
    diff = np.abs(got[:, :G] - g["cur_probs"][lo:hi, :G]).max()
    print("case %d (G=%d, lookback=%d, %d episodes): largest |device - reference| %r" % (case, G, lookback, N, diff))
    assert diff <= CURRICULUM_BOUND, diff
    assert np.array_equal(best.cpu().numpy(), g["cur_best"][lo:hi, :G])
    assert (d.host("count") > 2 * lookback).all() and d.host("episodes").sum() == N


# ----------------------------------------------------------------------------------------------------------- end to end

WRAPPERS = dict(movement_bonus=0.1, movement_bonus_power=0.01, movement_bonus_period=4, as_penalty=True, exit_bonus=0.5,
                penalty_coef=0.3, ignore_reward_cells=False)
ENV_KW = dict(time_limit=7, view_shape=(15, 15), auto_reset=True, wrappers=WRAPPERS, env_offset=128)
B_E2E, T_E2E, N_LEVELS = 70, 60, 12


def _two_family_lists():
    a = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=N_LEVELS)[0].levels
    b = util.pool_from_fixture("append_spawn_25", util.oracle_counts, n=N_LEVELS)[0].levels
    return a, b


def _fraction(t):
    return 0.001 if t < 15 else (0.5 if t < 35 else 1.0)


def _run_scheduled(sched, actions, on_step=None):
    """Step a scheduled env through `actions`; the schedule's training step is the step index.  -> per-step outputs, and
    per env the slots it loaded with the fraction in force at each load."""
    from safelife_amd.vector_env import SafeLifeVectorEnv
    env = SafeLifeVectorEnv(sched.pool, B_E2E, level_schedule=sched, **ENV_KW)
    sched.training_steps = 0
    obs = env.reset()
    frac = sched.fraction()
    loaded = [[(int(s), frac, -1)] for s in env.numpy("level_idx")]
    steps = [dict(obs=obs.cpu().numpy().copy(), board=env.numpy("board").copy())]
    for t in range(len(actions)):
        sched.training_steps = t
        before = env.numpy("level_idx").copy()
        env.step(actions[t])
        frac = sched.fraction()
        rec = dict(obs=env.numpy("obs").copy(), board=env.numpy("board").copy(), reward=env.numpy("reward").copy(),
                   shaped=env.shaped_reward.cpu().numpy().copy(), done=env.numpy("done").copy(),
                   level_idx=env.numpy("level_idx").copy(), before=before)
        for k in env.info:                              # (the step's records, not the envs' running counters)
            rec[k] = env.info[k].cpu().numpy().copy()
        steps.append(rec)
        for e in np.flatnonzero(rec["done"]):
            loaded[e].append((int(rec["level_idx"][e]), frac, t))
        if on_step is not None:
            on_step(t, env, rec)
    return env, steps, loaded


def _replay_on_a_plain_env(sched, actions, steps, loaded):
    """A plain LevelPool whose levels are each env's sequence laid end to end -- the same rng words, required_step of the
    fraction in force when the env loaded the level -- and a plain env walking it with level_stride 1 must give what the
    scheduled env gave, at every step."""
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool = sched.pool
    lv, frac, first, at = [], [], [], 0
    for seq in loaded:
        first.append(at)
        for slot, f, _ in seq:
            src = pool.levels[slot]
            lv.append(levels.Level(src.board, src.goals, src.agent_locs, src.spawn_prob, src.min_performance, src.points_table,
                                   rng_words=pool.pool_rng[slot]))
            frac.append((slot, f))
        at += len(seq)
    flat = levels.LevelPool(lv, counts_fn=util.oracle_counts, exit_slots=pool.exit_slots)
    for k, (slot, f) in enumerate(frac):
        flat.pool_required_step[k] = levels.required_points(np.float64(sched.min_performance[slot]) * f, int(sched.available[slot]))
    assert np.array_equal(flat.pool_required_reset, pool.pool_required_reset[[s for s, _ in frac]])
    env = SafeLifeVectorEnv(flat, B_E2E, first_level=np.array(first), level_stride=1, **ENV_KW)
    assert not env.struct.pool_next
    obs = env.reset()
    assert np.array_equal(obs.cpu().numpy(), steps[0]["obs"]) and np.array_equal(env.numpy("board"), steps[0]["board"])
    for t in range(len(actions)):
        env.step(actions[t])
        want = steps[t + 1]
        assert np.array_equal(env.numpy("reward").view(np.int32), want["reward"].view(np.int32)), t
        assert np.array_equal(env.shaped_reward.cpu().numpy().view(np.int64), want["shaped"].view(np.int64)), t
        assert np.array_equal(env.numpy("done"), want["done"]), t
        for k in env.info:
            assert np.array_equal(env.info[k].cpu().numpy(), want[k]), (t, k)
        assert np.array_equal(env.numpy("obs"), want["obs"]), t
        assert np.array_equal(env.numpy("board"), want["board"]), t


def test_switching_run_equals_a_plain_env_on_the_chosen_levels():
    """70 envs (they cross a wave), time_limit 7 (every env plays several episodes in 60 steps), scripted actions, wrappers
    and observations on, on spawner pools; p goes 0 -> 1 and the exit-difficulty fraction changes twice.  The successor
    of every load is the host model's draw, group membership follows p, and the whole run equals the plain path."""
    a, b = _two_family_lists()
    p = schedule.LinearSchedule([20, 40], [0.0, 1.0])
    sched = schedule.LevelSchedule.from_pools([a, b], pool_args=dict(counts_fn=util.oracle_counts), mode="switching", seed=11,
                                              p_switch=p, min_performance_fraction=_fraction)
    actions = np.random.default_rng(3).integers(0, 9, (T_E2E, B_E2E)).astype(np.int32)
    seed = (11 + sr.G64 * ENV_KW["env_offset"]) & M64
    L = len(sched.pool)

    def check(t, env, rec):
        pt = p(t)
        table = sr.draw(sched.groups, [1.0 - pt, pt], seed, t + 1, L)       # (the reset took draw 0)
        assert np.array_equal(env.level_schedule.t["pool_next"].cpu().numpy(), table), t
        d = rec["done"] != 0
        assert np.array_equal(rec["level_idx"][d], table[rec["before"][d]]), t
        assert np.array_equal(rec["level_idx"][~d], rec["before"][~d]), t

    env, steps, loaded = _run_scheduled(sched, actions, check)
    sched.training_steps = 0                                            # (first_levels reads the schedule where the env did)
    assert np.array_equal([seq[0][0] for seq in loaded], sched.first_levels(B_E2E, ENV_KW["env_offset"]))
    assert all(seq[0][0] < N_LEVELS for seq in loaded)                   # p = 0 at step 0: everybody starts in family 0
    n_loads = [len(seq) for seq in loaded]
    assert min(n_loads) >= 5
    late = [slot for seq in loaded for slot, _, t in seq if t >= 40]
    early = [slot for seq in loaded for slot, _, t in seq if 0 <= t <= 20]
    assert late and early and all(s >= N_LEVELS for s in late) and all(s < N_LEVELS for s in early)
    assert len({f for seq in loaded for _, f, _ in seq}) == 3           # the fraction changed twice
    st = sched.stats()
    assert st["episodes"].sum() == sum(n_loads) - B_E2E and st["status"] == 0
    _replay_on_a_plain_env(sched, actions, steps, loaded)


def test_curriculum_run_equals_the_model_fed_its_own_records():
    """Curriculum mode (lookback 5, so the slopes count from early on), with a finished-episode queue attached: the
    probabilities the device draws from are the model's -- fed the run's own done flags, episode rewards and slots --
    within the measured bound, every load is the model's draw from them, and the counters are the model's bit for bit."""
    from safelife_amd.vector_env import SafeLifeVectorEnv
    a, b = _two_family_lists()
    sched = schedule.LevelSchedule.from_pools([a, b[:5], b[5:]], pool_args=dict(counts_fn=util.oracle_counts),
                                              mode="curriculum", seed=12, lookback=5, min_performance_fraction=0.25)
    actions = np.random.default_rng(4).integers(0, 9, (T_E2E, B_E2E)).astype(np.int32)
    kw = dict(ENV_KW, side_effects=dict(capacity=1024, num_samples=8))
    env = SafeLifeVectorEnv(sched.pool, B_E2E, level_schedule=sched, **kw)
    env.reset()
    L = len(sched.pool)
    possible = sched.available.astype(np.int64) + 1
    m = sr.ScheduleModel(sched.groups, 5, possible, env.numpy("level_idx"))
    seed = (12 + sr.G64 * ENV_KW["env_offset"]) & M64
    worst, episodes, old_slots = 0.0, 0, []
    for t in range(T_E2E):
        before = env.numpy("level_idx").copy()
        want_p = m.curriculum()
        env.step(actions[t])
        got_p = sched.stats()["probabilities"]
        worst = max(worst, np.abs(got_p - want_p).max())
        assert np.abs(got_p - want_p).max() <= CURRICULUM_BOUND, t
        table = sr.draw(sched.groups, want_p, seed, t + 1, L)
        assert np.array_equal(sched.t["pool_next"].cpu().numpy(), table), t
        done, now = env.numpy("done") != 0, env.numpy("level_idx")
        assert np.array_equal(now[done], table[before[done]]) and np.array_equal(now[~done], before[~done])
        m.harvest(done.astype(np.uint8), env.info["episode_reward"].cpu().numpy(), now)
        for name in ("ring", "count", "episodes", "pos", "best", "mean", "cur_slot"):
            got = sched.t[name].cpu().numpy()
            assert np.array_equal(got, getattr(m, name)), (t, name)
        episodes += int(done.sum())
        old_slots += before[done].tolist()
    print("largest |device - model| of the probabilities over the run: %r" % worst)
    st = sched.stats()
    assert st["episodes"].sum() == episodes > 4 * B_E2E and st["status"] == 0 and (st["records"] > 10).all()
    # required points of the fraction 0.25, on every slot
    want = [levels.required_points(np.float64(sched.min_performance[l]) * 0.25, int(sched.available[l])) for l in range(L)]
    assert np.array_equal(env.t["pool_scalars"].cpu().numpy()[:, 3], want)
    # the finished-episode queue saw the same episodes on the same (old) slots
    rec = env.side_effects_flush().records()
    assert sorted(rec["level"].tolist()) == sorted(old_slots)


def test_without_a_schedule_nothing_changes():
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool = util.pool_from_fixture("append_spawn_25", util.oracle_counts, n=N_LEVELS)[0]
    actions = np.random.default_rng(5).integers(0, 9, (20, B_E2E)).astype(np.int32)
    one = SafeLifeVectorEnv(pool, B_E2E, level_schedule=None, **ENV_KW)
    two = SafeLifeVectorEnv(pool, B_E2E, **ENV_KW)
    assert one.level_schedule is None and not one.struct.pool_next and not two.struct.pool_next
    assert np.array_equal(one.reset().cpu().numpy(), two.reset().cpu().numpy())
    for t in range(len(actions)):
        one.step(actions[t]), two.step(actions[t])
        for name in ("reward", "done", "obs", "board", "level_idx", "success", "rng"):
            assert np.array_equal(one.numpy(name), two.numpy(name)), (t, name)
        assert np.array_equal(one.shaped_reward.cpu().numpy(), two.shaped_reward.cpu().numpy())
    assert not one.struct.pool_next


def test_what_cannot_drive_a_schedule_says_so():
    torch = _torch()
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=8)[0]
    sched = schedule.LevelSchedule(pool, [(0, 4), (4, 4)], mode="uniform", seed=1)
    env = SafeLifeVectorEnv(pool, 128, level_schedule=sched, slices=2, time_limit=5)
    assert env.struct.pool_next == sched.t["pool_next"].data_ptr()
    env.reset()
    a = torch.zeros(128, dtype=torch.int32, device=env.device)
    for call in (lambda: env.rollout(a[None]), lambda: env.step_async(a), lambda: env.step_slice(0, a),
                 lambda: env.step_queues(a), lambda: env.step_queues_many(a[None]), lambda: env.queues_open(),
                 lambda: env.set_step_outputs(a.data_ptr())):
        with pytest.raises(ValueError, match="level schedule"):
            call()
    env.step(a)                                          # the one way in still works
    with pytest.raises(ValueError, match="already serves"):
        SafeLifeVectorEnv(pool, 8, level_schedule=sched)
    other = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=8)[0]
    with pytest.raises(ValueError, match="another pool"):
        SafeLifeVectorEnv(other, 8, level_schedule=schedule.LevelSchedule(pool, [(0, 8)], mode="uniform", seed=1))
    assert np.array_equal(SafeLifeVectorEnv(pool, 8, first_level=3, level_schedule=schedule.LevelSchedule(
        pool, [(0, 8)], mode="uniform", seed=1)).numpy("level_idx"), np.full(8, 3))
