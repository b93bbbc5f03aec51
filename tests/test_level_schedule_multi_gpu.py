"""
Level schedules for multi-agent envs on the device (csrc/sl_schedule.hip: k_schedule_required_multi,
k_schedule_harvest_multi; safelife_amd/schedule.py, multi_env.py): the two kernels against the host restatement of
tests/schedule_multi_ref.py, the reference's own multi-agent curriculum episodes through them, and a scheduled
SafeLifeMultiAgentVectorEnv against the plain one replaying the levels the schedule chose.
"""
import ctypes as C
import os

import numpy as np
import pytest

from safelife_amd import _hip, levels, schedule
from tests import schedule_multi_ref as smr
from tests import schedule_ref as sr
from tests import util
from tests.test_level_schedule_multi_host import CURRICULUM_MULTI_BOUND

pytestmark = pytest.mark.gpu

M64 = 2 ** 64 - 1
STATE = ("ring", "count", "episodes", "pos", "best", "mean", "cur_slot")


def _torch():
    import torch
    return torch


class DeviceScheduleMulti(object):
    """A struct sl_level_schedule_multi with its device arrays, fresh (ring[g][0] = 0.0, count = pos = 1)."""

    def __init__(self, groups, L, A, lookback=100, B=1, cur_slot=None, reward_possible=None, min_performance=None,
                 available=None, pool_agents=None):
        torch = _torch()
        dev = _hip.device()
        G = len(groups)
        t = self.t = {}
        t["min_performance"] = torch.from_numpy(np.zeros(L) if min_performance is None else np.asarray(min_performance, np.float64)).to(dev)
        t["available"] = torch.from_numpy(np.zeros((L, A), np.int32) if available is None
                                          else np.asarray(available, np.int32).reshape(L, A)).to(dev)
        t["reward_possible"] = torch.from_numpy(np.ones((L, A), np.int32) if reward_possible is None
                                                else np.asarray(reward_possible, np.int32).reshape(L, A)).to(dev)
        t["cur_slot"] = torch.from_numpy(np.zeros(B, np.int32) if cur_slot is None else np.asarray(cur_slot, np.int32)).to(dev)
        t["ring"] = torch.zeros((G, lookback), dtype=torch.float64, device=dev)
        t["count"] = torch.ones(G, dtype=torch.int64, device=dev)
        t["episodes"] = torch.zeros(G, dtype=torch.int64, device=dev)
        t["pos"] = torch.ones(G, dtype=torch.int32, device=dev)
        t["best"] = torch.zeros(G, dtype=torch.float64, device=dev)
        t["mean"] = torch.zeros(G, dtype=torch.float64, device=dev)
        t["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
        m = self.struct = _hip.LevelScheduleMulti()
        m.s.G, m.s.lookback, m.s.L, m.n_agents = G, lookback, L, A
        for g, (a, n) in enumerate(groups):
            m.s.start[g], m.s.len[g] = a, n
        for name in ("min_performance", "cur_slot", "ring", "count", "episodes", "pos", "best", "mean", "status"):
            setattr(m.s, name, t[name].data_ptr())
        m.available, m.reward_possible = t["available"].data_ptr(), t["reward_possible"].data_ptr()
        if pool_agents is not None:
            m.pool_agents = pool_agents.data_ptr()
        self.ref, self.sref = C.byref(m), C.byref(m.s)

    def host(self, name):
        return self.t[name].cpu().numpy()


def _ulp_neighbours(x):
    return [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]


@pytest.mark.parametrize("L,A", [(1, 1), (1, 8), (65, 3), (1000, 2)])
def test_required_points_bit_for_bit(L, A, golden_dir):
    """slhip_schedule_required_multi against the restatement on every (slot, agent), the other seven words of every record
    untouched and nothing written outside the table.  Fractions: the fixture's nine, and fractions that put
    mp * fraction * available on an integer for the pairs built for it (mp 0.5, 24 points: 0.75 -> 9 exactly; mp 0.3, 50
    points: 0.2 -> about 3) with one ulp to either side."""
    torch = _torch()
    lib, st, dev = _hip.lib(), _hip.current_stream_ptr(), _hip.device()
    with np.load(os.path.join(golden_dir, "schedule_multi_cases.npz")) as z:
        fractions = z["req_fraction"].tolist()
    fractions += _ulp_neighbours(0.75) + _ulp_neighbours(0.2)
    rng = np.random.default_rng(100 * L + A)
    mp = rng.choice([-1.0, 0.0, 0.5, 0.3, 1.0 / 3.0, 1.0, 0.001, 0.999], L)
    avail = rng.integers(-40, 200, (L, A)).astype(np.int32)
    special = [(0.5, 24), (0.3, 50), (-1.0, 30), (-1.0, -30), (1.0, 2 ** 31 - 1), (0.5, -2 ** 31), (1.0, 0), (0.5, 26)]
    if A == 8:                                          # one slot, every special value in an agent of its own
        mp[0] = 0.5
        avail[0] = [24, 26, 2 ** 31 - 1, -2 ** 31, 0, 50, -30, 25]
    else:
        for k, (m, a) in enumerate(special[:L]):
            mp[k], avail[k, k % A] = m, a
    PAD = 4
    records = rng.integers(-2 ** 31, 2 ** 31 - 1, (L + 2 * PAD, A, 8)).astype(np.int32)
    on_integer = 0
    for f in fractions:
        pa = torch.from_numpy(records).to(dev)
        d = DeviceScheduleMulti([(0, L)], L, A, min_performance=mp, available=avail, pool_agents=pa[PAD:])
        _hip.check(lib.slhip_schedule_required_multi(d.ref, float(f), st))
        got = pa.cpu().numpy()
        want = np.array([smr.required_points_multi(mp[l], f, avail[l]) for l in range(L)]).reshape(L, A)
        assert np.array_equal(got[PAD:PAD + L, :, 3], want), f
        keep = [0, 1, 2, 4, 5, 6, 7]
        assert np.array_equal(got[PAD:PAD + L][:, :, keep], records[PAD:PAD + L][:, :, keep]), f
        assert np.array_equal(got[:PAD], records[:PAD]) and np.array_equal(got[PAD + L:], records[PAD + L:]), f
        v = (mp[:, None] * f) * avail.astype(np.float64)
        on_integer += int(((v == np.round(v)) & (v > 0)).sum())
    assert on_integer > 0


def _out_records(reward, done, episode_reward):
    """struct sl_step_out rows as int32 [B, A, 4]."""
    B, A = done.shape
    rec = np.zeros((B, A, 4), np.int32)
    rec[:, :, 0] = np.asarray(reward, np.float32).view(np.int32)
    flags = np.zeros((B, A, 4), np.uint8)
    flags[:, :, 0] = done
    rec[:, :, 1] = flags.view(np.int32)[:, :, 0]
    rec[:, :, 2] = np.asarray(episode_reward, np.float32).view(np.int32)
    rec[:, :, 3] = 1
    return rec


def _assert_state(d, m, where):
    for name in STATE:
        got, want = d.host(name), getattr(m, name)
        if got.dtype.kind == "f":       # bit for bit
            assert np.array_equal(got.view(np.int64), np.asarray(want, np.float64).view(np.int64)), (where, name, got, want)
        else:
            assert np.array_equal(got, want), (where, name, got, want)


@pytest.mark.parametrize("B,A", [(1, 1), (1, 8), (63, 2), (64, 3), (65, 8), (1025, 2), (16449, 2)])   # (past the 16384 tile)
def test_harvest_and_curriculum_equal_the_model(B, A):
    """Scripted [B, A] step records: rings and counters bit for bit after every step, the curriculum's probabilities within
    the measured bound.  Agents finish on their own steps and stay done (their episode reward carried) until the env's
    last agent is done; steps with every env finished (more records per group than the ring holds: lookback 4), with none,
    and random ones; slots outside every group and (slot, agent) pairs whose reward_possible is 0.  A second schedule gets
    the same steps with the records of the envs that have NOT finished poisoned -- NaN rewards, other done bytes that
    still leave an agent out -- and must end every step in the same state."""
    torch = _torch()
    lib, st, dev = _hip.lib(), _hip.current_stream_ptr(), _hip.device()
    rng = np.random.default_rng(100 * B + A)
    L, lookback = 40, 4
    groups = [(2, 10), (13, 1), (20, 15)]                          # 0, 1, 12, 14..19, 35..39 in no group
    possible = rng.integers(5, 60, (L, A)).astype(np.int32)
    possible[4, 0] = possible[25, A - 1] = 0
    def slots():                                                    # (one in five on the group of a single slot)
        return np.where(rng.random(B) < 0.2, 13, rng.integers(0, L, B)).astype(np.int32)
    cur = slots()
    runs = [DeviceScheduleMulti(groups, L, A, lookback=lookback, B=B, cur_slot=cur, reward_possible=possible) for _ in range(2)]
    m = smr.ScheduleModelMulti(groups, lookback, possible, cur)
    probs = [torch.zeros(3, dtype=torch.float64, device=dev) for _ in range(2)]
    patterns = ["none", "random", "all", "random", "random", "all", "none", "random", "one", "random", "all", "random"]
    gone = np.zeros((B, A), bool)                                   # agents done since an earlier step
    carried = np.zeros((B, A), np.float32)
    level_now = cur.copy()
    worst, partial_seen, staggered = 0.0, 0, 0
    for t, pattern in enumerate(patterns):
        fresh = {"none": np.zeros((B, A), bool), "all": np.ones((B, A), bool), "random": rng.random((B, A)) < 0.35,
                 "one": np.repeat(np.arange(B) == B - 1, A).reshape(B, A)}[pattern]
        done = gone | fresh
        ep = np.round(rng.normal(10.0 + 2.0 * t, 8.0, (B, A))).astype(np.float32)
        ep[rng.random((B, A)) < 0.1] = 0.0
        ep = np.where(gone, carried, ep)
        finished = done.all(axis=1)
        staggered += int((finished & gone.any(axis=1)).sum())
        partial_seen += int((done.any(axis=1) & ~finished).sum())
        level_idx = np.where(finished, slots(), level_now).astype(np.int32)     # only a finished env moves on
        scal = np.zeros((B, 16), np.int32)
        scal[:, _hip.SCALAR_COLS["level_idx"]] = level_idx
        scalars = torch.from_numpy(scal).to(dev)
        reward = rng.normal(0, 1, (B, A))
        rec = _out_records(reward, done, ep)
        bad_done = np.full((B, A), 255, np.uint8)
        bad_done[np.arange(B), (np.arange(B) + t) % A] = 0             # another agent is the one that is missing
        poisoned = _out_records(np.full((B, A), np.nan), np.where(finished[:, None], done, bad_done),
                                np.where(finished[:, None], ep, np.float32(np.nan)))
        for d, p, records in zip(runs, probs, (rec, poisoned)):
            out = torch.from_numpy(records).to(dev)
            d.struct.out = out.data_ptr()
            _hip.check(lib.slhip_schedule_harvest_multi(d.ref, _hip.ptr(scalars), B, st))
            _hip.check(lib.slhip_schedule_curriculum(d.sref, _hip.ptr(p), st))
            torch.cuda.synchronize()
        m.harvest(done.astype(np.uint8), ep, level_idx)
        for d in runs:
            _assert_state(d, m, (t, pattern))
        got = probs[0].cpu().numpy()
        assert np.array_equal(got.view(np.int64), probs[1].cpu().numpy().view(np.int64)), (t, pattern)
        diff = np.abs(got - m.curriculum()).max()
        worst = max(worst, diff)
        assert diff <= CURRICULUM_MULTI_BOUND, (t, pattern, diff)
        gone = np.where(finished[:, None], False, done)
        carried = np.where(gone, ep, 0.0).astype(np.float32)
        level_now = level_idx
    print("B=%d A=%d: largest |device - model| of the probabilities %r" % (B, A, worst))
    if B >= 63:
        assert (m.count > 2 * lookback).all()
        if A > 1:
            assert partial_seen > 0 and staggered > 0


@pytest.mark.parametrize("case", [0, 1, 2, 3, 4, 5])
def test_golden_episodes_one_per_step(case, golden_dir):
    """The golden multi-agent curricula (the reference's CurricularLevelIterator fed scripted episodes of 2, 3 and 8
    agents) through the two kernels, one episode per harvest: the performance filed is the reference's bit for bit, every
    logged probability within the measured bound, best_perf_lvl* exact."""
    torch = _torch()
    lib, st, dev = _hip.lib(), _hip.current_stream_ptr(), _hip.device()
    with np.load(os.path.join(golden_dir, "schedule_multi_cases.npz")) as z:
        g = {k: z[k] for k in z.files}
    A, G, lookback = int(g["cur_agents"][case]), int(g["cur_groups"][case]), int(g["cur_lookback"][case])
    lo, hi = int(g["cur_offsets"][case]), int(g["cur_offsets"][case + 1])
    N = hi - lo
    # one slot per episode, the slots of a group side by side: slot -> that episode's reward_possible
    group = g["cur_group"][lo:hi]
    order = np.argsort(group, kind="stable")
    slot = np.zeros(N, np.int64)
    slot[order] = np.arange(N)
    sizes = np.bincount(group, minlength=G)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    possible = np.ones((N, A), np.int32)
    possible[slot] = g["cur_possible"][lo:hi, :A]
    d = DeviceScheduleMulti([(int(starts[k]), int(sizes[k])) for k in range(G)], N, A, lookback=lookback, B=1,
                            cur_slot=slot[:1], reward_possible=possible)
    out = torch.from_numpy(_out_records(np.zeros((N, A)), np.ones((N, A), np.uint8), g["cur_reward"][lo:hi, :A])).to(dev)
    scal = np.zeros((N, 16), np.int32)
    scal[:-1, _hip.SCALAR_COLS["level_idx"]] = slot[1:]                 # after episode e the env stands on episode e+1's slot
    scalars = torch.from_numpy(scal).to(dev)
    probs = torch.zeros((N, 8), dtype=torch.float64, device=dev)
    best = torch.zeros((N, G), dtype=torch.float64, device=dev)
    filed = torch.zeros(N, dtype=torch.float64, device=dev)
    ring = d.t["ring"].view(-1)
    where = torch.from_numpy(group.astype(np.int64) * lookback).to(dev)
    for e in range(N):
        d.struct.out = out.data_ptr() + 16 * A * e
        at = (where[e] + d.t["pos"][int(group[e])]).clone()             # where this episode's record goes
        _hip.check(lib.slhip_schedule_harvest_multi(d.ref, scalars.data_ptr() + 64 * e, 1, st))
        _hip.check(lib.slhip_schedule_curriculum(d.sref, probs.data_ptr() + 64 * e, st))
        best[e].copy_(d.t["best"])
        filed[e] = ring[at]
    assert np.array_equal(filed.cpu().numpy().view(np.int64), g["cur_perf"][lo:hi].view(np.int64))
    got = probs.cpu().numpy()
    diff = np.abs(got[:, :G] - g["cur_probs"][lo:hi, :G]).max()
    print("case %d (A=%d, G=%d, lookback=%d, %d episodes): largest |device - reference| %r" % (case, A, G, lookback, N, diff))
    assert diff <= CURRICULUM_MULTI_BOUND, diff
    assert np.array_equal(best.cpu().numpy(), g["cur_best"][lo:hi, :G])
    assert (d.host("count") > lookback).all() and d.host("episodes").sum() == N


# ----------------------------------------------------------------------------------------------------------- end to end

TRAIN = dict(movement_bonus=0.1, movement_bonus_power=1e-100, movement_bonus_period=4, as_penalty=True, exit_bonus=0.5,
             penalty_coef=0.3, ignore_reward_cells=False)
B_E2E, A_E2E, T_E2E, OFFSET = 21, 2, 50, 64
FRACTION = schedule.LinearSchedule([10, 40], [0.0, 1.0])           # 0 at the start: the exits are open, agents leave early


def _families():
    return [util.levels_from_trace(util.load_trace(name)) for name in ("multi_asym1", "multi_build_coop", "multi_build_compete")]


def _counts(boards, goals):
    from safelife_amd.levels import _device_counts
    return _device_counts(boards, goals)


def _env(pool, wrapped, **kw):
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    if wrapped:
        kw["wrappers"] = TRAIN
    return SafeLifeMultiAgentVectorEnv(pool, B_E2E, auto_reset=True, time_limit=9, view_shape=(7, 11),
                                       output_channels=tuple(range(12)) + (25, 26, 27), policy_layout="uint8",
                                       with_obs=False, env_offset=OFFSET, **kw)


def _schedule(mode, **kw):
    return schedule.LevelSchedule.from_pools(_families(), pool_args=dict(counts_fn=_counts, n_agents=A_E2E), mode=mode,
                                             seed=21, min_performance_fraction=FRACTION, **kw)


def _actions(env, policy, rng):
    """Fixed pseudo-random actions, except that two agents in three take the policy's favourite -- towards an exit they
    see -- so that agents do leave before the time limit, one of an env ahead of the other."""
    torch = _torch()
    o = env.policy_tensor
    fav = policy(o.view((-1,) + tuple(o.shape[2:])))[1].argmax(dim=1).view(B_E2E, A_E2E).to(torch.int32)
    rnd = torch.from_numpy(rng.integers(0, 9, (B_E2E, A_E2E)).astype(np.int32)).to(env.device)
    use = torch.from_numpy(rng.random((B_E2E, A_E2E)) < 0.67).to(env.device)
    return torch.where(use, fav, rnd)


def _snapshot(env, wrapped):
    rec = dict(reward=env.numpy("reward").copy(), done=env.numpy("done").copy(), board=env.numpy("board").copy(),
               policy=env.policy_tensor.cpu().numpy().copy(), level_idx=env.numpy("level_idx").copy(),
               required=env.numpy("required_points").copy())
    if wrapped:
        rec["shaped"] = env.shaped_reward.cpu().numpy().copy()
    for k in env.info:
        rec[k] = env.info[k].cpu().numpy().copy()
    return rec


def _run_scheduled(sched, wrapped, check):
    from tests.test_training_batch_multi_gpu import ExactPolicy
    torch = _torch()
    env = _env(sched.pool, wrapped, level_schedule=sched)
    assert env.level_schedule is sched and env.base.struct.pool_next == sched.t["pool_next"].data_ptr()
    policy = ExactPolicy(torch, tuple(env.policy_tensor.shape[2:]), env.device)
    rng = np.random.default_rng(17)
    sched.training_steps = 0
    env.reset()
    first = dict(board=env.numpy("board").copy(), policy=env.policy_tensor.cpu().numpy().copy(),
                 level_idx=env.numpy("level_idx").copy(), required=env.numpy("required_points").copy())
    loaded = [[(int(s), sched.fraction())] for s in first["level_idx"]]
    actions, steps = [], []
    for t in range(T_E2E):
        sched.training_steps = t
        a = _actions(env, policy, rng)
        before = env.numpy("level_idx").copy()
        env.step(a)
        rec = _snapshot(env, wrapped)
        rec["before"] = before
        actions.append(a.cpu().numpy().copy()), steps.append(rec)
        for e in np.flatnonzero(rec["done"].all(axis=1)):
            loaded[e].append((int(rec["level_idx"][e]), sched.fraction()))
        check(t, env, rec)
    return env, first, actions, steps, loaded


def _required_of(sched, slot, fraction):
    return smr.required_points_multi(sched.min_performance[slot], fraction, sched.available[slot])


def _replay_on_a_plain_env(sched, wrapped, first, actions, steps, loaded):
    """A plain multi-agent pool whose levels are each env's sequence laid end to end -- the same rng words, every agent's
    required_step of the fraction in force when the env loaded the level -- and a plain env walking it with level_stride 1
    must give what the scheduled env gave, at every step."""
    pool = sched.pool
    lv, frac, start, at = [], [], [], 0
    for seq in loaded:
        start.append(at)
        for slot, f in seq:
            src = pool.levels[slot]
            lv.append(levels.Level(src.board, src.goals, src.agent_locs, src.spawn_prob, src.min_performance, src.points_table,
                                   rng_words=pool.pool_rng[slot]))
            frac.append((slot, f))
        at += len(seq)
    flat = levels.LevelPool(lv, counts_fn=_counts, n_agents=A_E2E, exit_slots=pool.exit_slots)
    for k, (slot, f) in enumerate(frac):
        flat.pool_agent_required_step[k] = _required_of(sched, slot, f)
    assert np.array_equal(flat.pool_agent_required_reset, pool.pool_agent_required_reset[[s for s, _ in frac]])
    env = _env(flat, wrapped, first_level=np.array(start), level_stride=1)
    assert env.level_schedule is None and not env.base.struct.pool_next
    env.reset()
    assert np.array_equal(env.numpy("board"), first["board"]) and np.array_equal(env.policy_tensor.cpu().numpy(), first["policy"])
    assert np.array_equal(env.numpy("required_points"), first["required"])
    for t in range(len(actions)):
        env.step(actions[t])
        got, want = _snapshot(env, wrapped), steps[t]
        for k in got:
            if k == "level_idx":
                continue
            a, b = got[k], want[k]
            if a.dtype.kind == "f":
                a, b = a.view(np.int32 if a.dtype == np.float32 else np.int64), b.view(np.int32 if b.dtype == np.float32 else np.int64)
            assert np.array_equal(a, b), (t, k)


@pytest.mark.parametrize("wrapped", [False, True], ids=["game reward", "wrapped reward"])
@pytest.mark.parametrize("mode", ["uniform", "curriculum"])
def test_scheduled_run_equals_a_plain_env_on_the_chosen_levels(mode, wrapped):
    """21 envs of 2 agents, time_limit 9, three level families as three groups, the exit-difficulty fraction 0 for ten steps
    and then rising to 1.  At every step: the successor table is the model's draw from the probabilities in force (equal
    ones, or the curriculum's from the model fed the run's own all-done steps), an env moves exactly when all its agents
    are done, the rings and counters are the model's bit for bit, and every reloaded agent's required points are the
    restatement's at the fraction in force.  Then the whole run equals a plain env on the chosen levels."""
    sched = _schedule(mode, **(dict(lookback=5) if mode == "curriculum" else {}))
    L = len(sched.pool)
    seed = (21 + sr.G64 * OFFSET) & M64
    state = dict(model=None, early=0, exits=0, worst=0.0, all_done=0)

    def check(t, env, rec):
        if state["model"] is None:
            assert np.array_equal(sched.reward_possible(1), sched.available + 1)
            state["model"] = smr.ScheduleModelMulti(sched.groups, sched.lookback, sched.reward_possible(1), rec["before"])
        m = state["model"]
        if mode == "curriculum":
            want_p = m.curriculum()
            got_p = sched.stats()["probabilities"]
            state["worst"] = max(state["worst"], np.abs(got_p - want_p).max())
            assert np.abs(got_p - want_p).max() <= CURRICULUM_MULTI_BOUND, t
        else:
            want_p = [1.0 / 3] * 3
        table = sr.draw(sched.groups, want_p, seed, t + 1, L)            # (the reset took draw 0)
        assert np.array_equal(sched.t["pool_next"].cpu().numpy(), table), t
        fin = rec["done"].all(axis=1)
        assert np.array_equal(rec["level_idx"][fin], table[rec["before"][fin]]), t
        assert np.array_equal(rec["level_idx"][~fin], rec["before"][~fin]), t
        f = sched.fraction()
        for e in np.flatnonzero(fin):                                    # a reload takes the fraction in force
            assert np.array_equal(rec["required"][e], _required_of(sched, rec["level_idx"][e], f)), (t, e)
        assert np.array_equal(env.t["pool_agents"].cpu().numpy()[:, :, 3],
                              [_required_of(sched, l, f) for l in range(L)]), t
        m.harvest(rec["done"], rec["episode_reward"], rec["level_idx"])
        for name in STATE:
            got = sched.t[name].cpu().numpy()
            want = getattr(m, name)
            if got.dtype.kind == "f":
                got, want = got.view(np.int64), np.asarray(want, np.float64).view(np.int64)
            assert np.array_equal(got, want), (t, name)
        some = rec["done"].any(axis=1) & ~fin
        state["early"] += int(some.sum())
        state["exits"] += int(((rec["success"] != 0) & (rec["times_up"] == 0) & (rec["done"] != 0)).sum())
        state["all_done"] += int(fin.sum())

    env, first, actions, steps, loaded = _run_scheduled(sched, wrapped, check)
    sched.training_steps = 0
    assert np.array_equal(first["level_idx"], sched.first_levels(B_E2E, OFFSET))
    for e in range(B_E2E):
        assert np.array_equal(first["required"][e], _required_of(sched, first["level_idx"][e], 0.0))
    # what the run is here for
    assert state["early"] > 0 and state["exits"] > 0                     # one agent away while its env goes on; real exits
    assert len({f for seq in loaded for _, f in seq}) > 3                # the fraction moved within the run
    st = sched.stats()
    assert st["episodes"].sum() == state["all_done"] == sum(len(seq) for seq in loaded) - B_E2E and st["status"] == 0
    assert state["all_done"] >= 4 * B_E2E
    if mode == "curriculum":
        assert (st["records"] > 5).all()                                 # every ring filled: the slopes counted
        print("largest |device - model| of the probabilities over the run: %r" % state["worst"])
    _replay_on_a_plain_env(sched, wrapped, first, actions, steps, loaded)


def test_without_a_schedule_nothing_changes():
    pool = levels.LevelPool([lv for fam in _families() for lv in fam], counts_fn=_counts, n_agents=A_E2E,
                            min_performance_fraction=0.0)
    rng = np.random.default_rng(5)
    one, two = _env(pool, True, level_schedule=None), _env(pool, True)
    assert one.level_schedule is None and not one.base.struct.pool_next and not two.base.struct.pool_next
    one.reset(), two.reset()
    assert np.array_equal(one.policy_tensor.cpu().numpy(), two.policy_tensor.cpu().numpy())
    for t in range(25):
        a = rng.integers(0, 9, (B_E2E, A_E2E)).astype(np.int32)
        one.step(a), two.step(a)
        for name in ("reward", "done", "board", "level_idx", "success", "rng", "required_points", "shaped_reward"):
            assert np.array_equal(one.numpy(name), two.numpy(name), equal_nan=True), (t, name)
        assert np.array_equal(one.policy_tensor.cpu().numpy(), two.policy_tensor.cpu().numpy())
    assert not one.base.struct.pool_next


def test_one_agent_pool_in_the_multi_env_and_reset_with_a_mask():
    """A = 1: a single-agent pool's schedule serves the multi-agent env class (pool_agents[:, 0]); reset(mask) draws first and
    rewinds the masked envs' slots; what cannot drive a schedule still says so through the base env."""
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    torch = _torch()
    pool = util.pool_from_fixture("prune_still_25", util.oracle_counts, n=12)[0]
    sched = schedule.LevelSchedule(pool, [(0, 6), (6, 6)], mode="uniform", seed=4, min_performance_fraction=0.5)
    env = SafeLifeMultiAgentVectorEnv(pool, 70, time_limit=5, level_schedule=sched, with_obs=False)
    env.reset()
    want = [sr.required_points(sched.min_performance[l], 0.5, sched.available[l]) for l in range(12)]
    assert np.array_equal(env.t["pool_agents"].cpu().numpy()[:, 0, 3], want)
    m = smr.ScheduleModelMulti(sched.groups, sched.lookback, sched.reward_possible(1)[:, None], env.numpy("level_idx"))
    rng = np.random.default_rng(2)
    for t in range(12):
        env.step(rng.integers(0, 9, (70, 1)).astype(np.int32))
        m.harvest(env.numpy("done"), env.info["episode_reward"].cpu().numpy(), env.numpy("level_idx"))
        if t == 6:
            mask = (np.arange(70) % 3 == 0).astype(np.uint8)
            before = env.numpy("level_idx").copy()
            env.reset(mask)
            table = sched.t["pool_next"].cpu().numpy()
            now = env.numpy("level_idx")
            assert np.array_equal(now[mask != 0], table[before[mask != 0]]) and np.array_equal(now[mask == 0], before[mask == 0])
            m.cur_slot[:] = now
        for name in STATE:
            assert np.array_equal(sched.t[name].cpu().numpy(), getattr(m, name)), (t, name)
    assert sched.stats()["episodes"].sum() >= 100
    a = torch.zeros(70, dtype=torch.int32, device=env.device)
    for call in (lambda: env.base.rollout(a[None]), lambda: env.base.step_async(a)):
        with pytest.raises(ValueError, match="level schedule"):
            call()
    with pytest.raises(ValueError, match="already serves"):
        SafeLifeMultiAgentVectorEnv(pool, 8, level_schedule=sched)


def test_runners_advance_the_training_step():
    """MultiAgentRunner.gen_training_batch for two windows on a scheduled env: every env step sees training_steps =
    num_steps as it stood before the step, and the schedule harvested exactly the all-done steps.  MultiAgentDQNRunner
    hands its num_steps on in the same way."""
    from safelife_amd.runner import MultiAgentDQNRunner, MultiAgentRunner
    from tests.test_training_batch_multi_gpu import ExactPolicy
    torch = _torch()
    T = 12
    sched = _schedule("curriculum", lookback=5)
    env = _env(sched.pool, True, level_schedule=sched)
    policy = ExactPolicy(torch, tuple(env.policy_tensor.shape[2:]), env.device)
    runner = MultiAgentRunner(env, policy, seed=3)
    seen, all_done, env_step = [], [], env.step

    def logging_step(actions):
        seen.append(sched.training_steps)
        out = env_step(actions)
        all_done.append(int(env.done.to(torch.bool).all(dim=1).sum().item()))
        return out

    env.step = logging_step
    for window in range(2):
        batch = runner.gen_training_batch(T)
        assert len(batch.actions) > 0
        assert runner.num_steps == (window + 1) * T * B_E2E
    assert seen == [k * B_E2E for k in range(2 * T)]
    st = sched.stats()
    assert st["episodes"].sum() == sum(all_done) > 0 and st["status"] == 0
    assert np.array_equal(runner.num_resets.cpu().numpy().sum(), sum(all_done))

    sched2 = _schedule("uniform")
    env2 = _env(sched2.pool, False, level_schedule=sched2)
    dqn = MultiAgentDQNRunner(env2, lambda o: policy(o)[1], seed=3)
    dqn.num_steps = 4321
    dqn.take_one_step(0.1)
    assert sched2.training_steps == 4321 and sched2.draws == 2           # (the reset's draw and the step's)
