"""The fused multi-agent step on the device (csrc/sl_generic.hip: k_env_step_multi<EX>, k_env_reset_multi<EX>) from 1 to 8
agents, at the three block sizes of the generic kernel family and on agents that meet: against the reference's recorded
runs (tests/golden/multi_step_cases.npz), against the oracle in batches, and at one agent against the single-agent env.
Everything is compared bit for bit.  (The fixture's own checks and the oracle's half are tests/test_multi_step_host.py.)"""
import numpy as np
import pytest

from tests import multi_step_cases as msc
from tests import util
from tests.multi_wrap_ref import MultiWrapConfig, MultiWrapState, side_effect_count

pytestmark = pytest.mark.gpu

SCRIPTED, DENSE, EDGE = msc.names("scripted"), msc.names("dense"), msc.names("edge")
TRAIN15 = tuple(range(12)) + (25, 26, 27)
TRAIN = dict(movement_bonus=0.1, as_penalty=True, exit_bonus=0.5, penalty_coef=0.3)


def _device_counts(boards, goals):
    from safelife_amd.levels import _device_counts as f
    return f(boards, goals)


@pytest.mark.parametrize("name", SCRIPTED + DENSE + EDGE)
def test_device_replays_case(name):
    """SafeLifeMultiAgentVectorEnv at B = 1 against the reference: every recorded array of every step and reset, the
    actions as recorded (agents that are done keep getting non-zero ones)."""
    tr = msc.case(name)
    assert util.replay_trace_multi(tr, util.DeviceMultiBackend, _device_counts) == len(tr["trace_reward"])


def test_execute_actions_primitive_on_scripted_boards():
    """slhip_execute_actions on the scripted cases' boards right before the action, one batch per (shape, agents): the
    board and the locations the reference had right after execute_actions."""
    import torch
    from safelife_amd import speedups
    groups = {}
    for name in SCRIPTED:
        tr = msc.case(name)
        for t in range(len(tr["trace_reward"])):
            key = tr["trace_pre_board"][t].shape + (msc.agents_of(tr),)
            groups.setdefault(key, []).append((name, t, tr))
    assert len(groups) >= 6
    for key, items in sorted(groups.items()):
        boards = np.stack([tr["trace_pre_board"][t] for _, t, tr in items])
        locs = np.stack([tr["trace_pre_locs"][t] for _, t, tr in items]).astype(np.int64)
        acts = np.stack([tr["trace_actions"][t] for _, t, tr in items]).astype(np.int64)
        d_boards, d_locs = speedups._to_device(boards, np.uint16), speedups._to_device(locs, np.int64)
        speedups.execute_actions_batch(d_boards, d_locs, speedups._to_device(acts, np.int64))
        torch.cuda.synchronize()
        got_b, got_l = speedups._to_host(d_boards, np.uint16), speedups._to_host(d_locs, np.int64)
        for i, (name, t, tr) in enumerate(items):
            assert np.array_equal(got_b[i], tr["trace_act_board"][t]), (name, t)
            assert np.array_equal(got_l[i], tr["trace_act_locs"][t]), (name, t)


def _compare_state(dev, cpu, where):
    for name in util.MULTI_STATE:
        assert np.array_equal(dev.get(name), cpu.get(name)), (where, name)


def _run_batch(levels, A, B, steps, view, chans, time_limit, use_table, idle_nonzero, seed, masked_reset_at=None):
    """Device against oracle on `levels`, envs starting on different levels, random actions per env and agent."""
    import torch
    from safelife_amd.levels import LevelPool
    L = len(levels)
    pool_d = LevelPool(levels, counts_fn=_device_counts, n_agents=A, min_performance_fraction=0.5)
    pool_c = LevelPool(levels, counts_fn=util.oracle_counts, n_agents=A, min_performance_fraction=0.5)
    kw = dict(first_level=(np.arange(B) * 3 + 1) % L, auto_reset=True, level_stride=1 if use_table else 3,
              time_limit=time_limit, view_shape=view, output_channels=chans, episode_streams=True)
    dev = util.DeviceMultiBackend(pool_d, B, **kw)
    cpu = util.OracleMultiBackend(pool_c, B, **kw)
    if use_table:       # sl_env_batch.pool_next: a successor table instead of the stride rule
        table = ((np.arange(L) * 3 + 2) % L).astype(np.int32)
        d_table = torch.from_numpy(table).to(dev.env.device)
        dev.env.base.struct.pool_next = d_table.data_ptr()
        cpu.env.set_pool_next(table)
    assert np.array_equal(dev.reset(), cpu.reset())
    _compare_state(dev, cpu, "reset")
    rng = np.random.default_rng(seed)
    for t in range(steps):
        acts = rng.integers(0, 9, (B, A)).astype(np.int32)
        if not idle_nonzero:
            acts[cpu.get("is_active") == 0] = 0
        od, rd, dd = dev.step(acts)
        oc, rc, dc = cpu.step(acts)
        assert np.array_equal(rd, rc) and np.array_equal(dd, dc), t
        assert np.array_equal(od, oc), t
        _compare_state(dev, cpu, t)
        if masked_reset_at == t:
            mask = (np.arange(B) % 3 == 1).astype(np.uint8)
            assert 0 < mask.sum() < B
            dev.env.reset(mask)
            assert np.array_equal(dev.env.numpy("obs"), cpu.env.reset(mask)), "masked reset"
            _compare_state(dev, cpu, "masked reset")
    assert cpu.get("episode_idx").min() >= 2


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("k", range(len(DENSE + EDGE)))
def test_batch_vs_oracle(k, B):
    """Every random family's (agents, shape) -- 4 x 4 to 32 x 33: 64, 128 and 256 threads, HW = 256 / 272 / 1024 / 1025 /
    1056 -- at B = 1 and B = 65: every array of util.MULTI_STATE and the observation after every one of 40 steps, the
    per-episode random streams on.  The parametrisations alternate between the raw view and the 15-channel list, the
    stride rule and a pool_next table, and zeroed or non-zero actions for agents that are done; at B = 65 a masked
    reset(mask) half way (a mask of one env cannot be neither all ones nor all zeros)."""
    name = (DENSE + EDGE)[k]
    tr = msc.case(name)
    chans, view = (None, (5, 5)) if (k + B) % 2 else (TRAIN15, (7, 9))
    _run_batch(msc.levels_of(tr), msc.agents_of(tr), B, 40, view, chans, int(tr["env_time_limit"]),
               use_table=k % 3 == 0, idle_nonzero=(k // 2 + B) % 2 == 0, seed=100 + k,
               masked_reset_at=20 if B > 1 else None)


def test_top_of_the_range_128x128_eight_agents():
    """SL_MAX_CELLS with eight agents and a staged 25 x 25 x 15 observation: 131 072 + 128 bytes of board buffers, 128 of
    per-agent words and 9 376 of staging -- under the 160 KB of a workgroup, so the launch is accepted (an error status
    raises here)."""
    levels = msc.random_levels(128, 4, 8, 128, 128, clustered=True)
    _run_batch(levels, 8, 2, 6, (25, 25), TRAIN15, 2, use_table=False, idle_nonzero=True, seed=7)


EX_CASES = [n for n in DENSE if n.split("/")[1] in ("1x4x4", "3x5x5", "8x6x7")]


def _ex_pools(tr):
    from safelife_amd.levels import LevelPool
    levels, A = msc.levels_of(tr), msc.agents_of(tr)
    return (levels, A, LevelPool(levels, counts_fn=_device_counts, n_agents=A, min_performance_fraction=0.5),
            LevelPool(levels, counts_fn=util.oracle_counts, n_agents=A, min_performance_fraction=0.5))


@pytest.mark.parametrize("name", EX_CASES)
def test_wrapped_batch_vs_oracle_1_3_8_agents(name):
    """k_env_step_multi<true> under the training wrappers at 1, 3 and 8 agents, B = 33, reloads inside the step: every env
    array against the oracle and every agent's shaped reward against the restatement fed with the oracle's outputs, as
    test_multi_wrap.py::test_wrapped_batch_vs_oracle does at two agents; actions for done agents are not zeroed."""
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    levels, A, pool_d, pool_c = _ex_pools(msc.case(name))
    B = 33
    kw = dict(first_level=(np.arange(B) * 3) % len(levels), auto_reset=True, level_stride=3, time_limit=11,
              view_shape=(5, 5), output_channels=None)
    dev = SafeLifeMultiAgentVectorEnv(pool_d, B, wrappers=TRAIN, **kw)
    cpu = util.OracleMultiBackend(pool_c, B, **kw)
    dev.reset()
    assert np.array_equal(dev.numpy("obs"), cpu.reset())
    cfg = MultiWrapConfig(**TRAIN)
    states = [MultiWrapState(cfg, cpu.get("agent_locs")[e]) for e in range(B)]
    baseline = cpu.get("board").copy()
    rng = np.random.default_rng(60 + A)
    for t in range(40):
        acts = msc.steered_actions(rng, cpu.get("board"), cpu.get("agent_locs"), np.arange(B) % 2 == 0)
        dev.step(acts)
        oc, rc, dc = cpu.step(acts)
        assert np.array_equal(dev.numpy("reward"), rc) and np.array_equal(dev.numpy("done"), dc), t
        assert np.array_equal(dev.numpy("obs"), oc), t
        for key in util.MULTI_STATE:
            assert np.array_equal(dev.numpy(key), cpu.get(key)), (t, key)
        board, goals, exits = cpu.get("board"), cpu.get("goals"), cpu.get("exit_locs")
        locs, ep_r, times_up = cpu.get("agent_locs"), cpu.get("episode_reward"), cpu.get("times_up")
        shaped = dev.numpy("shaped_reward")
        for e in range(B):
            if dc[e].all():         # reloaded: the restatement restarts with the new episode
                states[e].reset(locs[e])
                baseline[e] = board[e]
                continue
            side = side_effect_count(board[e], baseline[e], goals[e], exits[e], cfg.ignore_reward_cells)
            want = states[e].step(rc[e], dc[e].astype(bool), bool(times_up[e, 0]), ep_r[e], locs[e], side)
            assert np.array_equal(shaped[e].view(np.uint32), want.view(np.uint32)), (t, e)
    assert cpu.get("episode_idx").min() >= 2


@pytest.mark.parametrize("name", EX_CASES)
def test_queue_end_to_end_1_3_8_agents(name):
    """The finished-episode queue of k_env_step_multi<true> at 1, 3 and 8 agents, B = 33: one entry per env episode, on the
    step where every agent is done and somebody was active -- record, finished_agents rows and the board as the agents
    left it against an oracle replay (auto_reset off: the terminal board stays), as
    test_multi_wrap.py::test_queue_end_to_end_multi does at two agents.  Half the envs are steered so that episodes end
    before the time limit.  Within one step the last agent to act on a victim survives it, so no episode's LAST active
    agent is ever killed: "ended by a kill" is an episode that ended before the time limit with an agent that is done
    without success in its rows -- the killed went first and the rest walked out."""
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    levels, A, pool_d, pool_c = _ex_pools(msc.case(name))
    B, T = 33, 14
    kw = dict(first_level=np.arange(B) % len(levels), auto_reset=False, time_limit=12, view_shape=(5, 5),
              output_channels=None)
    dev = SafeLifeMultiAgentVectorEnv(pool_d, B, wrappers=TRAIN, side_effects=dict(capacity=64, num_samples=4), **kw)
    cpu = util.OracleMultiBackend(pool_c, B, **kw)
    dev.reset()
    cpu.reset()
    rng = np.random.default_rng(80 + A)
    ended = {}
    for t in range(T):
        acts = msc.steered_actions(rng, cpu.get("board"), cpu.get("agent_locs"), np.arange(B) % 2 == 0)
        was_active = cpu.get("is_active").astype(bool).any(axis=1)
        dev.step(acts)
        _, rc, dc = cpu.step(acts)
        for e in np.nonzero(dc.astype(bool).all(axis=1) & was_active)[0]:
            assert int(e) not in ended
            ended[int(e)] = dict(reward=rc[e].copy(), done=dc[e].copy(), board=cpu.get("board")[e].copy(),
                                 num_steps=int(cpu.get("num_steps")[e]), success=cpu.get("success")[e].copy(),
                                 times_up=bool(cpu.get("times_up")[e, 0]), ep_r=cpu.get("episode_reward")[e].copy(),
                                 ep_l=cpu.get("episode_length")[e].copy())
    assert len(ended) == B
    batch = dev.side_effects_flush()
    recs, agents = batch.records(), batch.agent_records()
    assert len(batch) == B and batch.dropped() == 0
    assert sorted(recs["env"].tolist()) == list(range(B))
    boards = batch.boards.cpu().numpy().view(np.uint16)
    by_limit = early_with_dead = early_all_out = 0
    for i, e in enumerate(recs["env"]):
        want = ended[int(e)]
        assert recs["level"][i] == kw["first_level"][e] and recs["episode_idx"][i] == 0
        assert recs["num_steps"][i] == want["num_steps"]
        assert recs["episode_reward"][i] == want["ep_r"][0] and recs["episode_length"][i] == want["ep_l"][0]
        assert np.array_equal(agents["reward"][i], want["reward"])
        assert np.array_equal(agents["done"][i], want["done"])
        assert np.array_equal(agents["success"][i], want["success"])
        assert np.array_equal(agents["episode_reward"][i], want["ep_r"])
        assert np.array_equal(agents["episode_length"][i], want["ep_l"])
        assert np.array_equal(boards[i], want["board"])
        by_limit += want["times_up"]
        early_with_dead += (not want["times_up"]) and not want["success"].all()
        early_all_out += (not want["times_up"]) and bool(want["success"].all())
    assert by_limit > 0
    assert (early_with_dead > 0) if A > 1 else (early_all_out > 0)      # (one agent alone has nobody to kill it)
    dev.step(np.zeros((B, A), np.int32))    # nothing more is queued once every agent is done
    assert len(dev.side_effects_flush()) == 0


def _one_agent_vs_single(levels, view, chans, steps, time_limit, seed):
    from safelife_amd.levels import LevelPool
    pool = LevelPool(levels, counts_fn=_device_counts, min_performance_fraction=0.5)
    B = 19
    kw = dict(first_level=(np.arange(B) * 2) % len(levels), auto_reset=True, level_stride=3, time_limit=time_limit,
              view_shape=view, output_channels=chans)
    multi, single = util.DeviceMultiBackend(pool, B, **kw), util.DeviceBackend(pool, B, **kw)
    assert np.array_equal(multi.reset()[:, 0], single.reset())
    rng = np.random.default_rng(seed)
    for t in range(steps):
        acts = rng.integers(0, 9, B).astype(np.int32)
        om, rm, dm = multi.step(acts[:, None])
        o1, r1, d1 = single.step(acts)
        assert np.array_equal(rm[:, 0], r1) and np.array_equal(dm[:, 0], d1) and np.array_equal(om[:, 0], o1), t
        for key in ("board", "goals", "rng", "num_steps", "level_idx", "episode_idx"):
            assert np.array_equal(multi.get(key), single.get(key)), (t, key)
        assert np.array_equal(multi.get("agent_locs")[:, 0], single.get("agent_loc")), t
    assert single.get("episode_idx").min() >= 2


def test_one_agent_multi_env_equals_single_agent_env_5x7():
    """No row kernel serves 5 x 7: both envs go through the generic family."""
    _one_agent_vs_single(msc.random_levels(57, 8, 1, 5, 7), (5, 5), None, 40, 9, 1)


def test_one_agent_multi_env_equals_single_agent_env_25x25():
    """... and at 25 x 25 the multi-agent kernel against the row kernels, 15-channel observation."""
    pool, _ = util.pool_from_fixture("append_spawn_25", _device_counts, n=8)
    _one_agent_vs_single(pool.levels, (9, 9), TRAIN15, 30, 11, 2)
