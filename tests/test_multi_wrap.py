"""Multi-agent envs under the training wrappers, with the finished-episode queue and the policy layout
(SafeLifeMultiAgentVectorEnv(wrappers=, side_effects=, policy_layout=); slhip_env_step_multi_ex / _reset_multi_ex).

CPU: the numpy restatement (tests/multi_wrap_ref.py) against the reference's recorded shaped rewards, and the ctypes
mirror of struct sl_multi_extras against gcc.  GPU: the device against the reference's traces, the oracle and the
restatement."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

from safelife_amd import _hip
from tests import util
from tests.multi_wrap_ref import MultiWrapConfig, MultiWrapState, exit_cells_of, replay_shaped, side_effect_count

REPO = util.REPO
WRAP_TRACES = sorted(os.path.basename(p)[len("trace_"):-4]
                     for p in glob.glob(os.path.join(util.GOLDEN, "trace_multi_wrap_*.npz")))
TRAIN = dict(movement_bonus=0.1, as_penalty=True, exit_bonus=0.5, penalty_coef=0.3)


def test_wrap_traces_present():
    assert len(WRAP_TRACES) >= 6
    for name in WRAP_TRACES:
        assert os.path.getsize(os.path.join(util.GOLDEN, "trace_%s.npz" % name)) < 100 * 1024


@pytest.mark.parametrize("name", WRAP_TRACES)
def test_restatement_reproduces_reference_shaped_rewards(name):
    """Every shaped reward of every agent and step, bit for bit, from the trace's unwrapped outputs, boards, locations
    and the wrapper's recorded baseline board; the side-effect count equals the wrapper's last_side_effect."""
    tr = util.load_trace(name)
    shaped, counts = replay_shaped(tr)
    assert shaped.dtype == np.float32
    assert np.array_equal(shaped.view(np.uint32), tr["trace_shaped_reward"].view(np.uint32))
    if "trace_last_side_effect" in tr:
        assert np.array_equal(counts, tr["trace_last_side_effect"])


def test_hand_exit_figures():
    """The hand-made exit level: agent 0 leaves at step 2 and keeps being shaped (exit bonus, movement penalty)."""
    tr = util.load_trace("multi_wrap_hand_exit")
    want = np.array([[-0.5, -0.51339746], [1.5, -0.02928932], [-0.01339746, -0.5292893], [0.7207107, 0.22071068]],
                    np.float32)
    assert np.allclose(tr["trace_shaped_reward"][:4], want, rtol=0, atol=1e-7)     # (the figures are printed to 8 digits)
    assert np.array_equal(tr["trace_shaped_reward"][7], np.float32([-0.1, -0.1]))
    assert tr["trace_times_up"][7]


def test_restatement_float32_rounding_per_wrapper():
    """Each wrapper rounds to float32 (a float64 accumulation would differ here)."""
    st = MultiWrapState(MultiWrapConfig(movement_bonus=0.1, movement_bonus_power=0.5, exit_bonus=0.5, penalty_coef=0.25),
                        [[0, 0], [3, 3]])
    r = st.step(np.float32([0.0, 0.0]), [False, False], False, np.float32([0.0, 0.0]), [[0, 1], [3, 3]], 1)
    r64 = 0.1 * (3 / 4) ** 0.5 - 0.1 - 0.25
    assert r.dtype == np.float32 and r[1] == np.float32(np.float32(np.float32(0.1 * (3 / 4) ** 0.5) - np.float32(0.1))
                                                        - 0.25)
    assert abs(float(r[1]) - r64) < 1e-6


def test_side_effect_count_ignores_player_bits_and_exits():
    b0 = np.zeros((4, 4), np.uint16)
    b0[1, 1] = 2 | 8 | 16 | (1 << 9)            # a red agent
    b0[3, 3] = 16 | 256                         # an exit
    b = b0.copy()
    b[3, 3] |= 1 << 9                           # the exit turned red: not counted
    assert side_effect_count(b, b0, np.zeros_like(b), [15], False) == 0
    b[1, 1], b[1, 2] = 0, b0[1, 1]              # the coloured agent moved: both cells count
    assert side_effect_count(b, b0, np.zeros_like(b), [15], False) == 2
    assert list(exit_cells_of(b0)) == [15]


def test_multi_extras_layout_matches_header(tmp_path):
    """ctypes mirror of struct sl_multi_extras against gcc's offsetof / sizeof."""
    st = _hip.MultiExtras
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "safelife_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(sl_multi_extras));']
    want = ["size %d" % C.sizeof(st)]
    for name, ctype in st._fields_:
        lines.append('printf("%s %%zu %%zu\\n", offsetof(sl_multi_extras, %s), sizeof(((sl_multi_extras *)0)->%s));'
                     % (name, name, name))
        want.append("%s %d %d" % (name, getattr(st, name).offset, C.sizeof(ctype)))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", exe])
    got = [g for g in subprocess.check_output([exe]).decode().split("\n") if g]
    assert got == want
    assert "slhip_env_step_multi_ex" in _hip.EXPORTS and "slhip_env_reset_multi_ex" in _hip.EXPORTS


# ---------------------------------------------------------------------------------------------------------------- GPU

def _device_counts(boards, goals):
    from safelife_amd.levels import _device_counts as f
    return f(boards, goals)


def _trace_pool(tr, counts_fn):
    from safelife_amd.levels import LevelPool
    levels = util.levels_from_trace(tr)
    frac = float(tr["min_performance_fraction"]) if "min_performance_fraction" in tr else 1.0
    return LevelPool(levels, counts_fn=counts_fn, n_agents=len(levels[0].agent_locs), min_performance_fraction=frac)


@pytest.mark.gpu
@pytest.mark.parametrize("name", WRAP_TRACES)
def test_device_replays_wrapped_trace(name):
    """slhip_env_step_multi_ex against the reference: the shaped reward of every agent and step (float32, bit for bit),
    the unwrapped outputs, boards and generators; the inaction traces' baselines seeded with the recorded words."""
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    tr = util.load_trace(name)
    env = SafeLifeMultiAgentVectorEnv(_trace_pool(tr, _device_counts), 1, first_level=0, auto_reset=True, level_stride=1,
                                      episode_streams=False, wrappers=util.wrappers_from_trace(tr),
                                      **util.env_kwargs_from_trace(tr))
    env.reset()
    assert np.array_equal(env.numpy("obs")[0], tr["trace_reset_obs"][0])
    assert np.array_equal(env.numpy("board")[0], tr["trace_reset_board"][0])
    if "trace_baseline_board" in tr and "wrap_inaction_rng" not in tr:
        assert np.array_equal(env.numpy("baseline")[0], tr["trace_reset_board"][0])
    episode, n_resets = 0, len(tr["trace_reset_at"])
    for t in range(len(tr["trace_reward"])):
        env.step(tr["trace_actions"][t][None].astype(np.int32))
        where = "step %d" % t
        assert np.array_equal(env.numpy("shaped_reward")[0].view(np.uint32),
                              tr["trace_shaped_reward"][t].view(np.uint32)), where
        assert np.array_equal(env.numpy("reward")[0], tr["trace_reward"][t]), where
        assert np.array_equal(env.numpy("done")[0].astype(bool), tr["trace_done"][t]), where
        assert np.array_equal(env.numpy("success")[0].astype(bool), tr["trace_success"][t]), where
        if "trace_last_side_effect" in tr and not np.all(tr["trace_done"][t]):     # (a reload resets the wrappers)
            assert np.all(env.numpy("wrap_state")[0, :, 1] == tr["trace_last_side_effect"][t]), where
        if "trace_inaction_rng_after" in tr:
            assert np.array_equal(env.numpy("inaction_rng")[0], tr["trace_inaction_rng_after"][t]), where
            if not np.all(tr["trace_done"][t]):
                assert np.array_equal(env.numpy("inaction_board")[0], tr["trace_baseline_board"][t]), where
        if np.all(tr["trace_done"][t]):
            episode += 1
            if episode >= n_resets:
                break
            assert np.array_equal(env.numpy("board")[0], tr["trace_reset_board"][episode]), where
            assert np.array_equal(env.numpy("obs")[0], tr["trace_reset_obs"][episode]), where
        else:
            assert np.array_equal(env.numpy("board")[0], tr["trace_board"][t]), where
            assert np.array_equal(env.numpy("agent_locs")[0], tr["trace_agent_locs"][t]), where
            assert np.array_equal(env.numpy("rng")[0], tr["trace_rng_after"][t]), where
            assert np.array_equal(env.numpy("obs")[0], tr["trace_obs"][t]), where
            assert np.array_equal(env.numpy("episode_reward")[0], tr["trace_ep_reward"][t]), where


def _spec_levels():
    levels = []
    for name in ("multi_asym1", "multi_build_coop", "multi_build_compete"):
        levels += util.levels_from_trace(util.load_trace(name))
    return levels


WRAP_COMBOS = [
    TRAIN,
    dict(movement_bonus=0.25, movement_bonus_power=0.5, movement_bonus_period=3, as_penalty=False, exit_bonus=1.5,
         penalty_coef=0.125, ignore_reward_cells=True),
    dict(movement_bonus=0.1, movement_bonus_period=8, movement_bonus_power=1.0),
    dict(exit_bonus=0.5),
]


@pytest.mark.gpu
@pytest.mark.parametrize("combo", range(len(WRAP_COMBOS)))
def test_wrapped_batch_vs_oracle(combo):
    """~96 two-agent envs on the three 26x26 multi-agent specs, 60 steps with reloads inside the step: every env array
    against the oracle (which knows no wrappers: they change nothing but the shaped reward), and the shaped reward
    against the restatement fed with the oracle's outputs.  (On a step that reloads an env the terminal board is gone
    from both sides, so the restatement checks that env's side-effect term from the next episode on.)"""
    from safelife_amd.levels import LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    levels = _spec_levels()
    wrappers = WRAP_COMBOS[combo]
    B = 96
    pool_d = LevelPool(levels, counts_fn=_device_counts, n_agents=2, min_performance_fraction=0.1)
    pool_c = LevelPool(levels, counts_fn=util.oracle_counts, n_agents=2, min_performance_fraction=0.1)
    kw = dict(first_level=(np.arange(B) * 3) % len(levels), auto_reset=True, level_stride=2, time_limit=17,
              view_shape=(9, 9), output_channels=None)
    dev = SafeLifeMultiAgentVectorEnv(pool_d, B, wrappers=wrappers, **kw)
    cpu = util.OracleMultiBackend(pool_c, B, **kw)
    dev.reset()
    assert np.array_equal(dev.numpy("obs"), cpu.reset())
    cfg = MultiWrapConfig(**wrappers)
    board = cpu.get("board")
    states = [MultiWrapState(cfg, cpu.get("agent_locs")[e]) for e in range(B)]
    baseline = board.copy()
    fresh = np.ones(B, bool)
    rng = np.random.default_rng(40 + combo)
    for t in range(60):
        acts = rng.integers(0, 9, (B, 2)).astype(np.int32)
        acts[cpu.get("is_active") == 0] = 0
        dev.step(acts)
        oc, rc, dc = cpu.step(acts)
        assert np.array_equal(dev.numpy("reward"), rc) and np.array_equal(dev.numpy("done"), dc), t
        assert np.array_equal(dev.numpy("obs"), oc), t
        for name in util.MULTI_STATE:
            assert np.array_equal(dev.get(name) if hasattr(dev, "get") else dev.numpy(name), cpu.get(name)), (t, name)
        board, goals, exits = cpu.get("board"), cpu.get("goals"), cpu.get("exit_locs")
        locs, ep_r = cpu.get("agent_locs"), cpu.get("episode_reward")
        times_up = cpu.get("times_up")
        shaped = dev.numpy("shaped_reward")
        all_done = dc.astype(bool).all(axis=1)
        for e in range(B):
            if all_done[e]:
                # reloaded: the restatement's state restarts with the new episode (nothing of the old one is left)
                states[e].reset(locs[e])
                baseline[e] = board[e]
                fresh[e] = True
                continue
            side = side_effect_count(board[e], baseline[e], goals[e], exits[e], cfg.ignore_reward_cells)
            want = states[e].step(rc[e], dc[e].astype(bool), bool(times_up[e, 0]), ep_r[e], locs[e], side)
            assert np.array_equal(shaped[e].view(np.uint32), want.view(np.uint32)), (t, e)
    assert cpu.get("episode_idx").min() >= 2


@pytest.mark.gpu
def test_queue_end_to_end_multi():
    """One queue entry per env episode, on the step where every agent is done: record, per-agent records and the board
    as the agents left it against an oracle replay (auto_reset off: the terminal board stays in place); then the
    occupancy tensors of every entry against the primitives under the entry's derived stream."""
    from safelife_amd import speedups
    from safelife_amd.levels import LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    levels = _spec_levels()
    B, T = 40, 24
    pool_d = LevelPool(levels, counts_fn=_device_counts, n_agents=2, min_performance_fraction=0.1)
    pool_c = LevelPool(levels, counts_fn=util.oracle_counts, n_agents=2, min_performance_fraction=0.1)
    kw = dict(first_level=np.arange(B) % len(levels), auto_reset=False, time_limit=20, view_shape=(9, 9),
              output_channels=None)
    dev = SafeLifeMultiAgentVectorEnv(pool_d, B, wrappers=TRAIN, side_effects=dict(capacity=64, num_samples=50), **kw)
    cpu = util.OracleMultiBackend(pool_c, B, **kw)
    dev.reset()
    cpu.reset()
    rng = np.random.default_rng(8)
    ended = {}
    for t in range(T):
        acts = rng.integers(0, 9, (B, 2)).astype(np.int32)
        acts[cpu.get("is_active") == 0] = 0
        was_active = cpu.get("is_active").astype(bool).any(axis=1)
        dev.step(acts)
        _, rc, dc = cpu.step(acts)
        for e in np.nonzero(dc.astype(bool).all(axis=1) & was_active)[0]:
            ended[int(e)] = dict(t=t, reward=rc[e].copy(), done=dc[e].copy(), board=cpu.get("board")[e].copy(),
                                 num_steps=int(cpu.get("num_steps")[e]), success=cpu.get("success")[e].copy(),
                                 ep_r=cpu.get("episode_reward")[e].copy(), ep_l=cpu.get("episode_length")[e].copy())
    assert len(ended) == B                      # every env's episode ended within T steps (time_limit 20)
    batch = dev.side_effects_flush()
    recs, agents = batch.records(), batch.agent_records()
    assert len(batch) == B and batch.dropped() == 0
    assert sorted(recs["env"].tolist()) == list(range(B))
    boards = batch.boards.cpu().numpy().view(np.uint16)
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
    # the pass: each entry's occupancy tensors under its derived streams (as test_side_effect_queue_end_to_end)
    counts = batch.counts.cpu().numpy()
    for i in range(0, B, 7):
        occ = _occupancy_by_primitives(speedups, pool_d, int(recs["level"][i]), boards[i], int(recs["env"][i]),
                                       int(recs["episode_idx"][i]), int(recs["num_steps"][i]), 50)
        assert np.array_equal(counts[0, i], occ[0]) and np.array_equal(counts[1, i], occ[1]), i
    # nothing more is queued once every agent is done (auto_reset off)
    dev.step(np.zeros((B, 2), np.int32))
    assert len(dev.side_effects_flush()) == 0


def _mix64(z):
    m = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def _occupancy_by_primitives(speedups, pool, level, board, env, episode, steps, num_samples):
    """The two occupancy tensors of one queue entry from the one-board primitives, under the entry's derived streams
    (the derivation test_side_effect_queue_end_to_end restates): run 0 rolls the starting board forward and samples it,
    run 1 samples the final board."""
    import oracle
    words = pool.arrays()["pool_rng"][level].copy()
    bg = np.random.PCG64(0)
    out = []
    for salt in (0x5EFFEC75, 0x2B0A2D5):
        a_ = _mix64((((salt ^ env) & 0xFFFFFFFF) << 32) | episode)
        words[0] ^= np.uint64(a_)
        words[1] ^= np.uint64(_mix64(a_))
        oracle.pcg64_set_state_words(bg, words)
        speedups.set_bit_generator(bg)
        lv = pool.levels[level]
        if not out:
            out.append(speedups.life_occupancy(speedups.advance_board(lv.board, lv.spawn_prob, steps), lv.spawn_prob,
                                               num_samples))
        else:
            out.append(speedups.life_occupancy(board, lv.spawn_prob, num_samples))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["uint8", "float32"])
def test_policy_layout_multi(layout):
    """policy_tensor [B, A, C, vw, vh] equals the [B, A, vh, vw, C] observation transposed, after the reset and every
    step; an env without the observation, driven by the same actions, writes the same tensor."""
    from safelife_amd.levels import LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    levels = _spec_levels()
    pool = LevelPool(levels, counts_fn=_device_counts, n_agents=2)
    B = 21
    kw = dict(first_level=np.arange(B) % len(levels), time_limit=9, view_shape=(7, 11),
              output_channels=tuple(range(12)) + (25, 26, 27))
    a = SafeLifeMultiAgentVectorEnv(pool, B, policy_layout=layout, **kw)
    b = SafeLifeMultiAgentVectorEnv(pool, B, policy_layout=layout, with_obs=False, wrappers=TRAIN, **kw)
    assert a.obs is not None and b.obs is None
    a.reset()
    b.reset()
    rng = np.random.default_rng(3)
    for t in range(20):
        pa = a.policy_tensor.cpu().numpy()
        want = a.numpy("obs").transpose(0, 1, 4, 3, 2).astype(pa.dtype)
        assert pa.shape == (B, 2, 15, 11, 7) and np.array_equal(pa, want), t
        assert np.array_equal(b.policy_tensor.cpu().numpy(), pa), t
        acts = rng.integers(0, 9, (B, 2)).astype(np.int32)
        a.step(acts)
        b.step(acts)


def _compat_env(tr):
    from safelife_amd import env_wrappers as W
    from safelife_amd.env import SafeLifeEnv
    from tests.test_hip_parity import _compat_games
    env = SafeLifeEnv(iter(_compat_games(tr)), single_agent=False, **util.env_kwargs_from_trace(tr))
    inner = {}
    inner_step = env.step

    def recording_step(a):
        ret = inner_step(a)
        inner["reward"] = ret[1].copy()
        return ret
    env.step = recording_step
    w = env
    if "wrap_movement" in tr:
        bonus, power, period, as_penalty = tr["wrap_movement"]
        w = W.MovementBonusWrapper(w, movement_bonus=float(bonus), movement_bonus_power=float(power),
                                   movement_bonus_period=int(period), as_penalty=bool(as_penalty))
    if "wrap_exit_bonus" in tr:
        w = W.ExtraExitBonus(w, bonus=float(tr["wrap_exit_bonus"]))
    if "wrap_side_effect" in tr:
        coef, ignore = tr["wrap_side_effect"]
        w = W.SimpleSideEffectPenalty(w, penalty_coef=float(coef), ignore_reward_cells=bool(ignore),
                                      baseline="inaction" if "wrap_inaction_rng" in tr else "starting-state")
    if "min_performance_fraction" in tr:
        w = W.MinPerformanceScheduler(w, min_performance_fraction=float(tr["min_performance_fraction"]))
    return w, inner


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in WRAP_TRACES if "inaction" not in n])
def test_compat_wrappers_replay_multi(name):
    """safelife_amd.env_wrappers over safelife_amd.env.SafeLifeEnv(single_agent=False) replays the reference's wrapped
    multi-agent traces: shaped and unwrapped rewards of every agent and step.  (The starting-state ones, as the
    single-agent compat test: the inaction baseline's process-wide generator is the fused path's to replay.)"""
    tr = util.load_trace(name)
    env, inner = _compat_env(tr)
    env.reset()
    episode = 0
    for t in range(len(tr["trace_reward"])):
        obs, reward, done, info = env.step(tr["trace_actions"][t].astype(np.int64))
        where = "step %d" % t
        assert reward.dtype == np.float32
        assert np.array_equal(reward.view(np.uint32), tr["trace_shaped_reward"][t].view(np.uint32)), where
        assert np.array_equal(inner["reward"], tr["trace_reward"][t]), where
        assert np.array_equal(info["board"], tr["trace_board"][t]), where
        if np.all(done):
            episode += 1
            if episode >= len(tr["trace_reset_at"]):
                break
            env.reset()


@pytest.mark.gpu
def test_side_effect_pass_reproduces_reference_multi_inputs():
    """slhip_side_effects with derive_streams=0 on queue entries of multi-agent games (tests/golden/
    side_effect_inputs_multi.npz: the reference's side_effect_score internals for 26x26 two-agent terminal games -- the
    coloured agents sit on both boards): roll-forward and both occupancy tensors, the generator after them."""
    import torch
    from safelife_amd import speedups as sp
    from safelife_amd.levels import Level, LevelPool
    from safelife_amd.vector_env import SafeLifeVectorEnv
    with np.load(os.path.join(util.GOLDEN, "side_effect_inputs_multi.npz")) as d:
        d = {k: d[k] for k in d.files}
    n, ns = int(d["n_games"]), int(d["num_samples"])
    starts = [Level(d["g%d_b0" % i], agent_locs=np.zeros((0, 2), int), spawn_prob=float(d["g%d_spawn_prob" % i]))
              for i in range(n)]
    env = SafeLifeVectorEnv(LevelPool(starts, counts_fn=_device_counts), 4, with_obs=False)
    dev, cap = env.device, 8
    H, W = d["g0_b0"].shape
    rec = np.zeros((cap, 8), np.int32)
    boards = np.zeros((cap, H, W), np.uint16)
    rng = np.zeros((2 * cap, 4), np.uint64)
    for i in range(n):
        rec[i, 0], rec[i, 1], rec[i, 2] = i, i, int(d["g%d_num_steps" % i])
        rec[i, 4] = np.float32(d["g%d_spawn_prob" % i]).view(np.int32)
        boards[i] = d["g%d_b2" % i]
        rng[i] = d["g%d_rng0" % i]
    bufs = dict(count=torch.tensor([n], dtype=torch.int32, device=dev), records=torch.from_numpy(rec).to(dev),
                boards=torch.from_numpy(boards.view(np.int16)).to(dev))
    q = _hip.EpisodeQueue()
    q.capacity, q.env_base = cap, 0
    q.count, q.records, q.boards = (bufs[k].data_ptr() for k in ("count", "records", "boards"))
    K = _hip.SL_SE_MAX_KEYS
    out = dict(work_boards=torch.zeros((2 * cap, H, W), dtype=torch.int16, device=dev),
               work_prob=torch.zeros(2 * cap, dtype=torch.float32, device=dev),
               work_steps=torch.zeros(2 * cap, dtype=torch.int32, device=dev),
               work_rng=sp._to_device(rng, np.uint64),
               counts=torch.zeros((2, cap, H, W, 8), dtype=torch.int32, device=dev),
               keys=torch.zeros((cap, K), dtype=torch.int16, device=dev),
               life_dist=torch.zeros((cap, 2, 8, H, W), dtype=torch.float64, device=dev),
               type_masks=torch.zeros((cap, 2, K - 8, H, W), dtype=torch.uint8, device=dev))
    _hip.check(_hip.lib().slhip_side_effects(env._sref, C.byref(q), ns, 0,
                                             *[_hip.ptr(out[k]) for k in ("work_boards", "work_prob", "work_steps",
                                                                          "work_rng", "counts", "keys", "life_dist",
                                                                          "type_masks")],
                                             _hip.current_stream_ptr()))
    counts = out["counts"].cpu().numpy()
    after = sp._to_host(out["work_rng"], np.uint64)
    for i in range(n):
        assert np.array_equal(counts[0, i], d["g%d_occ0" % i]), i
        assert np.array_equal(counts[1, i], d["g%d_occ1" % i]), i
        assert np.array_equal(after[i], d["g%d_rng_end" % i]), i
