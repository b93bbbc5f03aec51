#!/usr/bin/env python3
"""
Generate the multi-agent training-wrapper fixtures in tests/golden/ by RUNNING THE REFERENCE:

    trace_multi_wrap_*.npz       SafeLifeEnv(single_agent=False) under the reference's own env_wrappers, stacked as
                                 training/env_factory.py:277-283 stacks them; per step and agent the shaped reward the
                                 outermost wrapper returns (float32 [A]) next to the inner env's outputs, the wrapper's
                                 baseline_board and last_side_effect
    side_effect_inputs_multi.npz side_effect_score internals (side_effects.py:103-113) of multi-agent terminal games

Runs only in the build container, as make_golden.py does (whose helpers it imports and which it leaves as it is):

    python tests/golden/make_golden_multi_wrap.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

TRAIN = dict(movement=dict(as_penalty=True), exit_bonus=0.5,
             side_effect=dict(baseline="starting-state", penalty_coef=0.3))


def run_trace_multi_wrapped(R, games, actions, env_kw, wrappers, min_perf_fraction=None, inaction_seed=None):
    """The reference SafeLifeEnv(single_agent=False) over `games` (one episode each) under the wrapper stack; the env
    is reset once EVERY agent is done (training/base_algo.py:231-236).  actions: int [T, A]."""
    global_gen = None
    if inaction_seed is not None:
        import safelife.random as sl_random
        global_gen = np.random.default_rng(inaction_seed)
        sl_random.random_gen = global_gen
        R.speedups.set_bit_generator(global_gen.bit_generator)
    env = R.env.SafeLifeEnv(iter(games), single_agent=False, **env_kw)
    inner = {}
    inner_step = env.step

    def recording_step(a):
        ret = inner_step(a)
        inner["reward"] = ret[1].copy()
        return ret
    env.step = recording_step
    W = R.wrappers
    wrapped = env
    if wrappers.get("movement") is not None:
        wrapped = W.MovementBonusWrapper(wrapped, **wrappers["movement"])
    if wrappers.get("exit_bonus") is not None:
        wrapped = W.ExtraExitBonus(wrapped, bonus=wrappers["exit_bonus"])
    se = None
    if wrappers.get("side_effect") is not None:
        wrapped = se = W.SimpleSideEffectPenalty(wrapped, **wrappers["side_effect"])
    if min_perf_fraction is not None:
        wrapped = W.MinPerformanceScheduler(wrapped, min_performance_fraction=min_perf_fraction)
    keys = ("obs", "reward", "shaped_reward", "done", "board", "goals", "agent_locs", "times_up", "ep_length", "ep_reward",
            "success", "reset_obs", "reset_board", "reset_rng", "reset_required", "rng_after", "num_steps",
            "baseline_board", "last_side_effect", "inaction_rng_after")
    rec = {k: [] for k in keys}
    rng0 = mg.words(global_gen.bit_generator) if global_gen is not None else None

    def note_reset(obs):
        rec["reset_obs"].append(obs.copy())
        rec["reset_board"].append(env.game.board.copy())
        rec["reset_rng"].append(mg.words(env.game._rng.bit_generator))
        rec["reset_required"].append(np.array(env.game.required_points(), np.int64))

    note_reset(wrapped.reset())
    reset_at = [0]
    for t, a in enumerate(actions):
        obs, reward, done, info = wrapped.step(np.array(a, np.int64))
        assert reward.dtype == np.float32, reward.dtype
        rec["obs"].append(obs.copy())
        rec["shaped_reward"].append(reward.copy())
        rec["reward"].append(inner["reward"])
        rec["done"].append(np.array(done, bool))
        rec["board"].append(info["board"].copy())
        rec["goals"].append(info["goals"].copy())
        rec["agent_locs"].append(np.array(info["agent_locs"], np.int64).copy())
        rec["times_up"].append(bool(info["times_up"]))
        rec["ep_length"].append(np.array(info["episode"]["length"], np.int64).copy())
        rec["ep_reward"].append(np.array(info["episode"]["reward"], np.float32).copy())
        rec["success"].append(np.array(info["episode"]["success"], bool))
        rec["rng_after"].append(mg.words(env.game._rng.bit_generator))
        rec["num_steps"].append(env.game.num_steps)
        if se is not None:
            rec["baseline_board"].append(se.baseline_board.copy())
            rec["last_side_effect"].append(np.int64(se.last_side_effect))
        if global_gen is not None:
            rec["inaction_rng_after"].append(mg.words(global_gen.bit_generator))
        if np.all(done):
            try:
                obs = wrapped.reset()
            except StopIteration:
                break
            note_reset(obs)
            reset_at.append(t + 1)
    for k in ("baseline_board", "last_side_effect", "inaction_rng_after"):
        if not rec[k]:
            del rec[k]
    out = {k: np.array(v) for k, v in rec.items()}
    out["reset_at"] = np.array(reset_at)
    out["actions"] = np.array(actions[:len(rec["reward"])], np.int32)
    return out, rng0


def blob_of(R, out, name, games_fn, actions, env_kw, wrappers, min_perf_fraction=None, inaction_seed=None):
    tr, rng0 = run_trace_multi_wrapped(R, games_fn(), actions, env_kw, wrappers, min_perf_fraction, inaction_seed)
    blob = {}
    games = games_fn()
    for i, g in enumerate(games):
        for k, v in mg.level_record(g).items():
            blob["level%d_%s" % (i, k)] = v
        blob["level%d_rng" % i] = mg.words(g._rng.bit_generator)
    blob["n_levels"] = np.array(len(games))
    for k, v in tr.items():
        blob["trace_" + k] = v
    for k, v in env_kw.items():
        blob["env_" + k] = np.array(-1 if v is None else v)
    if min_perf_fraction is not None:
        blob["min_performance_fraction"] = np.array(min_perf_fraction)
    mv, se = wrappers.get("movement"), wrappers.get("side_effect")
    if mv is not None:
        blob["wrap_movement"] = np.array([mv.get("movement_bonus", 0.1), mv.get("movement_bonus_power", 1e-100),
                                          mv.get("movement_bonus_period", 4), float(mv.get("as_penalty", True))])
    if wrappers.get("exit_bonus") is not None:
        blob["wrap_exit_bonus"] = np.array(float(wrappers["exit_bonus"]))
    if se is not None:
        assert (se.get("baseline", "starting-state") == "inaction") == (inaction_seed is not None)
        blob["wrap_side_effect"] = np.array([se.get("penalty_coef", 0.0), float(se.get("ignore_reward_cells", False))])
        if inaction_seed is not None:
            blob["wrap_inaction_rng"] = rng0
    path = os.path.join(out, "trace_multi_wrap_%s.npz" % name)
    np.savez_compressed(path, **blob)
    print("multi-agent wrapped trace %-22s steps=%4d episodes=%d shaped_sum=%s bytes=%d" % (
        name, len(tr["reward"]), len(tr["reset_at"]), tr["shaped_reward"].sum(0), os.path.getsize(path)))


def spec_games(R, spec, seed, n_levels):
    def games_fn():
        it = R.levels.SafeLifeLevelIterator("random/multi-agent/" + spec, seed=seed, num_workers=0)
        return [next(it) for _ in range(n_levels)]
    return games_fn


def hand_games(R, board, goals, locs, seeds, spawn_prob=None):
    Game = R.game.SafeLifeGame

    def games_fn():
        gs = []
        for s in seeds:
            g = Game(board_size=board.shape)
            g.board = board.copy()
            g.goals = goals.copy()
            g.agent_locs = np.array(locs)
            g.min_performance = -1
            if spawn_prob is not None:
                g.spawn_prob = spawn_prob
            g.reset_points_table()
            g.update_exit_locs()
            gs.append(mg.seeded(Game.loaddata(g.serialize()), s))
        return gs
    return games_fn


def gen_traces(R, out):
    rng = np.random.default_rng(2077)
    CT = R.game.CellTypes
    # the env_factory stack over the reference's 26x26 multi-agent specs, exits scheduled down (min_performance_fraction)
    for spec, seed, n_levels, frac, kw in (
            ("asym1", 15, 3, 0.3, dict(view_shape=(9, 9), output_channels=None, time_limit=30)),
            ("build-coop", 16, 3, 0.2, dict(view_shape=(7, 7), output_channels=None, time_limit=28)),
            ("build-compete", 17, 3, 0.5, dict(view_shape=(7, 7), output_channels=None, time_limit=25))):
        acts = rng.integers(0, 9, (80, 2))
        blob_of(R, out, "train_" + spec.replace("-", "_"), spec_games(R, spec, seed, n_levels), acts,
                dict(should_calculate_side_effects=False, **kw), TRAIN, min_perf_fraction=frac)
    # a real exponent, a bonus instead of a penalty, period 3, reward cells ignored
    other = dict(movement=dict(as_penalty=False, movement_bonus=0.25, movement_bonus_power=0.5, movement_bonus_period=3),
                 exit_bonus=1.5, side_effect=dict(penalty_coef=0.125, ignore_reward_cells=True))
    blob_of(R, out, "other_build_coop", spec_games(R, "build-coop", 18, 3), rng.integers(0, 9, (80, 2)),
            dict(view_shape=(7, 7), output_channels=None, time_limit=30, should_calculate_side_effects=False), other)

    # hand-made levels: two agents, exits open from the start (min_performance -1)
    b = np.zeros((10, 10), np.uint16)
    b[5, 5] = CT.level_exit
    b[2, 7] = CT.level_exit
    b[5, 3] = CT.player | CT.color_r
    b[2, 2] = CT.player | CT.color_b
    for y, x in ((7, 7), (7, 8), (8, 7), (8, 8)):
        b[y, x] = CT.life | CT.color_g
    goals = np.zeros_like(b)
    goals[1, 1] = CT.color_g
    # agent 0 leaves at step 2 while agent 1 plays on until the time limit; then both walk out
    ep1 = [[2, 0], [2, 5], [0, 2], [0, 2], [0, 6], [0, 3], [0, 0], [0, 1]]
    ep2 = [[2, 2], [2, 2], [0, 2], [0, 2], [0, 2], [0, 0]]
    hand = dict(movement=dict(as_penalty=True, movement_bonus_power=0.5), exit_bonus=0.5,
                side_effect=dict(penalty_coef=0.25))
    blob_of(R, out, "hand_exit", hand_games(R, b, goals, [[5, 3], [2, 2]], [40, 41]), np.array(ep1 + ep2),
            dict(view_shape=(7, 7), output_channels=None, time_limit=8, should_calculate_side_effects=False), hand)
    # the inaction baseline on a level with spawners: the baseline's draws come from the process-wide generator
    s = np.zeros((12, 12), np.uint16)
    s[6, 9] = CT.level_exit
    s[3, 2] = CT.player | CT.color_r
    s[9, 4] = CT.player | CT.color_b
    s[1, 8] = CT.spawner | CT.color_g
    s[10, 10] = CT.spawner
    s[5, 5] = CT.spawner | CT.color_r
    for y, x in ((2, 8), (1, 9), (6, 5), (5, 6)):
        s[y, x] = CT.life
    sg = np.zeros_like(s)
    sg[8:11, 1:4] = CT.color_b
    sg[0:3, 5:7] = CT.color_g
    acts = rng.integers(0, 9, (70, 2))
    stack = dict(movement=dict(as_penalty=True), exit_bonus=0.5, side_effect=dict(baseline="inaction", penalty_coef=0.3))
    blob_of(R, out, "inaction_spawn", hand_games(R, s, sg, [[3, 2], [9, 4]], [60, 61, 62], spawn_prob=0.4), acts,
            dict(view_shape=(7, 7), output_channels=None, time_limit=24, should_calculate_side_effects=False), stack,
            inaction_seed=5151)
    stack_ig = dict(movement=dict(as_penalty=True, movement_bonus_power=0.5), exit_bonus=0.5,
                    side_effect=dict(baseline="inaction", penalty_coef=0.5, ignore_reward_cells=True))
    blob_of(R, out, "inaction_asym1", spec_games(R, "asym1", 19, 2), rng.integers(0, 9, (50, 2)),
            dict(view_shape=(7, 7), output_channels=None, time_limit=25, should_calculate_side_effects=False), stack_ig,
            inaction_seed=5252)


def gen_side_effect_inputs_multi(R, out):
    """side_effect_score's occupancy tensors (side_effects.py:103-113) for multi-agent games played until every agent is
    done; EMD itself is unpinned.  One process-wide generator per game, its words before / between the draws."""
    sp = R.speedups
    rng = np.random.default_rng(31)
    blob = {}
    for i, (spec, seed, n_steps) in enumerate((("asym1", 21, 30), ("build-coop", 22, 26), ("build-compete", 23, 22))):
        game = spec_games(R, spec, seed, 1)()[0]
        game.update_exit_colors()
        for _ in range(n_steps):
            game.execute_actions(rng.integers(0, 9, len(game.agent_locs)))
            game.advance_board()
            game.update_exit_colors()
        glob = np.random.PCG64(7000 + i)
        w0 = mg.words(glob)
        sp.set_bit_generator(glob)
        b0 = game._init_data["board"]
        b1 = sp.advance_board(b0, game.spawn_prob, game.num_steps)
        occ0 = sp.life_occupancy(b1, game.spawn_prob, 200)
        occ1 = sp.life_occupancy(game.board, game.spawn_prob, 200)
        blob.update({"g%d_b0" % i: np.array(b0, np.uint16), "g%d_b2" % i: np.array(game.board, np.uint16),
                     "g%d_num_steps" % i: np.array(game.num_steps), "g%d_spawn_prob" % i: np.array(game.spawn_prob),
                     "g%d_rng0" % i: w0, "g%d_rng_end" % i: mg.words(glob),
                     "g%d_occ0" % i: occ0.astype(np.int32), "g%d_occ1" % i: occ1.astype(np.int32)})
    blob["n_games"] = np.array(3)
    blob["num_samples"] = np.array(200)
    np.savez_compressed(os.path.join(out, "side_effect_inputs_multi.npz"), **blob)
    print("side_effect_inputs_multi: %d bytes" % os.path.getsize(os.path.join(out, "side_effect_inputs_multi.npz")))


def main():
    R = mg.import_reference()
    gen_traces(R, HERE)
    gen_side_effect_inputs_multi(R, HERE)


if __name__ == "__main__":
    main()
