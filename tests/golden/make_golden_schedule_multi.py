#!/usr/bin/env python3
"""
Writes tests/golden/schedule_multi_cases.npz by RUNNING THE REFERENCE on the CPU: what tests/schedule_multi_ref.py and the
multi-agent level schedule kernels (csrc/sl_schedule.hip: k_schedule_required_multi, k_schedule_harvest_multi) are held to.

    python tests/golden/make_golden_schedule_multi.py

Runs where make_golden_schedule.py runs (the reference's Python through make_golden.import_reference(), scipy).

  syn_*   a few synthetic levels with 1, 3 and 8 agents whose agents have DIFFERENT points tables (syn_agents the count;
          syn_board / syn_goals [n, H, W]; syn_agent_locs [n, 8, 2] and syn_points_table [n, 8, 8, 9], rows past the level's
          agents are -1 / 0; syn_min_performance).
  req_*   MinPerformanceScheduler.reset() (env_wrappers.py:142-145) on the reference's SafeLifeGame of every level of the
          trace fixtures multi_asym1, multi_build_coop, multi_build_compete and multi_hand_exit (req_source 0..3, req_level)
          and of the synthetic levels (req_source 4), for every fraction of req_fraction (make_golden_schedule.FRACTIONS):
          req_agents the level's agent count, req_min_performance its own value, req_available [levels, 8] =
          initial_available_points() and req_points [levels, fractions, 8] = required_points() after the reset, all agents
          (columns past the level's agents are 0).
  cur_*   CurricularLevelIterator.get_next_parameters (env_factory.py:104-146) fed scripted MULTI-AGENT episodes through a
          stub logger: last_data['reward'] a list of A floats taken from float32 values, 'reward_possible' a list of A ints
          (safelife_logger.py:283-300 for a multi-agent game).  Per case i (cur_agents, cur_groups, cur_lookback): episodes
          [cur_offsets[i], cur_offsets[i+1]) with cur_group, cur_reward float32 [episode, 8] and cur_possible int32
          [episode, 8] (columns past the case's agents are 0 / 1); cur_perf the performance the iterator appended for the
          episode (np.average of the quotients, 0 where that is NaN or inf), cur_probs [episode, 3] the probability_lvl* it
          logged after the episode (columns past the case's groups are 0), cur_best / cur_recent the best_perf_lvl* /
          recent<lookback>_perf_lvl*.
          Performances carry a trend plus noise, as in make_golden_schedule.py, and the script asserts that no window the
          reference fits is constant.  Special episodes: an agent with reward_possible 0 (x / 0: the average is inf; 0 / 0:
          NaN -- both file 0.0), negative rewards, one agent at 0 reward.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

TRACES = ("multi_asym1", "multi_build_coop", "multi_build_compete", "multi_hand_exit")
SYNTHETIC = ((1, 0.5), (3, 0.3), (3, 1.0), (8, 0.5), (8, 1.0 / 3.0), (8, -1.0))       # agents, min_performance
CURRICULA = ((2, 2, 100, 400), (2, 3, 5, 150), (3, 3, 5, 150), (3, 2, 100, 400), (8, 2, 5, 120), (8, 3, 100, 500))
MAX_A, MAX_G = 8, 3


def synthetic_levels(CellTypes, default_table):
    """12 x 12 boards: life and trees of several colours, coloured goals under some of them and elsewhere, the agents in
    one row.  Agent a's table is the default one with its colour columns rolled by a and one entry changed, so that the
    agents' available points differ."""
    rng = np.random.default_rng(812)
    H = W = 12
    out = dict(syn_agents=[], syn_board=[], syn_goals=[], syn_agent_locs=[], syn_points_table=[], syn_min_performance=[])
    for A, mp in SYNTHETIC:
        board = np.zeros((H, W), np.uint16)
        goals = np.zeros((H, W), np.uint16)
        colors = rng.integers(1, 8, (H, W)).astype(np.uint16) << CellTypes.color_bit
        kind = rng.random((H, W))
        board[kind < 0.25] = CellTypes.life
        board[(kind >= 0.25) & (kind < 0.3)] = CellTypes.tree
        board[board > 0] |= colors[board > 0]
        goal_colors = rng.integers(1, 8, (H, W)).astype(np.uint16) << CellTypes.color_bit
        goals[rng.random((H, W)) < 0.3] = 1
        goals = (goals * goal_colors).astype(np.uint16)
        board[0, :] = 0
        locs = np.full((MAX_A, 2), -1, np.int64)
        for a in range(A):
            locs[a] = (0, a)
            board[0, a] = CellTypes.player | (np.uint16((a % 7) + 1) << CellTypes.color_bit)
        tables = np.zeros((MAX_A, 8, 9), np.int64)
        for a in range(A):
            t = default_table.copy()
            t[:, :8] = np.roll(t[:, :8], a, axis=1)
            t[1 + a % 7, (a * 3) % 8] += a + 1
            tables[a] = t
        out["syn_agents"].append(A), out["syn_board"].append(board), out["syn_goals"].append(goals)
        out["syn_agent_locs"].append(locs), out["syn_points_table"].append(tables), out["syn_min_performance"].append(mp)
    return dict(syn_agents=np.array(out["syn_agents"], np.int32), syn_board=np.array(out["syn_board"], np.uint16),
                syn_goals=np.array(out["syn_goals"], np.uint16), syn_agent_locs=np.array(out["syn_agent_locs"], np.int32),
                syn_points_table=np.array(out["syn_points_table"], np.int32),
                syn_min_performance=np.array(out["syn_min_performance"], np.float64))


def required_cases(SafeLifeGame, MinPerformanceScheduler, syn, fractions):
    class Env(object):
        def __init__(self, game):
            self.game = game

        def reset(self):
            return None
    levels = []                                                 # (source, level, data)
    for s, name in enumerate(TRACES):
        with np.load(os.path.join(HERE, "trace_%s.npz" % name)) as d:
            for k in range(int(d["n_levels"])):
                pre = "level%d_" % k
                levels.append((s, k, {key: d[pre + key] for key in ("board", "goals", "agent_locs", "spawn_prob",
                                                                    "min_performance", "points_table")}))
    for k, A in enumerate(syn["syn_agents"]):
        levels.append((len(TRACES), k, dict(board=syn["syn_board"][k], goals=syn["syn_goals"][k],
                                            agent_locs=syn["syn_agent_locs"][k, :A].astype(np.int64), spawn_prob=0.0,
                                            min_performance=syn["syn_min_performance"][k],
                                            points_table=syn["syn_points_table"][k, :A].astype(np.int64))))
    rows = {k: [] for k in ("req_source", "req_level", "req_agents", "req_available", "req_min_performance", "req_points")}
    for s, k, data in levels:
        A = len(data["agent_locs"])
        points = np.zeros((len(fractions), MAX_A), np.int64)
        mp = float(data["min_performance"])
        for j, f in enumerate(fractions):
            # (a copy per game: the wrapper's `game.min_performance *= fraction` works in place on an array it is handed)
            game = SafeLifeGame.loaddata(dict(data, min_performance=np.float64(mp)), auto_cls=False)
            assert float(game.min_performance) == mp
            assert len(game.agent_locs) == A and game.points_table.shape == (A, 8, 9)
            MinPerformanceScheduler(Env(game), min_performance_fraction=f).reset()
            points[j, :A] = game.required_points()
        avail = np.zeros(MAX_A, np.int64)
        avail[:A] = game.initial_available_points()
        rows["req_source"].append(s), rows["req_level"].append(k), rows["req_agents"].append(A)
        rows["req_available"].append(avail), rows["req_min_performance"].append(mp)
        rows["req_points"].append(points)
    assert np.abs(np.array(rows["req_points"])).max() < 2 ** 31
    differ = [len(set(a[:n].tolist())) > 1 for a, n, s in zip(rows["req_available"], rows["req_agents"], rows["req_source"])
              if s == len(TRACES) and n > 1]
    assert differ and all(differ)                              # the synthetic agents' available points do differ
    return dict(req_source=np.array(rows["req_source"], np.int32), req_level=np.array(rows["req_level"], np.int32),
                req_agents=np.array(rows["req_agents"], np.int32), req_available=np.array(rows["req_available"], np.int32),
                req_min_performance=np.array(rows["req_min_performance"], np.float64),
                req_points=np.array(rows["req_points"], np.int32), req_fraction=np.array(fractions, np.float64))


def scripted_episodes(rng, A, G, lookback, n):
    """(group, rewards float32 [A], reward_possible int [A]) per episode: each group's performance follows its own trend
    plus noise, every agent with noise of its own."""
    weights = np.array([0.4, 0.35, 0.25][:G])
    weights = weights / weights.sum()
    seen = np.zeros(G, np.int64)
    out = []
    for k in range(n):
        g = int(rng.choice(G, p=weights))
        i = seen[g]
        seen[g] += 1
        span = float(max(3 * lookback, 40))
        trend = (0.1 + 0.7 * i / span, 0.6 - 0.4 * i / span, 0.3 + 0.5 * max(0.0, i / span - 0.5))[g]
        possible = rng.integers(20, 90, A)
        perf = trend + rng.normal(0.0, 0.05) + rng.normal(0.0, 0.1, A)
        reward = np.round(perf * possible).astype(np.float32)
        a = int(rng.integers(0, A))
        if k % 97 == 41:
            possible[a], reward[a] = 0, 0.0                     # 0 / 0 in one agent: the average is NaN
        elif k % 97 == 77:
            possible[a] = 0                                     # x / 0: the average is +-inf
            reward[a] = max(1.0, abs(float(reward[a])))
        elif k % 53 == 17:
            reward[a] = -3.0
        elif k % 31 == 5:
            reward[a] = 0.0
        elif k % 41 == 9:
            reward[:] = -np.abs(reward)
        out.append((g, reward, possible.astype(np.int64)))
    return out


def curriculum_cases(env_factory):
    class Game(object):
        file_name = None

    class Logger(object):
        last_data, last_game, logdir = None, Game(), None

        def log_scalars(self, record):
            self.record = record

    class Iterator(env_factory.CurricularLevelIterator):
        def __init__(self, G, lookback, logger):          # (no file loading: the level iterator's own __init__ is skipped)
            from collections import defaultdict
            self.logger, self.lookback = logger, lookback
            self.max_stage = G - 1
            self.file_data = [("family%d" % g,) for g in range(G)]
            self.perf_records = defaultdict(lambda: [0.0])
            self.best = defaultdict(lambda: 0)

        def record_video(self, lvl, perf):
            pass

    rows = {k: [] for k in ("cur_group", "cur_reward", "cur_possible", "cur_perf", "cur_probs", "cur_best", "cur_recent")}
    offsets = [0]
    rng = np.random.default_rng(20261020)
    np.random.seed(7)                                          # (get_next_parameters draws its choice from numpy's global)
    for A, G, lookback, n in CURRICULA:
        log = Logger()
        it = Iterator(G, lookback, log)
        special = dict(nan=0, inf=0, negative=0, zero=0)
        for g, reward, possible in scripted_episodes(rng, A, G, lookback, n):
            log.last_data = {"reward": [float(r) for r in reward], "reward_possible": [int(p) for p in possible]}
            log.last_game = Game()
            log.last_game.file_name = "family%d" % g
            with np.errstate(all="ignore"):
                it.get_next_parameters()
                q = reward.astype(np.float64) / possible
            special["nan"] += int(np.isnan(np.average(q)))
            special["inf"] += int(np.isinf(np.average(q)))
            special["negative"] += int((reward < 0).any())
            special["zero"] += int((reward == 0).sum() == 1)
            for h in range(G):                                 # the script's own inputs: no window the fit sees is constant
                rec = it.perf_records["family%d" % h]
                assert len(rec) < lookback or len(set(rec[-lookback:])) > 1, (A, G, lookback, h)
            rec = log.record
            r8, p8 = np.zeros(MAX_A, np.float32), np.ones(MAX_A, np.int32)
            r8[:A], p8[:A] = reward, possible
            rows["cur_group"].append(g), rows["cur_reward"].append(r8), rows["cur_possible"].append(p8)
            rows["cur_perf"].append(float(it.perf_records["family%d" % g][-1]))
            for key, name in (("cur_probs", "probability_lvl%d"), ("cur_best", "best_perf_lvl%d"),
                              ("cur_recent", "recent%d_perf_lvl%%d" % lookback)):
                rows[key].append([float(rec[name % h]) if h < G else 0.0 for h in range(MAX_G)])
        offsets.append(len(rows["cur_group"]))
        counts = [len(it.perf_records["family%d" % h]) for h in range(G)]
        print("curriculum A=%d G=%d lookback=%d: %d episodes, records per group %s, special %s"
              % (A, G, lookback, n, counts, special), flush=True)
        assert min(counts) > lookback and min(special.values()) > 0     # every ring filled and wrapped; every special kind met
    return dict(cur_agents=np.array([c[0] for c in CURRICULA], np.int32),
                cur_groups=np.array([c[1] for c in CURRICULA], np.int32),
                cur_lookback=np.array([c[2] for c in CURRICULA], np.int32), cur_offsets=np.array(offsets, np.int64),
                cur_group=np.array(rows["cur_group"], np.int32), cur_reward=np.array(rows["cur_reward"], np.float32),
                cur_possible=np.array(rows["cur_possible"], np.int32), cur_perf=np.array(rows["cur_perf"], np.float64),
                cur_probs=np.array(rows["cur_probs"], np.float64), cur_best=np.array(rows["cur_best"], np.float64),
                cur_recent=np.array(rows["cur_recent"], np.float64))


def main():
    import make_golden
    from make_golden_gae import write_npz
    from make_golden_schedule import FRACTIONS
    make_golden.import_reference()
    # env_factory imports the renderer for record_video (imageio is not installed; nothing here renders)
    import types
    graphics = types.ModuleType("safelife.render_graphics")
    graphics.render_file = lambda *a, **kw: None
    sys.modules["safelife.render_graphics"] = graphics
    from safelife.env_wrappers import MinPerformanceScheduler
    from safelife.safelife_game import CellTypes, SafeLifeGame
    from training import env_factory

    arrays = synthetic_levels(CellTypes, np.asarray(SafeLifeGame.default_points_table, np.int64))
    arrays.update(required_cases(SafeLifeGame, MinPerformanceScheduler, arrays, FRACTIONS))
    arrays.update(curriculum_cases(env_factory))
    out = os.path.join(HERE, "schedule_multi_cases.npz")
    write_npz(out, arrays)
    print("schedule_multi_cases: %d levels x %d fractions, %d curriculum episodes, %d bytes"
          % (len(arrays["req_level"]), len(FRACTIONS), len(arrays["cur_group"]), os.path.getsize(out)))
    assert os.path.getsize(out) < os.path.getsize(os.path.join(HERE, "schedule_cases.npz"))


if __name__ == "__main__":
    main()
