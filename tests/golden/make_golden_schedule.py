#!/usr/bin/env python3
"""
Writes tests/golden/schedule_cases.npz by RUNNING THE REFERENCE on the CPU: what tests/schedule_ref.py and the level
schedule kernels (csrc/sl_schedule.hip) are held to.

    python tests/golden/make_golden_schedule.py

Runs where make_golden.py runs (it needs the reference's Python, loaded through make_golden.import_reference(), and scipy).

  lin_*   training/env_factory.py LinearSchedule (UnivariateSpline k=1, s=0, ext='const') with a stub logger:
          lin_t / lin_y the knots of every schedule laid end to end (lin_knots: offsets), lin_x the training steps
          asked for (lin_offsets) -- both ends, every knot, points between and outside -- and lin_value what it returned.
  req_*   MinPerformanceScheduler.reset() (env_wrappers.py:142-145) on the reference's SafeLifeGame of every level of the
          fixtures pool_prune_still_25 and pool_append_spawn_25 (req_pool 0 / 1, req_level), for every fraction of
          req_fraction: req_available = initial_available_points()[0], req_min_performance the level's own value,
          req_points [levels, fractions] = required_points()[0] after the reset.
  cur_*   CurricularLevelIterator.get_next_parameters (env_factory.py:104-146), the object built without its file loading
          and fed one scripted episode at a time through a stub logger.  Per case i (cur_groups, cur_lookback): episodes
          [cur_offsets[i], cur_offsets[i+1]) with cur_group (whose file the episode was), cur_reward float32 and
          cur_possible int32 (what safelife_logger.py:286-300 logs as reward and reward_possible); cur_probs [episode, 8]
          the probability_lvl* it logged after that episode (columns past the case's groups are 0), cur_progress the
          normalised_progress_lvl*, cur_best / cur_recent the best_perf_lvl* / recent<lookback>_perf_lvl*.
          Performances carry a trend plus noise: with all records of a window equal the reference's polyfit returns
          rounding noise that the division by `scale` blows up (a degenerate input), so the script asserts that no window
          the reference fits is constant.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

LINEAR = (([5e5, 2e6], [0.001, 1.0]),           # env.exit_difficulty
          ([1e5, 1.5e6], [0.1, 1.0]),           # env.task_switch
          ([1e6, 2e6], [0.0, 1.0]),             # side_effect.schedule
          ([0.0, 10.0, 30.0, 31.0], [1.0, 0.0, 5.0, 4.5]))
FRACTIONS = (0.0, 0.001, 0.25, 0.5, 1.0 / 3.0, 0.999, 1.0, 1.0 - 2.0 ** -53, 1.5)
CURRICULA = ((2, 100, 800), (3, 100, 1300), (2, 5, 200), (3, 5, 300))       # groups, lookback, episodes


def linear_cases(LinearSchedule):
    class Logger(object):
        cumulative_stats = {"training_steps": 0}
    out = {k: [] for k in ("lin_t", "lin_y", "lin_x", "lin_value")}
    knots, offsets = [0], [0]
    for t, y in LINEAR:
        log = Logger()
        sched = LinearSchedule(log, t=t, y=y)
        xs = [t[0] - 1e9, t[0] - 1.0, t[-1] + 1.0, t[-1] + 1e9, 0.0]
        for a, b in zip(t, t[1:]):
            xs += [a, b, (a + b) / 2, a + (b - a) / 3, a + (b - a) * 0.999, np.nextafter(a, b), np.nextafter(b, a)]
        xs += np.random.default_rng(5).uniform(t[0], t[-1], 20).tolist()
        for x in xs:
            log.cumulative_stats = {"training_steps": x}
            out["lin_x"].append(x)
            out["lin_value"].append(float(sched()))
        out["lin_t"] += list(t)
        out["lin_y"] += list(y)
        knots.append(len(out["lin_t"]))
        offsets.append(len(out["lin_x"]))
    arrays = {k: np.array(v, np.float64) for k, v in out.items()}
    arrays["lin_knots"], arrays["lin_offsets"] = np.array(knots, np.int64), np.array(offsets, np.int64)
    return arrays


def required_cases(SafeLifeGame, MinPerformanceScheduler):
    class Env(object):
        def __init__(self, game):
            self.game = game

        def reset(self):
            return None
    rows = {k: [] for k in ("req_pool", "req_level", "req_available", "req_min_performance", "req_points")}
    for p, name in enumerate(("prune_still_25", "append_spawn_25")):
        with np.load(os.path.join(HERE, "pool_%s.npz" % name)) as d:
            for k in range(int(d["n_levels"])):
                data = dict(board=d["board"][k], goals=d["goals"][k], agent_locs=d["agent_locs"][k],
                            spawn_prob=d["spawn_prob"][k], min_performance=d["min_performance"][k],
                            points_table=d["points_table"][k])
                points = []
                for f in FRACTIONS:
                    game = SafeLifeGame.loaddata(data, auto_cls=False)
                    assert int(game.required_points()[0]) == int(d["required_points"][k])
                    MinPerformanceScheduler(Env(game), min_performance_fraction=f).reset()
                    points.append(int(game.required_points()[0]))
                rows["req_pool"].append(p), rows["req_level"].append(k)
                rows["req_available"].append(int(game.initial_available_points()[0]))
                rows["req_min_performance"].append(float(d["min_performance"][k]))
                rows["req_points"].append(points)
    return dict(req_pool=np.array(rows["req_pool"], np.int32), req_level=np.array(rows["req_level"], np.int32),
                req_available=np.array(rows["req_available"], np.int32),
                req_min_performance=np.array(rows["req_min_performance"], np.float64),
                req_points=np.array(rows["req_points"], np.int32), req_fraction=np.array(FRACTIONS, np.float64))


def scripted_episodes(rng, G, lookback, n):
    """(group, reward float32, reward_possible int32) per episode: each group's performance follows its own trend (one
    rises, one falls, one stalls and then rises) plus noise; a few episodes have reward_possible 0 (a NaN and an inf
    ratio) or a negative reward."""
    weights = np.array([0.5, 0.3, 0.2][:G])
    weights = weights / weights.sum()
    seen = np.zeros(G, np.int64)
    out = []
    for k in range(n):
        g = int(rng.choice(G, p=weights))
        i = seen[g]
        seen[g] += 1
        span = float(max(6 * lookback, 40))
        trend = (0.1 + 0.7 * i / span, 0.6 - 0.4 * i / span, 0.3 + 0.5 * max(0.0, i / span - 0.5))[g]
        perf = trend + rng.normal(0.0, 0.05)
        possible = int(rng.integers(20, 90))
        reward = np.float32(round(perf * possible))
        if k % 97 == 41:
            possible, reward = 0, np.float32(0.0)               # 0 / 0
        elif k % 97 == 77:
            possible = 0                                         # x / 0
        elif k % 53 == 17:
            reward = np.float32(-3.0)
        out.append((g, reward, possible))
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

    rows = {k: [] for k in ("cur_group", "cur_reward", "cur_possible", "cur_probs", "cur_progress", "cur_best",
                            "cur_recent")}
    offsets = [0]
    rng = np.random.default_rng(20261019)
    np.random.seed(7)                                          # (get_next_parameters draws its choice from numpy's global)
    for G, lookback, n in CURRICULA:
        log = Logger()
        it = Iterator(G, lookback, log)
        for g, reward, possible in scripted_episodes(rng, G, lookback, n):
            log.last_data = {"reward": float(reward), "reward_possible": int(possible)}
            log.last_game = Game()
            log.last_game.file_name = "family%d" % g
            with np.errstate(all="ignore"):
                it.get_next_parameters()
            for h in range(G):                                 # the script's own inputs: no window the fit sees is constant
                rec = it.perf_records["family%d" % h]
                assert len(rec) < lookback or len(set(rec[-lookback:])) > 1, (G, lookback, h)
            rec = log.record
            rows["cur_group"].append(g), rows["cur_reward"].append(reward), rows["cur_possible"].append(possible)
            for key, name in (("cur_probs", "probability_lvl%d"), ("cur_progress", "normalised_progress_lvl%d"),
                              ("cur_best", "best_perf_lvl%d"), ("cur_recent", "recent%d_perf_lvl%%d" % lookback)):
                rows[key].append([float(rec[name % h]) if h < G else 0.0 for h in range(8)])
        offsets.append(len(rows["cur_group"]))
        counts = [len(it.perf_records["family%d" % h]) for h in range(G)]
        print("curriculum G=%d lookback=%d: %d episodes, records per group %s" % (G, lookback, n, counts), flush=True)
        assert min(counts) > 2 * lookback                      # every ring wraps more than twice
    return dict(cur_groups=np.array([c[0] for c in CURRICULA], np.int32),
                cur_lookback=np.array([c[1] for c in CURRICULA], np.int32), cur_offsets=np.array(offsets, np.int64),
                cur_group=np.array(rows["cur_group"], np.int32), cur_reward=np.array(rows["cur_reward"], np.float32),
                cur_possible=np.array(rows["cur_possible"], np.int32), cur_probs=np.array(rows["cur_probs"], np.float64),
                cur_progress=np.array(rows["cur_progress"], np.float64), cur_best=np.array(rows["cur_best"], np.float64),
                cur_recent=np.array(rows["cur_recent"], np.float64))


def main():
    import make_golden
    from make_golden_gae import write_npz
    make_golden.import_reference()
    # env_factory imports the renderer for record_video (imageio is not installed; nothing here renders)
    import types
    graphics = types.ModuleType("safelife.render_graphics")
    graphics.render_file = lambda *a, **kw: None
    sys.modules["safelife.render_graphics"] = graphics
    from safelife.env_wrappers import MinPerformanceScheduler
    from safelife.safelife_game import SafeLifeGame
    from training import env_factory

    arrays = {}
    arrays.update(linear_cases(env_factory.LinearSchedule))
    arrays.update(required_cases(SafeLifeGame, MinPerformanceScheduler))
    arrays.update(curriculum_cases(env_factory))
    out = os.path.join(HERE, "schedule_cases.npz")
    write_npz(out, arrays)
    print("schedule_cases: %d schedule values, %d levels x %d fractions, %d curriculum episodes, %d bytes"
          % (len(arrays["lin_x"]), len(arrays["req_level"]), len(FRACTIONS), len(arrays["cur_group"]),
             os.path.getsize(out)))


if __name__ == "__main__":
    main()
