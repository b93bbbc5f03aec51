"""
Writes tests/golden/episode_log_multi_cases.npz: scripted MULTI-AGENT runs with what the REFERENCE's own ``SafeLifeLogger``
logged for them, for tests/test_episode_log_multi_host.py and tests/test_episode_log_multi_gpu.py.

Runs only in the build container (``python tests/golden/make_golden_episode_log_multi.py``), as make_golden_episode_log.py
does and with its stubs: a ``wandb`` whose ``.log()`` captures every scalar, games with ``title``, ``agent_names``,
``points_on_level_exit``, ``min_performance`` and array-valued ``initial_available_points()`` / ``required_points()``.
``SafeLifeLogWrapper`` does the step counting and decides when to log: B scripted envs of A agents are stepped in index
order against the one shared counter; an env's ``done`` is an array over its agents, an agent that finished early keeps its
flag, and the env is reset after the step on which all of them are done.  Inputs and the reference's outputs only are stored.

Every case ``c`` of ``cases`` has, with N episodes in log order, A agents and M distinct agent names ``c_names``,
    c_B, c_T, c_A, c_polyak
    inputs   c_env, c_step int32 [N] (which env's agents were all done on which step), c_done_step int32 [N,A] (the step on
             which each agent finished, <= c_step), c_length int32 [N,A], c_reward float32 [N,A], c_success uint8 [N,A],
             c_available, c_required int32 [N,A], c_exit_points int32 [N] (the stub game's), c_name_id int32 [N,A] (the
             agent's name in c_names), c_total float64 [N,2] (the episode's info['side_effects']['total'])
    logged   c_training_steps int64 [N]; c_reward_possible, c_reward_needed int64 [N,A] (``last_data``); c_score float64
             [N,A] and c_side_effects_frac float64 [N]: combined_score() as log_episode() calls it; c_scalars float64
             [N,M,4]: training/<name>-length, -reward, -success, -score as wandb saw them, and c_present bool [N,M] (was
             the name's key in that call); c_stats float64 [N,M,4] / c_counts int64 [N,M,4]: summary_stats and
             summary_counts after the episode (NaN: no such key yet)
             c_se_in_wandb bool [N]: did wandb see a training/side_effects key in that call (log_scalars hands it only
             what is real and np.isscalar); c_se_isscalar bool [N]: np.isscalar of the shape-(1,) fraction combined_score()
             returns; c_n_keys int32 [N]: the number of keys wandb saw (four per distinct name of the level,
             reward_frac_needed, and the two cumulative counters); c_se_summarised bool: is training/side_effects in
             summary_stats after the run
    run      c_run float64 [12]: rows, success, avg_length, side_effects, reward, score, std side_effects, std reward,
             std score, mean and std of the successful length, successes -- summarize_run_file over the run's JSON log and
             lines :727-740's own expressions
"""
import os
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference    # noqa: E402
from make_golden_episode_log import EDGES, INFS, NAN, StubWandb    # noqa: E402

QUANTITIES = ("length", "reward", "success", "score")


class StubGame(object):
    def __init__(self, ep):
        self.title, self.points_on_level_exit, self.min_performance = "level-%d" % ep["n"], int(ep["exit_points"]), 0.5
        self.agent_names = np.array(ep["names"])
        self._available, self._required = np.array(ep["available"]), np.array(ep["required"])

    def initial_available_points(self):
        return self._available.copy()       # (log_episode adds the exit's points in place)

    def required_points(self):
        return self._required.copy()


class ScriptedEnv(object):
    """A agents; every agent of the env's current episode is done from its own step on, and the step on which the last one
    finishes carries the episode's info."""

    def __init__(self, episodes, A, clock):
        self.episodes, self.A, self.clock, self.game, self.at = episodes, A, clock, None, 0

    def reset(self):
        return None

    def step(self, action):
        t = self.clock[0]
        reward = np.zeros(self.A, np.float32)
        if self.at >= len(self.episodes):
            return None, reward, np.zeros(self.A, bool), {}
        ep = self.episodes[self.at]
        done = np.array([t >= s for s in ep["done_step"]])
        if not done.all():
            return None, reward, done, {}
        assert t == ep["step"]
        self.at += 1
        self.game = StubGame(ep)
        info = {"length": np.array(ep["length"]), "reward": np.array(ep["reward"], np.float32),
                "success": np.array(ep["success"], bool),
                "side_effects": {"total": [float(ep["total"][0]), float(ep["total"][1])]}}
        return None, reward, done, {"episode": info}


def make_episodes(seed, B, T, A, p_end, success_rate, name_sets, specials):
    """Episodes in log order (step, then env).  `specials`: the single-agent generator's overrides, applied to ONE agent of
    the episode they land on (scalars go to agent n % A; `total` is the episode's)."""
    rng = np.random.default_rng(seed)
    eps, last_end = [], [-1] * B
    for t in range(T):
        for e in range(B):
            if t > last_end[e] and rng.random() < p_end:
                avail = rng.integers(0, 60, A)
                early = np.maximum(t - rng.integers(0, 4, A) * (rng.random(A) < 0.6), last_end[e] + 1)
                early[rng.integers(0, A)] = t
                eps.append(dict(env=e, step=t, done_step=[int(s) for s in early],
                                length=[int(v) for v in rng.integers(1, 1000, A)],
                                reward=[np.float32(rng.integers(-20, 80) + rng.integers(0, 4) * 0.25) for _ in range(A)],
                                success=[bool(rng.random() < success_rate) for _ in range(A)],
                                available=[int(v) for v in avail], exit_points=1,
                                required=[int(rng.integers(0, v + 1)) for v in avail],
                                names=list(name_sets[int(rng.integers(0, len(name_sets)))]),
                                total=[float(rng.random() * 3), float(rng.choice([0.0, 0.3, 0.999, 1.0, 2.5, 17.25]) if
                                                                      rng.random() < 0.5 else rng.random() * 6)]))
                last_end[e] = t
    at = np.linspace(3, len(eps) - 3, len(specials)).astype(int)
    for i, sp in zip(at, specials):
        a = int(i) % A
        for key, val in sp.items():
            if key in ("total", "exit_points"):
                eps[i][key] = val
            else:
                eps[i][key][a] = val
    for n, ep in enumerate(eps):
        ep["n"] = n
    return eps


AGENTS8 = ["agent%d" % k for k in range(8)]
CASES = {
    # two agents: the default names, a level with two agents of one name, a level with another name set
    "a2_polyak099": dict(seed=11, B=4, T=700, A=2, p_end=0.3, polyak=0.99, success_rate=0.6, specials=EDGES + INFS + EDGES,
                         name_sets=[["agent0", "agent1"], ["agent0", "agent1"], ["agent0", "agent0"], ["agent1", "scout"]]),
    "a1_polyak1": dict(seed=12, B=3, T=300, A=1, p_end=0.35, polyak=1.0, success_rate=0.5, specials=EDGES,
                       name_sets=[["agent0"], ["agent0"], ["solo"]]),
    "a3_polyak0": dict(seed=13, B=5, T=60, A=3, p_end=0.5, polyak=0.0, success_rate=0.5, specials=EDGES + INFS,
                       name_sets=[["agent0", "agent1", "agent2"], ["agent0", "agent0", "agent1"], ["agent2", "red", "red"]]),
    "a8_polyak099": dict(seed=14, B=2, T=200, A=8, p_end=0.4, polyak=0.99, success_rate=0.7, specials=EDGES + INFS,
                         name_sets=[AGENTS8, AGENTS8, ["p%d" % k for k in range(8)], AGENTS8[:4] + AGENTS8[:4]]),
    "a2_nosuccess": dict(seed=15, B=2, T=60, A=2, p_end=0.4, polyak=1.0, success_rate=0.0, specials=EDGES[:4],
                         name_sets=[["agent0", "agent1"]]),
}


def distinct_names(eps):
    names = []
    for ep in eps:
        for n in ep["names"]:
            if n not in names:
                names.append(n)
    return names


def run_case(L, cfg, logdir=None):
    eps = make_episodes(cfg["seed"], cfg["B"], cfg["T"], cfg["A"], cfg["p_end"], cfg["success_rate"], cfg["name_sets"],
                        cfg["specials"])
    names = distinct_names(eps)
    L.SafeLifeLogger.cumulative_stats = {}
    wandb = StubWandb()
    logger = L.SafeLifeLogger(logdir=logdir, episode_type="training", summary_writer=False, wandb=wandb,
                              summary_polyak=cfg["polyak"], video_name=None)
    clock = [0]
    envs = []
    for e in range(cfg["B"]):
        envs.append(L.SafeLifeLogWrapper(ScriptedEnv([ep for ep in eps if ep["env"] == e], cfg["A"], clock), logger=logger,
                                         record_history=False))
        envs[-1].reset()
    rows = []
    for t in range(cfg["T"]):
        clock[0] = t
        for env in envs:
            n_logged = len(wandb.logged)
            _, _, done, info = env.step(0)
            if not np.all(done):
                assert len(wandb.logged) == n_logged
                continue
            assert len(wandb.logged) == n_logged + 1
            w, ep = wandb.logged[-1], eps[len(rows)]
            present = [("training/%s-length" % name) in w for name in names]
            scalars = [[float(w["training/%s-%s" % (name, q)]) if here else NAN for q in QUANTITIES]
                       for name, here in zip(names, present)]
            stats = [[logger.summary_stats.get("training/%s-%s" % (name, q), NAN) for q in QUANTITIES] for name in names]
            counts = [[logger.summary_counts.get("training/%s-%s" % (name, q), 0) for q in QUANTITIES] for name in names]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                rp = np.array(ep["available"]) + ep["exit_points"]
                frac, score = L.combined_score({"reward_possible": rp, **info["episode"]})
            assert np.shape(frac) == (1,) and np.shape(score) == (cfg["A"],)
            rows.append(dict(training_steps=w["training/steps"], episodes=w["training/episodes"],
                             reward_possible=logger.last_data["reward_possible"], reward_needed=logger.last_data["reward_needed"],
                             agents=logger.last_data["agents"], score=score, side_effects_frac=float(frac[0]), scalars=scalars,
                             present=present, stats=stats, counts=counts, se_in_wandb="training/side_effects" in w,
                             se_isscalar=bool(np.isscalar(frac)), n_keys=len(w)))
            assert rows[-1]["agents"] == ep["names"]
            env.reset()
    assert len(rows) == len(eps) and [r["episodes"] for r in rows] == list(range(1, len(eps) + 1))
    se_summarised = "training/side_effects" in logger.summary_stats
    if logger._episode_log is not None:
        logger._episode_log.close()
    return eps, rows, names, se_summarised


def run_summary(L, logfile):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s = L.summarize_run_file(logfile)
        data = L.load_safelife_log(logfile)
        reward_frac = data["reward"] / np.maximum(data["reward_possible"], 1)
        length, success = data["length"], data["success"]
        clength = length.ravel()[success.ravel()]
        side_effects, score = L.combined_score(data, None)
        assert side_effects.shape == (len(length), 1) and score.shape == length.shape
        return np.array([len(length), s["success"], s["avg_length"], s["side_effects"], s["reward"], s["score"],
                         np.std(side_effects), np.std(reward_frac), np.std(score), np.average(clength), np.std(clength),
                         len(clength)], np.float64)


def main():
    import_reference()
    imageio = types.ModuleType("imageio")
    imageio.imread = lambda path: np.zeros((70, 70, 4), np.uint8)
    sys.modules["imageio"] = imageio
    from safelife import safelife_logger as L
    out = {"cases": np.array(sorted(CASES)), "quantities": np.array(QUANTITIES)}
    for name, cfg in sorted(CASES.items()):
        with tempfile.TemporaryDirectory() as tmp:
            eps, rows, names, se_summarised = run_case(L, cfg)
            eps2, rows2, _, _ = run_case(L, cfg, logdir=tmp)        # the same run once more, with the JSON log
            assert len(rows2) == len(rows) and eps2 == eps
            run = run_summary(L, os.path.join(tmp, "training-log.json"))
        for key in ("B", "T", "A", "polyak"):
            out["%s_%s" % (name, key)] = cfg[key]
        out[name + "_names"] = np.array(names)
        out[name + "_name_id"] = np.array([[names.index(n) for n in ep["names"]] for ep in eps], np.int32)
        for key, dtype in (("env", np.int32), ("step", np.int32), ("done_step", np.int32), ("length", np.int32),
                           ("reward", np.float32), ("success", np.uint8), ("available", np.int32), ("exit_points", np.int32),
                           ("required", np.int32), ("total", np.float64)):
            out["%s_%s" % (name, key)] = np.array([ep[key] for ep in eps], dtype)
        for key, dtype in (("training_steps", np.int64), ("reward_possible", np.int64), ("reward_needed", np.int64),
                           ("score", np.float64), ("side_effects_frac", np.float64), ("scalars", np.float64),
                           ("present", bool), ("stats", np.float64), ("counts", np.int64), ("se_in_wandb", bool),
                           ("se_isscalar", bool), ("n_keys", np.int32)):
            out["%s_%s" % (name, key)] = np.array([r[key] for r in rows], dtype)
        out[name + "_se_summarised"] = bool(se_summarised)
        out[name + "_run"] = run
        print(name, len(eps), "episodes,", len(names), "names; side_effects summarised:", se_summarised, "; run summary",
              run.tolist())
    path = os.path.join(HERE, "episode_log_multi_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
