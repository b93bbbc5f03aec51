"""
Writes tests/golden/episode_log_cases.npz: scripted runs with what the REFERENCE's own ``SafeLifeLogger`` logged for them, for
tests/test_episode_log_host.py and tests/test_episode_log_gpu.py.

Runs only in the build container (``python tests/golden/make_golden_episode_log.py``).  The logger runs on the CPU with
``summary_writer=False`` and a stub ``wandb`` whose ``.log()`` captures every scalar; the games are stubs with ``title``,
``points_on_level_exit``, ``min_performance``, ``initial_available_points()`` and ``required_points()``; ``imageio`` is a
placeholder, as in make_golden_render.py.  ``SafeLifeLogWrapper`` does the step counting: B scripted envs are stepped in
index order, every wrapper against the one shared counter, and an env that ended an episode is reset at once.  The run
summary comes from a second logger that writes ``training-log.json`` to a temporary directory, ``summarize_run_file`` over
it (the five means) and lines :727-740's own expressions over ``load_safelife_log`` / ``combined_score`` (the standard
deviations and the successful length, which the reference only prints).  Inputs and the reference's outputs only are stored.

Every case ``c`` of ``cases`` has, with N episodes in log order,
    c_B, c_T, c_polyak
    inputs   c_env, c_step int32 [N] (which env ended an episode on which step), c_length int32, c_reward float32,
             c_success uint8, c_available, c_exit_points, c_required int32 (the stub game's), c_total float64 [N,2] (the
             episode's info['side_effects']['total'])
    logged   c_training_steps, c_reward_possible, c_reward_needed int64 [N]; c_scalars float64 [N,5]: training/side_effects,
             length, reward, success, score as wandb saw them; c_stats float64 [N,5] / c_counts int64 [N,5]: summary_stats
             and summary_counts after the episode (NaN: no such key yet)
    run      c_run float64 [12]: rows, success, avg_length, side_effects, reward, score, std side_effects, std reward,
             std score, mean and std of the successful length, successes
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

KEYS = ("side_effects", "length", "reward", "success", "score")


class StubGame(object):
    def __init__(self, title, available, exit_points, required):
        self.title, self.points_on_level_exit, self.min_performance = title, int(exit_points), 0.5
        self._available, self._required = int(available), int(required)

    def initial_available_points(self):
        return np.array([self._available])

    def required_points(self):
        return np.array([self._required])


class ScriptedEnv(object):
    """Ends an episode on the steps its script names, with the info the script holds."""

    def __init__(self, script, clock):
        self.script, self.clock, self.game = script, clock, None

    def reset(self):
        return None

    def step(self, action):
        ep = self.script.get(self.clock[0])
        if ep is None:
            return None, np.float32(0), False, {}
        self.game = StubGame("level-%d" % ep["n"], ep["available"], ep["exit_points"], ep["required"])
        info = {"length": int(ep["length"]), "reward": np.float32(ep["reward"]), "success": bool(ep["success"]),
                "side_effects": {"total": [float(ep["total"][0]), float(ep["total"][1])]}}
        return None, np.float32(0), True, {"episode": info}


class StubWandb(object):
    Video = type("Video", (), {})

    def __init__(self):
        self.logged = []

    def log(self, data):
        self.logged.append(dict(data))


def make_episodes(seed, B, T, p_end, success_rate, specials):
    """Episodes in log order (step, then env): random, with `specials` (dicts of overrides) dealt over the run."""
    rng = np.random.default_rng(seed)
    eps = []
    for t in range(T):
        for e in range(B):
            if rng.random() < p_end:
                avail = int(rng.integers(0, 60))
                eps.append(dict(env=e, step=t, length=int(rng.integers(1, 1000)),
                                reward=np.float32(rng.integers(-20, 80) + rng.integers(0, 4) * 0.25),
                                success=bool(rng.random() < success_rate), available=avail, exit_points=1,
                                required=int(rng.integers(0, avail + 1)),
                                total=[float(rng.random() * 3), float(rng.choice([0.0, 0.3, 0.999, 1.0, 2.5, 17.25]) if
                                                                      rng.random() < 0.5 else rng.random() * 6)]))
    at = np.linspace(3, len(eps) - 3, len(specials)).astype(int)
    for i, sp in zip(at, specials):
        eps[i].update(sp)
    for n, ep in enumerate(eps):
        ep["n"] = n
    return eps


NAN, INF = float("nan"), float("inf")
EDGES = [dict(available=0, exit_points=1), dict(available=0, exit_points=0),
         dict(reward=np.float32(-7.5)), dict(total=[0.7, 0.25]), dict(total=[0.7, 0.0]), dict(total=[0.0, 0.0]),
         dict(length=0), dict(length=1000), dict(length=1001), dict(total=[NAN, NAN])]
INFS = [dict(total=[INF, 2.0]), dict(total=[1.0, INF]), dict(total=[INF, INF]), dict(total=[NAN, 1.0])]
CASES = {
    "polyak099": dict(seed=1, B=4, T=2600, p_end=0.3, polyak=0.99, success_rate=0.6, specials=EDGES + INFS + EDGES),
    "polyak1": dict(seed=2, B=3, T=300, p_end=0.35, polyak=1.0, success_rate=0.5, specials=EDGES),
    "polyak0": dict(seed=3, B=5, T=40, p_end=0.5, polyak=0.0, success_rate=0.5, specials=EDGES + INFS),
    "nosuccess": dict(seed=4, B=2, T=60, p_end=0.4, polyak=1.0, success_rate=0.0, specials=EDGES[:4]),
}


def run_case(L, cfg, logdir=None):
    eps = make_episodes(cfg["seed"], cfg["B"], cfg["T"], cfg["p_end"], cfg["success_rate"], cfg["specials"])
    L.SafeLifeLogger.cumulative_stats = {}
    wandb = StubWandb()
    logger = L.SafeLifeLogger(logdir=logdir, episode_type="training", summary_writer=False, wandb=wandb,
                              summary_polyak=cfg["polyak"], video_name=None)
    clock = [0]
    envs = []
    for e in range(cfg["B"]):
        script = {ep["step"]: ep for ep in eps if ep["env"] == e}
        envs.append(L.SafeLifeLogWrapper(ScriptedEnv(script, clock), logger=logger, record_history=False))
        envs[-1].reset()
    rows = []
    for t in range(cfg["T"]):
        clock[0] = t
        for env in envs:
            n_logged = len(wandb.logged)
            _, _, done, _ = env.step(0)
            if done:
                assert len(wandb.logged) == n_logged + 1
                w = wandb.logged[-1]
                stats = [logger.summary_stats.get("training/" + k, NAN) for k in KEYS]
                counts = [logger.summary_counts.get("training/" + k, 0) for k in KEYS]
                rows.append(dict(training_steps=w["training/steps"], episodes=w["training/episodes"],
                                 reward_possible=logger.last_data["reward_possible"],
                                 reward_needed=logger.last_data["reward_needed"],
                                 scalars=[float(w["training/" + k]) for k in KEYS], stats=stats, counts=counts))
                env.reset()
    assert len(rows) == len(eps) and [r["episodes"] for r in rows] == list(range(1, len(eps) + 1))
    if logger._episode_log is not None:
        logger._episode_log.close()
    return eps, rows


def run_summary(L, logfile):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s = L.summarize_run_file(logfile)
        data = L.load_safelife_log(logfile)
        reward_frac = data["reward"] / np.maximum(data["reward_possible"], 1)
        length, success = data["length"], data["success"]
        clength = length.ravel()[success.ravel()]
        side_effects, score = L.combined_score(data, None)
        return np.array([len(length), s["success"], s["avg_length"], s["side_effects"], s["reward"], s["score"],
                         np.std(side_effects), np.std(reward_frac), np.std(score), np.average(clength), np.std(clength),
                         len(clength)], np.float64)


def main():
    import_reference()
    imageio = types.ModuleType("imageio")
    imageio.imread = lambda path: np.zeros((70, 70, 4), np.uint8)
    sys.modules["imageio"] = imageio
    from safelife import safelife_logger as L
    out = {"cases": np.array(sorted(CASES)), "keys": np.array(KEYS)}
    for name, cfg in sorted(CASES.items()):
        with tempfile.TemporaryDirectory() as tmp:
            eps, rows = run_case(L, cfg)
            eps2, rows2 = run_case(L, cfg, logdir=tmp)      # the same run once more, with the JSON log
            assert len(rows2) == len(rows) and eps2 == eps
            run = run_summary(L, os.path.join(tmp, "training-log.json"))
        out[name + "_B"], out[name + "_T"], out[name + "_polyak"] = cfg["B"], cfg["T"], cfg["polyak"]
        for key, dtype in (("env", np.int32), ("step", np.int32), ("length", np.int32), ("reward", np.float32),
                           ("success", np.uint8), ("available", np.int32), ("exit_points", np.int32),
                           ("required", np.int32), ("total", np.float64)):
            out["%s_%s" % (name, key)] = np.array([ep[key] for ep in eps], dtype)
        for key, dtype in (("training_steps", np.int64), ("reward_possible", np.int64), ("reward_needed", np.int64),
                           ("scalars", np.float64), ("stats", np.float64), ("counts", np.int64)):
            out["%s_%s" % (name, key)] = np.array([r[key] for r in rows], dtype)
        out[name + "_run"] = run
        print(name, len(eps), "episodes; run summary", run.tolist())
    path = os.path.join(HERE, "episode_log_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
