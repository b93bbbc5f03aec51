"""
Writes tests/golden/episode_run_cases.npz: what the REFERENCE's own ``BaseAlgo.run_episodes`` (training/base_algo.py:278-318)
plays and logs over scripted stub envs, for tests/test_episode_run_host.py.

Runs only in the build container (``python tests/golden/make_golden_episode_run.py``).  The envs are stubs that share ONE
iterator of numbered stub levels, as the reference's evaluation envs share their level iterator; an episode's length, reward,
success, available points and side-effect totals are functions of the level number alone (the tables below, stored with the
cases).  Every env is wrapped in the reference's ``SafeLifeLogWrapper`` around one ``SafeLifeLogger(episode_type=
"benchmark")`` with the stub ``wandb`` of make_golden_episode_log.py; ``take_one_step`` is ``obs_for_envs`` / ``act_on_envs``
with action 0.  Inputs and the reference's outputs only are stored.

Every case ``c`` of ``cases`` has
    inputs   c_B (envs), c_N (num_episodes handed over; -1: None, the reference then takes the env count), c_L (levels in the
             list the iterator cycles over), c_parity (1: a parity case, B <= N; 0: more envs than episodes -- recorded so that
             the documented difference is a recorded fact)
    logged   c_levels int32 [n]: the level numbers of the episodes the logger logged, in log order; c_handed: levels the
             iterator handed out in all; c_steps: calls of take_one_step; c_stats float64 [5]: summary_stats after
             log_summary(), benchmark/side_effects, length, reward, success, score; c_counts int64 [5]
and the tables of the stub levels: level_length int32 [LMAX], level_reward float32, level_success uint8, level_available
int32, level_total float64 [LMAX, 2].
"""
import itertools
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference    # noqa: E402
from make_golden_episode_log import KEYS, StubGame, StubWandb    # noqa: E402

LMAX = 300
_n = np.arange(LMAX)
LEVEL_LENGTH = (1 + (_n * 7) % 11 + (_n % 3) * 4).astype(np.int32)
LEVEL_REWARD = ((_n * 5) % 9 - 2 + 0.25 * (_n % 4)).astype(np.float32)
LEVEL_SUCCESS = (_n % 3 != 0).astype(np.uint8)
LEVEL_AVAILABLE = (10 + _n % 13).astype(np.int32)
LEVEL_TOTAL = np.stack([(_n % 5) * 0.3, 0.5 + (_n % 4)], axis=1).astype(np.float64)


class StubEvalEnv(object):
    """One episode per level the shared iterator hands out; done after the level's length."""
    single_agent = True

    def __init__(self, levels, handed):
        self.levels, self.handed, self.game = levels, handed, None

    def reset(self):
        self.level = next(self.levels)
        self.handed[0] += 1
        self.count = 0
        n = self.level
        self.game = StubGame("level-%d" % n, LEVEL_AVAILABLE[n], 1, 0)
        return np.zeros(1)

    def step(self, action):
        self.count += 1
        n = self.level
        if self.count < LEVEL_LENGTH[n]:
            return np.zeros(1), np.float32(0), False, {}
        info = {"length": int(self.count), "reward": np.float32(LEVEL_REWARD[n]), "success": bool(LEVEL_SUCCESS[n]),
                "side_effects": {"total": LEVEL_TOTAL[n].tolist()}}
        return np.zeros(1), np.float32(0), True, {"episode": info}


def cases():
    out = {}
    for B in (1, 5, 20, 64):
        for tag, N in (("eq", B), ("plus1", B + 1), ("mult", 3 * B), ("nonmult", 3 * B - 1 if B > 1 else 4), ("none", -1)):
            for L in (7, LMAX):
                out["b%d_%s_l%d" % (B, tag, L)] = dict(B=B, N=N, L=L, parity=1)
    out["more_envs_than_episodes"] = dict(B=20, N=7, L=LMAX, parity=0)
    return out


def run_case(L, base_algo, cfg):
    L.SafeLifeLogger.cumulative_stats = {}
    wandb = StubWandb()
    logger = L.SafeLifeLogger(logdir=None, episode_type="benchmark", summary_writer=False, wandb=wandb, video_name=None)
    logged = []
    log_episode = logger.log_episode

    def spy(game, info={}, history=None):
        logged.append(int(game.title.split("-")[1]))
        return log_episode(game, info, history)

    logger.log_episode = spy
    handed = [0]
    levels = itertools.cycle(range(cfg["L"]))
    envs = [L.SafeLifeLogWrapper(StubEvalEnv(levels, handed), logger=logger, record_history=False) for _ in range(cfg["B"])]

    class Algo(base_algo.BaseAlgo):
        steps_taken = 0

        @base_algo.named_output("obs actions rewards done next_obs agent_ids")
        def take_one_step(self, envs):
            obs, agent_ids = self.obs_for_envs(envs)
            actions = np.zeros(len(obs), np.int64)
            next_obs, rewards, done = self.act_on_envs(envs, actions)
            self.steps_taken += 1
            return obs, actions, rewards, done, next_obs, agent_ids

    algo = Algo()
    algo.run_episodes(envs, num_episodes=None if cfg["N"] < 0 else cfg["N"])
    stats = [logger.summary_stats.get("benchmark/" + k, float("nan")) for k in KEYS]
    counts = [logger.summary_counts.get("benchmark/" + k, 0) for k in KEYS]
    return dict(levels=np.array(logged, np.int32), handed=handed[0], steps=algo.steps_taken,
                stats=np.array(stats, np.float64), counts=np.array(counts, np.int64))


def main():
    import_reference()
    imageio = types.ModuleType("imageio")
    imageio.imread = lambda path: np.zeros((70, 70, 4), np.uint8)
    sys.modules["imageio"] = imageio
    from safelife import safelife_logger as L
    from training import base_algo
    all_cases = cases()
    out = {"cases": np.array(sorted(all_cases)), "keys": np.array(KEYS), "level_length": LEVEL_LENGTH,
           "level_reward": LEVEL_REWARD, "level_success": LEVEL_SUCCESS, "level_available": LEVEL_AVAILABLE,
           "level_total": LEVEL_TOTAL}
    for name, cfg in sorted(all_cases.items()):
        res = run_case(L, base_algo, cfg)
        for k in ("B", "N", "L", "parity"):
            out["%s_%s" % (name, k)] = cfg[k]
        for k, v in res.items():
            out["%s_%s" % (name, k)] = v
        print(name, cfg, "logged", len(res["levels"]), "handed", res["handed"], "steps", res["steps"])
    path = os.path.join(HERE, "episode_run_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
