"""
Writes tests/golden/episode_history_cases.npz: what the REFERENCE's own ``SafeLifeEnv`` + ``SafeLifeLogWrapper`` +
``SafeLifeLogger`` saved as episode histories, for tests/test_episode_history_host.py and tests/test_episode_history_gpu.py.

Runs only in the build container (``python tests/golden/make_golden_episode_history.py``).  Five envs play the committed 7x7
levels of ``trace_worked_7x7_exit`` and ``trace_worked_7x7_noop`` (no spawners: no generator takes part; two moves to the right
reach the first one's exit, so episodes end at different lengths and the envs drift apart), env e's k-th episode on level
``(e + k) % 2``, under scripted actions; the envs are stepped in index order against ONE logger
with ``logdir`` a temporary directory and a ``video_name``, and an env that ended an episode is reset at once.  ``imageio`` is
a placeholder and ``render_file`` a no-op, as in make_golden_render.py.  Inputs and the reference's outputs only are stored.

Every run ``r`` of ``runs`` has
    r_interval, r_time_limit   the logger's ``video_interval`` and the envs' ``time_limit``
    r_actions    int32 [S,5]   the actions, step by step
    r_env, r_length, r_level int32 [N]   the N episodes in log order (number 0 .. N-1): which env, how long, which level
    r_kept       int32 [M]     the episode numbers that got an ``.npz``
    r_board_<i>, r_goals_<i>  uint16 [length,7,7]   the saved stacks of kept episode number i
and ``levels`` names the traces whose ``level0_*`` arrays are the pool, in slot order.
"""
import glob
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference    # noqa: E402

LEVELS = ("worked_7x7_exit", "worked_7x7_noop")
B = 5
RUNS = {"interval1": dict(interval=1, time_limit=8, seed=11, episodes=20),
        "interval3": dict(interval=3, time_limit=11, seed=12, episodes=21)}


def level_data(name):
    with np.load(os.path.join(HERE, "trace_%s.npz" % name)) as d:
        return {k[len("level0_"):]: d[k] for k in d.files if k.startswith("level0_") and k != "level0_rng"}


def run(R, L, cfg):
    datas = [level_data(n) for n in LEVELS]
    rng = np.random.default_rng(cfg["seed"])
    L.SafeLifeLogger.cumulative_stats = {}
    episodes, actions = [], []
    with tempfile.TemporaryDirectory() as tmp:
        logger = L.SafeLifeLogger(logdir=tmp, episode_type="training", summary_writer=False, wandb=None,
                                  video_name="episode-{training_episodes}", video_interval=cfg["interval"])

        def games(e):
            k = 0
            while True:
                yield R.game.SafeLifeGame.loaddata(datas[(e + k) % len(datas)])
                k += 1
        envs = []
        for e in range(B):
            env = R.env.SafeLifeEnv(games(e), time_limit=cfg["time_limit"], view_shape=(15, 15))
            envs.append(L.SafeLifeLogWrapper(env, logger=logger))
            envs[-1].reset()
        played = [0] * B
        while len(episodes) < cfg["episodes"]:
            # half of the actions move right: towards the exit
            acts = rng.choice(9, B, p=[0.06, 0.1, 0.5, 0.1, 0.06, 0.06, 0.04, 0.04, 0.04]).astype(np.int32)
            actions.append(acts)
            for e, env in enumerate(envs):
                _, _, done, info = env.step(int(acts[e]))
                if done:
                    episodes.append((e, int(info["episode"]["length"]), (e + played[e]) % len(datas)))
                    played[e] += 1
                    env.reset()
        if logger._episode_log is not None:
            logger._episode_log.close()
        saved = {}
        for path in glob.glob(os.path.join(tmp, "episode-*.npz")):
            number = int(os.path.basename(path)[len("episode-"):-4]) - 1
            with np.load(path) as d:
                assert sorted(d.files) == ["board", "goals"]
                saved[number] = (d["board"].astype(np.uint16), d["goals"].astype(np.uint16))
    return np.array(actions, np.int32), episodes, saved


def main():
    R = import_reference()
    imageio = types.ModuleType("imageio")
    imageio.imread = lambda path: np.zeros((70, 70, 4), np.uint8)
    sys.modules["imageio"] = imageio
    from safelife import safelife_logger as L
    L.render_file = lambda *a, **kw: None
    out = {"runs": np.array(sorted(RUNS)), "levels": np.array(LEVELS)}
    for name, cfg in sorted(RUNS.items()):
        actions, episodes, saved = run(R, L, cfg)
        out[name + "_interval"], out[name + "_time_limit"] = cfg["interval"], cfg["time_limit"]
        out[name + "_actions"] = actions
        out[name + "_env"] = np.array([e for e, _, _ in episodes], np.int32)
        out[name + "_length"] = np.array([n for _, n, _ in episodes], np.int32)
        out[name + "_level"] = np.array([lv for _, _, lv in episodes], np.int32)
        kept = sorted(saved)
        assert kept == [i for i in range(len(episodes)) if i % cfg["interval"] == 0], kept
        out[name + "_kept"] = np.array(kept, np.int32)
        for i in kept:
            board, goals = saved[i]
            assert len(board) == len(goals) == episodes[i][1]
            out["%s_board_%d" % (name, i)], out["%s_goals_%d" % (name, i)] = board, goals
        print(name, len(actions), "steps,", len(episodes), "episodes, lengths", [n for _, n, _ in episodes], "kept", kept)
    path = os.path.join(HERE, "episode_history_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
