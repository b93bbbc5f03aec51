"""
Writes tests/golden/episode_history_multi_cases.npz: what the REFERENCE's own ``SafeLifeEnv(single_agent=False)`` +
``SafeLifeLogWrapper`` + ``SafeLifeLogger`` saved as episode histories of envs with several agents, for
tests/test_episode_history_multi_host.py and tests/test_episode_history_multi_gpu.py.

Runs only in the build container (``python tests/golden/make_golden_episode_history_multi.py``).  Every run has four envs of
A agents on two 7x7 levels built here (no spawners: no generator takes part).  On level 0 every row that holds agents has
an exit at its right end and every agent may leave (min_performance -1), so agents that walk right leave one after the
other, the one in front first; level 1 is the same board without exits, so its episodes end at the time limit -- and two
envs that start one together end on ONE step.  Env e's k-th episode is on level ``(e + k) % 2``; the envs are stepped in index
order against ONE logger with ``logdir`` a temporary directory and a ``video_name``; an env whose agents are ALL done is
reset at once, and an agent that is done is fed action 0 (training/base_algo.py:216-219).  ``imageio`` is a placeholder and
``render_file`` a no-op, as in make_golden_episode_history.py.  Inputs and the reference's outputs only are stored.

Every run ``r`` of ``runs`` has
    r_agents, r_interval, r_time_limit
    r_lv_<key>                  the two levels, stacked: what ``Level.from_data`` takes (board, goals, agent_locs, ...)
    r_actions    int32 [S,4,A]  the actions, step by step
    r_env, r_level, r_num_steps int32 [N], r_times_up bool [N]      the N episodes in log order (number 0 .. N-1)
    r_lengths    int32 [N,A], r_success bool [N,A]                  info['episode'] of the step that ended each
    r_kept       int32 [M]      the episode numbers that got an ``.npz``
    r_board_<i>, r_goals_<i>  uint16 [num_steps,7,7]   the saved stacks of kept episode number i
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

import make_golden                              # noqa: E402
from make_golden import import_reference        # noqa: E402
from make_golden_multi_step import LEVEL_EXIT, WALL, RED, agent_cell, agent_tables    # noqa: E402

B, H, W = 4, 7, 7
RUNS = {"a2_interval1": dict(A=2, interval=1, time_limit=9, seed=21, episodes=14),
        "a2_interval3": dict(A=2, interval=3, time_limit=7, seed=22, episodes=16),
        "a3_interval3": dict(A=3, interval=3, time_limit=10, seed=23, episodes=13),
        "a8_interval1": dict(A=8, interval=1, time_limit=12, seed=24, episodes=10)}
# where the agents start, (row, col), in index order: agent 0 stands in front of agent 1 in one row, so it tends to leave first
STARTS = [(1, 3), (1, 1), (3, 2), (3, 0), (5, 3), (5, 1), (2, 4), (4, 2)]


def level_datas(Game, A):
    datas = []
    for k in range(2):
        board, goals = np.zeros((H, W), np.uint16), np.zeros((H, W), np.uint16)
        board[0, 0] = board[6, 6] = WALL
        board[6, 2] = 1 | 8 | RED                       # a still life cell apart from everyone: the boards are not empty
        goals[0, 3] = RED
        locs = np.array(STARTS[:A], np.int64)
        for a in range(A):
            board[tuple(locs[a])] = agent_cell(a)
        if k == 0:
            for row in sorted(set(int(r) for r, _ in locs)):
                board[row, 6] = LEVEL_EXIT
        g = Game(board_size=(H, W))
        g.board, g.goals, g.agent_locs = board, goals, locs
        g.min_performance, g.spawn_prob = -1, 0.0
        g.points_table = agent_tables(Game.default_points_table, A)
        g.agent_names = np.array(["agent-%d" % i for i in range(A)])       # (the logger names its scalars by them)
        g.update_exit_locs()
        datas.append(g.serialize())
    return datas


def run(R, L, cfg):
    Game = R.game.SafeLifeGame
    A = cfg["A"]
    datas = level_datas(Game, A)
    rng = np.random.default_rng(cfg["seed"])
    L.SafeLifeLogger.cumulative_stats = {}
    episodes, actions = [], []
    with tempfile.TemporaryDirectory() as tmp:
        logger = L.SafeLifeLogger(logdir=tmp, episode_type="training", summary_writer=False, wandb=None,
                                  video_name="episode-{training_episodes}", video_interval=cfg["interval"])

        def games(e):
            k = 0
            while True:
                yield make_golden.seeded(Game.loaddata(datas[(e + k) % 2]), 100 * e + k)
                k += 1
        envs = []
        for e in range(B):
            env = R.env.SafeLifeEnv(games(e), single_agent=False, time_limit=cfg["time_limit"], view_shape=(5, 5))
            envs.append(L.SafeLifeLogWrapper(env, logger=logger))
            envs[-1].reset()
        played, done_now = [0] * B, np.zeros((B, A), bool)
        while len(episodes) < cfg["episodes"]:
            # two of three actions move right, towards the exits; an agent that is done takes 0
            acts = rng.choice(9, (B, A), p=[0.06, 0.06, 0.68, 0.06, 0.06, 0.02, 0.02, 0.02, 0.02]).astype(np.int32)
            acts[done_now] = 0
            actions.append(acts)
            for e, env in enumerate(envs):
                _, _, done, info = env.step(acts[e].astype(np.int64))
                done_now[e] = done
                if np.all(done):
                    ep = info["episode"]
                    episodes.append(dict(env=e, level=(e + played[e]) % 2, num_steps=int(env.game.num_steps),
                                         times_up=bool(info["times_up"]), lengths=np.array(ep["length"], np.int32),
                                         success=np.array(ep["success"], bool)))
                    played[e] += 1
                    env.reset()
                    done_now[e] = False
        if logger._episode_log is not None:
            logger._episode_log.close()
        saved = {}
        for path in glob.glob(os.path.join(tmp, "episode-*.npz")):
            number = int(os.path.basename(path)[len("episode-"):-4]) - 1
            with np.load(path) as d:
                assert sorted(d.files) == ["board", "goals"]
                saved[number] = (d["board"].astype(np.uint16), d["goals"].astype(np.uint16))
    levels = [make_golden.level_record(Game.loaddata(d)) for d in datas]
    return np.array(actions, np.int32), episodes, saved, levels


def check_events(name, cfg, actions, episodes):
    """What the stored episodes must show (asserted on the reference's output)."""
    A = cfg["A"]
    lengths = np.array([ep["lengths"] for ep in episodes])
    steps = np.array([ep["num_steps"] for ep in episodes])
    assert (lengths.max(axis=1) == steps).all(), "the agent that finished last was active on every step"
    spread = lengths.max(axis=1) - lengths.min(axis=1)
    assert (spread > 0).sum() >= 3, (name, "agents that finish on different steps")
    assert (spread >= 3).any(), (name, "an agent that leaves while another plays on for several frames")
    assert (lengths[:, 0] < steps).sum() >= 2, (name, "agent 0 is not always the last")
    limit = [ep for ep in episodes if ep["times_up"] and ep["success"].any() and not ep["success"].all()]
    assert limit, (name, "an episode ended by the time limit with one agent gone and one active")
    # the step every episode ended on: the envs are stepped in lockstep
    ends, clock = [], [0] * B
    for ep in episodes:
        clock[ep["env"]] += ep["num_steps"]
        ends.append(clock[ep["env"]])
    assert len(set(ends)) < len(ends), (name, "two envs that end on one step")
    assert any(ep["success"][1:].any() for ep in episodes), (name, "success that agent 0 alone does not tell")
    assert len(actions) >= max(ends) and A == lengths.shape[1]


def main():
    R = import_reference()
    imageio = types.ModuleType("imageio")
    imageio.imread = lambda path: np.zeros((70, 70, 4), np.uint8)
    sys.modules["imageio"] = imageio
    from safelife import safelife_logger as L
    L.render_file = lambda *a, **kw: None
    out = {"runs": np.array(sorted(RUNS))}
    for name, cfg in sorted(RUNS.items()):
        actions, episodes, saved, levels = run(R, L, cfg)
        check_events(name, cfg, actions, episodes)
        out[name + "_agents"], out[name + "_interval"], out[name + "_time_limit"] = cfg["A"], cfg["interval"], cfg["time_limit"]
        for k in levels[0]:
            out["%s_lv_%s" % (name, k)] = np.stack([np.asarray(lv[k]) for lv in levels])
        out[name + "_actions"] = actions
        for k, dt in (("env", np.int32), ("level", np.int32), ("num_steps", np.int32), ("times_up", bool),
                      ("lengths", np.int32), ("success", bool)):
            out["%s_%s" % (name, k)] = np.array([ep[k] for ep in episodes], dt)
        kept = sorted(saved)
        assert kept == [i for i in range(len(episodes)) if i % cfg["interval"] == 0], kept
        out[name + "_kept"] = np.array(kept, np.int32)
        for i in kept:
            board, goals = saved[i]
            assert len(board) == len(goals) == episodes[i]["num_steps"]
            out["%s_board_%d" % (name, i)], out["%s_goals_%d" % (name, i)] = board, goals
        print(name, len(actions), "steps,", len(episodes), "episodes, lengths",
              [ep["lengths"].tolist() for ep in episodes], "kept", kept)
    path = os.path.join(HERE, "episode_history_multi_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
