"""GPU suite: the fused step's epilogue -- everything a wave takes out of LDS behind the end barrier (the hand-over word,
the goals' dirty flag, generator words, the records' copy, the goal-word cache's look at goals_static, the span chunks)
comes in one batch of reads behind one wait, and a workgroup that reloads a level fetches the batch again behind the
reload.  Bit for bit against the oracle after EVERY step of 7 steps at time_limit = 3: steps 2 and 5 end every episode, so
reloading workgroups take the read-again path and the steps behind them run without cached goal words.

Shapes are the smallest at which a chunk mask, a leftover-cell tail or a group of chunks changes:
  25x25  625 chunks in a full workgroup of 8 boards (the third slot is live for 113 threads); a last workgroup of 1, 3 or
         7 boards leaves 1, 3 and 3 cells behind its last whole chunk       B = 1, 3, 8, 9, 15
  26x26  odd board counts leave 4 cells                                     B = 9
  10x10  24 boards per workgroup, 12.5 chunks per board                     B = 25
  64x64  swizzled image, 8 chunks per lane in two groups                    B = 1, 4, 5
  32x32  the other swizzle                                                  B = 5
Variants: the plain step without observation (the headline's kernel, goal-word cache and all), a spawner pool (the generator
words written back are the point), the training wrappers with the inaction baseline (second span, second generator), the
step with observation, a 3-step rollout launch (plain and with the wrappers); reset() with a mask and an
observation-only launch at 25x25 and 64x64; the plain 25x25 case through the library's queues in each fence mode.
"""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

STEPS, TIME_LIMIT = 7, 3
STATE = ("board", "goals", "rng", "agent_loc", "num_steps", "episode_idx", "level_idx", "exit_locs")
RECORDS = ("reward", "done", "success", "times_up", "episode_reward", "episode_length")
WRAPPERS = dict(movement_bonus=0.1, movement_bonus_power=1e-100, movement_bonus_period=4, as_penalty=True,
                exit_bonus=0.5, penalty_coef=0.3, ignore_reward_cells=False)
SHAPES = ((25, 1), (25, 3), (25, 8), (25, 9), (25, 15), (26, 9), (10, 25), (64, 1), (64, 4), (64, 5), (32, 5))
VARIANTS = {
    "plain":   dict(with_obs=False),
    "spawn":   dict(with_obs=False, spawn=True),
    "wrap":    dict(with_obs=False, spawn=True, wrap=True),
    "obs":     dict(with_obs=True),
    "rollout": dict(with_obs=False, spawn=True, rollout=True),
    "wrap_rollout": dict(with_obs=False, spawn=True, wrap=True, rollout=True),
}

#            still pool         spawner pool
_FIXTURE = {25: ("prune_still_25", "append_spawn_25"), 26: ("append_still_26",) * 2, 10: ("prune_still_25", "append_spawn_25"),
            64: ("navigation_64",) * 2, 32: ("navigation_64",) * 2}
_loaded, _pools = {}, {}


def _pool(H, spawn):
    """Three levels of H x H from the fixtures (a window around the agent where the fixture is larger: the boards wrap, any
    window is a board), two exits each, spawners in every level or in none.  Built once per (shape, kind) and shared."""
    from safelife_amd.cell_types import CellTypes as CT
    from safelife_amd.levels import Level, LevelPool
    if (H, spawn) in _pools:
        return _pools[H, spawn]
    name = _FIXTURE[H][1 if spawn else 0]
    if name not in _loaded:
        _loaded[name] = util.pool_from_fixture(name, util.oracle_counts, n=3)[0].levels
    levels = []
    for k, src in enumerate(_loaded[name]):
        board, goals = src.board.copy(), src.goals.copy()
        ay, ax = (int(v) for v in src.agent_locs[0])
        if H < board.shape[0]:
            rows, cols = (np.arange(H) + ay - H // 2) % board.shape[0], (np.arange(H) + ax - H // 2) % board.shape[1]
            board, goals = board[np.ix_(rows, cols)], goals[np.ix_(rows, cols)]
            ay = ax = H // 2
        assert board.shape == (H, H) and board[ay, ax] & CT.agent
        board[(board & (CT.exit | CT.agent)) == CT.exit] = CT.empty
        if not spawn:
            board[(board & CT.spawning) != 0] = CT.wall
            goals[(goals & CT.spawning) != 0] = CT.empty
        elif not ((board | goals) & CT.spawning).any():
            board[(ay + 2) % H, (ax - 2) % H] = CT.spawner
        assert bool(((board | goals) & CT.spawning).any()) == spawn
        for j in range(2):          # exit cells three moves or more from the agent
            board[(ay + 3 + 2 * j) % H, (ax + 2 + 3 * j + k) % H] = CT.level_exit
        levels.append(Level(board, goals, [[ay, ax]], spawn_prob=src.spawn_prob, min_performance=src.min_performance,
                            points_table=src.points_table, rng_words=src.rng_words))
    pool = LevelPool(levels, counts_fn=util.oracle_counts, min_performance_fraction=0.5)
    assert pool.exit_slots == 2 and pool.has_spawner == spawn and pool.shape == (H, H)
    _pools[H, spawn] = pool
    return pool


class _Pair(object):
    """A device env and an oracle env on the same three levels."""

    def __init__(self, H, B, with_obs=False, spawn=False, wrap=False, rollout=False):
        pool = _pool(H, spawn)
        wrappers = None
        if wrap:
            words = np.random.default_rng(7 * H + B).integers(0, 2 ** 63, (B, 4), dtype=np.uint64)
            words[:, 3] |= 1                    # a PCG64 increment is odd
            wrappers = dict(WRAPPERS, baseline="inaction", inaction_rng=words)
        kw = dict(first_level=np.arange(B) % 3, auto_reset=True, level_stride=2, time_limit=TIME_LIMIT, view_shape=(15, 15),
                  with_obs=with_obs, wrappers=wrappers)
        self.dev = util.DeviceBackend(pool, B, **kw)
        self.cpu = util.OracleBackend(pool, B, **kw)
        self.env = self.dev.env
        assert self.env.row_kernels()
        self.B, self.wrap, self.with_obs = B, wrap, with_obs
        self.actions = np.random.default_rng(1000 * H + B).integers(0, 9, (STEPS, B)).astype(np.int32)
        self.prev_done = np.zeros(B, bool)

    def same(self, where, names):
        for name in names:
            got, want = self.dev.get(name), self.cpu.get(name)
            assert got.shape == want.shape and np.array_equal(got, want), "%s, %s: envs %r differ" % (
                where, name, np.nonzero((got != want).reshape(self.B, -1).any(axis=1))[0].tolist())

    def same_wrappers(self, where):
        """Shaped reward, the wrappers' own state, the inaction baseline's generator and board."""
        self.same(where, ("shaped_reward", "inaction_rng"))
        st, wa = self.dev.get("wrap_state"), self.cpu.env.wa
        assert np.array_equal(st[:, 0], wa["n_prior"]) and np.array_equal(st[:, 1], wa["last_side_effect"]), where
        prior = np.ascontiguousarray(st[:, 2:10]).view(np.int16).reshape(self.B, 8, 2)
        held = np.arange(8)[None, :, None] < wa["n_prior"][:, None, None]
        assert np.array_equal(np.where(held, prior, 0), np.where(held, wa["prior"], 0)), where
        # (the oracle copies the board into the baseline when it resets an env, the library when the env next steps:
        #  compare the envs that did not just finish)
        keep = ~self.cpu.get("done").astype(bool)
        assert np.array_equal(self.dev.get("inaction_board")[keep], self.cpu.get("inaction_board")[keep]), where

    def reset(self):
        self.env.reset()
        self.cpu.env.reset()
        self.same("reset", STATE)

    def after_step(self, t, all_end=True):
        self.cpu.env.step(self.actions[t])
        where = "step %d" % t
        self.same(where, STATE + RECORDS)
        if self.wrap:
            self.same_wrappers(where)
        if self.with_obs:
            assert np.array_equal(self.dev.get("obs"), self.cpu.env.obs), where
        if all_end and t % TIME_LIMIT == TIME_LIMIT - 1:
            assert self.cpu.get("done").all() and (self.cpu.get("num_steps") == 0).all(), t


CASES = [(H, B, v) for H, B in SHAPES for v in VARIANTS]


@pytest.mark.parametrize("H,B,variant", CASES, ids=["%dx%d-B%d-%s" % (H, H, B, v) for H, B, v in CASES])
def test_every_step_against_the_oracle(H, B, variant):
    """Seven steps at time_limit = 3: steps 2 and 5 end every episode of the batch at once."""
    kw = dict(VARIANTS[variant])
    pair = _Pair(H, B, **kw)
    env = pair.env
    pair.reset()
    if kw.get("rollout"):
        # the loop form: launches of 3, 3 and 1 steps; state, the last step's records and the per-step rewards and dones
        for t0 in range(0, STEPS, 3):
            n = min(3, STEPS - t0)
            r_t, d_t = env.rollout(pair.actions[t0:t0 + n])
            r_t, d_t = r_t.cpu().numpy(), d_t.cpu().numpy()
            for t in range(t0, t0 + n):
                pair.cpu.env.step(pair.actions[t])
                assert np.array_equal(r_t[t - t0], pair.cpu.get("reward")) and np.array_equal(d_t[t - t0], pair.cpu.get("done")), t
            pair.same("launch of steps %d..%d" % (t0, t0 + n - 1), STATE + RECORDS)
            if pair.wrap:
                pair.same_wrappers("launch of steps %d..%d" % (t0, t0 + n - 1))
    else:
        for t in range(STEPS):
            env.step(pair.actions[t])
            pair.after_step(t)
    assert (pair.cpu.get("episode_idx") >= STEPS // TIME_LIMIT).all()


@pytest.mark.parametrize("H,B", [(25, 15), (64, 5)])
def test_masked_reset_and_observation_launch(H, B):
    """env.reset(mask) runs the reload behind the end barrier of a launch that steps nothing; get_obs() is a launch that
    neither steps nor reloads.  Both write back what they read, and the steps behind them agree."""
    pair = _Pair(H, B, with_obs=True, spawn=True)
    env = pair.env
    mask = (np.arange(B) % 3 != 1).astype(np.uint8)
    pair.reset()
    for t in range(5):
        env.step(pair.actions[t])
        pair.after_step(t, all_end=False)
        if t in (0, 3):
            env.reset(mask)
            pair.cpu.env.reset(mask)
            pair.same("masked reset behind step %d" % t, STATE)
        if t in (1, 2):
            env.obs.zero_()
            env.get_obs()
            assert np.array_equal(pair.dev.get("obs"), pair.cpu.env.obs), t
            pair.same("observation launch behind step %d" % t, STATE)


def _open_queues(env, release_free):
    """True with the queues open; False where the runtime has no HSA queue to give (the one refusal a box may answer with).
    Any other refusal -- the queues refuse a step kernel that keeps private memory -- fails the test."""
    from safelife_amd._hip import SafeLifeHipError
    try:
        env.queues_open(1, release_free=release_free)
    except SafeLifeHipError as e:
        assert "AQL queues unavailable" in str(e), e
        return False
    if release_free and not env.queue_release_free:
        pytest.skip("release-free stepping not granted on this box: %s" % env.queue_mode_note)
    return True


@pytest.mark.parametrize("release_free", [False, True], ids=["agent-fences", "release-free"])
def test_plain_step_through_the_queues(release_free):
    import torch
    pair = _Pair(25, 15)
    env = pair.env
    pair.reset()
    acts = torch.from_numpy(pair.actions).to(env.device)
    torch.cuda.synchronize()
    queued = _open_queues(env, release_free)
    if queued:
        assert env.queue_release_free == release_free
    for t in range(STEPS):
        if queued:
            env.step_queues_many(acts[t:t + 1])
            env.queues_sync()
        else:                   # what a caller does that was refused: the same steps on the slice streams
            env.step_async(acts[t])
            env.join()
        pair.after_step(t)
    if queued:
        env.queues_close()
