"""A numpy restatement of the training wrappers over a multi-agent env (SafeLifeEnv(single_agent=False) under
env_wrappers.MovementBonusWrapper / ExtraExitBonus / SimpleSideEffectPenalty, stacked as training/env_factory.py:277-283).

The reward is a float32 array [A] that every wrapper updates in place, so each wrapper rounds to float32 once:
r = f32(f64(r) + term), in the order movement, exit bonus, side effect.  Agents that are done keep being shaped (their
``done`` stays True and their location stays put).  One side-effect count per env is subtracted from every agent.

The tests feed it the reference's recorded unwrapped outputs (trace_multi_wrap_*) or the oracle's, and compare with the
recorded / device shaped rewards bit for bit.
"""
import numpy as np

ALIVE, AGENT, DESTRUCTIBLE, FROZEN, PRESERVING, INHIBITING, EXIT = 1, 2, 8, 16, 32, 64, 256
COLOR_R, COLOR_B, COLORS = 1 << 9, 1 << 11, 7 << 9
PLAYER = AGENT | DESTRUCTIBLE | FROZEN | PRESERVING | INHIBITING       # CellTypes.player


class MultiWrapConfig(object):
    """Keyword form of SafeLifeMultiAgentVectorEnv(wrappers=...) / util.wrappers_from_trace."""

    def __init__(self, movement_bonus=None, movement_bonus_power=1e-100, movement_bonus_period=4, as_penalty=True,
                 exit_bonus=None, penalty_coef=None, ignore_reward_cells=False, baseline="starting-state", **_):
        self.movement_bonus, self.power, self.period = movement_bonus, movement_bonus_power, int(movement_bonus_period)
        self.as_penalty, self.exit_bonus, self.penalty_coef = bool(as_penalty), exit_bonus, penalty_coef
        self.ignore_reward_cells, self.baseline = bool(ignore_reward_cells), baseline


def side_effect_count(board, baseline, goals, exit_cells, ignore_reward_cells):
    """SimpleSideEffectPenalty's count (env_wrappers.py:183-208) for one env; exit_cells: flat indices."""
    b = board.astype(np.int64) & ~PLAYER
    b0 = baseline.astype(np.int64) & ~PLAYER
    b = b.reshape(-1).copy()
    b0 = b0.reshape(-1)
    ex = np.asarray([i for i in exit_cells if i >= 0], np.int64)
    b[ex] = b0[ex]
    unchanged = b == b0
    if ignore_reward_cells:
        red_life = ALIVE | COLOR_R
        start_red = (b0 & red_life) == red_life
        end_red = (b & red_life) == red_life
        goal_cell = (goals.reshape(-1).astype(np.int64) & COLORS) == COLOR_B
        end_alive = (b & red_life) == ALIVE
        return int(np.sum(~(unchanged | (start_red & ~end_red) | (goal_cell & end_alive))))
    return int(np.sum(~unchanged))


class MultiWrapState(object):
    """Per-env wrapper state: every agent's trail of locations, the last side-effect count."""

    def __init__(self, cfg, locs):
        self.cfg = cfg
        self.reset(locs)

    def reset(self, locs):
        self.prior = [np.array(locs, np.int64).copy()]
        self.last_side_effect = 0

    def step(self, reward, done, times_up, episode_reward, locs, side_effect=0):
        """One wrapped step: float32 [A] shaped rewards from the inner env's float32 [A] rewards."""
        cfg = self.cfg
        r = np.array(reward, np.float32).copy()
        if cfg.movement_bonus is not None:
            p0 = np.array(locs, np.int64)
            n = cfg.period
            if len(self.prior) >= n:
                dist = np.sum(np.abs(p0 - self.prior[-n]), axis=-1)
            else:
                dist = np.sum(np.abs(p0 - self.prior[0]), axis=-1)
                dist += n - len(self.prior)
            speed = dist / n
            r += cfg.movement_bonus * speed ** cfg.power
            if cfg.as_penalty:
                r -= cfg.movement_bonus
            self.prior.append(p0.copy())
            self.prior = self.prior[-n:]
        if cfg.exit_bonus is not None and not times_up:
            r += np.asarray(done, bool) * cfg.exit_bonus * np.asarray(episode_reward, np.float32)
        if cfg.penalty_coef is not None:
            delta = np.int64(side_effect) - np.int64(self.last_side_effect)
            r -= delta * cfg.penalty_coef
            self.last_side_effect = int(side_effect)
        assert r.dtype == np.float32
        return r


def exit_cells_of(board):
    """Flat indices of a level's exits (frozen exit cells without an agent)."""
    b = np.asarray(board, np.int64).reshape(-1)
    return np.nonzero((b & (EXIT | AGENT | FROZEN)) == (EXIT | FROZEN))[0]


def replay_shaped(tr, cfg=None):
    """The restatement over a trace_multi_wrap_* trace: its recorded unwrapped outputs, boards and locations in, the
    shaped rewards [T, A] out, plus the side-effect counts it computed against the recorded baseline boards [T]."""
    if cfg is None:
        from tests import util
        cfg = MultiWrapConfig(**(util.wrappers_from_trace(tr) or {}))
    T = len(tr["trace_reward"])
    resets = list(tr["trace_reset_at"])
    st = None
    exits = None
    shaped = np.zeros(tr["trace_reward"].shape, np.float32)
    counts = np.zeros(T, np.int64)
    ep = 0
    for t in range(T):
        if ep < len(resets) and resets[ep] == t:
            board0 = tr["trace_reset_board"][ep]
            exits = exit_cells_of(tr["level%d_board" % ep] if "level%d_board" % ep in tr else board0)
            locs0 = tr["level%d_agent_locs" % ep]
            if st is None:
                st = MultiWrapState(cfg, locs0)
            else:
                st.reset(locs0)
            ep += 1
        side = 0
        if cfg.penalty_coef is not None:
            side = side_effect_count(tr["trace_board"][t], tr["trace_baseline_board"][t], tr["trace_goals"][t], exits,
                                     cfg.ignore_reward_cells)
        counts[t] = side
        shaped[t] = st.step(tr["trace_reward"][t], tr["trace_done"][t], bool(tr["trace_times_up"][t]),
                            tr["trace_ep_reward"][t], tr["trace_agent_locs"][t], side)
    return shaped, counts
