"""
Episode histories in plain numpy, sharing nothing with the kernels: what include/safelife_hip.h says slhip_history_capture and
slhip_history_rewind do, one watched env at a time in ascending order -- the sequential reading of the model ("the next env
that needs a slot takes the lowest free one"), which the kernels' scans must equal.  tests/test_episode_history_host.py
holds it against what the reference's SafeLifeLogWrapper and SafeLifeLogger saved (tests/golden/episode_history_cases.npz);
tests/test_episode_history_gpu.py holds the kernels against it, bit for bit.
"""
import numpy as np

ENTRY_DTYPE = np.dtype([("row", "<i8"), ("env", "<i4"), ("level", "<i4"), ("episode_idx", "<i4"), ("length", "<i4"),
                        ("slot", "<i4"), ("success", "u1"), ("times_up", "u1"), ("flags", "u1"), ("reserved", "u1")])
LIVE, NO_FINAL = 1, 2
FREE, ENV, ENTRY = 0, 1, 2
POISON = 0xDEAD


class HistoryModel(object):
    def __init__(self, B, watch, slots, T, H, W, interval=1):
        self.B, self.K, self.T, self.H, self.W, self.interval = int(B), int(slots), int(T), int(H), int(W), int(interval)
        self.watch = np.asarray(watch, np.int32)
        assert (np.diff(self.watch) > 0).all() and self.watch.min() >= 0 and self.watch.max() < B
        n = len(self.watch)
        self.owner = np.full(n, -1, np.int32)
        self.cur_level, self.cur_episode = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.slot_state = np.zeros(self.K, np.int32)
        self.entries = np.zeros(self.K, ENTRY_DTYPE)
        self.goals = np.full((self.K, H, W), POISON, np.uint16)
        self.frames = np.full((self.K, self.T, H, W), POISON, np.uint16)
        self.episodes = self.kept = self.missed = self.incomplete = self.cursor = 0

    def counters(self):
        return dict(episodes=self.episodes, kept=self.kept, missed=self.missed, incomplete=self.incomplete,
                    cursor=self.cursor)

    def _lowest_free(self):
        free = np.flatnonzero(self.slot_state == FREE)
        return int(free[0]) if len(free) else -1

    def _start(self, i, e, level_idx, episode_idx, goals):
        """An episode of watched env i starts: a slot if it has none and one is free, the level and counter noted, the
        goals plane written."""
        if self.owner[i] < 0:
            s = self._lowest_free()
            if s >= 0:
                self.slot_state[s] = ENV
            self.owner[i] = s
        self.cur_level[i], self.cur_episode[i] = level_idx[e], episode_idx[e]
        if self.owner[i] >= 0:
            self.goals[self.owner[i]] = goals[e]

    def rewind(self, goals, level_idx, episode_idx, mask=None):
        for i, e in enumerate(self.watch):
            if mask is None or mask[e]:
                self._start(i, e, level_idx, episode_idx, goals)

    def capture(self, board, goals, level_idx, episode_idx, length_now, out, queue=None, active=None):
        """board, goals uint16 [B,H,W]; level_idx, episode_idx, length_now int [B]: the scalars after the step; out: dict of
        arrays [B] (done, success, times_up, episode_length); queue: None or (count, env [C], episode_idx [C], boards
        [C,H,W]); active: None or [B]."""
        on = np.ones(self.B, bool) if active is None else np.asarray(active) != 0
        done = (np.asarray(out["done"]) != 0) & on
        rank = np.cumsum(done) - done
        q_end = 0
        if queue is not None:
            count, q_env, q_episode, q_boards = queue
            q_end = min(max(int(count), 0), len(q_env))
        first = min(max(self.cursor, 0), q_end)
        final = {}
        for j in range(first, q_end):
            hit = np.flatnonzero(self.watch == q_env[j])
            if len(hit) and q_episode[j] == self.cur_episode[hit[0]]:
                final.setdefault(int(hit[0]), j)
        for i, e in enumerate(self.watch):
            if not on[e]:
                continue
            s = int(self.owner[i])
            if not done[e]:
                f = int(length_now[e]) - 1
                if s >= 0 and 0 <= f < self.T:
                    self.frames[s, f] = board[e]
                continue
            number = self.episodes + int(rank[e])
            if number % self.interval == 0:
                if s < 0:
                    self.missed += 1
                else:
                    j = final.get(i)
                    length = int(out["episode_length"][e])
                    self.entries[s] = (number, e, self.cur_level[i], self.cur_episode[i], length, s, out["success"][e],
                                       out["times_up"][e], LIVE | (NO_FINAL if j is None else 0), 0)
                    self.slot_state[s] = ENTRY
                    self.kept += 1
                    if j is None:
                        self.incomplete += 1
                    elif 0 <= length - 1 < self.T:
                        self.frames[s, length - 1] = q_boards[j]
                    self.owner[i] = -1
            self._start(i, e, level_idx, episode_idx, goals)
        self.episodes += int(done.sum())
        if queue is not None:
            self.cursor = q_end

    def release(self, slots):
        for s in slots:
            assert self.slot_state[s] == ENTRY
            self.slot_state[s] = FREE
            self.entries[s] = 0

    def listing(self):
        """The live entries, sorted by row."""
        live = self.entries[(self.entries["flags"] & LIVE) != 0]
        return live[np.argsort(live["row"], kind="stable")]

    def history(self, entry):
        """{'board': [length,H,W], 'goals': [length,H,W]} of one entry (one frame fewer with NO_FINAL)."""
        n = int(entry["length"]) - (1 if entry["flags"] & NO_FINAL else 0)
        s = int(entry["slot"])
        return {"board": self.frames[s, :n].copy(), "goals": np.broadcast_to(self.goals[s], (n, self.H, self.W)).copy()}


AGENT = 1 << 1      # CellTypes.agent


def as_the_reference_saved(board, next_actions):
    """The frames [n,H,W] of one episode as the reference's ``.npz`` holds them.  ``SafeLifeLogWrapper`` appends
    ``game.board`` itself, not a copy (safelife_logger.py:569), and the NEXT step's ``execute_actions`` writes into that very
    array before ``advance_board`` replaces it (safelife_env.py:151-152): a saved frame t < n - 1 is the board after step t
    with the action of step t + 1 already carried out; only the last frame is the board as the step left it.
    ``next_actions[t]``: the action of the step behind frame t (t < n - 1).  The recorder keeps the boards as the steps left
    them (what ``info['board']`` and the traces hold); this function is the bridge to the reference's saved bytes."""
    import oracle
    out = np.ascontiguousarray(board, np.uint16).copy()
    for f in range(len(out) - 1):
        loc = np.argwhere((out[f] & AGENT) != 0)[:1].astype(np.int64)
        if len(loc):
            oracle.execute_actions(out[f], np.ascontiguousarray(loc), np.array([next_actions[f]], np.int64))
    return out


class OracleDrive(object):
    """The restatement driven by the oracle's env.  The oracle steps without auto-reset, so that the board as the agent
    left it can be read off -- the finished-episode queue's entry -- and the finished envs are then reloaded from outside,
    which leaves the state an in-step reload leaves (tests/test_episode_history_host.py holds the two against each other).
    ``queue_capacity``: entries beyond it are dropped, in ascending env order within a step."""

    def __init__(self, pool, B, time_limit, watch, slots, interval=1, first_level=None, level_stride=1,
                 queue_capacity=1 << 20, **env_kw):
        from tests import util
        first = (np.arange(B) % len(pool)) if first_level is None else first_level
        self.be = util.OracleBackend(pool, B, first_level=first, auto_reset=False, time_limit=time_limit,
                                     level_stride=level_stride, **env_kw)
        self.be.reset()
        H, W = pool.shape
        self.B, self.A = B, self.be.arrays
        self.model = HistoryModel(B, watch, slots, time_limit, H, W, interval)
        self.capacity, self.queue, self.pushed = int(queue_capacity), [], 0
        self.ended, self.actions, self.t = {}, [], 0
        self.model.rewind(self.A["goals"], self.A["level_idx"], self.A["episode_idx"])

    def step(self, actions):
        A = self.A
        self.be.step(np.asarray(actions, np.int32))
        self.actions.append(np.asarray(actions, np.int32).copy())
        done = A["done"].copy()
        out = {k: A[k].copy() for k in ("done", "success", "times_up", "episode_length")}
        for e in np.flatnonzero(done):
            self.ended[(int(e), int(A["episode_idx"][e]))] = self.t
            self.pushed += 1
            if len(self.queue) < self.capacity:
                self.queue.append((int(e), int(A["episode_idx"][e]), A["board"][e].copy()))
        if done.any():
            self.be.env.reset(mask=done)
        q = (self.pushed, np.array([e for e, _, _ in self.queue], np.int64), np.array([k for _, k, _ in self.queue], np.int64),
             [b for _, _, b in self.queue])
        self.model.capture(A["board"], A["goals"], A["level_idx"], A["episode_idx"], A["episode_length"], out, q)
        self.t += 1
        return out

    def flush(self):
        """The env installs a fresh queue: the cursor starts over."""
        self.queue, self.pushed, self.model.cursor = [], 0, 0

    def reset(self, mask=None):
        m = None if mask is None else np.asarray(mask, np.uint8)
        self.be.env.reset(mask=m)
        self.model.rewind(self.A["goals"], self.A["level_idx"], self.A["episode_idx"], m)

    def next_actions(self, entry):
        """The actions of the steps behind an entry's frames 0 .. length - 2 (for ``as_the_reference_saved``)."""
        end, n, e = self.ended[(int(entry["env"]), int(entry["episode_idx"]))], int(entry["length"]), int(entry["env"])
        return [int(self.actions[end - n + 2 + f][e]) for f in range(n - 1)]
