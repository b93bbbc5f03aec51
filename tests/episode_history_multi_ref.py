"""
Episode histories of multi-agent envs in plain numpy, sharing nothing with the kernels: what include/safelife_hip.h says
slhip_history_capture_multi does.  The model of tests/episode_history_ref.py holds unchanged; this file states the three
things that are defined over the agents -- when an env's episode ends, how long it was, what its entry says -- and hands
the rest to that model.  tests/test_episode_history_multi_host.py holds it against what the reference's
``SafeLifeEnv(single_agent=False)`` + ``SafeLifeLogWrapper`` + ``SafeLifeLogger`` saved
(tests/golden/episode_history_multi_cases.npz); tests/test_episode_history_multi_gpu.py holds the kernels against it.

``reading`` names the rule; "all" is the model.  The others are the mistakes a reader of ``out [B, A]`` can make, kept here so
that the host test can show that the fixture tells each of them from the model:
    "any"        the episode ends when ANY agent is done
    "length0"    the entry's length is agent 0's
    "stop0"      nothing is captured once agent 0 is done
    "per_agent"  the numbering counts every agent's done flag
    "success0"   success is agent 0's alone
"""
import numpy as np

from tests import episode_history_ref as hr

ENTRY_DTYPE, LIVE, NO_FINAL, FREE, ENV, ENTRY, POISON = (hr.ENTRY_DTYPE, hr.LIVE, hr.NO_FINAL, hr.FREE, hr.ENV, hr.ENTRY,
                                                         hr.POISON)
READINGS = ("all", "any", "length0", "stop0", "per_agent", "success0")


def success_bits(mask, A):
    return ((int(mask) >> np.arange(A)) & 1).astype(bool)


class MultiHistoryModel(hr.HistoryModel):
    def __init__(self, B, A, watch, slots, T, H, W, interval=1, reading="all"):
        super().__init__(B, watch, slots, T, H, W, interval)
        assert reading in READINGS
        self.A, self.reading = int(A), reading

    def capture_multi(self, board, goals, level_idx, episode_idx, num_steps, out, queue=None, active=None):
        """board, goals uint16 [B,H,W]; level_idx, episode_idx, num_steps int [B]: the scalars after the step; out: dict of
        arrays [B,A] (done, success, times_up, episode_length); queue, active: as ``HistoryModel.capture``."""
        A, reading = self.A, self.reading
        done_a = np.asarray(out["done"]).reshape(self.B, A) != 0
        done = done_a.any(axis=1) if reading == "any" else done_a.all(axis=1)
        length_a = np.asarray(out["episode_length"]).reshape(self.B, A).astype(np.int64)
        length = length_a[:, 0] if reading == "length0" else length_a.max(axis=1)
        success_a = np.asarray(out["success"]).reshape(self.B, A) != 0
        if reading == "success0":
            success = success_a[:, 0].astype(np.uint8)
        else:
            success = (success_a * (1 << np.arange(A))).sum(axis=1).astype(np.uint8)
        times_up = (np.asarray(out["times_up"]).reshape(self.B, A) != 0).any(axis=1).astype(np.uint8)
        # only the done bytes count while an episode goes on: whatever else the records hold then is not looked at
        length = np.where(done, length, -1)
        on = np.ones(self.B, bool) if active is None else np.asarray(active) != 0
        saved, first = self.frames.copy(), self.episodes
        self.capture(board, goals, level_idx, episode_idx, num_steps,
                     dict(done=done.astype(np.uint8), success=success, times_up=times_up, episode_length=length), queue, active)
        if reading == "stop0":                  # (the live frames of an env whose agent 0 has left are not written)
            for i, e in enumerate(self.watch):
                if done_a[e, 0] and not done[e] and self.owner[i] >= 0:
                    self.frames[self.owner[i]] = saved[self.owner[i]]
        if reading == "per_agent":
            # every agent's flag is an episode of the count (masked envs apart)
            self.episodes = first + int((done_a & on[:, None]).sum())
        # (the entries of this call are the live ones numbered from `first` on)
        self.entries["reserved"][((self.entries["flags"] & LIVE) != 0) & (self.entries["row"] >= first)] = A


def as_the_reference_saved(board, locs, next_actions):
    """The frames [n,H,W] of one multi-agent episode as the reference's ``.npz`` holds them: ``SafeLifeLogWrapper`` appends
    ``game.board`` itself (safelife_logger.py:569) and the next step's ``execute_actions`` writes into that very array before
    ``advance_board`` replaces it, so a saved frame t < n - 1 is the board after step t with ALL agents' actions of step t + 1
    carried out, in index order (advance_board.c:217-220); the last frame is the board as the step left it.
    ``locs[t]`` int [A,2]: where the agents stood after step t; ``next_actions[t]`` int [A]: the actions of step t + 1 (an agent
    that is done takes 0, which moves nothing)."""
    import oracle
    out = np.ascontiguousarray(board, np.uint16).copy()
    for f in range(len(out) - 1):
        loc = np.ascontiguousarray(locs[f], np.int64).copy()
        oracle.execute_actions(out[f], loc, np.asarray(next_actions[f], np.int64))
    return out


class MultiOracleDrive(object):
    """The restatement driven by the oracle's multi-agent env.  The oracle steps without auto-reset, so that the board as
    the agents left it can be read off -- the finished-episode queue's entry, filed once, on the step where every agent is
    done -- and the finished envs are then reloaded from outside.  ``queue_capacity``: entries beyond it are dropped."""

    def __init__(self, pool, B, time_limit, watch, slots, interval=1, first_level=None, level_stride=1,
                 queue_capacity=1 << 20, reading="all", **env_kw):
        from tests import util
        first = (np.arange(B) % len(pool)) if first_level is None else first_level
        self.be = util.OracleMultiBackend(pool, B, first_level=first, auto_reset=False, time_limit=time_limit,
                                          level_stride=level_stride, **env_kw)
        self.be.reset()
        H, W = pool.shape
        self.B, self.n_agents, self.A, self.ma = B, int(pool.n_agents), self.be.arrays, self.be.env.ma
        self.model = MultiHistoryModel(B, self.n_agents, watch, slots, time_limit, H, W, interval, reading)
        self.capacity, self.queue, self.pushed = int(queue_capacity), [], 0
        self.ended, self.actions, self.locs, self.t = {}, [], [], 0
        self.model.rewind(self.A["goals"], self.A["level_idx"], self.A["episode_idx"])

    def step(self, actions):
        A, ma = self.A, self.ma
        actions = np.asarray(actions, np.int32).reshape(self.B, self.n_agents)
        self.be.step(actions)
        self.actions.append(actions.copy())
        self.locs.append(ma["agent_loc"].copy())
        out = dict(done=ma["done"].copy(), success=ma["success"].copy(), episode_length=ma["episode_length"].copy(),
                   times_up=np.repeat(np.asarray(A["times_up"])[:, None], self.n_agents, axis=1).copy())
        done = (ma["done"] != 0).all(axis=1)
        for e in np.flatnonzero(done):
            # (end step, the record's num_steps, every agent's length and success)
            self.ended[(int(e), int(A["episode_idx"][e]))] = (self.t, int(A["num_steps"][e]), out["episode_length"][e].copy(),
                                                              out["success"][e].copy())
            self.pushed += 1
            if len(self.queue) < self.capacity:
                self.queue.append((int(e), int(A["episode_idx"][e]), A["board"][e].copy()))
        if done.any():
            self.be.env.reset(mask=done.astype(np.uint8))
        q = (self.pushed, np.array([e for e, _, _ in self.queue], np.int64), np.array([k for _, k, _ in self.queue], np.int64),
             [b for _, _, b in self.queue])
        self.model.capture_multi(A["board"], A["goals"], A["level_idx"], A["episode_idx"], A["num_steps"], out, q)
        self.t += 1
        return out

    def flush(self):
        self.queue, self.pushed, self.model.cursor = [], 0, 0

    def reset(self, mask=None):
        m = None if mask is None else np.asarray(mask, np.uint8)
        self.be.env.reset(mask=m)
        self.model.rewind(self.A["goals"], self.A["level_idx"], self.A["episode_idx"], m)

    def bridge(self, entry):
        """(locs, next_actions) of an entry's frames 0 .. length - 2, for ``as_the_reference_saved``."""
        end, n, e = self.ended[(int(entry["env"]), int(entry["episode_idx"]))][0], int(entry["length"]), int(entry["env"])
        first = end - n + 1                     # the step behind frame 0
        return ([self.locs[first + f][e] for f in range(n - 1)], [self.actions[first + 1 + f][e] for f in range(n - 1)])
