"""
The evaluation run (safelife_amd/episode_run.py, include/safelife_hip.h) restated in plain numpy, one env at a time.  It
shares nothing with the kernels.

A run is N tickets over L slots and G envs: ticket t -> (slot, env, k) = (t % L, t % G, t // G).  ``RunModel`` holds one
shard's state (envs ``env_offset .. env_offset + B - 1``) and is fed the per-step output records, ``STEP_OUT`` [B] or [B, A].
"""
import numpy as np

#: ``struct sl_step_out``
STEP_OUT = np.dtype([("reward", "<f4"), ("done", "u1"), ("success", "u1"), ("times_up", "u1"), ("reserved", "u1"),
                     ("episode_reward", "<f4"), ("episode_length", "<i4")])
ROW = np.dtype([("slot", "<i4"), ("env", "<i4"), ("episode_idx", "<i4"), ("step", "<i4"), ("length", "<i4"),
                ("reward", "<f4"), ("success", "u1"), ("times_up", "u1"), ("flags", "u1"), ("reserved", "u1"),
                ("reserved2", "<i4")])
AGENT = np.dtype([("length", "<i4"), ("reward", "<f4"), ("success", "u1"), ("times_up", "u1"), ("reserved", "u1", (2,)),
                  ("reserved2", "<i4")])
WRITTEN = 1


def deal(t, L, G):
    """ticket -> (slot, env, k)"""
    return t % L, t % G, t // G


def tickets_of_env(g, G, N):
    return list(range(g, N, G))


class RunModel(object):
    def __init__(self, B, G, env_offset, N, L, A=1, base_episode=None):
        assert 0 <= env_offset and env_offset + B <= G
        self.B, self.G, self.env_offset, self.N, self.L, self.A = B, G, env_offset, N, L, A
        self.base_episode = np.zeros(B, np.int32) if base_episode is None else np.asarray(base_episode, np.int32).copy()
        self.active = np.array([1 if env_offset + e < N else 0 for e in range(B)], np.uint8)
        self.played = np.zeros(B, np.int32)
        self.completed, self.in_progress, self.env_steps = 0, int(self.active.sum()), 0
        self.results = np.zeros(N, ROW)
        self.agent_results = np.zeros((N, A), AGENT)
        self.writes = np.zeros(N, np.int64)         # how often every ticket has been filed
        self.steps = 0

    def counters(self):
        return dict(completed=self.completed, in_progress=self.in_progress, env_steps=self.env_steps)

    def finished(self):
        return self.in_progress == 0

    def step(self, out):
        """One step's records in, the masked records out (a copy); the state moves on."""
        out = np.array(out, STEP_OUT).reshape(self.B, self.A)
        self.steps += 1
        for e in range(self.B):
            if not self.active[e]:
                out[e] = np.zeros(self.A, STEP_OUT)
                continue
            self.env_steps += 1
            if not all(out[e, a]["done"] for a in range(self.A)):
                continue
            g = self.env_offset + e
            k = int(self.played[e])
            t = g + self.G * k
            assert t < self.N
            o = out[e, 0]
            self.results[t] = (t % self.L, g, self.base_episode[e] + k, self.steps, o["episode_length"],
                               o["episode_reward"], o["success"], o["times_up"], WRITTEN, 0, 0)
            for a in range(self.A):
                oa = out[e, a]
                self.agent_results[t, a] = (oa["episode_length"], oa["episode_reward"], oa["success"], oa["times_up"],
                                            (0, 0), 0)
            self.writes[t] += 1
            self.played[e] = k + 1
            self.completed += 1
            if g + self.G * (k + 1) >= self.N:
                self.active[e] = 0
                self.in_progress -= 1
        return out

    def ticket(self, env, episode_idx):
        """The ticket of local env `env`'s episode with the counter `episode_idx`, -1 if it is none of this run's."""
        if not 0 <= env < self.B:
            return -1
        k = int(episode_idx) - int(self.base_episode[env])
        if k < 0:
            return -1
        t = self.env_offset + env + self.G * k
        return t if t < self.N else -1


def play(B, G, env_offset, N, L, episode, extra_steps=0):
    """A whole run of one shard over scripted envs: env g starts on slot g % L and moves on by G % L whenever an episode
    ends (the stride rule under auto_reset -- for ever, retired or not), and the episode on slot s is ``episode(s) ->
    (length, reward, success)``.  Yields, per step, (model, the masked records [B], the envs' scalars AFTER the step: slot
    loaded and episode counter) until the run has finished and `extra_steps` more."""
    m = RunModel(B, G, env_offset, N, L)
    slot = np.array([(env_offset + e) % L for e in range(B)], np.int64)
    count, episodes = np.zeros(B, np.int64), np.zeros(B, np.int32)
    extra = 0
    while not m.finished() or extra < extra_steps:
        extra += m.finished()
        out = np.zeros(B, STEP_OUT)
        for e in range(B):
            count[e] += 1
            length, reward, success = episode(int(slot[e]))
            if count[e] >= length:
                out[e] = (0.0, 1, success, 0, 0, reward, count[e])
                count[e], episodes[e] = 0, episodes[e] + 1
                slot[e] = (slot[e] + G % L) % L
        masked = m.step(out)
        yield m, masked.reshape(B), dict(level_idx=slot.astype(np.int32), episode_idx=episodes.copy())
