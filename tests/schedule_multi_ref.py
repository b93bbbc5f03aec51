"""
The multi-agent level-schedule kernels (csrc/sl_schedule.hip: k_schedule_required_multi, k_schedule_harvest_multi;
include/safelife_hip.h "level schedules for envs with several agents") restated on the host, on top of tests/schedule_ref.py.
numpy and Python floats only; nothing here loads the library or imports safelife_amd.schedule.

Everything is an EXACT model: one IEEE float64 operation at a time in the kernels' order.

    required[l][a] = ceil((min_performance[l] * fraction) * available[l][a]), clamped as the single-agent value is
    an env has finished on a step when ALL its A step records have done != 0
    its performance is np.average(reward / reward_possible) over its agents, 0.0 where THAT is NaN or +-inf
"""
import math

import numpy as np

from tests import schedule_ref as sr

MAX_AGENTS = 8


def required_points_multi(min_performance, fraction, available):
    """[A] required points of one level: schedule_ref.required_points per agent (the products rounded one after the
    other)."""
    return np.array([sr.required_points(min_performance, fraction, a) for a in np.asarray(available).ravel()], np.int32)


def add_reduce(q):
    """np.add.reduce of a contiguous float64 array of at most 8 elements: the identity 0.0 plus -- fewer than 8 elements --
    their sum in index order, or -- exactly 8 -- numpy's eight accumulators combined pairwise."""
    q = [float(v) for v in q]
    assert 1 <= len(q) <= MAX_AGENTS
    if len(q) == 8:
        s = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))
    else:
        s = q[0]
        for v in q[1:]:
            s = s + v
    return 0.0 + s


def performance_multi(episode_reward, reward_possible):
    """env_factory.py:91-101 for one env: episode_reward float32 [A], reward_possible int [A] -> float."""
    r = np.asarray(episode_reward, np.float32).ravel()
    p = np.asarray(reward_possible).ravel()
    assert len(r) == len(p)
    with np.errstate(all="ignore"):
        q = [float(np.float64(r[a]) / np.float64(p[a])) for a in range(len(r))]
    perf = add_reduce(q) / float(len(q))
    if perf != perf or math.isinf(perf):
        perf = 0.0
    return perf


class ScheduleModelMulti(sr.ScheduleModel):
    """ScheduleModel with reward_possible [L, A] and step records [B, A]."""

    def __init__(self, groups, lookback, reward_possible, cur_slot):
        rp = np.asarray(reward_possible, np.int32)
        assert rp.ndim == 2 and 1 <= rp.shape[1] <= MAX_AGENTS
        sr.ScheduleModel.__init__(self, groups, lookback, rp, cur_slot)
        self.n_agents = rp.shape[1]

    def harvest(self, done, episode_reward, level_idx):
        """slhip_schedule_harvest_multi: done uint8 [B, A], episode_reward float32 [B, A] (sl_step_out), level_idx int32
        [B] (sl_env_scalars after the step).  Records of envs that have not finished are not looked at beyond `done`."""
        done = np.asarray(done).reshape(-1, self.n_agents)
        episode_reward = np.asarray(episode_reward, np.float32).reshape(-1, self.n_agents)
        touched = set()
        for e in np.flatnonzero((done != 0).all(axis=1)):
            slot = int(self.cur_slot[e])
            g = self.group_of(slot)
            if g < 0:
                continue
            perf = performance_multi(episode_reward[e], self.reward_possible[slot])
            self.ring[g, self.pos[g]] = perf
            self.pos[g] = (self.pos[g] + 1) % self.lookback
            self.count[g] += 1
            self.episodes[g] += 1
            if perf > self.best[g]:
                self.best[g] = perf
            touched.add(g)
        for g in touched:
            rec = self.records(g)
            s = 0.0
            for v in rec:
                s = s + v
            self.mean[g] = s / float(len(rec))
        self.cur_slot[:] = np.asarray(level_idx, np.int32)
