"""The flow every case of the fused-step matrices takes, on the device and on the oracle side by side: `Pair` steps a device
env and an oracle env on one pool, `run_matrix_case` is the flow itself -- reset, 24 scripted single steps, a masked reset in
the plain cases, a 6-step launch and one single step behind it.  tests/test_step_matrix_gpu.py runs it on the row kernels,
tests/test_step_generic_gpu.py on the size-generic family.  Integer work and float64 sums made in the oracle's order: every
comparison is np.array_equal.
"""
import numpy as np

from tests import step_matrix_cases as smc
from tests import util

# what a reset writes: the state without the outputs of the step before it
RESET_STATE = tuple(n for n in smc.ENV_STATE if n not in ("success", "times_up"))


def _same(case, got, want, field, step):
    """Bit-exact, and on a mismatch name the case, the step, the field and the first differing env."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want):
        return
    where = "%s %s B=%d, step %s, %s" % (smc.case_id(case.H, case.cfg, case.W), case.batch, case.B, step, field)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (
        where, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    e = int(bad[0])
    on = ""
    if isinstance(step, int) and got.shape[0] == case.B:
        on = " (level %d, %d steps into its episode before the step)" % tuple(case.schedule[step, e])
    raise AssertionError("%s: %d rows differ, first %d%s: device %r, oracle %r" % (
        where, len(bad), e, on, got[e].ravel()[:12], want[e].ravel()[:12]))


class Pair(object):
    """A device env and an oracle env on one pool, stepped together."""

    def __init__(self, case, pools=None, **device_kw):
        """pools: (the device env's pool, the oracle's) where the test replaces levels while the envs step."""
        self.case = case
        pool, pool_cpu = pools if pools else (case.pool(util.oracle_counts),) * 2
        self.dev = util.DeviceBackend(pool, case.B, **dict(case.backend_kw(device=True), **device_kw))
        self.cpu = util.OracleBackend(pool_cpu, case.B, **case.backend_kw(device=False))
        self.env = self.dev.env
        self.run = smc.OracleRun(case, self.cpu, finished=bool(case.queue_capacity))
        self.queued = {}            # (env, episode_idx) -> the oracle's finished episode, since the last flush
        self.n_queue_checks = self.n_dropped = 0
        self.last_done = np.ones(case.B, np.uint8)          # (nothing stepped yet)

    def state(self, step, names=smc.ENV_STATE):
        for name in names:
            _same(self.case, self.dev.get(name), self.cpu.get(name), name, step)
        if self.case.wrapped and "inaction_rng" in self.env.t:
            _same(self.case, self.dev.get("inaction_rng"), self.cpu.get("inaction_rng"), "inaction_rng", step)
            # (the oracle copies the board into the baseline when it resets an env, the library when the env next steps:
            #  the envs that did not just finish)
            keep = self.last_done == 0
            _same(self.case, self.dev.get("inaction_board")[keep], self.cpu.get("inaction_board")[keep], "inaction_board", step)

    def obs(self, step, want):
        case = self.case
        if not case.with_obs:
            return
        _same(case, self.dev.get("obs"), want, "obs", step)
        if case.policy_layout:
            got = self.env.policy_tensor.cpu().numpy()
            dt = np.uint8 if case.policy_layout == "uint8" else np.float32
            _same(case, got, np.ascontiguousarray(np.transpose(want, (0, 3, 2, 1))).astype(dt), "policy_tensor", step)

    def reset(self):
        self.env.reset()
        self.obs("reset", self.cpu.env.reset())

    def oracle_step(self):
        """One scripted oracle step -> (obs, reward, done, shaped reward or None)."""
        obs, r, d = self.run.step()
        for rec in self.run.finished:
            self.queued[rec[:2]] = rec
        self.last_done = d
        return obs, r, d, self.cpu.get("shaped_reward") if self.case.wrapped else None

    def outputs(self, step, want):
        obs, r, d, shaped = want
        _same(self.case, self.dev.get("reward"), r, "reward", step)
        _same(self.case, self.dev.get("done"), d, "done", step)
        if shaped is not None:
            _same(self.case, self.dev.get("shaped_reward"), shaped, "shaped_reward", step)
        self.obs(step, obs)

    def queue(self, step):
        """The finished-episode queue since the last flush against the oracle's finished episodes, in env order: the
        count of all that ended (kept or dropped), and every kept record and board."""
        case = self.case
        if not case.queue_capacity:
            return
        batch = self._take_queue_raw() if case.queue_raw else self.env.side_effects_flush()
        n, dropped = len(batch), batch.dropped()
        assert n + dropped == len(self.queued), "%s step %s: %d episodes queued or dropped, the oracle finished %d" % (
            smc.case_id(case.H, case.cfg, case.W), step, n + dropped, len(self.queued))
        assert n == min(len(self.queued), case.queue_capacity)
        recs = batch.records()
        boards = batch.boards[:n].cpu().numpy().view(np.uint16)
        keys = [(int(recs["env"][i]), int(recs["episode_idx"][i])) for i in range(n)]
        assert len(set(keys)) == n, "an episode was queued twice"
        for i in np.lexsort(([k[1] for k in keys], [k[0] for k in keys])) if n else ():
            assert keys[i] in self.queued, "%s step %s: queued %r, which the oracle did not finish" % (
                smc.case_id(case.H, case.cfg, case.W), step, keys[i])
            _, _, level, num_steps, board, success, times_up, ep_reward, ep_length = self.queued[keys[i]]
            got = (int(recs["level"][i]), int(recs["num_steps"][i]), int(recs["success"][i]), int(recs["times_up"][i]),
                   float(recs["episode_reward"][i]), int(recs["episode_length"][i]))
            assert got == (level, num_steps, success, times_up, ep_reward, ep_length), (step, keys[i], got)
            _same(case, boards[i:i + 1], board[None], "queued board of env %d" % keys[i][0], step)
        self.n_dropped += dropped
        self.queued = {}
        self.n_queue_checks += 1

    def _take_queue_raw(self):
        """What side_effects_flush() does to the queue, without the pass (which refuses generic boards of more than 4096
        cells): the step kernels get a fresh queue, the filled one's buffers come back as a batch without outputs."""
        from safelife_amd.vector_env import SideEffectBatch
        env = self.env
        env._settle()
        _, bufs = env._se["queue"]
        env._se["queue"] = env._new_queue()
        env.struct.finished = env._se["queue"][0]
        env._caller_ahead = True
        return SideEffectBatch(env, bufs, dict(counts=None, keys=None, life_dist=None, type_masks=None), 2)

    def cache_flags(self, step, seen):
        """After a single-step launch a group's flag is up exactly when every board of it has static goals."""
        env, case = self.env, self.case
        if not env.goal_cache_group:
            return
        nb = env.goal_cache_group
        static = self.cpu.get("goals_static") == 1
        want = np.array([static[g:g + nb].all() for g in range(0, case.B, nb)], np.int32)
        _same(case, env.goal_cache_flags().astype(np.int32), want, "goal-cache flags", step)
        level = self.cpu.get("level_idx")
        seen["raised"] |= bool(want.any())
        seen["evolving"] |= any(want[g // nb] == 0 and (level[g:g + nb] == smc.EVOLVING_LEVEL).any() for g in range(0, case.B, nb))


def _check_geometry(case, env):
    """The test's model of the geometry against the library's."""
    NB = case.geom["NB"]
    assert NB == smc.EXPECTED_NB[case.H]
    if env.goal_cache_group:
        assert env.goal_cache_group == NB
    if case.front == "plain":
        assert bool(env.goal_cache_group) == smc.goal_cache_expected(case.H, case.W, case.spawn)
        if case.spawn == "still":
            assert bool(env.goal_cache_group) == (case.H not in (20, 12, 10))
    else:
        assert env.goal_cache_group == 0


def _refused_rollout(pair, actions, last):
    """The inaction baseline advances between steps, which the size-generic T-step launch cannot do: the launch is refused
    with its reason and changes nothing -- the state still equals the oracle's (which has not moved) and the outputs are
    those of the step before (`last`)."""
    from safelife_amd._hip import SafeLifeHipError
    import pytest
    env = pair.env
    with pytest.raises(SafeLifeHipError, match="T must be 1"):
        env.rollout(actions)
    assert env.struct.wrap.shaped_reward_t is None
    pair.state("refused rollout")
    pair.outputs("refused rollout", last)


def run_matrix_case(case, generic=False, **device_kw):
    """generic: the batch must run on the size-generic kernels (else on the row kernels); there a case with the inaction
    baseline is refused its 6-step launch and plays those six steps one by one."""
    pair = Pair(case, **device_kw)
    env = pair.env
    if generic:
        assert not env.row_kernels(), "the batch runs on the row kernels"
        assert env.goal_cache_group == 0
    else:
        assert env.row_kernels(), "the batch runs on the size-generic kernels"
        _check_geometry(case, env)
    pair.reset()
    pair.state("reset", ("board", "goals", "agent_loc", "exit_locs", "rng", "level_idx", "required_points"))
    seen = dict(raised=False, evolving=False)
    for t in range(smc.T_SINGLE):                       # scripted single steps: every output at every step
        env.step(case.actions[t])
        last = pair.oracle_step()
        pair.outputs(t, last)
        pair.queue(t)
        if case.front == "plain":
            pair.cache_flags(t, seen)
        if t % 4 == 3:
            pair.state(t)
        if t == case.reset_at:                          # a masked reset in the middle: those envs take their next level now
            env.reset(case.reset_mask)
            pair.cpu.env.reset(case.reset_mask)
            pair.state("%d (masked reset)" % t, RESET_STATE)
    pair.state(smc.T_SINGLE - 1)
    t0 = smc.T_SINGLE                                   # the same variant's T-step kernel: six steps in one launch
    if generic and case.inaction:
        _refused_rollout(pair, case.actions[t0:t0 + smc.T_ROLLOUT], last)
        for t in range(t0, t0 + smc.T_ROLLOUT):
            env.step(case.actions[t])
            pair.outputs(t, pair.oracle_step())
        want = None
    else:
        r_t, d_t = env.rollout(case.actions[t0:t0 + smc.T_ROLLOUT])
        want = [pair.oracle_step() for _ in range(smc.T_ROLLOUT)]
        _same(case, r_t.cpu().numpy(), np.stack([w[1] for w in want]), "reward_t", "rollout")
        _same(case, d_t.cpu().numpy(), np.stack([w[2] for w in want]), "done_t", "rollout")
        _same(case, pair.dev.get("reward"), want[-1][1], "reward", "rollout")
        _same(case, pair.dev.get("done"), want[-1][2], "done", "rollout")
        if case.wrapped:
            _same(case, env.shaped_reward_t.cpu().numpy(), np.stack([w[3] for w in want]), "shaped_reward_t", "rollout")
            _same(case, pair.dev.get("shaped_reward"), want[-1][3], "shaped_reward", "rollout")
        pair.obs("rollout", want[-1][0])
    pair.queue("rollout")
    pair.state("rollout")
    t = t0 + smc.T_ROLLOUT                              # and a single step behind it (the cache starts over)
    env.step(case.actions[t])
    pair.outputs(t, pair.oracle_step())
    pair.queue(t)
    pair.state(t)
    if case.front == "plain":
        pair.cache_flags(t, seen)
        if env.goal_cache_group:
            assert seen["raised"] and seen["evolving"], seen
    if case.queue_capacity:
        assert pair.n_queue_checks == smc.T_SINGLE + 2 and pair.n_dropped > 0, "the queue never overflowed"
    return pair
