"""GPU suite: the fused step of every row-kernel shape, in every variant pick_rollout_t chooses from, against the oracle on
the constructed cases of tests/step_matrix_cases.py (what the cases exercise is asserted by tests/test_step_matrix_host.py
on the oracle alone).  Fourteen shapes x twelve configurations: one or several points tables x spawner-free or spawner
pool x plain / observation-or-queue / wrappers, each through single-step launches and one T-step launch; per shape also a
batch that ends inside a wave, two slices, and the library's own queues.  Integer work and float64 sums made in the
oracle's order: every comparison is np.array_equal.
"""
import numpy as np
import pytest

from tests import step_matrix_cases as smc
from tests import util

pytestmark = pytest.mark.gpu

ALL = smc.all_cases()
# what a reset writes: the state without the outputs of the step before it
RESET_STATE = tuple(n for n in smc.ENV_STATE if n not in ("success", "times_up"))


def _same(case, got, want, field, step):
    """Bit-exact, and on a mismatch name the case, the step, the field and the first differing env."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want):
        return
    where = "%s %s B=%d, step %s, %s" % (smc.case_id(case.H, case.cfg), case.batch, case.B, step, field)
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

    def __init__(self, case, **device_kw):
        self.case = case
        pool = case.pool(util.oracle_counts)
        self.dev = util.DeviceBackend(pool, case.B, **dict(case.backend_kw(device=True), **device_kw))
        self.cpu = util.OracleBackend(pool, case.B, **case.backend_kw(device=False))
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
        batch = self.env.side_effects_flush()
        n, dropped = len(batch), batch.dropped()
        assert n + dropped == len(self.queued), "%s step %s: %d episodes queued or dropped, the oracle finished %d" % (
            smc.case_id(case.H, case.cfg), step, n + dropped, len(self.queued))
        assert n == min(len(self.queued), case.queue_capacity)
        recs = batch.records()
        boards = batch.boards[:n].cpu().numpy().view(np.uint16)
        keys = [(int(recs["env"][i]), int(recs["episode_idx"][i])) for i in range(n)]
        assert len(set(keys)) == n, "an episode was queued twice"
        for i in np.lexsort(([k[1] for k in keys], [k[0] for k in keys])) if n else ():
            assert keys[i] in self.queued, "%s step %s: queued %r, which the oracle did not finish" % (
                smc.case_id(case.H, case.cfg), step, keys[i])
            _, _, level, num_steps, board, success, times_up, ep_reward, ep_length = self.queued[keys[i]]
            got = (int(recs["level"][i]), int(recs["num_steps"][i]), int(recs["success"][i]), int(recs["times_up"][i]),
                   float(recs["episode_reward"][i]), int(recs["episode_length"][i]))
            assert got == (level, num_steps, success, times_up, ep_reward, ep_length), (step, keys[i], got)
            _same(case, boards[i:i + 1], board[None], "queued board of env %d" % keys[i][0], step)
        self.n_dropped += dropped
        self.queued = {}
        self.n_queue_checks += 1

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


def _run_matrix_case(case):
    pair = Pair(case)
    env = pair.env
    assert env.row_kernels(), "the batch runs on the size-generic kernels"
    _check_geometry(case, env)
    pair.reset()
    pair.state("reset", ("board", "goals", "agent_loc", "exit_locs", "rng", "level_idx", "required_points"))
    seen = dict(raised=False, evolving=False)
    for t in range(smc.T_SINGLE):                       # scripted single steps: every output at every step
        env.step(case.actions[t])
        pair.outputs(t, pair.oracle_step())
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
    r_t, d_t = env.rollout(case.actions[t0:t0 + smc.T_ROLLOUT])
    want = [pair.oracle_step() for _ in range(smc.T_ROLLOUT)]
    _same(case, r_t.cpu().numpy(), np.stack([w[1] for w in want]), "reward_t", "rollout")
    _same(case, d_t.cpu().numpy(), np.stack([w[2] for w in want]), "done_t", "rollout")
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


@pytest.mark.parametrize("H,cfg", ALL, ids=[smc.case_id(H, cfg) for H, cfg in ALL])
def test_fused_step_vs_oracle(H, cfg):
    """One (shape, configuration): reset, 24 scripted single steps, a masked reset in the plain ones, a 6-step launch and a
    single step behind it -- reward, done, observation, shaped reward and queue at every step, the whole state every
    four -- and, on the wide shapes, the plain configurations once more with a finished-episode queue."""
    _run_matrix_case(smc.Case(H, cfg))
    if cfg[2] == "plain" and smc.geometry(H, H)["lean_takes_queue"]:
        _run_matrix_case(smc.Case(H, cfg, queue=True))


@pytest.mark.parametrize("H", smc.SHAPES)
def test_batch_that_ends_inside_a_wave(H):
    """NB - 1 envs: the only workgroup's last wave is one board short -- partly filled where a wave holds several boards,
    empty where it holds one (40, 48 and 64 rows) -- with wrappers, the inaction baseline and several tables."""
    _run_matrix_case(smc.Case(H, ("many", "spawn", "wrap"), batch="small"))


def test_row_kernels_answer_tells_the_families_apart():
    """env.row_kernels() is what every case above asserts: it must say no for a batch the size-generic kernels run."""
    from safelife_amd.cell_types import CellTypes as CT
    from safelife_amd.levels import Level, LevelPool
    board = np.zeros((9, 13), np.uint16)
    board[4, 6] = CT.player
    pool = LevelPool([Level(board, None, [[4, 6]], min_performance=-1)], counts_fn=util.oracle_counts)
    assert not util.DeviceBackend(pool, 3, first_level=0).env.row_kernels()
    wide = smc.Case(64, ("one", "still", "obs"))
    kw = dict(wide.backend_kw(device=True), view_shape=(40, 40), output_channels=smc.CHANNELS_15)
    assert util.DeviceBackend(wide.pool(util.oracle_counts), wide.B, **kw).env.row_kernels()
    # (a view of 1600 cells is more than the fused policy-layout epilogue of 64-cell rows can stage)
    assert not util.DeviceBackend(wide.pool(util.oracle_counts), wide.B, policy_layout="uint8", **kw).env.row_kernels()


def _sliced_case(H):
    return smc.Case(H, ("one", "spawn", "plain"), B=129, n_steps=12)


@pytest.mark.parametrize("H", smc.SHAPES)
def test_two_slices_vs_oracle(H):
    """slices=2 at 129 envs through step_async(): the second slice starts at env 128 (on shapes whose workgroups hold 12, 20
    or 24 boards that is off the workgroups' grid of the whole batch) and is a workgroup of one board."""
    import torch
    case = _sliced_case(H)
    pair = Pair(case, slices=2)
    env = pair.env
    assert env.slices == 2 and env.slice_bounds == (0, 128, 129) and env.row_kernels()
    pair.reset()
    acts = torch.from_numpy(case.actions).to(env.device)
    torch.cuda.synchronize()
    for t in range(case.n_steps):
        env.step_async(acts[t])
        pair.outputs(t, pair.oracle_step())
        if t % 4 == 3:
            pair.state(t)
        if t == case.reset_at:
            env.reset(case.reset_mask)
            pair.cpu.env.reset(case.reset_mask)
    env.join()
    pair.state(case.n_steps - 1)
    if env.goal_cache_group:                # a raised flag implies static goals on every board of its group
        static = pair.cpu.get("goals_static") == 1
        for g in np.nonzero(env.goal_cache_flags())[0]:
            assert static[g * env.goal_cache_group:(g + 1) * env.goal_cache_group].all(), g


def _open_queues(env, case):
    """queues_open(2) -> True, or None where the runtime has no HSA queue to give (the one refusal a box may answer with).
    A batch the library's queues cannot dispatch must be one of smc.QUEUES_CANNOT_DISPATCH, refused when they are opened
    and for that reason -> False; and such a batch must be refused."""
    from safelife_amd._hip import SafeLifeHipError
    known = (case.H, case.spawn) in smc.QUEUES_CANNOT_DISPATCH
    try:
        env.queues_open(2)
    except SafeLifeHipError as e:
        if "AQL queues unavailable" in str(e):
            print("no HSA queue on this box, the same steps on the streams:", e)
            return None
        assert known and "AQL queues cannot dispatch this batch" in str(e) and "private memory" in str(e), e
        return False
    assert not known, "the queues opened for a batch listed in QUEUES_CANNOT_DISPATCH: take it off the list"
    assert env.queue_slices == 2
    return True


def _queue_run(case):
    import torch
    pair = Pair(case)
    env = pair.env
    assert env.row_kernels()
    pair.reset()
    acts = torch.from_numpy(case.actions).to(env.device)
    torch.cuda.synchronize()
    for t in range(4):
        env.step(acts[t])
        pair.outputs(t, pair.oracle_step())
    queued = _open_queues(env, case)
    for lo, hi in ((4, case.reset_at + 1), (case.reset_at + 1, case.n_steps)):
        if queued:
            env.step_queues_many(acts[lo:hi])
            env.queues_sync()
        else:                                   # what a caller does that was refused: the same steps on the streams
            for t in range(lo, hi):
                env.step_async(acts[t])
        for t in range(lo, hi):
            want = pair.oracle_step()
        pair.outputs(hi - 1, want)
        pair.state(hi - 1)
        if hi == case.reset_at + 1:
            env.reset(case.reset_mask)
            pair.cpu.env.reset(case.reset_mask)
            pair.state("%d (masked reset)" % (hi - 1), RESET_STATE)
    env.queues_close()
    return queued


@pytest.mark.parametrize("H", smc.SHAPES)
def test_queue_steps_vs_oracle(H):
    """The library's own AQL queues on the same batch: the prepared launch takes its LDS size and its grid from the
    shape.  Four stream steps, six steps in one queue call, a masked reset, two more queue steps.  Only a runtime without
    HSA queues may send the steps to the streams instead.  The one exception is pinned as such: 32x32 spawner pools, whose
    single-step kernels spill, are refused by queues_open() -- never by a step -- so the queues are NOT exercised on that
    batch; its steps go through step_async(), and the shape's queue launch runs on the spawner-free pool instead."""
    queued = _queue_run(_sliced_case(H))
    if (H, "spawn") in smc.QUEUES_CANNOT_DISPATCH:
        assert queued in (False, None)
        assert _queue_run(smc.Case(H, ("one", "still", "plain"), B=129, n_steps=12)) in (True, None)
    else:
        assert queued in (True, None)
