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
from tests.step_matrix_flow import RESET_STATE, Pair, run_matrix_case as _run_matrix_case

pytestmark = pytest.mark.gpu

ALL = smc.all_cases()


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
