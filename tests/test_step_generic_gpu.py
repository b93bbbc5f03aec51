"""GPU suite: the size-generic single-agent kernels (k_env_rollout_generic, k_env_reset_generic, k_env_obs_generic,
k_inaction_generic) against the oracle on the constructed cases of tests/step_generic_cases.py -- what the cases exercise is
asserted by tests/test_step_generic_host.py on the oracle alone.  Twelve shapes on the edges of the family's three
workgroup sizes, of ca_step_block's 64-bit eligibility mask and of the row index taken from a float reciprocal; the flow of
the row-kernel matrix (tests/step_matrix_flow.py); sliced stepping, compact records, the successor table, episode streams,
get_obs(), the row-kernel shapes that fall back to the family, and hand-made 3x3 / 3x86 pools.  Integer work and float64
sums made in the oracle's order: every comparison is np.array_equal.
"""
import numpy as np
import pytest

from tests import obs_ref
from tests import step_generic_cases as sgc
from tests import step_matrix_cases as smc
from tests import util
from tests.step_matrix_flow import RESET_STATE, Pair, _same, run_matrix_case

pytestmark = pytest.mark.gpu

ALL = sgc.all_cases()


@pytest.mark.parametrize("H,W,cfg", ALL, ids=[sgc.case_id(*c) for c in ALL])
def test_generic_step_vs_oracle(H, W, cfg):
    """One (shape, configuration) on the size-generic kernels: reset, 24 scripted single steps, a masked reset in the plain
    ones, a 6-step launch -- refused, with nothing changed, where the wrappers carry the inaction baseline, and played as six
    single steps there -- and a single step behind it: reward, done, observation, shaped reward and queue at every step,
    the whole state every four."""
    case = sgc.case(H, W, cfg)
    pair = run_matrix_case(case, generic=True)
    assert pair.env.struct.H * pair.env.struct.W == H * W and smc.generic_threads(H * W) == sgc.SHAPES[(H, W)][0]


@pytest.mark.parametrize("kind", sgc.FALLBACKS)
def test_row_shapes_that_fall_back(kind):
    """A row-kernel shape that use_rowlane() sends to the size-generic family -- a ninth exit slot, points outside int8, a
    policy-layout view too large to stage -- runs the whole flow there; the same batch without the change is one the row
    kernels take."""
    plain = sgc.fallback_case(kind, changed=False)
    assert Pair(plain).env.row_kernels(), "the unchanged batch left the row kernels"
    run_matrix_case(sgc.fallback_case(kind), generic=True)


def test_flush_refuses_generic_boards_above_4096_cells():
    """Why the queues of the cases above smc.GENERIC_QUEUE_MAX_CELLS are read without a flush (Pair._take_queue_raw): the
    step kernel queues their finished episodes, but the pass a flush runs takes generic boards of up to 4096 cells and
    says so."""
    from safelife_amd._hip import SafeLifeHipError
    case = sgc.case(100, 100, ("many", "still", "obs"))
    assert case.queue_raw and not sgc.case(25, 41, ("many", "still", "obs")).queue_raw
    dev = util.DeviceBackend(case.pool(util.oracle_counts), case.B, **case.backend_kw(device=True))
    assert not dev.env.row_kernels() and dev.env.struct.finished.capacity == case.queue_capacity > 0
    dev.env.reset()
    dev.env.step(case.actions[0])
    with pytest.raises(SafeLifeHipError, match="more than 4096 cells"):
        dev.env.side_effects_flush()


def _sliced(B):
    return sgc.case(13, 20, ("one", "spawn", "plain"), B=B, n_steps=12)


@pytest.mark.parametrize("B", [1, 129])
def test_generic_slices_vs_oracle(B):
    """slices=2 at 13x20 through step_async(): one env (a single slice, one workgroup) and 129 (the second slice is env 128
    alone: slhip_env_step_slices -> env_slice).  The family has no launch for the library's own queues, which step slices
    T at a time: opening them is refused with that reason, and changes nothing."""
    import torch
    from safelife_amd._hip import SafeLifeHipError
    case = _sliced(B)
    pair = Pair(case, slices=2)
    env = pair.env
    assert not env.row_kernels()
    assert (env.slices, env.slice_bounds) == ((2, (0, 128, 129)) if B == 129 else (1, (0, 1)))
    pair.reset()
    acts = torch.from_numpy(case.actions).to(env.device)
    torch.cuda.synchronize()
    for t in range(case.n_steps):
        env.step_async(acts[t])
        pair.outputs(t, pair.oracle_step())
        if t % 4 == 3:
            pair.state(t)
        if t == 5:
            with pytest.raises(SafeLifeHipError, match="queue stepping needs the row kernels"):
                env.queues_open(env.slices)
            pair.state("%d (refused queues)" % t)
        if t == case.reset_at:
            env.reset(case.reset_mask)
            pair.cpu.env.reset(case.reset_mask)
            pair.state("%d (masked reset)" % t, RESET_STATE)
    env.join()
    pair.state(case.n_steps - 1)


def test_generic_compact_records():
    """set_step_outputs(ptr, compact=True) at 13x20: after every single step, and after a 6-step launch, the 8-byte records
    in the test's own tensor are (reward bits, done, success, times_up, 0) of the oracle, and the env's own record tensor is
    never written."""
    import torch
    case = sgc.case(13, 20, ("one", "spawn", "plain"))
    pair = Pair(case)
    env, cpu = pair.env, pair.cpu
    assert not env.row_kernels()
    pair.reset()
    mine = torch.full((case.B,), -1, dtype=torch.int64, device=env.device)
    own = env.t["out"]
    own.fill_(0x5A5A5A5A)
    own0 = own.cpu().numpy().copy()
    env.set_step_outputs(mine.data_ptr(), compact=True)

    def records(step, want):
        _, r, d, _ = want
        rec = mine.cpu().numpy().view(np.uint8).reshape(case.B, 8)
        _same(case, rec[:, :4].copy().view(np.uint32)[:, 0], r.astype(np.float32).view(np.uint32), "record.reward bits", step)
        flags = np.stack([d.astype(np.uint8), cpu.get("success").astype(np.uint8), cpu.get("times_up").astype(np.uint8),
                          np.zeros(case.B, np.uint8)], axis=1)
        _same(case, rec[:, 4:], flags, "record.flags (done, success, times_up, 0)", step)
        assert np.array_equal(own.cpu().numpy(), own0), "step %s wrote the env's own records" % step

    seen = np.zeros(3, bool)
    for t in range(smc.T_SINGLE):
        env.step(case.actions[t])
        want = pair.oracle_step()
        records(t, want)
        seen |= [bool(want[2].any()), bool(cpu.get("success").any()), bool(cpu.get("times_up").any())]
        if t % 4 == 3:
            pair.state(t, [n for n in smc.ENV_STATE if n not in ("success", "times_up")])
        if t == case.reset_at:
            env.reset(case.reset_mask)
            cpu.env.reset(case.reset_mask)
    assert seen.all(), "done, success and times_up were all reported at some step"
    t0 = smc.T_SINGLE
    r_t, d_t = env.rollout(case.actions[t0:t0 + smc.T_ROLLOUT])
    want = [pair.oracle_step() for _ in range(smc.T_ROLLOUT)]
    _same(case, r_t.cpu().numpy(), np.stack([w[1] for w in want]), "reward_t", "rollout")
    _same(case, d_t.cpu().numpy(), np.stack([w[2] for w in want]), "done_t", "rollout")
    records("rollout", want[-1])
    env.set_step_outputs(None)                      # back on the env's own tensor: whole records again
    assert env.struct.out_compact == 0
    before = mine.clone()
    env.step(case.actions[t0 + smc.T_ROLLOUT])
    pair.outputs(t0 + smc.T_ROLLOUT, pair.oracle_step())
    pair.state(t0 + smc.T_ROLLOUT)
    assert torch.equal(mine, before)


def test_generic_successor_table():
    """A LevelPool(refreshable=True) at 13x20: two levels are replaced between steps (pool_stage / pool_commit), then one
    of them again together with a third; the device follows the successor table exactly as the oracle does -- through the
    in-kernel resets, a masked reset and a 6-step launch -- and envs load from both banks."""
    from safelife_amd.levels import LevelPool
    case = sgc.case(13, 20, ("one", "spawn", "plain"))
    other = smc.build_levels(13, 20, "one", "still")
    pools = [LevelPool(case.levels, counts_fn=util.oracle_counts, min_performance_fraction=1.0, refreshable=True) for _ in range(2)]
    pool_dev, pool_cpu = pools
    assert pool_dev.n_slots == 2 * smc.N_LEVELS
    pair = Pair(case, pools=pools)
    env, cpu = pair.env, pair.cpu
    assert not env.row_kernels()
    cpu.env.set_pool_next(pool_cpu.next_table(1))
    pair.reset()
    plan = {5: ([2, 5], [other[4], other[1]]), 13: ([2, 7], [other[6], other[0]])}      # staged behind step t, committed two later
    staged, banks = None, set()

    def commit():
        env.pool_commit()
        assert pool_cpu.replace(*staged[:2]) == staged[2]           # the same spare slots on both sides
        cpu.env.set_pool_next(pool_cpu.next_table(1))

    for t in range(smc.T_SINGLE):
        env.step(case.actions[t])
        pair.outputs(t, pair.oracle_step())
        pair.state(t)
        banks |= {int(l) // smc.N_LEVELS for l in cpu.get("level_idx")}
        if t in plan:
            staged = plan[t] + (env.pool_stage(*plan[t]),)
        if t - 2 in plan:
            commit()
        if t == case.reset_at:
            env.reset(case.reset_mask)
            cpu.env.reset(case.reset_mask)
            pair.state("%d (masked reset)" % t, RESET_STATE)
            banks |= {int(l) // smc.N_LEVELS for l in cpu.get("level_idx")}
    assert banks == {0, 1}
    lvl = cpu.get("level_idx")
    assert np.array_equal(pool_dev.bank, pool_cpu.bank) and pool_cpu.bank[2] == 0 and pool_cpu.bank[5] == 1 and pool_cpu.bank[7] == 1
    t0 = smc.T_SINGLE
    r_t, d_t = env.rollout(case.actions[t0:t0 + smc.T_ROLLOUT])
    want = [pair.oracle_step() for _ in range(smc.T_ROLLOUT)]
    _same(case, r_t.cpu().numpy(), np.stack([w[1] for w in want]), "reward_t", "rollout")
    _same(case, d_t.cpu().numpy(), np.stack([w[2] for w in want]), "done_t", "rollout")
    pair.state("rollout")
    assert (cpu.get("level_idx") != lvl).any()


@pytest.mark.parametrize("streams", [True, False])
def test_generic_episode_streams(streams):
    """episode_streams on (stream_salt = 1 + env_offset: every episode of every env draws from a stream of its own) and off
    (the pool's generators as they are), at 7x11 on a spawner pool: the generator words equal the oracle's after the
    reset, after every step -- so after every in-kernel reset -- and after a masked reset."""
    case = sgc.case(7, 11, ("many", "spawn", "plain"))
    case.kw.update(episode_streams=streams, env_offset=5)
    pair = Pair(case)
    env, cpu = pair.env, pair.cpu
    assert not env.row_kernels() and env.struct.stream_salt == (6 if streams else 0)
    pair.reset()
    pair.state("reset", ("rng", "board"))
    pool_rng = case.pool(util.oracle_counts).arrays()["pool_rng"]
    same_as_pool = (cpu.get("rng") == pool_rng[case.first_level]).all(axis=1)
    assert same_as_pool.all() if not streams else not same_as_pool.any()
    n_resets = 0
    for t in range(smc.T_SINGLE):
        env.step(case.actions[t])
        want = pair.oracle_step()
        pair.outputs(t, want)
        pair.state(t, ("rng", "episode_idx", "level_idx", "board"))
        n_resets += int(want[2].sum())
        if t == case.reset_at:
            env.reset(case.reset_mask)
            cpu.env.reset(case.reset_mask)
            pair.state("%d (masked reset)" % t, RESET_STATE)
    assert n_resets >= 2 * case.B


@pytest.mark.parametrize("H,W", [(31, 33), (128, 128)])
def test_generic_get_obs_after_steps(H, W):
    """get_obs() (k_env_obs_generic) behind ten steps: the observation tensor, wiped first, comes back equal to the
    oracle's and to tests/obs_ref.py on the state read back from the device; the state is left alone."""
    case = sgc.case(H, W, ("one", "still", "obs"))              # the raw view, larger than the board
    vh, vw = case.kw["view_shape"]
    assert vh > H and vw > W and case.kw["output_channels"] is None
    pair = Pair(case)
    env = pair.env
    assert not env.row_kernels()
    pair.reset()
    for t in range(10):
        env.step(case.actions[t])
        want = pair.oracle_step()
    pair.outputs(9, want)
    state = {n: pair.dev.get(n) for n in smc.ENV_STATE}
    env.obs.fill_(-1)
    env.get_obs()
    _same(case, pair.dev.get("obs"), want[0], "obs", "get_obs")
    for e in range(case.B):
        ref = obs_ref.get_obs(state["board"][e], state["goals"][e], state["agent_loc"][e], state["exit_locs"][e], (vh, vw), None)
        assert obs_ref.first_difference(pair.dev.get("obs")[e].view(np.uint32), ref) is None, (e, obs_ref.first_difference(
            pair.dev.get("obs")[e].view(np.uint32), ref))
    for n in smc.ENV_STATE:
        _same(case, pair.dev.get(n), state[n], n, "get_obs (state left alone)")
    pair.state("get_obs")


@pytest.mark.parametrize("H,W", sgc.FLOOR_SHAPES)
def test_generic_floor(H, W):
    """3x3 (every cell a neighbour of every other; a 5x7 view larger than the board) and 3x86 (W = 3 neighbours in y, 86-cell
    rows on 128 threads): the hand-made pools of tests/step_generic_cases.py under their fixed 20-step scripts -- reward,
    done, observation and the whole state at every step, through in-kernel resets and a masked reset."""
    pool = sgc.floor_pool(H, W, util.oracle_counts)
    kw = sgc.floor_kw()
    dev = util.DeviceBackend(pool, sgc.FLOOR_B, **kw)
    cpu = util.OracleBackend(pool, sgc.FLOOR_B, **kw)
    assert not dev.env.row_kernels()

    def same(what, t, names=smc.ENV_STATE):
        for n in names:
            got, want = dev.get(n), cpu.get(n)
            assert got.dtype == want.dtype and np.array_equal(got, want), "%dx%d step %s (%s): %s differs in envs %s" % (
                H, W, t, what, n, np.nonzero((got != want).reshape(sgc.FLOOR_B, -1).any(axis=1))[0])

    assert np.array_equal(dev.reset(), cpu.reset())
    same("reset", "reset", RESET_STATE)
    for t in range(sgc.FLOOR_STEPS):
        a = sgc.floor_actions(cpu.get("level_idx"), t)
        o1, r1, d1 = dev.step(a)
        o2, r2, d2 = cpu.step(a)
        assert np.array_equal(r1, r2) and np.array_equal(d1, d2), (t, r1, r2, d1, d2)
        assert o1.shape == o2.shape == (sgc.FLOOR_B,) + sgc.FLOOR_VIEW and np.array_equal(o1.view(np.uint32), o2.view(np.uint32)), t
        same("step", t)
        if t == sgc.FLOOR_RESET_AT:
            dev.env.reset(sgc.FLOOR_RESET_MASK)
            cpu.env.reset(sgc.FLOOR_RESET_MASK)
            same("masked reset", t, RESET_STATE)
            assert np.array_equal(dev.get("obs").view(np.uint32), cpu.env.obs.view(np.uint32))
