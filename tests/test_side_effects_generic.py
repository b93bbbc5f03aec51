"""The episode-end pass of side_effect_score on board shapes WITHOUT row kernels (and on unaligned boards): the
size-generic occupancy kernel (csrc/sl_generic.hip: k_occupancy_generic, uint16 counters in LDS) and slhip_side_effects
on top of it, through the C-ABI, SafeLifeVectorEnv(side_effects=...) and SafeLifeMultiAgentVectorEnv(side_effects=...).

The reference of every occupancy tensor is the CPU oracle's one-board primitives (oracle.advance_board, then
oracle.life_occupancy) under the entry's own generator; integer work, every comparison bit-exact.  Levels are hand-made
(random palette cells, spawners of several colours, frozen and destructible cell types, agent, exit, spawn_prob 0.3 or
0.9); every level a pass test uses is checked, on the oracle, to hold a spawner and to have at least two colours of
countable life after its roll-forward.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from tests import util

PAL = np.array([0] * 14 + [9] * 5 + [1, 16, 17, 32788, 48, 53, 85, 32884, 9 | 0x200, 9 | 0x400, 9 | 0x800, 9 | 0xE00,
                              4 | 8, 32, 64], np.uint16)
SPAWN = np.array([152, 152 | 0x200, 152 | 0x600, 144 | 0x800], np.uint16)
PLAYER, EXIT_CELL = 122, 16 | 256
ALIVE, AGENT, FROZEN, SPAWNING, EXIT = 1, 2, 16, 128, 256


def _device_counts(boards, goals):
    from safelife_amd.levels import _device_counts as f
    return f(boards, goals)


def make_level(rng, H, W, n_agents=1):
    """Palette soup + max(2, H*W/50) spawners cycling through four colours + one exit + the agents, all on distinct cells."""
    from safelife_amd.levels import Level
    b = PAL[rng.integers(0, len(PAL), (H, W))]
    n_sp = max(2, H * W // 50)
    cells = rng.permutation(H * W)[:n_sp + 1 + n_agents]
    flat = b.reshape(-1)
    for k in range(n_sp):
        flat[cells[k]] = SPAWN[k % len(SPAWN)]
    flat[cells[n_sp]] = EXIT_CELL
    locs = []
    for a in range(n_agents):
        flat[cells[n_sp + 1 + a]] = PLAYER
        locs.append([int(cells[n_sp + 1 + a]) // W, int(cells[n_sp + 1 + a]) % W])
    g = ((rng.integers(0, 8, (H, W)) << 9) * (rng.random((H, W)) < 0.3)).astype(np.uint16)
    return Level(b, g, locs, spawn_prob=float(rng.choice([0.3, 0.9])), min_performance=-1)


def make_pool(seed, H, W, n, n_agents=1, counts_fn=_device_counts):
    from safelife_amd.levels import LevelPool
    rng = np.random.default_rng(seed)
    levels = [make_level(rng, H, W, n_agents) for _ in range(n)]
    kw = dict(n_agents=n_agents) if n_agents > 1 else {}
    return LevelPool(levels, counts_fn=counts_fn, **kw)


def countable_colours(board):
    """The colours (0..7) of the cells life_occupancy would count on `board`."""
    b = np.asarray(board, np.uint16).astype(np.int64)
    m = ((b & ALIVE) != 0) & ((b & (AGENT | EXIT | FROZEN)) == 0)
    return set(((b[m] >> 9) & 7).tolist())


def _mix64(z):
    m = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def derived_reference(pool, level, final_board, env_id, episode, steps, n_samples):
    """(b1, inaction tensor, action tensor) of one queue entry from the oracle's one-board primitives under the entry's
    two derived streams (k_se_gather: the level's generator XOR mix64 words of (salt ^ env, episode), run 1 derived from
    run 0's).  Also checks the level: a spawner, and two colours of countable life after the roll-forward."""
    lv = pool.levels[level]
    p = float(np.float32(lv.spawn_prob))
    words = pool.arrays()["pool_rng"][level].copy()
    bg = np.random.PCG64(0)
    out = []
    for salt in (0x5EFFEC75, 0x2B0A2D5):
        a_ = _mix64((((salt ^ env_id) & 0xFFFFFFFF) << 32) | episode)
        words[0] ^= np.uint64(a_)
        words[1] ^= np.uint64(_mix64(a_))
        oracle.pcg64_set_state_words(bg, words)
        if not out:
            b1 = oracle.advance_board(lv.board, p, steps, bitgen=bg)
            out += [b1, oracle.life_occupancy(b1, p, n_samples, bitgen=bg)]
        else:
            out.append(oracle.life_occupancy(final_board, p, n_samples, bitgen=bg))
    assert (lv.board & SPAWNING).any(), level
    assert len(countable_colours(out[0])) >= 2, (level, steps)
    return out


# ------------------------------------------------------------------ CPU: the levels are what the tests say they are

@pytest.mark.parametrize("shape", [(13, 17), (20, 40), (7, 11), (25, 25), (9, 13)])
def test_hand_made_levels_have_spawners_and_two_colours(shape):
    """Every level of the pools below holds spawners of several colours, frozen and destructible cell types, an agent
    and an exit, and shows at least two colours of countable life after 0, 9 and 11 oracle steps."""
    pool = make_pool(100 + shape[0], shape[0], shape[1], 6, n_agents=2 if shape == (9, 13) else 1,
                     counts_fn=util.oracle_counts)
    probs = set()
    for k, lv in enumerate(pool.levels):
        b = lv.board.astype(np.int64)
        assert ((b & SPAWNING) != 0).sum() >= 2 and len(set((b[(b & SPAWNING) != 0] >> 9).tolist())) >= 2
        assert ((b & FROZEN) != 0).any() and ((b & 8) != 0).any() and (b == PLAYER).sum() == len(lv.agent_locs)
        assert (b == EXIT_CELL).sum() == 1
        probs.add(round(lv.spawn_prob, 1))
        for n in (0, 9, 11):
            after = oracle.advance_board(lv.board, lv.spawn_prob, n, rng_words=pool.arrays()["pool_rng"][k].copy())[0]
            assert len(countable_colours(after)) >= 2, (k, n)
    assert probs <= {0.3, 0.9}


# ------------------------------------------------------------------ 1. the kernel against the oracle, shape sweep

SWEEP = [(3, 3), (3, 64), (64, 3), (7, 11), (13, 17), (33, 64), (63, 64), (64, 63), (25, 25)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SWEEP)
def test_life_occupancy_generic_shapes(shape):
    """slhip_life_occupancy on B = 5 boards of every sweep shape (all but 25x25 have no row kernel), 1, 2 and 257 steps:
    counts and generator state after the call equal the oracle's, bit for bit.  (The public entry keeps its global-
    memory counters on these shapes, DESIGN 4.4: a guard for the day that changes; the LDS-counter kernel itself is
    swept through the pass, test_pass_kernel_sweep_on_a_hand_filled_queue.)"""
    import torch
    from safelife_amd import speedups as sp
    H, W = shape
    rng = np.random.default_rng(7 * H + W)
    boards = np.stack([make_level(rng, H, W).board for _ in range(5)])
    assert all((b & SPAWNING).any() for b in boards)
    p = rng.choice([0.3, 0.9], 5).astype(np.float32)
    words = util.random_rng_words(rng, 5)
    d_b = sp._to_device(boards, np.uint16)
    d_p = torch.from_numpy(p).to(d_b.device)
    total = 0
    for n_steps in (1, 2, 257):
        w_cpu = words.copy()
        want = oracle.life_occupancy_batch(boards, p, n_steps, w_cpu, n_threads=4)
        d_rng = sp._to_device(words.copy(), np.uint64)
        got = sp.life_occupancy_batch(d_b, d_p, d_rng, n_steps).cpu().numpy()
        assert np.array_equal(got, want), n_steps
        assert np.array_equal(sp._to_host(d_rng, np.uint64), w_cpu), n_steps
        total = want.reshape(-1, 8).sum(axis=0)
    if H * W >= 77:         # (boards of a few cells may die out; the others tick at least two colours in 257 steps)
        assert (total > 0).sum() >= 2


@pytest.mark.gpu
def test_life_occupancy_generic_counter_reaches_65535():
    """n_steps = 65535 on 3x3 boards whose every cell is alive, preserving and not frozen (nothing on them ever dies):
    counters end at 65535, the top of a uint16 (through the public entry; test_pass_counter_reaches_65535 does the same
    through the pass, which is where the uint16 LDS counters are)."""
    import torch
    from safelife_amd import speedups as sp
    rng = np.random.default_rng(3)
    boards = np.full((5, 3, 3), ALIVE | 32, np.uint16)
    boards[1] |= 0x200
    boards[2, 1, 1] = 9 | 0x400
    boards[3] = PAL[rng.integers(0, len(PAL), (3, 3))]
    boards[4] = (ALIVE | 32) | (rng.integers(0, 8, (3, 3)) << 9).astype(np.uint16)
    assert not (boards[[0, 1, 2, 4]] & FROZEN).any()
    p = np.full(5, 0.9, np.float32)
    words = util.random_rng_words(rng, 5)
    w_cpu = words.copy()
    want = oracle.life_occupancy_batch(boards, p, 65535, w_cpu, n_threads=4)
    assert want[0].max() == 65535 and want[1, ..., 1].min() == 65535
    d_rng = sp._to_device(words.copy(), np.uint64)
    got = sp.life_occupancy_batch(sp._to_device(boards, np.uint16), torch.from_numpy(p).to(d_rng.device), d_rng, 65535)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(sp._to_host(d_rng, np.uint64), w_cpu)


# ------------------------------------------------------------------ the pass through the C-ABI on a hand-filled queue

CANARY = dict(counts=0x5A5A5A5A, keys=-21846, life_dist=-7.5, type_masks=0xA5, work_rng=0x0123456789ABCDEF,
              work_boards=0x3C3C)


def run_pass(env, H, W, recs, finals, count, cap, n_samples, derive_streams, work_rng=None, offset=0):
    """slhip_side_effects on a hand-filled queue of capacity `cap` whose device-side count is `count`; every output
    starts filled with a canary.  offset: int16 elements by which work_boards and queue.boards are shifted off their
    (256-byte aligned) allocations.  Returns the outputs as host arrays, plus the status code."""
    import torch
    from safelife_amd import _hip
    dev, K = env.device, _hip.SL_SE_MAX_KEYS
    rec = np.zeros((cap, 8), np.int32)
    n = min(len(recs), cap)
    rec[:n] = recs[:n]
    qb = torch.zeros(cap * H * W + 8, dtype=torch.int16, device=dev)
    wb = torch.full((2 * cap * H * W + 8,), CANARY["work_boards"], dtype=torch.int16, device=dev)
    qboards = qb[offset:offset + cap * H * W].view(cap, H, W)
    wboards = wb[offset:offset + 2 * cap * H * W].view(2 * cap, H, W)
    assert qboards.data_ptr() % 16 == 2 * offset and wboards.data_ptr() % 16 == 2 * offset
    qboards[:n] = torch.from_numpy(np.ascontiguousarray(finals[:n]).view(np.int16)).to(dev)
    bufs = dict(count=torch.tensor([count], dtype=torch.int32, device=dev), records=torch.from_numpy(rec).to(dev),
                boards=qboards)
    q = _hip.EpisodeQueue()
    q.capacity, q.env_base = cap, 0
    q.count, q.records, q.boards = (bufs[k].data_ptr() for k in ("count", "records", "boards"))
    rng_t = torch.full((2 * cap, 4), CANARY["work_rng"], dtype=torch.int64, device=dev)
    if work_rng is not None:
        rng_t[:len(work_rng)] = torch.from_numpy(np.ascontiguousarray(work_rng).view(np.int64)).to(dev)
    out = dict(work_boards=wboards,
               work_prob=torch.zeros(2 * cap, dtype=torch.float32, device=dev),
               work_steps=torch.zeros(2 * cap, dtype=torch.int32, device=dev),
               work_rng=rng_t,
               counts=torch.full((2, cap, H, W, 8), CANARY["counts"], dtype=torch.int32, device=dev),
               keys=torch.full((cap, K), CANARY["keys"], dtype=torch.int16, device=dev),
               life_dist=torch.full((cap, 2, 8, H, W), CANARY["life_dist"], dtype=torch.float64, device=dev),
               type_masks=torch.full((cap, 2, K - 8, H, W), CANARY["type_masks"], dtype=torch.uint8, device=dev))
    rc = _hip.lib().slhip_side_effects(env._sref, C.byref(q), n_samples, derive_streams,
                                       *[_hip.ptr(out[k]) for k in ("work_boards", "work_prob", "work_steps", "work_rng",
                                                                    "counts", "keys", "life_dist", "type_masks")],
                                       _hip.current_stream_ptr())
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    host["keys"] = host["keys"].view(np.uint16)
    host["work_boards"] = host["work_boards"].view(np.uint16)
    host["work_rng"] = host["work_rng"].view(np.uint64)
    host["records"] = bufs["records"].cpu().numpy()
    return rc, host


def hand_queue(pool, seed, n, steps_of):
    """n hand-made queue entries over the pool's levels: records (env, level, num_steps, episode_idx, spawn_prob) and
    a terminal board each (the level a few oracle steps on, with a few cells knocked out: what an agent leaves)."""
    rng = np.random.default_rng(seed)
    L = len(pool.levels)
    recs = np.zeros((n, 8), np.int32)
    finals = []
    for i in range(n):
        level = i % L
        lv = pool.levels[level]
        recs[i, 0], recs[i, 1], recs[i, 2], recs[i, 3] = 3 * i + 1, level, steps_of(i), i // L
        recs[i, 4] = np.float32(lv.spawn_prob).view(np.int32)
        b = oracle.advance_board(lv.board, lv.spawn_prob, steps_of(i), rng_words=util.random_rng_words(rng, 1)[0])[0]
        b.reshape(-1)[rng.integers(0, b.size, 5)] = 0
        finals.append(b)
    return recs, np.stack(finals)


def quiet_env(pool):
    from safelife_amd.vector_env import SafeLifeVectorEnv
    return SafeLifeVectorEnv(pool, 8, with_obs=False)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SWEEP)
def test_pass_kernel_sweep_on_a_hand_filled_queue(shape):
    """The sweep of test_life_occupancy_generic_shapes once more THROUGH THE PASS, which always takes the size-generic
    launcher on these shapes (25x25: by boards 2 bytes off alignment): entries with num_steps = 0 under the caller's
    generators (derive_streams = 0), so counts[0] is life_occupancy of the level itself, counts[1] that of the queue
    board on the same generator; 1, 2 and 257 samples, counts and generators against the oracle."""
    from safelife_amd.levels import Level, LevelPool
    H, W = shape
    rng = np.random.default_rng(11 * H + W)
    levels = [make_level(rng, H, W) for _ in range(5)]
    pool = LevelPool([Level(lv.board, agent_locs=np.zeros((0, 2), int), spawn_prob=lv.spawn_prob) for lv in levels],
                     counts_fn=_device_counts)
    env = quiet_env(pool)
    recs, finals = hand_queue(pool, 13, 5, lambda i: 0)
    recs[:, 2] = 0
    bg = np.random.PCG64(0)
    for ns in (1, 2, 257):
        words = util.random_rng_words(rng, 5)
        rc, got = run_pass(env, H, W, recs, finals, 5, 5, ns, 0, work_rng=words, offset=1 if shape == (25, 25) else 0)
        assert rc == 0
        for i in range(5):
            lv = pool.levels[i]
            p = float(np.float32(lv.spawn_prob))
            oracle.pcg64_set_state_words(bg, words[i])
            c0 = oracle.life_occupancy(lv.board, p, ns, bitgen=bg)
            c1 = oracle.life_occupancy(finals[i], p, ns, bitgen=bg)
            assert np.array_equal(got["work_boards"][i], lv.board), (ns, i)
            assert np.array_equal(got["counts"][0, i], c0) and np.array_equal(got["counts"][1, i], c1), (ns, i)
            assert np.array_equal(got["work_rng"][i], oracle.pcg64_state_words(bg)), (ns, i)


@pytest.mark.gpu
def test_pass_counter_reaches_65535():
    """num_samples = 65535 through the pass on 3x3 levels whose every cell is alive, preserving and not frozen: the
    size-generic kernel's uint16 counters end at 65535 without wrapping (oracle: every cell counted on every step)."""
    from safelife_amd.levels import Level, LevelPool
    boards = np.full((2, 3, 3), ALIVE | 32, np.uint16)
    boards[1] |= 0x400
    pool = LevelPool([Level(b, agent_locs=np.zeros((0, 2), int), spawn_prob=0.9) for b in boards], counts_fn=_device_counts)
    env = quiet_env(pool)
    recs = np.zeros((2, 8), np.int32)
    recs[:, 0], recs[:, 1], recs[:, 4] = [0, 1], [0, 1], np.float32(0.9).view(np.int32)
    words = util.random_rng_words(np.random.default_rng(1), 2)
    rc, got = run_pass(env, 3, 3, recs, boards[::-1].copy(), 2, 2, 65535, 0, work_rng=words)
    assert rc == 0
    bg = np.random.PCG64(0)
    for i in range(2):
        oracle.pcg64_set_state_words(bg, words[i])
        c0 = oracle.life_occupancy(boards[i], np.float32(0.9), 65535, bitgen=bg)
        c1 = oracle.life_occupancy(boards[1 - i], np.float32(0.9), 65535, bitgen=bg)
        assert c0.max() == 65535 and c0.sum() == 9 * 65535
        assert np.array_equal(got["counts"][0, i], c0) and np.array_equal(got["counts"][1, i], c1), i
        assert np.array_equal(got["work_rng"][i], oracle.pcg64_state_words(bg)), i


@pytest.mark.gpu
def test_pass_on_unaligned_boards_equals_the_row_kernels():
    """25x25 (a row-kernel shape) with work_boards and queue.boards 2 bytes past a 16-byte boundary: SL_OK, and counts,
    keys, life_dist and type masks equal those of the aligned call on the same entries -- the size-generic kernels
    against the row kernels."""
    pool = make_pool(125, 25, 25, 6)
    env = quiet_env(pool)
    n, cap = 20, 24
    recs, finals = hand_queue(pool, 5, n, lambda i: 9 + i % 3)
    rc0, want = run_pass(env, 25, 25, recs, finals, n, cap, 80, 1)
    rc1, got = run_pass(env, 25, 25, recs, finals, n, cap, 80, 1, offset=1)
    assert rc0 == 0 and rc1 == 0
    for name in ("counts", "keys", "life_dist", "type_masks", "work_rng"):
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(got["records"], want["records"])          # (n_cell_types is written by the pass)
    assert got["counts"][:, :n].sum() > 0 and (got["keys"][:n, 8] != 0xFFFF).all()
    for i in (0, 7, n - 1):                                         # and both against the oracle
        b1, c0, c1 = derived_reference(pool, int(recs[i, 1]), finals[i], int(recs[i, 0]), int(recs[i, 3]),
                                       int(recs[i, 2]), 80)
        assert np.array_equal(got["counts"][0, i], c0) and np.array_equal(got["counts"][1, i], c1), i


@pytest.mark.gpu
def test_pass_reference_order_on_one_generator_7x11():
    """derive_streams = 0 on 7x11: the reference's order on ONE caller-given generator per entry -- roll-forward,
    inaction tensor, action tensor -- boards, tensors and the generator's state after the pass against the oracle."""
    H, W = 7, 11
    pool = make_pool(107, H, W, 6)
    env = quiet_env(pool)
    n, cap, ns = 10, 12, 120
    recs, finals = hand_queue(pool, 9, n, lambda i: 9 + i % 3)
    words = util.random_rng_words(np.random.default_rng(4), cap)
    rc, got = run_pass(env, H, W, recs, finals, n, cap, ns, 0, work_rng=words)
    assert rc == 0
    bg = np.random.PCG64(0)
    for i in range(n):
        lv = pool.levels[int(recs[i, 1])]
        p = float(np.float32(lv.spawn_prob))
        oracle.pcg64_set_state_words(bg, words[i])
        b1 = oracle.advance_board(lv.board, p, int(recs[i, 2]), bitgen=bg)
        c0 = oracle.life_occupancy(b1, p, ns, bitgen=bg)
        c1 = oracle.life_occupancy(finals[i], p, ns, bitgen=bg)
        assert (lv.board & SPAWNING).any() and len(countable_colours(b1)) >= 2, i
        assert np.array_equal(got["work_boards"][i], b1), i
        assert np.array_equal(got["counts"][0, i], c0) and np.array_equal(got["counts"][1, i], c1), i
        assert np.array_equal(got["work_rng"][i], oracle.pcg64_state_words(bg)), i
    assert np.array_equal(got["work_rng"][n:cap], words[n:])                    # entries past the count: untouched
    assert (got["counts"][:, n:] == CANARY["counts"]).all() and (got["keys"][n:] == 0xFFFF).all()


@pytest.mark.gpu
def test_pass_queue_edges_13x17():
    """The device-side count on 13x17: 0 writes nothing into the canary-filled outputs (an empty slot's keys read
    0xFFFF, the pass's rule for every slot past the count); a count above the capacity processes exactly `capacity`
    entries; a count of 1 processes one; an entry with num_steps = 0 is sampled without a roll-forward."""
    H, W = 13, 17
    pool = make_pool(113, H, W, 6)
    env = quiet_env(pool)
    cap, ns = 6, 60
    recs, finals = hand_queue(pool, 2, cap, lambda i: 0 if i == 2 else 9 + i % 3)

    def untouched(got, lo):
        for name in ("counts", "life_dist", "type_masks"):
            part = got[name][:, lo:] if name == "counts" else got[name][lo:]
            assert (part == np.array(CANARY[name]).astype(part.dtype)).all(), (name, lo)
        assert (got["keys"][lo:] == 0xFFFF).all()
        assert (got["work_rng"][lo:cap] == CANARY["work_rng"]).all() and (got["work_rng"][cap + lo:] == CANARY["work_rng"]).all()
        assert (got["work_boards"][lo:cap] == CANARY["work_boards"]).all()
        assert (got["work_boards"][cap + lo:] == CANARY["work_boards"]).all()

    def processed(got, i):
        b1, c0, c1 = derived_reference(pool, int(recs[i, 1]), finals[i], int(recs[i, 0]), int(recs[i, 3]), int(recs[i, 2]), ns)
        assert np.array_equal(got["counts"][0, i], c0) and np.array_equal(got["counts"][1, i], c1), i
        assert np.array_equal(got["life_dist"][i, 0], np.moveaxis(c0, -1, 0) / float(ns)), i
        assert np.array_equal(got["life_dist"][i, 1], np.moveaxis(c1, -1, 0) / float(ns)), i
        return b1

    rc, got = run_pass(env, H, W, recs, finals, 0, cap, ns, 1)
    assert rc == 0
    untouched(got, 0)
    rc, got = run_pass(env, H, W, recs, finals, cap + 3, cap, ns, 1)
    assert rc == 0
    for i in range(cap):
        b1 = processed(got, i)
        if i == 2:
            assert int(recs[i, 2]) == 0 and np.array_equal(b1, pool.levels[int(recs[i, 1])].board)
    assert (got["keys"][:, :8] != 0xFFFF).any(axis=1).all()
    rc, got = run_pass(env, H, W, recs, finals, 1, cap, ns, 1)
    assert rc == 0
    processed(got, 0)
    untouched(got, 1)


# ------------------------------------------------------------------ 3. end to end through SafeLifeVectorEnv

@pytest.mark.gpu
@pytest.mark.parametrize("shape,time_limit,deferred", [((13, 17), 9, False), ((20, 40), 11, True)])
def test_side_effect_queue_end_to_end_generic(shape, time_limit, deferred):
    """SafeLifeVectorEnv(side_effects=...) on a pool shape without row kernels, auto_reset, 48 envs, 34 random steps
    next to the oracle: the queue's records and terminal boards against the oracle's replay, every 5th entry's two
    occupancy tensors against the oracle primitives under the derived streams, a finite device score for every
    (entry, key), and device scores against the host LP (the tolerance of tests/test_emd.py's end-to-end test).  The 20x40
    case flushes with overlap=True, defer=True and launches the pass by hand."""
    H, W = shape
    B, T, n_samples = 48, 34, 60
    pool = make_pool(100 + H, H, W, 6)
    first = np.arange(B) % len(pool.levels)
    kw = dict(first_level=first, auto_reset=True, level_stride=1, time_limit=time_limit, view_shape=(9, 9))
    dev = util.DeviceBackend(pool, B, side_effects=dict(capacity=256, num_samples=n_samples), **kw)
    cpu = util.OracleBackend(pool, B, **kw)
    dev.reset(), cpu.reset()
    rng = np.random.default_rng(31)
    want = {}                      # (env, episode_idx) -> (level, num_steps, final board)
    for t in range(T):
        a = rng.integers(0, 9, B).astype(np.int32)
        before = {k: cpu.get(k) for k in ("level_idx", "episode_idx", "is_active")}
        cpu.env.s.auto_reset = 0           # look at the terminal boards, then let the oracle reset
        _, _, d2 = cpu.step(a)
        boards_before_reset = cpu.get("board")
        steps_now = cpu.get("num_steps")
        for e in np.nonzero(d2 & (before["is_active"] != 0))[0]:
            want[(int(e), int(before["episode_idx"][e]))] = (int(before["level_idx"][e]), int(steps_now[e]),
                                                            boards_before_reset[e].copy())
        cpu.env.s.auto_reset = 1
        for e in np.nonzero(d2)[0]:        # the oracle's auto-reset, by hand
            cpu.arrays["level_idx"][e] = (cpu.arrays["level_idx"][e] + 1) % len(pool.levels)
            cpu.arrays["episode_idx"][e] += 1
        if d2.any():
            m = d2.astype(np.uint8)
            cpu.arrays["loaded"][m != 0] = 0
            cpu.env.reset(m)
        _, _, d1 = dev.step(a)
        assert np.array_equal(d1, d2), t
    if deferred:
        batch = dev.env.side_effects_flush(overlap=True, defer=True)
        dev.env.side_effects_launch()
    else:
        batch = dev.env.side_effects_flush()
    recs = batch.records()
    assert len(batch) == len(want) and len(want) >= 3 * B and batch.dropped() == 0
    boards = batch.boards.cpu().numpy().view(np.uint16)
    counts = batch.counts.cpu().numpy()
    for i in range(len(batch)):
        key = (int(recs["env"][i]), int(recs["episode_idx"][i]))
        level, steps, board = want.pop(key)
        assert (int(recs["level"][i]), int(recs["num_steps"][i])) == (level, steps), key
        assert np.array_equal(boards[i], board), key
        if i % 5 == 0:
            _, c0, c1 = derived_reference(pool, level, board, key[0], key[1], steps, n_samples)
            assert np.array_equal(counts[0, i], c0) and np.array_equal(counts[1, i], c1), key
    assert not want
    # the distances: one launch for the whole batch, finite wherever there is a key
    n = len(batch)
    emd = batch.scores_all()
    batch.wait()
    scores, keys = emd["scores"].cpu().numpy()[:n], batch.keys.cpu().numpy().view(np.uint16)[:n]
    assert (emd["n_cells"].cpu().numpy()[:n, 0] >= 0).all()
    assert np.isfinite(scores[keys != 0xFFFF]).all() and (keys != 0xFFFF).sum() >= 3 * n
    with np.load(os.path.join(util.GOLDEN, "emd_cases.npz")) as d:
        lp_spread = float(d["lp_spread"])       # how far two LP solves of one problem differ (tests/test_emd.py)
    # against the host LP: every key of the entry with at most 250 participating cells (on 13x17 that is every key;
    # one LP over more cells takes seconds on the host)
    n_cells = emd["n_cells"].cpu().numpy()[:n]
    for i in ((0, n - 1) if H * W <= 250 else (0,)):
        small = [int(k) for k, c in zip(keys[i], n_cells[i]) if k != 0xFFFF and c <= 250]
        large = [int(k) for k, c in zip(keys[i], n_cells[i]) if k != 0xFFFF and c > 250]
        print("entry %d: %d keys compared with the host LP, %d (more than 250 cells) not" % (i, len(small), len(large)))
        assert len(small) >= 3 and (H * W > 250 or not large), (i, n_cells[i])
        host = batch.scores(i, include=small, strkeys=False)
        got = batch.scores(i, include=small, strkeys=False, device=True)
        assert set(host) == set(got) == set(small)
        for k in host:
            for g, h in zip(got[k], host[k]):       # (distance, inaction mass): test_scores_all_end_to_end_25's bound
                print("entry %d key %d: device %.17g host %.17g" % (i, k, g, h))
                assert abs(g - h) <= max(10 * lp_spread, 1e-9 * max(1.0, abs(h))), (i, k, got[k], host[k])
    assert len(dev.env.side_effects_flush()) == 0          # the fresh queue starts empty


# ------------------------------------------------------------------ 6. multi-agent

@pytest.mark.gpu
def test_side_effect_queue_multi_agent_9x13():
    """A two-agent 9x13 pool through SafeLifeMultiAgentVectorEnv(side_effects=...): one flush, one entry per env
    episode, both occupancy tensors of every entry against the oracle primitives under the derived streams."""
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    H, W, B, n_samples = 9, 13, 12, 50
    pool = make_pool(109, H, W, 6, n_agents=2)
    env = SafeLifeMultiAgentVectorEnv(pool, B, first_level=np.arange(B) % 6, auto_reset=False, time_limit=10,
                                      view_shape=(9, 9), output_channels=None,
                                      side_effects=dict(capacity=16, num_samples=n_samples))
    env.reset()
    rng = np.random.default_rng(6)
    for t in range(10):
        env.step(rng.integers(0, 9, (B, 2)).astype(np.int32))
    batch = env.side_effects_flush()
    recs = batch.records()
    assert len(batch) == B and batch.dropped() == 0 and sorted(recs["env"].tolist()) == list(range(B))
    boards = batch.boards.cpu().numpy().view(np.uint16)
    counts = batch.counts.cpu().numpy()
    for i in range(B):
        assert 1 <= recs["num_steps"][i] <= 10 and recs["level"][i] == recs["env"][i] % 6
        _, c0, c1 = derived_reference(pool, int(recs["level"][i]), boards[i], int(recs["env"][i]),
                                      int(recs["episode_idx"][i]), int(recs["num_steps"][i]), n_samples)
        assert np.array_equal(counts[0, i], c0) and np.array_equal(counts[1, i], c1), i
    assert counts[:, :B].sum() > 0
