"""GPU suite for the pattern generator: every case of tests/golden/gen_pattern_cases.npz (the compiled reference's
gen_pattern) through slhip_gen_pattern_batch, one launch per (H, W, period) group; the same with the cases replicated to
1 .. 257 problems per launch inside poisoned buffers; and the speedups.gen_pattern drop-in with the process-global
generator."""
import collections
import os

import numpy as np
import pytest

from safelife_amd import speedups
from tests import gen_pattern_ref as gpr
from tests import util

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(util.REPO, "tests", "golden", "gen_pattern_cases.npz")
GUARD = 64          # poisoned elements in front of and behind every buffer the kernel writes
POISON16, POISON32, POISON64 = 0x5A5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def cases():
    return gpr.load_cases(FIXTURE)


def groups_of(cases):
    g = collections.OrderedDict()
    for c in cases:
        g.setdefault(c["board"].shape + (c["period"],), []).append(c)
    return g


def stacked(group):
    """a group's cases as gen_pattern_batch takes them (seeds=None written out as the mask, which is what it means)"""
    boards = np.stack([c["board"] for c in group]).astype(np.uint16)
    masks = np.stack([c["mask"] for c in group]).astype(np.int32)
    seeds = np.stack([c["mask"] if c["seeds"] is None else c["seeds"] for c in group]).astype(np.int32)
    params = np.stack([speedups.gen_pattern_params(**c["kwargs"]) for c in group])
    rng = np.stack([c["w0"] for c in group]).astype(np.uint64)
    return boards, masks, seeds, params, rng


def check_group(group, boards, status, iters, rng, what=""):
    for k, c in enumerate(group):
        tag = "%s %s" % (c["name"], what)
        assert int(status[k]) == c["status"], tag
        assert np.array_equal(boards[k], c["out"]), tag
        assert np.array_equal(rng[k], c["w1"]), tag
        assert int(iters[k]) == c["iters"], tag


def test_fixture_one_launch_per_group(cases):
    groups = groups_of(cases)
    assert sum(len(g) for g in groups.values()) == len(cases) >= 55
    for key, group in groups.items():
        boards, masks, seeds, params, rng = stacked(group)
        before = [a.copy() for a in (boards, masks, seeds, params)]
        out, status, iters = speedups.gen_pattern_batch(boards, masks, key[2], seeds, params, rng)
        assert out.dtype == np.uint16 and status.dtype == np.int32 and iters.dtype == np.int32
        check_group(group, out, status, iters, rng)
        for a, b in zip(before, (boards, masks, seeds, params)):
            assert np.array_equal(a, b)                                     # the inputs are only read


def test_seeds_none_is_the_mask(cases):
    group = [c for c in cases if c["seeds"] is None and c["board"].shape == (10, 10) and c["period"] == 1]
    assert len(group) >= 5
    boards, masks, _, params, rng = stacked(group)
    out, status, iters = speedups.gen_pattern_batch(boards, masks, 1, None, params, rng)
    check_group(group, out, status, iters, rng, "(seeds=None)")


@pytest.mark.parametrize("n_problems", [1, 63, 64, 65, 257])
def test_replicated_in_poisoned_buffers(cases, n_problems):
    """The cases of every group dealt round-robin over n_problems problems of one launch; the buffers the kernel writes sit
    between poisoned guards, the inputs are compared afterwards, and replicas of a case must agree with the record (and so
    with each other)."""
    import torch
    from safelife_amd import _hip
    dev = _hip.device()
    for key, group in groups_of(cases).items():
        H, W, period = key
        if n_problems > 65 and H * W > 200:
            picked = group[:3]              # the long 26x26 chain once per launch is enough at 257 problems
        else:
            picked = group
        deal = [picked[k % len(picked)] for k in range(n_problems)]
        boards, masks, seeds, params, rng = stacked(deal)
        N = n_problems

        def guarded(shape, dtype, poison):
            flat = torch.full((2 * GUARD + int(np.prod(shape)),), poison, dtype=dtype, device=dev)
            return flat, flat[GUARD:GUARD + int(np.prod(shape))].view(*shape)

        out_all, out = guarded((N, H, W), torch.int16, POISON16)
        st_all, status = guarded((N,), torch.int32, POISON32)
        it_all, iters = guarded((N,), torch.int32, POISON32)
        rng_all, d_rng = guarded((N, 6), torch.int64, POISON64)
        d_rng.copy_(torch.from_numpy(rng.view(np.int64)))
        d_in = [torch.from_numpy(a).to(dev) for a in (boards.view(np.int16), masks, seeds, params)]
        keep = [t.clone() for t in d_in]
        speedups.gen_pattern_batch(d_in[0], d_in[1], period, d_in[2], d_in[3], d_rng, out=(out, status, iters))
        torch.cuda.synchronize()
        for t, k in zip(d_in, keep):
            assert torch.equal(t, k), key
        for flat, poison in ((out_all, POISON16), (st_all, POISON32), (it_all, POISON32), (rng_all, POISON64)):
            assert bool((flat[:GUARD] == poison).all()) and bool((flat[-GUARD:] == poison).all()), key
        check_group(deal, out.cpu().numpy().view(np.uint16), status.cpu().numpy(), iters.cpu().numpy(),
                    d_rng.cpu().numpy().view(np.uint64), "(x%d)" % n_problems)


def test_workspace_shapes_agree_with_lds_shapes():
    """Shapes whose state does not fit 64 KiB of LDS run the same code out of a global workspace: a 62x62 period-1 problem
    (just over the limit) against the restatement, and 64x64 at period 4 -- the largest state there is -- for a short run whose
    replicas must agree and which must leave the cells outside its mask alone."""
    rs = np.random.RandomState(5)
    H = W = 62
    board = np.zeros((H, W), np.uint16)
    mask = np.zeros((H, W), np.int32)
    mask[3:12, 40:52] = 7
    mask[2:13, 39:53] |= 4
    words = gpr.words6(np.random.PCG64(321))
    want = gpr.gen_pattern(board, mask, 1, words=words)
    assert want["margin"] >= 1e-12 and want["iterations"] > 20
    rng = np.stack([words, words]).astype(np.uint64)
    out, status, iters = speedups.gen_pattern_batch(np.stack([board, board]), np.stack([mask, mask]), 1, None, None, rng)
    for k in range(2):
        assert int(status[k]) == want["status"] and int(iters[k]) == want["iterations"]
        assert np.array_equal(out[k], want["board"]) and np.array_equal(rng[k], want["words"])
    # 64x64 at period 4: the largest state there is; a short run, replicas equal, poison in the masked-off cells untouched
    board = (rs.rand(64, 64) < 0.02).astype(np.uint16) * 16
    mask = np.zeros((64, 64), np.int32)
    mask[60:64, 0:5] = 7                                    # a region that wraps neither way but touches both edges
    params = np.tile(speedups.gen_pattern_params(max_iter=0.3), (3, 1))
    rng = np.stack([words] * 3).astype(np.uint64)
    out, status, iters = speedups.gen_pattern_batch(np.stack([board] * 3), np.stack([mask] * 3), 4, None, params, rng)
    assert (status == status[0]).all() and (iters == iters[0]).all() and iters[0] > 0
    assert (out == out[0]).all() and (rng == rng[0]).all()
    assert np.array_equal(out[0][mask == 0], board[mask == 0])


def test_drop_in_with_the_global_generator(cases):
    by_name = {c["name"]: c for c in cases}
    picked = [by_name[n] for n in ("p1-10x10-full-s1", "p1-10x10-buffered", "p1-26x26-walls-trees", "p2-10x10-start-board-buffered",
                                   "p3-4x5-start-board")]
    assert all(c["status"] == 0 for c in picked)
    bg = np.random.PCG64(0)
    speedups.set_bit_generator(bg)
    for c in picked:
        speedups.pcg64_set_words6(bg, c["w0"])
        board, mask = c["board"].copy(), c["mask"].copy()
        got = speedups.gen_pattern(board, mask, c["period"], seeds=c["seeds"], **c["kwargs"])
        assert got.dtype == np.uint16 and np.array_equal(got, c["out"]), c["name"]
        assert np.array_equal(speedups.pcg64_words6(bg), c["w1"]), c["name"]
        assert np.array_equal(board, c["board"]) and np.array_equal(mask, c["mask"])
    failing = by_name["p2-10x10-start-board"]
    assert failing["status"] == -1
    speedups.pcg64_set_words6(bg, failing["w0"])
    with pytest.raises(speedups.MaxIterException, match="Max-iter hit. Aborting!"):
        speedups.gen_pattern(failing["board"], failing["mask"], failing["period"], seeds=failing["seeds"], **failing["kwargs"])
    assert np.array_equal(speedups.pcg64_words6(bg), failing["w1"])         # the generator has advanced exactly
    assert not np.array_equal(failing["w0"], failing["w1"])


# ---- whole levels: safelife_amd.proc_gen with the device as backend ---------------------------------------------------------------

SPECS = os.path.join(util.REPO, "tests", "golden", "procgen")


def spec(name):
    from safelife_amd import proc_gen
    return proc_gen.load_params(os.path.join(SPECS, name + ".yaml"), defaults=os.path.join(SPECS, "_defaults.yaml"))


def restated_backend(requests):
    out = []
    for rq in requests:
        g = gpr.gen_pattern(rq.board, rq.mask, rq.period, seeds=rq.seeds, words=rq.words, **rq.kwargs)
        out.append((g["board"], g["status"], g["words"]))
    return out


def exact_levels(name, params, seeds):
    """What gen_games makes of `seeds` with the compiled reference's gen_pattern as backend: computed here where the
    reference extension has been built (it travels with the tree), else as tests/golden/procgen_levels.npz recorded it from
    that same backend -- with the Python restatement as a live backend beside it for the first two seeds (it takes seconds
    per level)."""
    import oracle
    from safelife_amd import proc_gen
    ref = oracle.load_ref()
    if ref is not None and hasattr(ref, "gen_pattern"):
        lv = proc_gen.gen_games(params, seeds, backend=proc_gen.function_backend(ref))
        return [(x.board, x.goals, x.agent_locs, x.initial_rng_words()) for x in lv]
    with np.load(os.path.join(util.REPO, "tests", "golden", "procgen_levels.npz")) as z:
        assert z[name + "_seeds"].tolist() == list(seeds)
        want = [(z[name + "_board"][k], z[name + "_goals"][k], z[name + "_agent_locs"][k], z[name + "_rng"][k])
                for k in range(len(seeds))]
    for k, x in enumerate(proc_gen.gen_games(params, seeds[:2], backend=restated_backend)):
        assert x.board.tobytes() == want[k][0].tobytes() and x.goals.tobytes() == want[k][1].tobytes(), (name, seeds[k])
    return want


def levels_equal(a, b):
    return (a.board.tobytes() == b.board.tobytes() and a.goals.tobytes() == b.goals.tobytes()
            and np.array_equal(a.agent_locs, b.agent_locs) and np.array_equal(a.points_table, b.points_table)
            and a.min_performance == b.min_performance and np.array_equal(a.initial_rng_words(), b.initial_rng_words()))


@pytest.mark.parametrize("name,n_seeds", [("append-still-easy", 32), ("prune-still", 32), ("append-spawn", 32),
                                          ("multi-agent-build-coop", 8)])
def test_whole_levels_device_against_exact_backend(name, n_seeds):
    from safelife_amd import proc_gen
    params = spec(name)
    seeds = list(range(1000, 1000 + n_seeds))
    want = exact_levels(name, params, seeds)
    got = proc_gen.gen_games(params, seeds)                              # the device
    for s, a, (board, goals, agent_locs, rng) in zip(seeds, got, want):
        assert a.board.tobytes() == np.asarray(board, np.uint16).tobytes(), (name, s)
        assert a.goals.tobytes() == np.asarray(goals, np.uint16).tobytes(), (name, s)
        assert np.array_equal(a.agent_locs, agent_locs) and np.array_equal(a.initial_rng_words(), rng), (name, s)
    order = seeds[1::2][::-1] + seeds[0::2]                              # another batch order, another composition
    again = dict(zip(order, proc_gen.gen_games(params, order)))
    for s, a in zip(seeds, got):
        assert levels_equal(a, again[s]), (name, s)
    assert any(((lv.board & 1) != 0).any() or ((lv.goals & 1) != 0).any() for lv in got)


def test_fill_pool_under_a_stepping_env():
    """fill_pool into a refreshable pool while a SafeLifeVectorEnv steps on it: after pool_commit the envs' next reloads play
    the new levels, step for step like an env built on those levels directly."""
    import torch
    from safelife_amd import proc_gen
    from safelife_amd.levels import LevelPool
    from safelife_amd.vector_env import SafeLifeVectorEnv
    params = spec("prune-still")
    B, LIMIT = 4, 5
    first = proc_gen.gen_games(params, range(2000, 2000 + B))
    pool = LevelPool(first, refreshable=True)
    kw = dict(time_limit=LIMIT, level_stride=0, episode_streams=False, with_obs=False)
    env = SafeLifeVectorEnv(pool, B, **kw)
    env.reset()
    actions = np.random.RandomState(3).randint(0, 9, size=(LIMIT + 20, B))
    for t in range(3):
        env.step(actions[t])
    new = proc_gen.fill_pool(pool, range(B), params, range(3000, 3000 + B), env=env)
    assert len(new) == B and not levels_equal(new[0], first[0])
    env.pool_commit()
    for t in range(3, LIMIT):
        _, _, done, _ = env.step(actions[t])
    assert bool(done.all())                                 # the time limit: every env reloads -- its slot's new content
    direct = SafeLifeVectorEnv(LevelPool(new), B, **kw)
    direct.reset()
    assert torch.equal(env.t["board"], direct.t["board"])
    played = env.t["board"].cpu().numpy().view(np.uint16)
    for e in range(B):                                      # the new level's cells (the reset may have opened the exit)
        differ = played[e] != new[e].board
        assert differ.sum() <= 1 and ((new[e].board[differ] & 256) != 0).all(), e
        assert (played[e] != first[e].board).sum() > 10, e
    for t in range(LIMIT, LIMIT + 20):
        _, r1, d1, _ = env.step(actions[t])
        _, r2, d2, _ = direct.step(actions[t])
        assert torch.equal(r1, r2) and torch.equal(d1, d2), t
        assert torch.equal(env.t["board"], direct.t["board"]), t
        assert torch.equal(env.t["goals"], direct.t["goals"]), t
