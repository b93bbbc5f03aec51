"""
The observation against an independent reference, on levels with several exits.

tests/obs_ref.py writes ``SafeLifeEnv.get_obs`` a second time in plain numpy; tests/golden/obs_cases.npz holds what the
reference itself returned for 62 hand-placed levels (tests/golden/make_golden_obs.py).  On the CPU: obs_ref reproduces
the fixture, the three host implementations (the oracle, ``safelife_amd.env.recenter_view``, the compat ``SafeLifeEnv``)
equal obs_ref, and the fixture tells eight wrong implementations from the right one.  On the GPU: every device path that
writes an observation is compared with obs_ref applied to the state read back from the device -- observation = f(state),
no oracle in between -- on pools whose levels have 0 to 8 (and 9) exits.
"""
import os
import types

import numpy as np
import pytest

from tests import obs_ref, util

with np.load(os.path.join(util.GOLDEN, "obs_cases.npz")) as _d:
    FIX = {k: _d[k] for k in _d.files}
CASE_NAMES = [str(n) for n in FIX["cases"]]
CHANNEL_LISTS = {str(k): (tuple(int(c) for c in FIX["channel_list_" + str(k)]) or None) for k in FIX["channel_lists"]}


def case(name):
    c = {k: FIX["%s_%s" % (name, k)] for k in ("board", "goals", "agent", "exits", "view", "channels", "rwg", "out")}
    c["view"] = tuple(int(v) for v in c["view"])
    c["channels"] = CHANNEL_LISTS[str(c["channels"])]
    c["rwg"] = bool(c["rwg"])
    return c


def ref_of(c, mutant=None):
    return obs_ref.get_obs(c["board"], c["goals"], c["agent"], c["exits"], c["view"], c["channels"], c["rwg"], mutant)


# ---------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("name", CASE_NAMES)
def test_obs_ref_reproduces_the_reference(name):
    c = case(name)
    got = ref_of(c)
    assert got.dtype == c["out"].dtype
    assert obs_ref.first_difference(got, c["out"]) is None, obs_ref.first_difference(got, c["out"])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_implementations_equal_obs_ref(name):
    from safelife_amd.env import SafeLifeEnv, recenter_view
    from safelife_amd.levels import Level, LevelPool
    c = case(name)
    H, W = c["board"].shape
    want = ref_of(c)
    flat = c["exits"][c["exits"] >= 0]
    locs = np.divmod(flat.astype(np.int64), W)
    centre = tuple(int(v) for v in c["agent"]) if c["agent"][0] >= 0 else (0, 0)
    # safelife_amd.env.recenter_view on the same words
    words = obs_ref.view_words(c["board"], c["goals"], c["rwg"])
    got = obs_ref.channel_bits(recenter_view(words, c["view"], centre, locs), c["channels"])
    assert obs_ref.first_difference(got, want) is None, "recenter_view: " + obs_ref.first_difference(got, want)
    # the compat env
    env = SafeLifeEnv(iter(()), view_shape=c["view"], output_channels=c["channels"], remove_white_goals=c["rwg"])
    agents = c["agent"][None].astype(np.int64) if c["agent"][0] >= 0 else np.zeros((0, 2), np.int64)
    env.game = types.SimpleNamespace(board=c["board"].copy(), goals=c["goals"].copy(), agent_locs=agents, exit_locs=locs)
    got = env.get_obs()
    assert got.dtype == want.dtype
    assert obs_ref.first_difference(got, want) is None, "SafeLifeEnv.get_obs: " + obs_ref.first_difference(got, want)
    # the oracle: a pool of this one level, reset (which repaints the exits) and two moves, against obs_ref on ITS state
    pool = LevelPool([Level(c["board"], c["goals"], agents)], counts_fn=util.oracle_counts, exit_slots=len(c["exits"]))
    assert np.array_equal(pool.pool_exit_locs[0], c["exits"])
    be = util.OracleBackend(pool, 1, auto_reset=True, episode_streams=False, view_shape=c["view"],
                            output_channels=c["channels"], remove_white_goals=c["rwg"], time_limit=1000)
    obs = be.reset()
    for action in (None, 3, 2):
        if action is not None:
            obs, _, _ = be.step(np.array([action], np.int32))
        want = obs_ref.get_obs(be.get("board")[0], be.get("goals")[0], be.get("agent_loc")[0], be.get("exit_locs")[0],
                               c["view"], c["channels"], c["rwg"])
        assert obs_ref.first_difference(obs[0], want) is None, \
            "oracle after action %s: %s" % (action, obs_ref.first_difference(obs[0], want))


@pytest.mark.parametrize("mutant", obs_ref.MUTANTS)
def test_fixture_tells_wrong_implementations_apart(mutant):
    """The case set is only worth something if a kernel with this mistake would fail on it."""
    caught = []
    for name in CASE_NAMES:
        c = case(name)
        if mutant == "policy_xy_swapped":
            if c["channels"] is None:
                continue
            got, want = obs_ref.policy_layout(c["out"], mutant=mutant), obs_ref.policy_layout(c["out"])
        else:
            got, want = ref_of(c, mutant), c["out"]
        if obs_ref.first_difference(got, want) is not None:
            caught.append(name)
    assert caught, "no fixture case tells '%s' from the reference: add cases" % mutant


# ---------------------------------------------------------------------------------------------- GPU

PLAYER, EXIT, WHITE = 122, 272, 0x0E00
#: cells of the seeded levels (the fixture's kind): mostly empty, walls, crates, coloured life and trees, a spawner
CELLS = np.array([0] * 14 + [16, 16, 16 | 4, 16 | 0x8000, 9, 9 | 0x200, 9 | 0x400, 9 | 0x800, 9 | 0xE00, 17 | 0x400, 152,
                  48 | 0x600, 53, 85], np.uint16)


def seeded_level(H, W, n_exits, rng, corner):
    """A random level with `n_exits` exits on random goals (some white) and an agent -- in a corner of the board for
    `corner`, so that a move takes the view across the seam -- with free cells along its row and column."""
    from safelife_amd.levels import Level
    board = CELLS[rng.integers(0, len(CELLS), (H, W))]
    goals = (rng.integers(0, 8, (H, W)) * (rng.random((H, W)) < 0.6)).astype(np.uint16) << 9
    agent = ((0, 0), (H - 1, W - 1), (0, W - 1))[corner] if corner is not None else \
        (int(rng.integers(0, H)), int(rng.integers(0, W)))
    for d in range(-3, 4):
        board[(agent[0] + d) % H, agent[1]] = 0
        board[agent[0], (agent[1] + d) % W] = 0
    board[agent] = PLAYER
    free = np.flatnonzero(board.ravel() != PLAYER)
    for k, cell in enumerate(rng.choice(free, n_exits, replace=False)):
        board.flat[cell] = EXIT
        goals.flat[cell] = WHITE if k % 3 == 0 else int(rng.integers(0, 8)) << 9
    return Level(board, goals, [agent], min_performance=-1.0)


def level_set(shape, seed, with_nine=False):
    """Levels of one board shape with different exit counts next to each other: the fixture's boards of that shape,
    then seeded ones with 0, 1, 2, 3, 5 and 8 exits (9 too for `with_nine`).  -> (levels, exit slots)."""
    from safelife_amd.levels import Level
    rng = np.random.default_rng(seed)
    H, W = shape
    levels = []
    picked = [case(name) for name in CASE_NAMES]
    picked = [c for c in picked if c["board"].shape == shape]
    picked.sort(key=lambda c: int((c["exits"] >= 0).sum()) != 9)         # (stable: the 9-exit case first, if wanted)
    for c in picked:
        n = int((c["exits"] >= 0).sum())
        if (n <= 8 or with_nine) and len(levels) < 6:
            agents = c["agent"][None].astype(np.int64) if c["agent"][0] >= 0 else None
            levels.append(Level(c["board"], c["goals"], agents, min_performance=-1.0))
    if with_nine:
        assert any(len(lv.exit_locs) == 9 for lv in levels)
    for k, n in enumerate((8, 0, 3, 1, 8, 2, 5)):
        levels.append(seeded_level(H, W, min(n, H * W // 4), rng, corner=k % 4 if k % 4 < 3 else None))
    order = rng.permutation(len(levels))
    return [levels[i] for i in order], 9 if with_nine else 8


_POOLS = {}


def pool_of(shape, with_nine=False):
    from safelife_amd.levels import LevelPool
    key = (shape, with_nine)
    if key not in _POOLS:
        levels, E = level_set(shape, 1000 + 64 * shape[0] + shape[1], with_nine)
        _POOLS[key] = LevelPool(levels, counts_fn=util.oracle_counts, exit_slots=E, seed=7)
    return _POOLS[key]


def coprime_stride(n):
    return next(s for s in (3, 5, 7, 11) if n % s)


class Checker(object):
    """Compares what a ``SafeLifeVectorEnv`` wrote with obs_ref on the state it holds."""

    def __init__(self, env, pool, what, chans_name, policy_calls=()):
        self.env, self.pool, self.what, self.policy_calls = env, pool, what, policy_calls
        self.chans_name, self.channels = chans_name, CHANNEL_LISTS[chans_name]
        self.rwg = bool(env.struct.remove_white_goals)
        self.exit_counts_seen, self.seam_crossed, self.reloads_to_other_count, self.piles = set(), False, 0, 0
        self._last = None

    def fail(self, entry, e, form, diff):
        H, W = self.pool.shape
        return ("board %dx%d, view %s, channels %s, %s, entry point %s, env %d, %s: %s"
                % (H, W, self.env.view_shape, self.chans_name, self.what, entry, e, form, diff))

    def check(self, entry):
        env, pool = self.env, self.pool
        H, W = pool.shape
        board, goals = env.numpy("board"), env.numpy("goals")
        loc, exits, level = env.numpy("agent_loc"), env.numpy("exit_locs"), env.numpy("level_idx")
        obs = env.numpy("obs") if env.obs is not None else None
        pol = env.policy_tensor.cpu().numpy() if env.policy_tensor is not None else None
        extra = [(ch, dt, env.policy_obs(CHANNEL_LISTS[ch], dtype=getattr(env.torch, dt)).cpu().numpy())
                 for ch, dt in self.policy_calls]
        vh, vw = env.view_shape
        for e in range(env.num_envs):
            # the env's exit table is its level's, empty slots included
            assert np.array_equal(exits[e], pool.pool_exit_locs[level[e]]), self.fail(entry, e, "exit_locs", exits[e])
            view = obs_ref.get_view(board[e], goals[e], loc[e], exits[e], (vh, vw), self.rwg)
            want = obs_ref.channel_bits(view, self.channels)
            if obs is not None:
                diff = obs_ref.first_difference(obs[e], want)
                assert diff is None, self.fail(entry, e, "obs (cell, channel)", diff)
            if pol is not None:
                diff = obs_ref.first_difference(pol[e], obs_ref.policy_layout(want, pol.dtype))
                assert diff is None, self.fail(entry, e, "fused policy layout %s (channel, x, y)" % pol.dtype, diff)
            for ch, dt, got in extra:
                ref = obs_ref.policy_layout(obs_ref.channel_bits(view, CHANNEL_LISTS[ch]), got.dtype)
                diff = obs_ref.first_difference(got[e], ref)
                assert diff is None, self.fail(entry, e, "policy_obs(%s, %s) (channel, x, y)" % (ch, dt), diff)
            # what this run has exercised
            n = int((exits[e] >= 0).sum())
            self.exit_counts_seen.add(n)
            y0, x0 = (loc[e] if loc[e][0] >= 0 else (0, 0))
            iy, ix = np.divmod(exits[e][exits[e] >= 0], W)
            jy = np.clip((iy - y0 + H // 2) % H - H // 2 + vh // 2, 0, vh - 1)
            jx = np.clip((ix - x0 + W // 2) % W - W // 2 + vw // 2, 0, vw - 1)
            self.piles += len(set(zip(jy.tolist(), jx.tolist()))) < n
        if self._last is not None:
            loc0, level0 = self._last
            same = (level0 == level) & (loc0[:, 0] >= 0) & (loc[:, 0] >= 0)
            self.seam_crossed |= bool((same & (np.abs(loc - loc0).max(axis=1) > 1)).any())
            counts = (pool.pool_exit_locs >= 0).sum(axis=1)
            self.reloads_to_other_count += int(((level0 != level) & (counts[level0] != counts[level])).sum())
        self._last = (loc, level)


def drive(env, pool, what, chans_name, seed, policy_calls=(), steps=6, rollout=True, expect_reloads=True):
    """reset, `steps` steps of moves (episodes end on the way: the time limit), get_obs, a 3-step rollout -- the
    observation checked after each."""
    B = env.num_envs
    rng = np.random.default_rng(seed)
    ck = Checker(env, pool, what, chans_name, policy_calls)
    env.reset()
    ck.check("reset")
    for t in range(steps):
        env.step(rng.integers(1, 5, B).astype(np.int32) if t % 4 != 3 else rng.integers(0, 9, B).astype(np.int32))
        ck.check("step %d" % t)
    if env.obs is not None:
        env.obs.zero_()
        env.get_obs()
        ck.check("get_obs")
    if rollout:
        if env.obs is not None:
            env.obs.zero_()
        if env.policy_tensor is not None:
            env.policy_tensor.zero_()
        env.rollout(rng.integers(1, 5, (3, B)).astype(np.int32))
        ck.check("rollout")
    if expect_reloads:
        assert ck.reloads_to_other_count > 0, ck.fail("-", -1, "coverage", "no env reloaded a level with another exit count")
        assert len(ck.exit_counts_seen) >= 3 and max(ck.exit_counts_seen) >= 8, ck.exit_counts_seen
        if env.view_shape[0] < pool.shape[0] or env.view_shape[1] < pool.shape[1]:     # (a view that shows every cell clips nothing)
            assert ck.piles > 0, ck.fail("-", -1, "coverage", "no two exits on one view cell")
    return ck


def make_env(pool, B, view, chans_name, policy_layout=None, with_obs=True, rwg=True, time_limit=4, **kw):
    from safelife_amd.vector_env import SafeLifeVectorEnv
    L = len(pool)
    return SafeLifeVectorEnv(pool, B, view_shape=view, output_channels=CHANNEL_LISTS[chans_name], time_limit=time_limit,
                             remove_white_goals=rwg, auto_reset=True, first_level=np.arange(B) % L,
                             level_stride=coprime_stride(L), policy_layout=policy_layout, with_obs=with_obs, **kw)


#: output forms: (name, channel list, fused policy layout, with_obs, policy_obs() calls on the raw view)
FORMS = (
    ("std15+u8", "std15", "uint8", True, ()),           # write_obs_block<15>, policy_direct_u8_std<15>
    ("std19+u8", "std19", "uint8", True, ()),           # write_obs_block<19>, policy_direct_u8_std<19>
    ("perm15+f32", "perm15", "float32", True, ()),      # write_obs_block<15> off the standard list, policy_planes<4>
    ("split19+u8", "split19", "uint8", True, ()),       # write_obs_block<19> (bit by bit groups), policy_planes<16>
    ("raw+policy_obs", "raw", None, True, (("std19", "float32"), ("perm15", "uint8"))),    # raw view, slhip_obs_to_policy
    ("one", "one", None, True, ()),                     # write_obs_block<0>
    ("three+u8_only", "three", "uint8", False, ()),     # with_obs=False: policy_planes<16> alone
    ("twenty+f32", "twenty", "float32", True, ()),      # write_obs_block<0>, policy_planes<4>
    ("std15+f32_only", "std15", "float32", False, ()),  # with_obs=False: policy_planes<4> alone
)
#: row-lane shapes -> (boards per workgroup, [odd view, even / mixed view])
ROWLANE = {(25, 25): (8, ((9, 9), (8, 6))), (26, 26): (8, ((15, 9), (8, 6))), (64, 64): (4, ((9, 9), (5, 8))),
           (8, 8): (32, ((9, 9), (8, 6))), (48, 48): (4, ((15, 9), (8, 6)))}


def rowlane_cases():
    out = []
    for si, (shape, (nb, views)) in enumerate(ROWLANE.items()):
        for fi, form in enumerate(FORMS):
            k = si + fi
            odd = k % 2 == 0
            view = views[0] if odd else views[1]
            # an odd view goes with one workgroup and five boards (the vector paths' leftover cells); even views
            # alternate less than one workgroup and a few of them
            B = nb + 5 if odd else ((nb - 1 if nb <= 8 else 5) if k % 4 == 1 else min(64, 3 * nb + 1))
            out.append(pytest.param(shape, view, B, form, k % 3 != 2, id="%dx%d-v%dx%d-B%d-%s" % (shape + view + (B, form[0]))))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape,view,B,form,rwg", rowlane_cases())
def test_rowlane_observation(shape, view, B, form, rwg):
    name, chans, layout, with_obs, calls = form
    pool = pool_of(shape)
    env = make_env(pool, B, view, chans, layout, with_obs, rwg)
    ck = drive(env, pool, "B=%d %s rwg=%d" % (B, name, rwg), chans, seed=B, policy_calls=calls, expect_reloads=B >= 8)
    if B >= 8:
        assert ck.seam_crossed, ck.fail("-", -1, "coverage", "no view walked across the board's seam")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,with_nine,view,B", [((7, 11), False, (5, 8), 9), ((7, 11), False, (3, 4), 11),
                                                    ((25, 25), True, (9, 9), 13), ((25, 25), True, (8, 6), 7)],
                         ids=["7x11-v5x8", "7x11-v3x4", "25x25-e9-v9x9", "25x25-e9-v8x6"])
@pytest.mark.parametrize("form", [FORMS[0], FORMS[2], FORMS[4], FORMS[6]], ids=lambda f: f[0])
def test_generic_observation(shape, with_nine, view, B, form):
    """Shapes without a row-lane kernel, and pools with more than 8 exit slots, run the size-generic ``write_obs``."""
    name, chans, layout, with_obs, calls = form
    pool = pool_of(shape, with_nine)
    assert pool.exit_slots == (9 if with_nine else 8)
    env = make_env(pool, B, view, chans, layout, with_obs)
    ck = drive(env, pool, "generic B=%d %s" % (B, name), chans, seed=B, policy_calls=calls)
    if with_nine:
        assert 9 in ck.exit_counts_seen


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["uint8", "float32"])
def test_view_past_the_fused_policy_room(layout):
    """33x33 = 1089 view cells do not fit the row kernels' policy staging of a 64x64 board (``rowlane_policy_room``: 1015
    cells): the batch takes the generic kernels."""
    pool = pool_of((64, 64))
    env = make_env(pool, 9, (33, 33), "std15", layout)
    drive(env, pool, "past the policy room, %s" % layout, "std15", seed=3, steps=5, rollout=False)


@pytest.mark.gpu
def test_sliced_observation():
    """Two slices; they meet at env 64 (the launcher cuts at multiples of 64 envs), the second holds 6 envs."""
    import torch
    pool = pool_of((25, 25))
    env = make_env(pool, 70, (8, 6), "std19", "uint8", slices=2)
    assert env.slices == 2 and env.slice_bounds == (0, 64, 70)
    ck = Checker(env, pool, "slices=2 B=70", "std19")
    rng = np.random.default_rng(70)
    env.reset()
    ck.check("reset")
    for t in range(5):
        a = torch.from_numpy(rng.integers(1, 5, 70).astype(np.int32)).to(env.device)
        torch.cuda.synchronize()
        env.step_async(a)
        env.join()
        ck.check("step_async %d" % t)
    assert ck.reloads_to_other_count > 0 and ck.piles > 0


def multi_levels(rng, n_levels):
    """10x10 levels with three agents close together and 3 to 5 exits at least four moves away from each of them."""
    from safelife_amd.levels import Level
    levels = []
    yy, xx = np.mgrid[0:10, 0:10]
    for k in range(n_levels):
        board = CELLS[rng.integers(0, len(CELLS), (10, 10))]
        goals = (rng.integers(0, 8, (10, 10)) * (rng.random((10, 10)) < 0.6)).astype(np.uint16) << 9
        oy, ox = (int(v) for v in rng.integers(0, 10, 2))
        agents = [((oy + dy) % 10, (ox + dx) % 10) for dy, dx in ((0, 0), (0, 2), (2, 1))]
        dist = np.minimum((yy - oy) % 10, (oy - yy) % 10) + np.minimum((xx - ox) % 10, (ox - xx) % 10)
        far = np.flatnonzero(dist.ravel() >= 7)
        for j, cell in enumerate(rng.choice(far, (5, 3, 4)[k % 3], replace=False)):
            board.flat[cell] = EXIT
            goals.flat[cell] = WHITE if j == 1 else int(rng.integers(0, 8)) << 9
        for a in agents:
            board[a] = PLAYER
        levels.append(Level(board, goals, agents, min_performance=-1.0))
    return levels


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [None, "float32"], ids=["uint8", "float32-policy"])
def test_multi_agent_observation(layout):
    """10x10, three agents, up to five exits, view (7, 6): every agent's view from the read-back ``agent_locs``."""
    from safelife_amd.levels import LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    rng = np.random.default_rng(310)
    pool = LevelPool(multi_levels(rng, 6), counts_fn=util.oracle_counts, n_agents=3, exit_slots=5, seed=3)
    B, view, chans = 5, (7, 6), obs_ref.STD19
    env = SafeLifeMultiAgentVectorEnv(pool, B, view_shape=view, output_channels=chans, time_limit=3, auto_reset=True,
                                      first_level=np.arange(B) % 6, level_stride=5, policy_layout=layout)
    piles = 0

    def check(entry):
        nonlocal piles
        board, goals, exits = env.numpy("board"), env.numpy("goals"), env.numpy("exit_locs")
        locs, level = env.numpy("agent_locs"), env.numpy("level_idx")
        obs = env.numpy("obs")
        pol = env.policy_tensor.cpu().numpy() if layout else None
        for e in range(B):
            assert np.array_equal(exits[e], pool.pool_exit_locs[level[e]]), (entry, e)
            for a in range(3):
                want = obs_ref.get_obs(board[e], goals[e], locs[e, a], exits[e], view, chans, True)
                where = "board 10x10, view %s, channels std19, multi-agent %s, entry point %s, env %d agent %d" \
                    % (view, layout or "uint8", entry, e, a)
                diff = obs_ref.first_difference(obs[e, a], want)
                assert diff is None, "%s, obs (cell, channel): %s" % (where, diff)
                if pol is not None:
                    diff = obs_ref.first_difference(pol[e, a], obs_ref.policy_layout(want, np.float32))
                    assert diff is None, "%s, policy layout (channel, x, y): %s" % (where, diff)
                y0, x0 = locs[e, a] if locs[e, a][0] >= 0 else (0, 0)
                iy, ix = np.divmod(exits[e][exits[e] >= 0], 10)
                cells = set(zip(np.clip((iy - y0 + 5) % 10 - 5 + 3, 0, 6).tolist(), np.clip((ix - x0 + 5) % 10 - 5 + 3, 0, 5).tolist()))
                piles += len(cells) < len(iy)
        return level

    env.reset()
    first = check("reset")
    for t in range(4):
        env.step(rng.integers(1, 5, (B, 3)).astype(np.int32))
        level = check("step %d" % t)
    assert not np.array_equal(first, level), "no env reloaded its next level"
    assert piles > 0, "no two exits on one view cell"
