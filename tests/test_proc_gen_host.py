"""CPU suite for safelife_amd.proc_gen: the level glue under the plain-Python restatement of gen_pattern as backend
(tests/gen_pattern_ref.py) -- determinism, independence from the batch, where agents, exit and regions lie, the round trip
through LevelPool -- and the still-life property of the generated levels.  No GPU."""
import os

import numpy as np
import pytest

import oracle
from safelife_amd import levels, proc_gen
from safelife_amd.cell_types import CellTypes
from tests import gen_pattern_ref as gpr
from tests import util

SPECS = os.path.join(util.REPO, "tests", "golden", "procgen")
SEEDS = list(range(200, 216))


def spec(name):
    return proc_gen.load_params(os.path.join(SPECS, name + ".yaml"), defaults=os.path.join(SPECS, "_defaults.yaml"))


class RestatedBackend(object):
    """gen_pattern_ref.gen_pattern per request.  A request is a pure function's argument, so equal requests are answered from a
    memo: a level whose requests depended on its batch would miss it (and, being another chain, come out different)."""

    def __init__(self):
        self.memo, self.calls, self.batches = {}, 0, []

    def __call__(self, requests):
        self.batches.append(len(requests))
        out = []
        for rq in requests:
            key = (rq.board.tobytes(), rq.mask.tobytes(), None if rq.seeds is None else rq.seeds.tobytes(), rq.period,
                   tuple(sorted(rq.kwargs.items())), np.asarray(rq.words).tobytes())
            if key not in self.memo:
                self.calls += 1
                g = gpr.gen_pattern(rq.board, rq.mask, rq.period, seeds=rq.seeds, words=rq.words, **rq.kwargs)
                self.memo[key] = (g["board"], g["status"], g["words"])
            b, s, w = self.memo[key]
            out.append((b.copy(), s, w.copy()))
        return out


@pytest.fixture(scope="module")
def backend():
    return RestatedBackend()


@pytest.fixture(scope="module")
def prune_still(backend):
    return proc_gen.gen_games(spec("prune-still"), SEEDS, backend=backend)


def same_level(a, b):
    return (np.array_equal(a.board, b.board) and np.array_equal(a.goals, b.goals) and np.array_equal(a.agent_locs, b.agent_locs)
            and np.array_equal(a.points_table, b.points_table) and a.min_performance == b.min_performance
            and np.array_equal(a.initial_rng_words(), b.initial_rng_words()) and a.board.tobytes() == b.board.tobytes())


def test_load_params_merges_like_the_level_iterator():
    p = spec("prune-still")
    d = proc_gen.load_params(os.path.join(SPECS, "_defaults.yaml"))
    assert p["later_regions"] == "prune medium" and p["min_performance"] == 0.5 and p["partitioning"]["max_regions"] == 3
    assert p["named_regions"] == d["named_regions"] and p["agents"] == ["agent0"] and "agent0" in p["agent_types"]
    own = proc_gen.load_params(os.path.join(SPECS, "prune-still.yaml"))
    assert "named_regions" not in own
    merged = proc_gen.load_params(os.path.join(SPECS, "prune-still.yaml"), defaults={"named_regions": {"x": []}, "agents": []})
    assert merged["named_regions"] == {"x": []} and merged["agents"] == []


def test_random_values():
    rng = np.random.default_rng(1)
    assert proc_gen._resolve({"a": 3, "b": [1, {"uniform": [2, 2]}]}, rng) == {"a": 3, "b": [1, 2.0]}
    picks = {proc_gen._resolve({"choices": ["x", "y"]}, rng) for _ in range(40)}
    assert picks == {"x", "y"}
    assert {proc_gen._resolve({"choices": {"x": 0, "y": 2}}, rng) for _ in range(20)} == {"y"}
    assert {proc_gen._resolve({"choices": ["x", "y"], "weights": [1, 0]}, rng) for _ in range(20)} == {"x"}
    assert all(1 <= proc_gen._resolve({"uniform": [1, 3]}, rng) < 3 for _ in range(20))
    with pytest.raises(ValueError):
        proc_gen._resolve({"choices": 5}, rng)
    with pytest.raises(ValueError):
        proc_gen._resolve({"choices": ["x"], "weights": [-1]}, rng)


def test_partition_keeps_regions_apart():
    for seed in range(12):
        shape = [(26, 26), (25, 25), (13, 20), (64, 64)][seed % 4]
        lo, hi = [(2, 3), (2, 4), (1, 1), (3, 5)][seed % 4]
        regions = proc_gen.partition(np.random.default_rng(seed), shape, min_regions=lo, max_regions=hi)
        assert regions.shape == shape and regions.min() == 0 and 1 <= regions.max() <= hi
        check_regions(regions)


def check_regions(regions):
    """different regions are never within two cells of each other (wrapped), and each is 4-connected"""
    H, W = regions.shape
    for k in range(1, int(regions.max()) + 1):
        mine = regions == k
        assert mine.any()
        others = (regions > 0) & ~mine
        assert not (proc_gen._grow(mine, 2) & others).any(), k
        seen = np.zeros_like(mine)
        seen.reshape(-1)[np.flatnonzero(mine)[0]] = True
        while True:
            grown = seen.copy()
            for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                grown |= np.roll(seen, (dy, dx), (0, 1))
            grown &= mine
            if (grown == seen).all():
                break
            seen = grown
        assert (seen == mine).all(), k


def test_levels_are_what_a_spec_says(prune_still):
    assert len(prune_still) == len(SEEDS)
    for lv, seed in zip(prune_still, SEEDS):
        assert isinstance(lv, levels.Level) and lv.board.shape == (26, 26) and lv.board.dtype == np.uint16
        assert lv.min_performance == 0.5 and lv.name.endswith(str(seed)) and lv.points_table.shape == (1, 8, 9)
        regions = lv.regions
        assert 2 <= regions.max() <= 3
        check_regions(regions)
        # agent and exit in the buffer region
        assert lv.agent_locs.shape == (1, 2)
        r, c = lv.agent_locs[0]
        assert regions[r, c] == 0 and lv.board[r, c] & CellTypes.agent
        assert len(lv.exit_locs) == 1 and regions.reshape(-1)[lv.exit_locs[0]] == 0
        # prune medium: green and red life inside the regions, none outside; red cells are what there is to remove
        alive = (lv.board & CellTypes.alive) != 0
        assert alive.any() and not (alive & (regions == 0)).any()
        colours = set(np.unique(lv.board[alive & ((lv.board & CellTypes.frozen) == 0)] & CellTypes.rainbow_color).tolist())
        assert colours <= {int(CellTypes.color_r), int(CellTypes.color_g)} and int(CellTypes.color_g) in colours
        assert ((lv.goals & CellTypes.rainbow_color) == CellTypes.rainbow_color)[regions == 0].all()     # the buffer shows white


def test_determinism_and_independence_from_the_batch(backend, prune_still):
    params = spec("prune-still")
    calls = backend.calls
    again = proc_gen.gen_games(params, SEEDS, backend=backend)
    reverse = proc_gen.gen_games(params, SEEDS[::-1], backend=backend)[::-1]
    alone = [proc_gen.gen_games(params, [s], backend=backend)[0] for s in SEEDS]
    mixed = proc_gen.gen_games(params, [SEEDS[5], 999, SEEDS[2]], backend=backend)
    assert backend.calls <= calls + 80          # only seed 999's chains are new: every other request was seen before
    for k in range(len(SEEDS)):
        assert same_level(prune_still[k], again[k]) and same_level(prune_still[k], reverse[k]), SEEDS[k]
        assert same_level(prune_still[k], alone[k]), SEEDS[k]
    assert same_level(mixed[0], prune_still[5]) and same_level(mixed[2], prune_still[2])
    assert not same_level(prune_still[0], prune_still[1])
    assert max(backend.batches) == len(SEEDS)           # a round's requests go to the backend in ONE call


def test_level_round_trips_through_level_pool(prune_still):
    pool = levels.LevelPool(prune_still[:4], counts_fn=util.oracle_counts, refreshable=True)
    for k, lv in enumerate(prune_still[:4]):
        assert np.array_equal(pool.pool_board[k], lv.board) and np.array_equal(pool.pool_goals[k], lv.goals)
        assert np.array_equal(pool.pool_agent_loc[k], lv.agent_locs[0]) and np.array_equal(pool.pool_rng[k], lv.initial_rng_words())
        assert pool.pool_exit_locs[k, 0] == lv.exit_locs[0]
        assert pool.pool_required_reset[k] > 0                   # min_performance 0.5 of something to do
    phys = pool.replace([1, 3], pool.prepare(prune_still[4:6]))
    assert phys == [5, 7] and np.array_equal(pool.pool_board[5], prune_still[4].board)
    data = prune_still[0].as_data()
    back = levels.Level.from_data(data)
    assert np.array_equal(back.board, prune_still[0].board) and np.array_equal(back.goals, prune_still[0].goals)


def test_fill_pool_on_the_host(backend, prune_still):
    pool = levels.LevelPool(prune_still[:3], counts_fn=util.oracle_counts, refreshable=True)
    new = proc_gen.fill_pool(pool, [0, 2], spec("prune-still"), [SEEDS[7], SEEDS[9]], backend=backend)
    assert same_level(new[0], prune_still[7]) and same_level(new[1], prune_still[9])
    assert pool.bank.tolist() == [1, 0, 1] and np.array_equal(pool.pool_board[pool.slot_of(2)], prune_still[9].board)
    with pytest.raises(ValueError):
        proc_gen.fill_pool(pool, [0], spec("prune-still"), [1, 2], backend=backend)


def test_still_levels_are_fixed_points(backend, prune_still):
    """The reference's own prune-still levels (tests/golden/pool_prune_still_25.npz) are fixed points of one step of the
    oracle's automaton; so are the generated still levels."""
    with np.load(os.path.join(util.REPO, "tests", "golden", "pool_prune_still_25.npz")) as z:
        theirs = z["board"][:24]
    assert all(np.array_equal(oracle.advance_board(b, 0.0, 1), b) for b in theirs)
    ours = list(prune_still) + proc_gen.gen_games(spec("append-still-easy"), SEEDS[:4], backend=backend)
    for lv in ours:
        assert np.array_equal(oracle.advance_board(lv.board, 0.0, 1), lv.board), lv.name
        goal_board = lv.goals & ~np.uint16(CellTypes.rainbow_color)         # the goal patterns are still lifes too
        assert np.array_equal(oracle.advance_board(goal_board, 0.0, 1) & 1, goal_board & 1), lv.name


def test_multi_agent_spec_and_spawner_spec(backend):
    multi = proc_gen.gen_games(spec("multi-agent-build-coop"), [1, 2], backend=backend)
    for lv in multi:
        assert lv.agent_locs.shape == (2, 2) and lv.points_table.shape == (2, 8, 9) and lv.agent_names == ["default", "default"]
        assert len({tuple(x) for x in lv.agent_locs.tolist()}) == 2
        assert all(lv.regions[r, c] == 0 for r, c in lv.agent_locs)
        assert ((lv.goals & CellTypes.alive) != 0).any()                    # build easy: blue goals to fill
    levels.LevelPool(multi, counts_fn=util.oracle_counts, n_agents=2)
    spawn = proc_gen.gen_games(spec("append-spawn"), [3], backend=backend)[0]
    assert ((spawn.board & CellTypes.spawning) != 0).any() and not ((spawn.goals & CellTypes.spawning) != 0).any()


def test_recorded_levels_are_the_reference_backends():
    """where the reference extension is built, the recorded levels are what its gen_pattern gives as backend now"""
    ref = oracle.load_ref()
    with np.load(os.path.join(util.REPO, "tests", "golden", "procgen_levels.npz")) as z:
        assert [str(s) for s in z["specs"]] == ["append-still-easy", "prune-still", "append-spawn", "multi-agent-build-coop"]
        if ref is None or not hasattr(ref, "gen_pattern"):
            return
        for name in z["specs"]:
            name = str(name)
            seeds = z[name + "_seeds"].tolist()
            lv = proc_gen.gen_games(spec(name), seeds, backend=proc_gen.function_backend(ref))
            assert np.array_equal(np.stack([x.board for x in lv]), z[name + "_board"]), name
            assert np.array_equal(np.stack([x.goals for x in lv]), z[name + "_goals"]), name
