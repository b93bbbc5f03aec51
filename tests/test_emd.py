"""
The earth-mover distances of side_effect_score on the device (slhip_emd_batch, SideEffectBatch.scores_all) against
the host LP (side_effects.earth_mover_distance: the full n x n transportation problem, HiGHS).

tests/golden/emd_cases.npz (make_golden_emd.py) holds the problems and the LP's answers (HiGHS with feasibility
tolerances below the comparison's: the generator says why).  Tolerance of a device value
against a recorded one: the device result is exact up to float64 summation, the LP is not; the fixture records how far
two LP solves (dual simplex, interior point) of the same problem differ at most (``lp_spread``), and a device value
may differ from the recorded one by ``max(10 * lp_spread, 1e-9 * max(1, value))``.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import util


@pytest.fixture(scope="module")
def cases():
    with np.load(os.path.join(util.GOLDEN, "emd_cases.npz")) as d:
        d = {k: d[k] for k in d.files}
    out = []
    for i, name in enumerate(d["names"]):
        shape = tuple(int(v) for v in d["shapes"][i])
        lo, hi = int(d["offsets"][i]), int(d["offsets"][i + 1])
        out.append(dict(name=str(name), shape=shape, den=int(d["den"][i]), a=d["a_flat"][lo:hi].reshape(shape),
                        b=d["b_flat"][lo:hi].reshape(shape), value=float(d["value"][i]), mass=float(d["mass"][i]),
                        n_cells=int(d["n_cells"][i])))
    return out, float(d["lp_spread"])


def _tol(value, lp_spread):
    return max(10 * lp_spread, 1e-9 * max(1.0, abs(value)))


# ---------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("shape", [(25, 25), (7, 12)])
@pytest.mark.parametrize("wrap", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("metric", ["manhattan", "euclidean"])
def test_ground_table_is_the_ground_distance(shape, wrap, metric):
    """ground_table[dr + H-1, dc + W-1] is, bit for bit, the ground distance of every pair of cells: the one
    `_ground_distance` returns, and the reference's formula (side_effects.py:38-56) written out on the pairs."""
    from safelife_amd import side_effects as se
    H, W = shape
    rows, cols = np.divmod(np.arange(H * W), W)
    table = se.ground_table(shape, metric, wrap[0], wrap[1], 5.0)
    assert table.shape == (2 * H - 1, 2 * W - 1) and table.dtype == np.float64
    looked_up = table[rows[:, None] - rows[None, :] + H - 1, cols[:, None] - cols[None, :] + W - 1]
    assert np.array_equal(looked_up, se._ground_distance(rows, cols, shape, metric, wrap[0], wrap[1], 5.0))
    gy, gx = rows[:, None] - rows[None, :], cols[:, None] - cols[None, :]
    if wrap[1]:
        gy = np.minimum(gy, H - gy)
    if wrap[0]:
        gx = np.minimum(gx, W - gx)
    direct = np.hypot(gx, gy) if metric == "euclidean" else np.abs(gx).astype(float) + np.abs(gy)
    assert np.array_equal(looked_up, np.tanh(direct / 5.0))
    assert table[H - 1, W - 1] == 0.0


def test_fixture_values_are_the_host_lp(cases):
    """The recorded values are what today's earth_mover_distance returns (cases with at most 150 cells)."""
    from safelife_amd.side_effects import earth_mover_distance
    cases, lp_spread = cases
    assert len([c for c in cases if c["name"].startswith("random")]) >= 40 and lp_spread < 1e-9
    for c in cases:
        if c["n_cells"] <= 150:
            got = earth_mover_distance(c["a"] / c["den"], c["b"] / c["den"])
            assert abs(got - c["value"]) <= _tol(c["value"], lp_spread), c["name"]
            gap = np.abs(c["a"] / c["den"] - c["b"] / c["den"])
            assert int((gap > 1e-3 * gap.max()).sum()) == c["n_cells"] or gap.max() == 0, c["name"]


def test_closed_forms_of_the_fixture(cases):
    """The seam cases carry the closed forms test_emd_restatement_known_answers lists (0.7 of mass, 6x7 board)."""
    by_name = {c["name"]: c for c in cases[0]}
    for name, want in _closed_forms().items():
        assert abs(by_name[name]["value"] - want) < 1e-9, name


def _closed_forms():
    t = lambda d: 0.7 * np.tanh(d / 5)      # noqa: E731
    return {"seam/col+2": t(2), "seam/col-2": t(2), "seam/col_1_to_6": t(5), "seam/col_6_to_1": t(2),
            "seam/row_0_to_5": t(5), "seam/row_5_to_0": t(1), "seam/both_0_0_to_5_6": t(5 + 6),
            "seam/both_5_6_to_0_0": t(1 + 1), "seam/col_6_to_1_plus_extra": t(2) + 0.3,
            "equal/zeros": 0.0, "equal/ramp": 0.0, "onesided/b_zero": sum(range(42)) * 3 / 1000,
            "onesided/a_zero": sum(range(42)) * 3 / 1000, "onesided/mask_gone": 21.0}


# ---------------------------------------------------------------------------------------------------- GPU

def _run_cases(group, shape, den, concurrency=None, repeat=1):
    """slhip_emd_batch on a queue with one entry per case (tests/emd_queue.py packs and runs it, and checks the
    sentinels: entries past the count untouched, NaN / 0 in empty key slots): occupancy-count cases (den > 1) sit in
    life-colour slot (index % 8), mask cases (den == 1) in cell-type slot 8 + index % 16.  Returns (scores [n,2],
    n_cells [n]) per run."""
    from safelife_amd import _hip
    from tests.emd_queue import run_queue
    K = _hip.SL_SE_MAX_KEYS
    assert all(c["den"] == den for c in group)
    placement = [(i, i % 8 if den > 1 else 8 + i % (K - 8)) for i in range(len(group))]
    return run_queue(group, shape, den, concurrency=concurrency, repeat=repeat, placement=placement)


def _groups(cases):
    out = {}
    for c in cases:
        out.setdefault((c["shape"], c["den"]), []).append(c)
    return out


def _group_ids():
    with np.load(os.path.join(util.GOLDEN, "emd_cases.npz")) as d:
        return sorted(set("%dx%d/%d" % (h, w, den) for (h, w), den in zip(d["shapes"], d["den"])))


@pytest.mark.gpu
@pytest.mark.parametrize("group_id", _group_ids())
def test_emd_batch_matches_the_host_lp_on_every_case(cases, group_id):
    """GPU test 1: every fixture case, packed as queue entries (one queue per board shape and denominator), against
    the recorded host LP value; n_cells exact.  A device value ABOVE the LP's by more than the tolerance would mean
    the solver is not optimal.

    The 64x64/1000 group is side_effect_inputs_64/life-yellow, n = 1735: device 9.8464126538634, recorded
    9.84641265387246 (HiGHS at feasibility tolerances of 1e-10; at its default 1e-7 it stops at 9.846412666445385,
    1.26e-08 off, which is why the fixture is not recorded with the defaults: make_golden_emd.py)."""
    cases, lp_spread = cases
    groups = {"%dx%d/%d" % (shape + (den,)): (shape, den, group) for (shape, den), group in _groups(cases).items()}
    shape, den, group = groups[group_id]
    (scores, n_cells), = _run_cases(group, shape, den)
    for c, (dist, mass), n in zip(group, scores, n_cells):
        print("%-48s n=%4d device=%.16g host=%.16g diff=%.3g" % (c["name"], n, dist, c["value"], dist - c["value"]))
    for c, (dist, mass), n in zip(group, scores, n_cells):
        assert n == c["n_cells"], c["name"]
        assert abs(dist - c["value"]) <= _tol(c["value"], lp_spread), (c["name"], dist, c["value"])
        assert abs(mass - c["mass"]) <= 1e-12 * max(1.0, c["mass"]), c["name"]


def test_fixture_has_the_cases(cases):
    cases = cases[0]
    assert max(c["n_cells"] for c in cases) == 1735 and sum(len(g) for g in _groups(cases).values()) == len(cases)
    assert {c["shape"] for c in cases} >= {(25, 25), (26, 26), (64, 64), (9, 13), (13, 9)}


@pytest.mark.gpu
def test_emd_batch_closed_forms(cases):
    """GPU test 2: seam cases in both directions, pure-penalty cases and n = 0, to 1e-12 relative."""
    cases = [c for c in cases[0] if c["name"] in _closed_forms()]
    want = _closed_forms()
    assert len(cases) == len(want)
    for (shape, den), group in _groups(cases).items():
        (scores, n_cells), = _run_cases(group, shape, den)
        for c, (dist, _), n in zip(group, scores, n_cells):
            assert abs(dist - want[c["name"]]) <= 1e-12 * max(1.0, want[c["name"]]), (c["name"], dist)
            if c["name"].startswith("equal/"):
                assert n == 0 and dist == 0.0


@pytest.mark.gpu
def test_emd_batch_is_deterministic(cases):
    """GPU test 3: two launches on the same inputs give bit-identical scores, whatever the concurrency."""
    group = [c for c in cases[0] if c["shape"] == (25, 25) and c["den"] == 1000]
    assert len(group) >= 5
    first, second = _run_cases(group, (25, 25), 1000, repeat=2)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    (third,) = _run_cases(group, (25, 25), 1000, concurrency=3)
    assert np.array_equal(first[0], third[0])


def test_emd_batch_rejects_bad_arguments():
    """Workspace rule and argument checks of the entry point (host side only: nothing is launched)."""
    from safelife_amd import _hip
    lib = _hip.lib()
    assert lib.slhip_emd_workspace_bytes(25, 25, 96, 4) == 256 + 4 * (196096 + 22784)
    assert lib.slhip_emd_workspace_bytes(65, 25, 96, 4) == 0
    q = _hip.EpisodeQueue()
    q.capacity = 4
    one = C.c_void_p(256)
    assert lib.slhip_emd_batch(C.byref(q), 65, 25, 1000, one, one, one, one, 1.0, one, 1 << 30, 4, one, one, None) == _hip.SL_E_SHAPE
    assert lib.slhip_emd_batch(C.byref(q), 25, 25, 1000, one, one, one, one, -1.0, one, 1 << 30, 4, one, one, None) == _hip.SL_E_UNSUPPORTED
    assert lib.slhip_emd_batch(C.byref(q), 25, 25, 1000, one, one, one, one, 1.0, one, 1 << 30, 4, one, one, None) == _hip.SL_E_ARG    # (null queue pointers)


def _replay_batch(d, cap, n, num_samples, levels=None):
    """A SideEffectBatch over `n` queue entries that replay pinned inputs of the reference's side_effect_score (the
    set-up of test_side_effect_pass_reproduces_reference_inputs): d = list of dicts b0, b2, num_steps, spawn_prob, rng0."""
    import torch
    from safelife_amd import _hip, speedups as sp
    from safelife_amd.levels import Level, LevelPool, _device_counts
    from safelife_amd.vector_env import SafeLifeVectorEnv, SideEffectBatch
    starts = [Level(g["b0"], agent_locs=np.zeros((0, 2), int), spawn_prob=float(g["spawn_prob"])) for g in d]
    env = SafeLifeVectorEnv(LevelPool(starts, counts_fn=_device_counts), 4, with_obs=False)
    dev = env.device
    H, W = d[0]["b0"].shape
    rec = np.zeros((cap, 8), np.int32)
    boards = np.zeros((cap, H, W), np.uint16)
    rng = np.zeros((2 * cap, 4), np.uint64)
    for i in range(n):
        g = d[i % len(d)]
        rec[i, 0], rec[i, 1], rec[i, 2] = i, i % len(d), int(g["num_steps"])
        rec[i, 4] = np.float32(g["spawn_prob"]).view(np.int32)
        boards[i], rng[i] = g["b2"], g["rng0"]
    bufs = dict(count=torch.tensor([n], dtype=torch.int32, device=dev), records=torch.from_numpy(rec).to(dev),
                boards=torch.from_numpy(boards.view(np.int16)).to(dev))
    q = _hip.EpisodeQueue()
    q.capacity, q.env_base = cap, 0
    q.count, q.records, q.boards = (bufs[k].data_ptr() for k in ("count", "records", "boards"))
    K = _hip.SL_SE_MAX_KEYS
    out = dict(work_boards=torch.zeros((2 * cap, H, W), dtype=torch.int16, device=dev),
               work_prob=torch.zeros(2 * cap, dtype=torch.float32, device=dev),
               work_steps=torch.zeros(2 * cap, dtype=torch.int32, device=dev),
               work_rng=sp._to_device(rng, np.uint64),
               counts=torch.zeros((2, cap, H, W, 8), dtype=torch.int32, device=dev),
               keys=torch.zeros((cap, K), dtype=torch.int16, device=dev),
               life_dist=torch.zeros((cap, 2, 8, H, W), dtype=torch.float64, device=dev),
               type_masks=torch.zeros((cap, 2, K - 8, H, W), dtype=torch.uint8, device=dev))
    _hip.check(_hip.lib().slhip_side_effects(env._sref, C.byref(q), num_samples, 0,
                                             *[_hip.ptr(out[k]) for k in ("work_boards", "work_prob", "work_steps",
                                                                          "work_rng", "counts", "keys", "life_dist",
                                                                          "type_masks")],
                                             _hip.current_stream_ptr()))
    return SideEffectBatch(env, bufs, out, num_samples)


def _recorded(cases, prefix):
    from safelife_amd.side_effects import name_to_cell
    return {name_to_cell(c["name"][len(prefix):]): c for c in cases if c["name"].startswith(prefix)}


def _check_entry(all_, i, want, lp_spread):
    keys = all_["keys"][i].cpu().numpy().view(np.uint16)
    scores = all_["scores"][i].cpu().numpy()
    n_cells = all_["n_cells"][i].cpu().numpy()
    assert set(int(k) for k in keys if k != 0xFFFF) == set(want)
    for k, key in enumerate(keys):
        if key == 0xFFFF:
            assert np.isnan(scores[k]).all()
            continue
        c = want[int(key)]
        assert n_cells[k] == c["n_cells"]
        assert abs(scores[k, 0] - c["value"]) <= _tol(c["value"], lp_spread), (i, c["name"], scores[k, 0], c["value"])
        assert abs(scores[k, 1] - c["mass"]) <= 1e-12 * max(1.0, c["mass"])


@pytest.mark.gpu
def test_scores_all_end_to_end_25(cases):
    """GPU test 4: the queue of test_side_effect_pass_reproduces_reference_inputs (80 entries replaying the 25x25
    fixture, capacity 96) -> scores_all(): every valid entry has the recorded scores, slots past the count are
    untouched (NaN as allocated), scores(i, device=True) has the keys of scores(i) and, for entry 0, its values."""
    cases, lp_spread = cases
    with np.load(os.path.join(util.GOLDEN, "side_effect_inputs.npz")) as d:
        d = {k: d[k] for k in d.files}
    n, cap = 80, 96
    batch = _replay_batch([d], cap, n, 1000)
    weights = {"life-blue": 2.0, "crate-gray": 0.5, "life-red": 1.0, "tree-green": 3.0}
    all_ = batch.scores_all(weights=weights)
    assert all_["scores"].is_cuda and tuple(all_["scores"].shape) == (cap, 24, 2) and tuple(all_["total"].shape) == (cap, 2)
    assert batch.scores_all()["scores"] is all_["scores"]                       # computed once per batch
    want = _recorded(cases, "side_effect_inputs/")
    assert len(want) == 4
    for i in range(n):
        _check_entry(all_, i, want, lp_spread)
    assert np.isnan(all_["scores"][n:].cpu().numpy()).all() and (all_["n_cells"][n:].cpu().numpy() == 0).all()
    host = batch.scores(0, weights=weights)
    for i in (0, 41, n - 1):
        got = batch.scores(i, weights=weights, device=True)
        assert set(got) == set(host)
        if i == 0:
            for key in host:
                for g, h in zip(got[key], host[key]):
                    assert abs(g - h) <= _tol(h, lp_spread), key
        total = all_["total"][i].cpu().numpy()
        assert np.allclose(total, got["total"], rtol=1e-12, atol=0)
    only = batch.scores(0, include=["life-blue", "life-red"], exclude=["life-red"], device=True)
    assert set(only) == {"life-blue"}
    raw = batch.scores(0, strkeys=False, device=True)
    assert set(raw) == set(want)
    with pytest.raises(IndexError):
        batch.scores(n, device=True)


@pytest.mark.gpu
def test_scores_all_end_to_end_64(cases):
    """GPU test 4, 64x64: the navigation fixture (life-yellow: 1735 participating cells) against its recorded value
    -- four minutes of HiGHS when the fixture was made, no host LP here."""
    cases, lp_spread = cases
    with np.load(os.path.join(util.GOLDEN, "side_effect_inputs_64.npz")) as d:
        d = {k: d[k] for k in d.files}
    batch = _replay_batch([d], 6, 4, 1000)
    all_ = batch.scores_all()
    want = _recorded(cases, "side_effect_inputs_64/")
    assert max(c["n_cells"] for c in want.values()) == 1735
    for i in range(4):
        _check_entry(all_, i, want, lp_spread)
    got = batch.scores(1, device=True)
    from safelife_amd.side_effects import name_to_cell
    value = want[name_to_cell("life-yellow")]["value"]
    assert abs(got["life-yellow"][0] - value) <= _tol(value, lp_spread)


@pytest.mark.gpu
def test_scores_of_an_entry_with_too_many_cell_types():
    """GPU test 5: more frozen cell types than key slots -- the entry is NaN-marked on the device (n_cells -1) and
    scores(i, device=True) still returns the host result."""
    from safelife_amd import _hip
    from safelife_amd.cell_types import CellTypes as CT
    from safelife_amd.levels import Level, LevelPool, _device_counts
    H = W = 25
    b = np.zeros((H, W), np.uint16)
    kinds = [int(CT.frozen) | int(CT.destructible) | (c << 9) | extra for c in range(8) for extra in (0, int(CT.pushable), int(CT.pullable))]
    for i, v in enumerate(kinds):
        b[2 + i // 8 * 3, 2 + (i % 8) * 2] = v
    b[20, 20] = CT.player
    b[10, 10:13] = CT.life | CT.color_g
    lv = Level(b, np.zeros_like(b), [[20, 20]], min_performance=-1)
    pool = LevelPool([lv], counts_fn=_device_counts)
    dev = util.DeviceBackend(pool, 4, auto_reset=True, time_limit=3, view_shape=(9, 9), with_obs=False,
                             side_effects=dict(capacity=16, num_samples=20))
    dev.env.reset()
    for t in range(3):
        dev.env.step(np.zeros(4, np.int32))
    batch = dev.env.side_effects_flush()
    assert len(batch) == 4 and len(kinds) > _hip.SL_SE_MAX_KEYS - 8
    all_ = batch.scores_all(weights={"life-green": 1.0})
    assert np.isnan(all_["scores"][:4].cpu().numpy()).all() and (all_["n_cells"][:4].cpu().numpy() == -1).all()
    assert np.isnan(all_["total"][:4].cpu().numpy()).all()
    host = batch.scores(2)
    got = batch.scores(2, device=True)
    assert got == host
    raw = batch.scores(2, strkeys=False, device=True)
    assert len([k for k in raw if k & int(CT.frozen)]) == len(kinds)


@pytest.mark.gpu
def test_scores_all_of_a_multi_agent_batch(cases):
    """GPU test 6: queue entries of multi-agent games (side_effect_inputs_multi.npz, 26x26, 200 samples) through
    SideEffectBatch.scores_all(); and the same distances from a pass that ran on the env's side stream."""
    cases, lp_spread = cases
    with np.load(os.path.join(util.GOLDEN, "side_effect_inputs_multi.npz")) as d:
        d = {k: d[k] for k in d.files}
    games = [dict(b0=d["g%d_b0" % g], b2=d["g%d_b2" % g], num_steps=d["g%d_num_steps" % g],
                  spawn_prob=d["g%d_spawn_prob" % g], rng0=d["g%d_rng0" % g]) for g in range(int(d["n_games"]))]
    batch = _replay_batch(games, 8, 6, int(d["num_samples"]))
    all_ = batch.scores_all()
    for i in range(6):
        _check_entry(all_, i, _recorded(cases, "side_effect_inputs_multi/g%d/" % (i % 3)), lp_spread)
    assert sum(len(_recorded(cases, "side_effect_inputs_multi/g%d/" % g)) for g in range(3)) == 6


@pytest.mark.gpu
def test_scores_all_behind_an_overlapped_pass():
    """scores_all() of a batch whose pass ran on the env's side stream (overlap=True, defer=True) is launched behind
    it and gives what the same queue gives on the caller's stream: device distances equal to the host LP's."""
    from safelife_amd.levels import _device_counts
    pool, _ = util.pool_from_fixture("append_spawn_25", _device_counts, n=4, min_performance_fraction=0.05)
    dev = util.DeviceBackend(pool, 8, auto_reset=True, time_limit=5, view_shape=(9, 9), with_obs=False,
                             side_effects=dict(capacity=32, num_samples=40))
    dev.env.reset()
    rng = np.random.default_rng(3)
    for t in range(6):
        dev.env.step(rng.integers(0, 9, 8).astype(np.int32))
    batch = dev.env.side_effects_flush(overlap=True, defer=True)
    all_ = batch.scores_all()
    dev.env.step(np.zeros(8, np.int32))
    assert len(batch) >= 8
    host = batch.scores(3)
    got = batch.scores(3, device=True)
    assert set(got) == set(host)
    for key in host:
        assert abs(got[key][0] - host[key][0]) <= 1e-9 * max(1.0, host[key][0]) and abs(got[key][1] - host[key][1]) <= 1e-12 * max(1.0, host[key][1])
    assert not np.isnan(all_["scores"][3].cpu().numpy()).all()
