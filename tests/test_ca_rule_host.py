"""CPU: the Life rule's restatement (tests/ca_ref.py) against the reference's recorded output
(tests/golden/ca_rule_cases.npz, written by tests/golden/make_golden_ca_rule.py), the oracle against the restatement on
every constructed case at every shape, what the cases reach (asserted on the restatement alone), and the wrong readings
of the rule that the fixture tells apart from it.  Integer work: every comparison is exact.
"""
import os

import numpy as np
import pytest

import oracle
from tests import ca_ref as ref
from tests import ca_rule_cases as crc
from tests import util

CASES = crc.host_cases()
CASE_IDS = [crc.case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(util.GOLDEN, "ca_rule_cases.npz")) as d:
        return {k: d[k] for k in d.files}


def _fixture_case(name):
    kind, shape = name.split("-")
    H, W = (int(v) for v in shape.split("x"))
    return kind, H, W


FIXTURE_CASES = (["tile-%dx%d" % crc.FIXTURE_TILE_SHAPE] + ["seam-%dx%d" % s for s in crc.FIXTURE_SEAM_SHAPES]
                 + ["soup-%dx%d" % s for s in crc.FIXTURE_SOUP_SHAPES])


def test_fixture_holds_the_cases_of_the_issue(fixture):
    assert list(fixture["cases"]) == FIXTURE_CASES
    assert os.path.getsize(os.path.join(util.GOLDEN, "ca_rule_cases.npz")) <= os.path.getsize(
        os.path.join(util.GOLDEN, "primitives.npz"))


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_restatement_reproduces_the_reference(fixture, name):
    """Boards after 1 and 3 steps, counts after 1, 2 and 7, and the generator's words after every call, bit for bit --
    on the boards the case module builds today (they are the fixture's inputs)."""
    kind, H, W = _fixture_case(name)
    b = crc.BATCHES[kind](H, W)
    assert np.array_equal(fixture[name + "_in"], b.boards) and np.array_equal(fixture[name + "_p"], b.p)
    assert np.array_equal(fixture[name + "_w0"], b.words)
    r = ref.trajectory(b.boards, b.p, b.words, 7, count_steps=(1, 2, 7))
    for n in (1, 3):
        assert np.array_equal(r["boards"][n], fixture["%s_adv%d" % (name, n)]), n
        assert np.array_equal(r["words"][n], fixture["%s_adv%d_w" % (name, n)]), n
    for n in (1, 2, 7):
        assert np.array_equal(r["counts"][n], fixture["%s_occ%d" % (name, n)]), n
        assert np.array_equal(r["words"][n], fixture["%s_occ%d_w" % (name, n)]), n
    # the one-call forms of the restatement (the wrong readings below go through them) say the same
    got, words = ref.advance(b.boards[:40], b.p[:40], 3, b.words[:40])
    assert np.array_equal(got, fixture[name + "_adv3"][:40]) and np.array_equal(words, fixture[name + "_adv3_w"][:40])
    got, words = ref.occupancy(b.boards[:40], b.p[:40], 7, b.words[:40])
    assert np.array_equal(got, fixture[name + "_occ7"][:40]) and np.array_equal(words, fixture[name + "_occ7_w"][:40])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_oracle_equals_the_restatement(case):
    """advance_board at n = 1 and 3 and with one step count per board, life_occupancy at 1, 2, 7 and (boards of up to
    4096 cells) 20 steps: boards, counts, words."""
    kind, H, W = case
    b = crc.BATCHES[kind](H, W)
    r = crc.run(kind, H, W)
    for n in (1, 3):
        w = b.words.copy()
        got = oracle.advance_board_batch(b.boards, b.p, n, w, n_threads=8)
        assert np.array_equal(got, r["boards"][n]) and np.array_equal(w, r["words"][n]), n
    each = crc.each_steps(len(b.boards))
    want, want_w = crc.each_from(r, each)
    for s in range(4):
        on = np.flatnonzero(each == s)
        w = np.ascontiguousarray(b.words[on])
        got = oracle.advance_board_batch(b.boards[on], b.p[on], s, w) if s else b.boards[on]
        assert np.array_equal(got, want[on]) and np.array_equal(w, want_w[on]), s
    for n in sorted(r["counts"]):
        w = b.words.copy()
        got = oracle.life_occupancy_batch(b.boards, b.p, n, w, n_threads=8)
        assert np.array_equal(got, r["counts"][n]) and np.array_equal(w, r["words"][n]), n
    assert set(r["counts"]) == {1, 2, 7} | ({crc.N_LONG} if H * W <= 4096 else set())


# ---------------------------------------------------------------------------------------------- what the cases reach

def test_tile_list():
    ts = crc.tiles()
    fam = lambda f: [t for t in ts if t.family == f]
    assert len(fam("triple")) == 512 and len({t.nb for t in fam("triple")}) == 512
    assert len({t.nb for t in fam("vote")}) == 64
    for cls, cells in crc.CENTRES.items():
        for c in cells:
            counts = sorted(sum(1 for x in t.nb if x & 1) for t in fam("count") if t.centre == c)
            assert counts == sorted(list(range(9)) * 2), (cls, c)       # 0-8 alive neighbours, two rotations each
            flagged = {(t.nb.index(max(t.nb)), max(t.nb)) for t in fam("flag") if t.centre == c}
            assert len(flagged) == 3 * 8 * 4, (cls, c)      # three flags x eight positions x dead/alive x frozen or not
    assert len(crc.seam_tiles()) == 40


@pytest.mark.parametrize("H,W", crc.TILE_SHAPES, ids=["%dx%d" % s for s in crc.TILE_SHAPES])
def test_tiles_reach_every_class_and_outcome(H, W):
    """At the tiles' centres, in the first step: every cell that stands for a centre class meets every outcome the rule
    allows the class, and no other.  Every tile sits on its board as it was made."""
    b = crc.tile_batch(H, W)
    ts = crc.tiles()
    outcome = crc.run("tile", H, W)["outcomes"][0]
    half = len(b.boards) // 2
    assert (b.p[:half] == 0.0).all() and (b.p[half:] == 1.0).all() and np.array_equal(b.boards[:half], b.boards[half:])
    seen = {}
    for board, y, x, k in b.where:
        t = ts[k]
        assert b.boards[board, y, x] == t.centre
        assert [b.boards[board, (y + dy) % H, (x + dx) % W] for dy, dx in crc.DIRS] == list(t.nb)
        seen.setdefault((t.cls, t.centre), set()).update((int(outcome[board, y, x]), int(outcome[board + half, y, x])))
    for cls, cells in crc.CENTRES.items():
        for c in cells:
            assert seen[(cls, c)] == crc.REACHABLE[cls], (cls, c, sorted(ref.OUTCOMES[o] for o in seen[(cls, c)]))
    assert set(ref.OUTCOMES[o] for s in seen.values() for o in s) == set(ref.OUTCOMES)


def test_seam_tiles_turn_on_every_direction_and_plane():
    """For every direction and every plane there is a seam tile that holds the plane at that neighbour, and ONLY the
    outcome with the bit in place is the rule's: with the bit cleared the centre ends as another cell."""
    need = {(d, name) for d in range(8) for name in crc.PLANES}
    for t in crc.seam_tiles():
        def centre_after(tile):
            board = np.zeros((1, 7, 7), np.uint16)
            crc.put(board[0], tile, 3, 3)
            return int(ref.advance(board, [1.0], 1, crc.rng_words(1, 1))[0][0, 3, 3])
        for d in range(8):
            for name, bit in crc.PLANES.items():
                if t.nb[d] & bit:
                    nb = list(t.nb)
                    nb[d] &= ~bit
                    if centre_after(t) != centre_after(t._replace(nb=tuple(nb))):
                        need.discard((d, name))
    assert not need, sorted(need)


SEAM_SHAPES = crc.ALL_SHAPES + crc.PASS_SHAPES + ((9, 11),)


@pytest.mark.parametrize("H,W", SEAM_SHAPES, ids=["%dx%d" % s for s in SEAM_SHAPES])
def test_seam_batch_places_every_tile_everywhere(H, W):
    """Every seam tile stands intact with its centre at every placement (so every direction carries every plane there),
    and the batch ends in a workgroup of one board."""
    b = crc.seam_batch(H, W)
    ts = crc.seam_tiles()
    places = crc.seam_placements(H, W)
    cells = {(y, x) for _, y, x in places}
    assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2 - 1), (H // 2, W // 2),
            (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)} <= cells
    assert len({x for y, x in cells if y == 0}) >= min(W, 4) and len({x for y, x in cells if y == H - 1}) >= min(W, 4)
    seen = set()
    for board, y, x, k, pi in b.where:
        t = ts[k]
        assert (y, x) == places[pi][1:] and b.boards[board, y, x] == t.centre
        assert [b.boards[board, (y + dy) % H, (x + dx) % W] for dy, dx in crc.DIRS] == list(t.nb)
        assert b.p[board] == 1.0
        seen.add((int(k), int(pi)))
    assert len(seen) == len(ts) * len(places)
    assert len(b.boards) % (4 * crc.boards_per_wave(H, W)) == 1


SOUP_SHAPES = crc.ALL_SHAPES + crc.PASS_SHAPES


@pytest.mark.parametrize("H,W", SOUP_SHAPES, ids=["%dx%d" % s for s in SOUP_SHAPES])
def test_soup_keeps_moving(H, W):
    """The first three steps of a shape's soup hold at least 20 births whose DESTRUCTIBLE bit depends on a parent's EXIT
    bit, 20 deaths of alive AGENT or EXIT cells that are not frozen, and 20 cells whose exclusion from the occupancy count
    changes from one step to the next; every spawn_prob of SOUP_P occurs, and the batch ends in a workgroup of one."""
    b = crc.soup_batch(H, W)
    ev = crc.soup_events(crc.run("soup", H, W))
    assert ev["exit_births"] >= 20 and ev["deaths"] >= 20 and ev["changes"] >= 20, ev
    assert set(b.p.tolist()) == set(np.array(crc.SOUP_P, np.float32).tolist())
    assert len(b.boards) % (4 * crc.boards_per_wave(H, W)) == 1
    alive, dead = b.boards[(b.boards & 1) != 0], b.boards[(b.boards & 1) == 0]
    for bit in range(1, 16):    # every bit occurs on alive and on dead cells
        assert (alive >> bit & 1).any() and (dead >> bit & 1).any(), bit


def test_soup_64_mixes_the_occupancy_instantiations():
    vary = [crc.varying_colour_bits(b) for b in crc.soup_batch(64, 64).boards]
    assert 3 in vary and any(v <= 2 for v in vary), vary


# ---------------------------------------------------------------------------------------------- wrong readings

WRONG_ON = ("tile-%dx%d" % crc.FIXTURE_TILE_SHAPE, "soup-%dx%d" % crc.FIXTURE_SOUP_SHAPES[0])


@pytest.mark.parametrize("reading", ref.WRONG_READINGS)
def test_fixture_tells_a_wrong_reading_apart(fixture, reading):
    """Each wrong reading of the rule gives other boards, counts or generator words than the reference recorded."""
    differs = []
    for name in WRONG_ON:
        boards, p, words = fixture[name + "_in"], fixture[name + "_p"], fixture[name + "_w0"]
        got, w = ref.advance(boards, p, 1, words, readings=(reading,))
        differs.append(not np.array_equal(got, fixture[name + "_adv1"]) or not np.array_equal(w, fixture[name + "_adv1_w"]))
        got, w = ref.occupancy(boards, p, 7, words, readings=(reading,))
        differs.append(not np.array_equal(got, fixture[name + "_occ7"]) or not np.array_equal(w, fixture[name + "_occ7_w"]))
    assert any(differs), reading
    if reading.startswith("occupancy"):         # (these two leave the boards alone: the counts tell)
        assert not differs[0] and not differs[2] and (differs[1] or differs[3])


# ---------------------------------------------------------------------------------------------- the fused step's levels

@pytest.mark.parametrize("kind", crc.STEP_KINDS)
@pytest.mark.parametrize("H,W", [(25, 25), (30, 30), (31, 33)], ids=["25x25", "30x30", "31x33"])
def test_step_levels_follow_the_restatement_in_the_oracle_env(H, W, kind):
    """The levels tests/test_ca_rule_gpu.py gives the fused step: at most eight exit slots, the agent walled in -- and
    the oracle env's no-op step is one step of the restatement on the env's own board and generator, everywhere but on
    the cells the env paints after the step (the exits and the agent's cell).  The soup levels still hold births whose
    DESTRUCTIBLE bit hangs on an EXIT bit."""
    from safelife_amd.levels import LevelPool
    levels, B, kw, actions = crc.step_case(kind, H, W, False)
    pool = LevelPool(levels, counts_fn=util.oracle_counts, min_performance_fraction=1.0)
    assert pool.exit_slots <= crc.MAX_EXITS
    for lv in levels:
        assert lv.board[H - 2, W - 2] == 122 and (np.delete(lv.board[H - 3:, W - 3:].reshape(-1), 4) == 16).all()
    cpu = util.OracleBackend(pool, B, **kw)
    cpu.reset()
    p = np.array([lv.spawn_prob for lv in levels], np.float32)
    exit_births = 0
    for t in range(crc.STEP_SINGLE):
        before, words = cpu.get("board"), cpu.get("rng")
        cpu.step(actions[t])
        gens = [ref.gen_from_words(w) for w in words]
        want, outcome = ref.step(before, p, gens)
        got = cpu.get("board")
        painted = np.zeros(got.shape, bool)
        painted[:, H - 2, W - 2] = True
        for e, locs in enumerate(cpu.get("exit_locs")):
            painted[e].reshape(-1)[locs[locs >= 0]] = True
        assert np.array_equal(got[~painted], want[~painted]), t
        assert np.array_equal(cpu.get("rng"), np.stack([ref.words_of(g) for g in gens])), t
        assert (cpu.get("agent_loc") == (H - 2, W - 2)).all()
        run_ = dict(boards=[before, want], outcomes=[outcome])
        exit_births += crc.soup_events(run_, steps=1)["exit_births"]
    assert exit_births >= 20


def test_four_wave_batches_reach_the_four_wave_kernel():
    """The repeated batches of tests/test_ca_rule_gpu.py are past launch_advance_t's threshold on 256 CUs and end in a
    workgroup of one board; every batch as it stands is below it; the shapes cover every layout and every way a lane
    reaches its neighbour rows."""
    from tests import step_matrix_cases as smc
    for kind in ("seam", "soup"):
        for H in crc.FOUR_WAVE_SHAPES:
            b, idx = crc.four_wave_batch(kind, H)
            NB = 4 * crc.boards_per_wave(H, H)
            assert crc.advance_kernel(H, H, len(b.boards), crc.FOUR_WAVE_CUS) == "four-wave" and len(b.boards) % NB == 1
            assert set(idx.tolist()) == set(range(len(crc.BATCHES[kind](H, H).boards)))
            assert np.array_equal(b.boards[-1], crc.BATCHES[kind](H, H).boards[idx[-1]])
    for kind, H, W in [c for c in crc.cases() if crc.family(c[1], c[2]) == "row"]:
        assert crc.advance_kernel(H, W, len(crc.BATCHES[kind](H, W).boards), crc.FOUR_WAVE_CUS) == "small"
    assert {smc.geometry(H, H)["VERT"] for H in crc.FOUR_WAVE_SHAPES} == {"rotate", "shift", "bpermute"}
    assert {smc.geometry(H, H)["G"] for H in crc.FOUR_WAVE_SHAPES} == {1, 2, 3}
