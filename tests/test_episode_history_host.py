"""
Episode histories without a GPU: the ABI of slhip_history_capture / _rewind, the numpy restatement
(tests/episode_history_ref.py) driven by the oracle's env against what the reference's ``SafeLifeEnv`` + ``SafeLifeLogWrapper``
+ ``SafeLifeLogger`` saved (tests/golden/episode_history_cases.npz, written by tests/golden/make_golden_episode_history.py)
and against the committed traces, the slot bookkeeping against hand-worked cases, and the argument checks of
safelife_amd.episode_history.

Every comparison is bit exact.  One thing about the reference's saved bytes, found while writing the fixture: the wrapper
appends ``game.board`` ITSELF to the history (safelife_logger.py:569) and the next step's ``execute_actions`` writes into
that array before ``advance_board`` replaces it, so every saved frame but the last shows the board after its step WITH THE
NEXT STEP'S ACTION already carried out.  The recorder keeps the boards as the steps left them -- ``info['board']``, what the
traces hold (``trace_board``) -- and ``episode_history_ref.as_the_reference_saved`` carries the next action out on a copy,
with the oracle's ``execute_actions``, before a history is held against the saved array: kept set, lengths, levels, goals
stacks and last frames are compared as they are, the other frames through that one function, all bit for bit.
"""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from safelife_amd import _hip, episode_history
from tests import episode_history_ref as hr
from tests import util

NAMES = ("slhip_history_capture", "slhip_history_rewind")


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "episode_history_cases.npz")) as d:
        return {k: d[k] for k in d.files}


def fixture_pool(g):
    from safelife_amd.levels import LevelPool
    levels = []
    for name in g["levels"]:
        levels += util.levels_from_trace(util.load_trace(str(name)))
    return LevelPool(levels, counts_fn=util.oracle_counts)


# ------------------------------------------------------------------------------------------------------------- the ABI

def test_symbols_and_version():
    lib = _hip.lib()
    for name in NAMES:
        assert name in _hip.EXPORTS and hasattr(lib, name)
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13


def test_layouts_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "safelife_hip.h"', 'int main(void) {',
             'printf("consts %d %d %d %d %d %d %d %d %d\\n", SL_HIST_LIVE, SL_HIST_NO_FINAL, SL_HIST_SLOT_FREE, '
             'SL_HIST_SLOT_ENV, SL_HIST_SLOT_ENTRY, SL_HIST_MAX_WATCH, SL_HIST_MAX_SLOTS, SL_HIST_COUNTERS, '
             'SL_HIST_ORDER_WORDS);',
             'printf("sizes %zu %zu\\n", sizeof(sl_episode_history), sizeof(sl_history_entry));']
    want = ["consts %d %d %d %d %d %d %d %d %d" % (_hip.HIST_LIVE, _hip.HIST_NO_FINAL, _hip.HIST_SLOT_FREE, _hip.HIST_SLOT_ENV,
                                                   _hip.HIST_SLOT_ENTRY, _hip.HIST_MAX_WATCH, _hip.HIST_MAX_SLOTS,
                                                   len(_hip.HIST_COUNTERS), _hip.HIST_ORDER_WORDS),
            "sizes %d %d" % (C.sizeof(_hip.EpisodeHistory), episode_history.ENTRY_DTYPE.itemsize)]
    for name, ctype in _hip.EpisodeHistory._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(sl_episode_history, %s));' % (name, name))
        want.append("%s %d" % (name, getattr(_hip.EpisodeHistory, name).offset))
    for name in episode_history.ENTRY_DTYPE.names:
        lines.append('printf("%s %%zu\\n", offsetof(sl_history_entry, %s));' % (name, name))
        want.append("%s %d" % (name, episode_history.ENTRY_DTYPE.fields[name][1]))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(util.REPO, "include"), str(src), "-o", exe])
    got = [g for g in subprocess.check_output([exe]).decode().split("\n") if g]
    assert got == want
    assert (C.sizeof(_hip.EpisodeHistory), episode_history.ENTRY_DTYPE.itemsize) == (112, 32)
    assert episode_history.ENTRY_DTYPE == hr.ENTRY_DTYPE
    assert (hr.LIVE, hr.NO_FINAL, hr.FREE, hr.ENV, hr.ENTRY) == (_hip.HIST_LIVE, _hip.HIST_NO_FINAL, _hip.HIST_SLOT_FREE,
                                                                 _hip.HIST_SLOT_ENV, _hip.HIST_SLOT_ENTRY)


def _description(**kw):
    """A description whose pointers are non-null but never dereferenced: every call below is refused first."""
    s = _hip.EpisodeHistory()
    s.B, s.n_watch, s.n_slots, s.T, s.H, s.W, s.interval = 8, 3, 4, 10, 5, 5, 1
    for name, ctype in _hip.EpisodeHistory._fields_:
        if ctype is C.c_void_p:
            setattr(s, name, 0x1000)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_bad_descriptions_are_refused_before_any_launch():
    lib, p = _hip.lib(), C.c_void_p(0x1000)

    def both(s):
        return (lib.slhip_history_capture(s, p, p, p, p, None, None, None), lib.slhip_history_rewind(s, p, p, None, None))

    for bad in (dict(B=0), dict(n_watch=0), dict(n_watch=9), dict(B=2000, n_watch=1025), dict(n_slots=0), dict(n_slots=1025),
                dict(T=0), dict(interval=0), dict(H=2), dict(W=2), dict(H=129, W=128)):
        assert both(C.byref(_description(**bad))) == (_hip.SL_E_SHAPE,) * 2, bad
        assert b"history" in lib.slhip_last_error()
    for name, ctype in _hip.EpisodeHistory._fields_:
        if ctype is C.c_void_p:
            assert both(C.byref(_description(**{name: None}))) == (_hip.SL_E_ARG,) * 2, name
    assert both(None) == (_hip.SL_E_ARG,) * 2
    ok = C.byref(_description())
    for k in range(1, 5):
        args = [ok, p, p, p, p, None, None, None]
        args[k] = None
        assert lib.slhip_history_capture(*args) == _hip.SL_E_ARG
    assert lib.slhip_history_rewind(ok, None, p, None, None) == lib.slhip_history_rewind(ok, p, None, None, None) == _hip.SL_E_ARG
    q = _hip.EpisodeQueue()
    q.capacity, q.count, q.records = 4, 0x1000, 0x1000                  # (a queue with slots and no boards)
    assert lib.slhip_history_capture(ok, p, p, p, p, C.byref(q), None, None) == _hip.SL_E_ARG


# ------------------------------------------------------------------------------------- the restatement against the reference

def test_the_fixture_is_what_the_issue_asks_for(golden):
    g = golden
    assert sorted(int(g[str(r) + "_interval"]) for r in g["runs"]) == [1, 3]
    for r in map(str, g["runs"]):
        assert g[r + "_actions"].shape[1] == 5 and 6 <= int(g[r + "_time_limit"]) <= 12
        n = len(g[r + "_length"])
        assert 20 <= n <= 26 and len(set(g[r + "_length"].tolist())) >= 3       # the envs drift apart
        assert g[r + "_kept"].tolist() == [i for i in range(n) if i % int(g[r + "_interval"]) == 0]
        for i in g[r + "_kept"]:
            assert g["%s_board_%d" % (r, i)].shape == g["%s_goals_%d" % (r, i)].shape == (g[r + "_length"][i], 7, 7)
    assert os.path.getsize(os.path.join(util.REPO, "tests", "golden", "episode_history_cases.npz")) < 300 * 1024


def drive_fixture(g, r, pool, slots=40):
    d = hr.OracleDrive(pool, 5, int(g[r + "_time_limit"]), np.arange(5), slots, int(g[r + "_interval"]),
                       episode_streams=False)
    for a in g[r + "_actions"]:
        d.step(a)
    return d


@pytest.mark.parametrize("r", ["interval1", "interval3"])
def test_the_restatement_reproduces_what_the_reference_saved(golden, r):
    g = golden
    d = drive_fixture(g, r, fixture_pool(g))
    listing = d.model.listing()
    assert listing["row"].tolist() == g[r + "_kept"].tolist()
    assert d.model.episodes == len(g[r + "_length"]) and d.model.missed == d.model.incomplete == 0
    assert d.model.kept == len(listing)
    frames = 0
    for en in listing:
        i = int(en["row"])
        assert (en["env"], en["length"], en["level"]) == (g[r + "_env"][i], g[r + "_length"][i], g[r + "_level"][i])
        h = d.model.history(en)
        want = g["%s_board_%d" % (r, i)]
        assert np.array_equal(h["goals"], g["%s_goals_%d" % (r, i)])
        assert np.array_equal(h["board"][-1], want[-1])                  # the board as the agent left it
        assert np.array_equal(hr.as_the_reference_saved(h["board"], d.next_actions(en)), want)
        frames += len(want)
    assert frames >= 40


def test_an_in_step_reload_leaves_what_the_drive_s_reload_leaves(golden):
    """The oracle with auto_reset against the drive's own way -- no auto-reset, the finished envs reset behind the step."""
    g, r = golden, "interval3"
    pool = fixture_pool(g)
    d = hr.OracleDrive(pool, 5, int(g[r + "_time_limit"]), np.arange(5), 8, 3, episode_streams=False)
    auto = util.OracleBackend(pool, 5, first_level=np.arange(5) % len(pool), auto_reset=True,
                              time_limit=int(g[r + "_time_limit"]), episode_streams=False)
    auto.reset()
    for a in g[r + "_actions"]:
        out = d.step(a)
        auto.step(a)
        assert np.array_equal(out["done"], auto.arrays["done"])
        for name in ("board", "goals", "level_idx", "episode_idx", "episode_length", "agent_loc"):
            assert np.array_equal(d.A[name], auto.arrays[name]), name


@pytest.mark.parametrize("name", ["ex_color_test", "ex_containment", "ex_sokuban", "worked_7x7_exit", "worked_7x7_noop"])
def test_the_first_episode_on_a_trace_level_is_the_trace(name):
    tr = util.load_trace(name)
    pool = util.pool_from_trace(tr, util.oracle_counts)
    kw = util.env_kwargs_from_trace(tr)
    T = kw.pop("time_limit")
    d = hr.OracleDrive(pool, 1, T, [0], 2, 1, episode_streams=False, **kw)
    first_end = int(np.flatnonzero(tr["trace_done"])[0])
    for a in tr["trace_actions"][:first_end + 1]:
        d.step([a])
    listing = d.model.listing()
    assert len(listing) == 1 and listing[0]["length"] == tr["trace_ep_length"][first_end] == first_end + 1
    h = d.model.history(listing[0])
    assert np.array_equal(h["board"], tr["trace_board"][:first_end + 1])
    assert np.array_equal(h["goals"], tr["trace_goals"][:first_end + 1])


# --------------------------------------------------------------------------------------------- the bookkeeping, by hand

H = W = 3


class Script(object):
    """Synthetic envs for the model: env e's board after its step is filled with 1000 * e + step; an env ends an episode on
    the steps its script names."""

    def __init__(self, B, watch, slots, interval=1, T=6, queue_capacity=100):
        self.B, self.m = B, hr.HistoryModel(B, watch, slots, T, H, W, interval)
        self.level, self.episode, self.length = np.arange(B) % 4, np.zeros(B, np.int64), np.zeros(B, np.int64)
        self.goals = np.stack([np.full((H, W), 7 + e, np.uint16) for e in range(B)])
        self.queue, self.pushed, self.capacity, self.t = [], 0, queue_capacity, 0
        self.m.rewind(self.goals, self.level, self.episode)

    def boards(self):
        return np.stack([np.full((H, W), 1000 * e + self.t, np.uint16) for e in range(self.B)])

    def step(self, ends=()):
        self.t += 1
        self.length += 1
        board = self.boards()
        out = dict(done=np.zeros(self.B, np.uint8), success=np.zeros(self.B, np.uint8), times_up=np.ones(self.B, np.uint8),
                   episode_length=self.length.copy())
        for e in sorted(ends):
            out["done"][e] = 1
            self.pushed += 1
            if len(self.queue) < self.capacity:
                self.queue.append((e, int(self.episode[e]), board[e] + 500))     # the board as the agent left it
            self.level[e], self.episode[e], self.length[e] = (self.level[e] + 1) % 4, self.episode[e] + 1, 0
            self.goals[e] += 100
        q = (self.pushed, [e for e, _, _ in self.queue], [k for _, k, _ in self.queue], [b for _, _, b in self.queue])
        self.m.capture(board, self.goals, self.level, self.episode, self.length, out, q)

    def reset(self, mask):
        for e in np.flatnonzero(mask):
            self.level[e], self.episode[e], self.length[e] = (self.level[e] + 1) % 4, self.episode[e] + 1, 0
            self.goals[e] += 100
        self.m.rewind(self.goals, self.level, self.episode, mask)


def test_exhaustion_release_and_pick_up_at_the_next_episode_start():
    s = Script(4, [0, 1, 2], slots=3)
    m = s.m
    assert m.owner.tolist() == [0, 1, 2] and m.slot_state.tolist() == [hr.ENV] * 3         # attach: ascending
    s.step()
    s.step(ends=[1])                                    # env 1's episode is kept: slot 1 goes to the entry, none is free
    assert m.owner.tolist() == [0, -1, 2] and m.slot_state.tolist() == [hr.ENV, hr.ENTRY, hr.ENV]
    assert (m.kept, m.missed) == (1, 0)
    en = m.listing()[0]
    assert (en["row"], en["env"], en["level"], en["episode_idx"], en["length"], en["slot"]) == (0, 1, 1, 0, 2, 1)
    h = m.history(en)
    assert h["board"][:, 0, 0].tolist() == [1001, 1502] and (h["goals"] == 8).all()
    s.step()
    m.release([1])                                      # a slot is free again ...
    s.step()
    assert m.owner.tolist() == [0, -1, 2]               # ... but env 1 is in mid-episode: it does not take it
    s.step(ends=[1])                                    # its episode ends: kept by rule, no slot -> missed; the next one records
    assert (m.kept, m.missed) == (1, 1) and m.owner.tolist() == [0, 1, 2]
    s.step()
    s.step(ends=[1])
    en = m.listing()[-1]
    assert (en["row"], en["episode_idx"], en["length"]) == (2, 2, 2) and (m.goals[en["slot"]] == 208).all()
    assert m.history(en)["board"][:, 0, 0].tolist() == [1006, 1507]     # from its frame 0: not partial at the front


def test_two_envs_that_end_on_one_step_take_the_free_slots_in_ascending_order():
    s = Script(6, [1, 3, 4], slots=6)
    m = s.m
    assert m.owner.tolist() == [0, 1, 2]
    s.step()
    s.step(ends=[0, 3, 4])                              # env 0 is not watched, but it counts: numbers 0, 1, 2
    assert m.listing()["row"].tolist() == [1, 2] and m.listing()["env"].tolist() == [3, 4]
    assert m.owner.tolist() == [0, 3, 4] and m.episodes == 3             # lowest free slot to the lower env
    m.release([1])
    s.step(ends=[1, 4])                                 # env 1 gives slot 0 up and takes 1; env 4 gives 4 up and takes 5
    assert m.owner.tolist() == [1, 3, 5] and m.listing()["slot"].tolist() == [2, 0, 4]


def test_the_interval_rule_counts_every_env():
    s = Script(5, [2], slots=4, interval=3)
    for ends in ([0, 1], [2], [3], [2, 4], [2], [0, 1, 2]):
        s.step(ends=ends)
    # numbers: step 1 -> 0 1; step 2 -> env 2 is 2; step 3 -> 3; step 4 -> env 2 is 4; step 5 -> env 2 is 6; step 6 -> 7 8 9
    assert s.m.listing()["row"].tolist() == [6, 9] and s.m.episodes == 10
    assert s.m.owner.tolist() == [2] and s.m.slot_state.tolist() == [hr.ENTRY, hr.ENTRY, hr.ENV, hr.FREE]


def test_a_reset_in_mid_episode_restarts_at_frame_zero():
    s = Script(3, [0, 2], slots=3)
    m = s.m
    s.step(), s.step()
    s.reset(np.array([0, 0, 1]))                        # env 2 is reloaded: new level, new goals, frame 0 again; nothing is kept
    assert (m.kept, m.episodes) == (0, 0) and m.owner.tolist() == [0, 1] and (m.goals[1] == 109).all()
    assert m.cur_level.tolist() == [0, 3] and m.cur_episode.tolist() == [0, 1]
    s.step(), s.step(ends=[0, 2])
    a, b = m.listing()
    assert (a["length"], b["length"], b["level"], b["episode_idx"]) == (4, 2, 3, 1)
    assert m.history(b)["board"][:, 0, 0].tolist() == [2003, 2504]


def test_an_overflowed_queue_gives_no_final():
    s = Script(3, [0, 1, 2], slots=6, queue_capacity=2)
    s.step()
    s.step(ends=[0, 1, 2])                              # the queue holds envs 0 and 1 only
    m = s.m
    assert m.listing()["flags"].tolist() == [hr.LIVE, hr.LIVE, hr.LIVE | hr.NO_FINAL] and m.incomplete == 1
    assert len(m.history(m.listing()[2])["board"]) == 1 and len(m.history(m.listing()[0])["board"]) == 2
    assert m.cursor == 2
    s.step(), s.step(ends=[1])                          # the queue stays full: every later history lacks its last frame
    assert m.listing()[3]["flags"] == hr.LIVE | hr.NO_FINAL and m.incomplete == 2


# ------------------------------------------------------------------------------------------------------------- the checks

@pytest.fixture(scope="module")
def pool():
    return util.pool_from_fixture("prune_still_25", util.oracle_counts, n=4)[0]


def test_constructor_checks(pool):
    from safelife_amd.levels import LevelPool
    h = episode_history.EpisodeHistory(pool, 8, [5, 1, 3], 4, interval=2)
    assert h.watch.tolist() == [1, 3, 5] and h.slot_bytes(10) == 4 * 11 * 25 * 25 * 2
    for bad in (dict(watch=[1, 1]), dict(watch=[]), dict(watch=[8]), dict(watch=[-1]), dict(slots=0), dict(slots=1025),
                dict(interval=0), dict(num_envs=0)):
        kw = dict(dict(num_envs=8, watch=[1], slots=2), **bad)
        with pytest.raises(ValueError):
            episode_history.EpisodeHistory(pool, kw.pop("num_envs"), kw.pop("watch"), kw.pop("slots"), **kw)
    with pytest.raises(TypeError):
        episode_history.EpisodeHistory(object(), 8, [0], 2)
    with pytest.raises(ValueError, match="refreshable"):
        episode_history.EpisodeHistory(LevelPool(list(pool.levels), counts_fn=util.oracle_counts, refreshable=True), 8, [0], 2)
    multi = []
    for name in ("multi_asym1", "multi_build_coop"):
        multi += util.levels_from_trace(util.load_trace(name))
    with pytest.raises(ValueError, match="multi-agent histories are out of scope"):
        episode_history.EpisodeHistory(LevelPool(multi, counts_fn=util.oracle_counts, n_agents=2), 8, [0], 2)
    with pytest.raises(ValueError, match="no device state"):
        h.counters()


def test_an_env_it_cannot_serve_is_refused_before_anything_is_allocated(pool):
    """These refusals come in front of the first device call: no device is needed to meet them."""
    from safelife_amd.vector_env import SafeLifeVectorEnv
    h = episode_history.EpisodeHistory(pool, 8, [0, 1], 4, max_bytes=100000)
    queue = dict(capacity=16)
    with pytest.raises(ValueError, match="finished-episode queue"):
        h._check_env(pool, 8, 10, None, None, None)
    with pytest.raises(ValueError, match="built for 8 envs"):
        h._check_env(pool, 9, 10, queue, None, None)
    with pytest.raises(ValueError, match="another pool"):
        h._check_env(util.pool_from_fixture("prune_still_25", util.oracle_counts, n=4)[0], 8, 10, queue, None, None)
    with pytest.raises(ValueError, match=r"need %d bytes.*max_bytes allows 100000" % (4 * 101 * 625 * 2)):
        h._check_env(pool, 8, 100, queue, None, None)
    # the sliced and queue steppers and rollout(): nothing would copy the frames
    stub = types.SimpleNamespace(level_schedule=None, episode_log=None, episode_run=None, episode_history=h)
    for what in ("step_async()", "step_slice()", "step_queues()", "queues_open()", "rollout()", "set_step_outputs()"):
        with pytest.raises(ValueError, match="cannot drive an episode history.*nothing would copy the frames"):
            SafeLifeVectorEnv._no_schedule(stub, what, "why", "why")
