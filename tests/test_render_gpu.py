"""
Rendering on the device (csrc/sl_render.hip through slhip_render_boards / slhip_env_render): every byte against the
frames the reference drew (tests/golden/render_cases.npz, render_table.npz) and against the host numpy path.
"""
import types

import numpy as np
import pytest

from tests import util
from tests.test_render_host import CASES, SHEETS

pytestmark = pytest.mark.gpu


def _device_counts(boards, goals):
    from safelife_amd.levels import _device_counts as f
    return f(boards, goals)


def _dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to("cuda")


#: the 20 tile cases of the fixture: 13 named types, empty, empty with other bits, the agent four ways, unknown
TILE_CASES = [9, 1, 53, 32789, 17, 32884, 48, 16, 32788, 85, 152, 272, 144, 0, 1 << 12] + [122 | (o << 12) for o in range(4)] + [64]

_sheets = {}


def _sheet(name):
    if name not in _sheets:
        _sheets[name] = _dev(SHEETS[name], np.float32)
    return _sheets[name]


def device_render(case, out=None):
    from safelife_amd import render
    kw = {}
    if "index" in case:
        kw["index"] = _dev(case["index"], np.int32)
    if "orientation" in case:
        kw["orientation"] = _dev(case["orientation"], np.int32)
    if "view" in case:
        kw.update(view_size=tuple(int(v) for v in case["view"]), centers=_dev(case["centers"], np.int32),
                  exits=_dev(case["exits"], np.int32))
    return render.render_batch(_dev(case["board"]), _dev(case["goals"]), _sheet(str(case["sheet"])), out=out, **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_reproduces_reference(name):
    case = CASES[name]
    got = device_render(case).cpu().numpy()
    assert got.shape == case["out"].shape
    assert np.array_equal(got, case["out"]), "%d bytes differ" % int(np.sum(got != case["out"]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_unaligned_out(name):
    """`out` 4 bytes past a 16-byte boundary: the dword-store path."""
    import torch
    case = CASES[name]
    n = case["out"].size
    buf = torch.full((n + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[4:4 + n].view(case["out"].shape)
    device_render(case, out=out)
    host = buf.cpu().numpy()
    assert np.array_equal(host[4:4 + n].reshape(case["out"].shape), case["out"])
    assert np.all(host[:4] == 0xA5) and np.all(host[4 + n:] == 0xA5)


def test_random_shapes_against_host_path():
    """About 200 seeded draws beyond the fixture: H, W in 3..12, N in 1..7, whole boards and views, every byte equal."""
    from safelife_amd import render
    rng = np.random.default_rng(7)
    sheet, d_sheet = SHEETS["synth"], _sheet("synth")
    for draw in range(200):
        N, H, W = int(rng.integers(1, 8)), int(rng.integers(3, 13)), int(rng.integers(3, 13))
        board = np.array(TILE_CASES, np.uint16)[rng.integers(0, 20, (N, H, W))] | (rng.integers(0, 8, (N, H, W)).astype(np.uint16) << 9)
        goals = rng.integers(0, 8, (N, H, W)).astype(np.uint16) << 9
        if draw % 2 == 0:
            got = render.render_batch(_dev(board), _dev(goals), d_sheet).cpu().numpy()
            want = render.render_board_host(board, goals, None, sheet)
        else:
            vh, vw = int(rng.integers(1, 15)), int(rng.integers(1, 15))
            centers = np.stack([rng.integers(0, H, N), rng.integers(0, W, N)], axis=1).astype(np.int32)
            centers[rng.random(N) < 0.2] = -1
            exits = rng.integers(-1, H * W, (N, 3)).astype(np.int32)
            got = render.render_batch(_dev(board), _dev(goals), d_sheet, view_size=(vh, vw), centers=_dev(centers),
                                      exits=_dev(exits)).cpu().numpy()
            want = []
            for n in range(N):
                e = exits[n][exits[n] >= 0]
                game = types.SimpleNamespace(board=board[n], goals=goals[n], exit_locs=(e // W, e % W),
                                             agent_locs=np.array([centers[n]] if centers[n][0] >= 0 else []).reshape(-1, 2))
                want.append(render.render_game_host(game, (vh, vw), sheet))
            want = np.stack(want)
        assert np.array_equal(got, want), (draw, N, H, W)


@pytest.mark.parametrize("shape", [(1, 3, 3), (3, 3, 3), (1, 5, 7)])
def test_bounds(shape):
    """Render into the middle of a buffer of 0xA5: nothing before or after the frames is written, for byte counts that
    are no multiple of 16 (N * vh * vw no multiple of 4)."""
    import torch
    from safelife_amd import render
    N, H, W = shape
    assert (N * H * W) % 4 != 0
    rng = np.random.default_rng(3)
    board = rng.integers(0, 2, shape).astype(np.uint16) * 9
    goals = np.zeros(shape, np.uint16)
    n = N * H * W * 588
    for lead in (64, 68):
        buf = torch.full((n + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        out = buf[lead:lead + n].view(N, H * 14, W * 14, 3)
        render.render_batch(_dev(board), _dev(goals), _sheet("real"), out=out)
        host = buf.cpu().numpy()
        assert np.all(host[:lead] == 0xA5) and np.all(host[lead + n:] == 0xA5)
        assert np.array_equal(host[lead:lead + n].reshape(out.shape), render.render_board_host(board, goals))


def test_argument_errors():
    import ctypes as C
    from safelife_amd import _hip
    lib = _hip.lib()
    a = _hip.RenderArgs()
    assert lib.slhip_render_boards(None, None) == _hip.SL_E_ARG
    assert lib.slhip_render_boards(C.byref(a), None) == _hip.SL_E_ARG          # N <= 0
    case = CASES["shape_2x4x6"]
    b, g, s = _dev(case["board"]), _dev(case["goals"]), _sheet("synth")
    import torch
    out = torch.empty(case["out"].shape, dtype=torch.uint8, device="cuda")
    a.N, a.H, a.W, a.n_source = 2, 4, 6, 2
    a.board_stride = a.goal_stride = 24
    a.board, a.goals, a.sprites = b.data_ptr(), g.data_ptr(), s.data_ptr()
    assert lib.slhip_render_boards(C.byref(a), None) == _hip.SL_E_ARG          # null out
    assert b"null" in lib.slhip_last_error()
    a.out = out.data_ptr()
    a.view_h, a.view_w = 3, 0
    assert lib.slhip_render_boards(C.byref(a), None) == _hip.SL_E_ARG          # a view with one side 0
    a.view_h = a.view_w = 0
    assert lib.slhip_render_boards(C.byref(a), _hip.current_stream_ptr()) == 0
    assert np.array_equal(out.cpu().numpy(), case["out"])


def _host_frames(board, goals, locs, exit_locs, ids, view):
    from safelife_amd import render
    frames = []
    for e in ids:
        ex = exit_locs[e][exit_locs[e] >= 0]
        W = board.shape[-1]
        loc = locs[e]
        game = types.SimpleNamespace(board=board[e], goals=goals[e], exit_locs=(ex // W, ex % W),
                                     agent_locs=np.array([loc] if loc[0] >= 0 else []).reshape(-1, 2))
        frames.append(render.render_game_host(game, view))
    return np.stack(frames)


def test_vector_env_render():
    import torch
    from safelife_amd._hip import SafeLifeHipError
    from safelife_amd.vector_env import SafeLifeVectorEnv
    pool, _ = util.pool_from_fixture("prune_still_25", _device_counts, n=8, min_performance_fraction=0.05)
    B = 6
    env = SafeLifeVectorEnv(pool, B, first_level=np.arange(B), auto_reset=True, time_limit=50)
    env.reset()
    rng = np.random.default_rng(5)

    def check():
        board, goals = env.numpy("board"), env.numpy("goals")
        locs, exits = env.numpy("agent_loc"), env.numpy("exit_locs")
        for view in (None, (15, 15)):
            got = env.render(view_size=view)
            assert got.dtype == torch.uint8 and got.is_cuda
            assert np.array_equal(got.cpu().numpy(), _host_frames(board, goals, locs, exits, range(B), view))
            got = env.render(env_ids=[4, 1, 1], view_size=view)
            assert np.array_equal(got.cpu().numpy(), _host_frames(board, goals, locs, exits, [4, 1, 1], view))

    for t in range(12):
        env.step(rng.integers(0, 9, B).astype(np.int32))
    check()
    before = env.numpy("board").copy()
    try:
        env.queues_open(1)
        queued = True
    except SafeLifeHipError:
        queued = False                      # (no queues on this runtime: the same steps through step())
    for t in range(12):
        acts = torch.from_numpy(rng.integers(1, 9, B).astype(np.int32)).to(env.device)
        if queued:
            if t == 0:
                torch.cuda.synchronize()
            env.step_queues(acts)
        else:
            env.step(acts)
    # render() right behind the queued steps must show the stepped boards: it settles the queues as get_obs() does
    frames = env.render().cpu().numpy()
    assert not np.array_equal(env.numpy("board"), before)
    assert np.array_equal(frames, _host_frames(env.numpy("board"), env.numpy("goals"), env.numpy("agent_loc"),
                                               env.numpy("exit_locs"), range(B), None))
    check()
    if queued:
        env.queues_close()


def test_multi_agent_env_render():
    from safelife_amd.levels import LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    levels = util.levels_from_trace(util.load_trace("multi_asym1"))
    pool = LevelPool(levels, counts_fn=_device_counts, n_agents=2, min_performance_fraction=0.1)
    B = 4
    env = SafeLifeMultiAgentVectorEnv(pool, B, first_level=np.arange(B) % len(levels), auto_reset=True, time_limit=50)
    env.reset()
    rng = np.random.default_rng(6)
    for t in range(12):
        env.step(rng.integers(0, 9, (B, 2)).astype(np.int32))
    board, goals = env.numpy("board"), env.numpy("goals")
    locs, exits = env.numpy("agent_locs")[:, 0], env.numpy("exit_locs")
    for view in (None, (15, 15)):
        for ids in (None, [3, 0, 0]):
            got = env.render(env_ids=ids, view_size=view).cpu().numpy()
            assert np.array_equal(got, _host_frames(board, goals, locs, exits, range(B) if ids is None else ids, view))
