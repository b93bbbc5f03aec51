"""
Drop-in counterpart of the reference's native module ``safelife.speedups``
(safelife/speedups_src/module.c:515-556) for the step hot path, running on
MI355X through ``libsafelife_hip.so``.

Same function names, argument meaning, dtypes and error behaviour as the
reference's Python-level functions:

* ``advance_board(board, spawn_prob=0.3, n_step=1)``         module.c:20-49
* ``life_occupancy(board, spawn_prob=0.3, n_step=1000)``     module.c:52-81
* ``alive_counts(board, goals)``                             module.c:99-132
* ``execute_actions(board, locations, actions)``             module.c:155-202
* ``set_bit_generator(bitgen)`` / ``seed(n)``                random.c:25-74

plus ``*_batch`` variants that take device tensors ``[B,H,W]`` and never leave
HBM.  Host arrays are staged through torch tensors (buffer holders only).

Random numbers: the reference draws from one process-global numpy
BitGenerator.  Here the generator's PCG64 state is copied to the device, the
kernel consumes draws in the reference's order, and the advanced state is
written back into the generator, so results *and* generator state afterwards
are identical to the reference.  Only PCG64 (numpy's default) is supported.

* ``_render_board(board, goals, sprites)``                    module.c:438-512

* ``gen_pattern(board, mask, period, seeds=None, ...)``       module.c:252-417

``gen_pattern`` is the level generator's Metropolis sampler (gen_board.c:316-510); ``gen_pattern_batch`` runs N
independent problems of one (H, W, period) in one launch, one wavefront per chain.  It draws 32-bit integers as well as
doubles, and numpy buffers the unused half of a 32-bit draw in the generator (``has_uint32`` / ``uinteger``), so this
function carries SIX words per generator (``pcg64_words6`` / ``pcg64_set_words6``) where the others carry four.  With
them the board, the exception and the generator's state afterwards equal the reference's, bit for bit.  It also provides
the reference's exceptions: ``BoardGenException`` and, derived from it, ``MaxIterException``,
``BadProbabilityException``, ``InsufficientAreaException``.

``partition_batch(words, shape, min_regions, max_regions)`` is the level generator's region partition
(``proc_gen.partition``, this project's own) for N generators in one launch, one wavefront per partition, bit-equal to the
host function: labels and the six words afterwards.

Not provided: wrapped_label (generation never calls it; only stability_mask does).
"""
import ctypes as C

import numpy as np

from . import _hip

NEW_CELL_MASK = 1          # module.c:580-582 (only procgen uses them)
CAN_OSCILLATE_MASK = 2
INCLUDE_VIOLATIONS_MASK = 4

_MASK64 = (1 << 64) - 1


class BoardShapeError(ValueError, SystemError):
    """Raised where the reference returns NULL without an exception (module.c:32-35), which
    CPython reports as SystemError; also a ValueError for callers that expect one."""


# --------------------------------------------------------------------------- RNG bridge

_bit_generator = None


def set_bit_generator(bitgen):
    """Use `bitgen` (an object with the numpy BitGenerator interface) for all further draws.

    Mirrors random.c:25-39; the generator is process-global exactly as in the reference.
    """
    global _bit_generator
    if not hasattr(bitgen, "capsule"):
        raise AttributeError("'%s' object has no attribute 'capsule'" % type(bitgen).__name__)
    _bit_generator = bitgen


def seed(n=0):
    """random.c:41-74: install ``numpy.random.default_rng(n)`` (n == 0: OS entropy)."""
    global _bit_generator
    gen = np.random.default_rng(int(n)) if n else np.random.default_rng()
    _bit_generator = gen.bit_generator


def _current_bitgen():
    if _bit_generator is None:
        seed(0)                      # random.c:76-81
    return _bit_generator


def pcg64_words(bitgen):
    """numpy PCG64 state -> uint64[4] (state_hi, state_lo, inc_hi, inc_lo)."""
    st = bitgen.state
    if st.get("bit_generator") != "PCG64":
        raise TypeError(
            "safelife_amd.speedups supports numpy's PCG64 bit generator only (got %r); the device "
            "kernels restate PCG64's recurrence to stay stream-identical with the reference"
            % (st.get("bit_generator"),))
    s, i = st["state"]["state"], st["state"]["inc"]
    return np.array([s >> 64, s & _MASK64, i >> 64, i & _MASK64], dtype=np.uint64)


def pcg64_set_words(bitgen, words):
    st = bitgen.state
    w = [int(x) for x in words]
    st["state"]["state"] = (w[0] << 64) | w[1]
    st["state"]["inc"] = (w[2] << 64) | w[3]
    bitgen.state = st


def pcg64_words6(bitgen):
    """numpy PCG64 state -> uint64[6]: ``pcg64_words`` and the buffered half of a 32-bit draw (has_uint32, uinteger)."""
    st = bitgen.state
    return np.concatenate([pcg64_words(bitgen), np.array([st["has_uint32"], st["uinteger"]], dtype=np.uint64)])


def pcg64_set_words6(bitgen, words):
    w = [int(x) for x in words]
    pcg64_set_words(bitgen, w[:4])
    st = bitgen.state
    st["has_uint32"], st["uinteger"] = w[4], w[5]
    bitgen.state = st


# --------------------------------------------------------------------------- staging helpers

def _torch():
    import torch
    return torch


def _to_device(arr, np_dtype):
    """Host ndarray -> device tensor holding the same bytes (uint16/uint64 travel as int16/int64)."""
    torch = _torch()
    a = np.ascontiguousarray(arr, dtype=np_dtype)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint64): np.int64}.get(a.dtype)
    if view is not None:
        a = a.view(view)
    return torch.from_numpy(a).to(_hip.device(), non_blocking=False)


def _to_host(t, np_dtype):
    a = t.cpu().numpy()
    return a.view(np_dtype) if a.dtype != np.dtype(np_dtype) else a


def _coerce_board(board):
    """module.c:28-35: force-cast to C-contiguous uint16, must be 2-d and non-empty."""
    b = np.ascontiguousarray(np.asarray(board).astype(np.uint16, copy=False))
    if b.ndim != 2 or b.size == 0:
        raise BoardShapeError("board must be a non-empty 2-dimensional array")
    return b


# --------------------------------------------------------------------------- batched (device) API

def advance_board_batch(boards, spawn_prob, rng, n_step=1, out=None):
    """boards: int16/uint16 tensor [B,H,W] on the device; spawn_prob: float32 [B];
    rng: int64 [B,4] PCG64 words, advanced in place; n_step: int, or an int32 tensor [B] of per-board
    step counts.  Returns `out` (may be `boards`)."""
    torch = _torch()
    B, H, W = boards.shape
    if out is None:
        out = torch.empty_like(boards)
    if isinstance(n_step, torch.Tensor):        # one step count per board: int32 [B] on the device
        n = n_step.to(device=boards.device, dtype=torch.int32).contiguous()
        if tuple(n.shape) != (B,):
            raise ValueError("n_step tensor must have shape [B]")
        rc = _hip.lib().slhip_advance_board_each(_hip.ptr(boards), _hip.ptr(out), B, H, W, _hip.ptr(spawn_prob),
                                                 _hip.ptr(n), _hip.ptr(rng), _hip.current_stream_ptr())
    else:
        rc = _hip.lib().slhip_advance_board(_hip.ptr(boards), _hip.ptr(out), B, H, W, _hip.ptr(spawn_prob),
                                            int(n_step), _hip.ptr(rng), _hip.current_stream_ptr())
    _hip.check(rc, "Board must be at least 3x3.")
    return out


def life_occupancy_batch(boards, spawn_prob, rng, n_step=1000, out=None):
    """int32 [B,H,W,8] occupancy counts of `n_step` steps per board (advance_board.c:153-189); `rng` advanced in place.
    ``out``: a caller-owned int32 tensor [B,H,W,8] to write into (every element is written) instead of a new one --
    at 4096 boards of 64x64 the result is 537 MB, and a fresh allocation of that size is not free."""
    torch = _torch()
    B, H, W = boards.shape
    if out is None:
        counts = torch.empty((B, H, W, 8), dtype=torch.int32, device=boards.device)
    else:
        counts = out
        if (counts.dtype != torch.int32 or tuple(counts.shape) != (B, H, W, 8) or not counts.is_contiguous()
                or counts.device != boards.device):
            raise ValueError("out must be a contiguous int32 tensor [B,H,W,8] on the boards' device")
    rc = _hip.lib().slhip_life_occupancy(_hip.ptr(boards), _hip.ptr(counts), B, H, W, _hip.ptr(spawn_prob),
                                         int(n_step), _hip.ptr(rng), _hip.current_stream_ptr())
    _hip.check(rc, "Board must be at least 3x3.")
    return counts


def alive_counts_batch(boards, goals):
    torch = _torch()
    if boards.shape != goals.shape:
        raise ValueError("Board and goals must have same size.")
    B = boards.shape[0]
    hw = boards[0].numel() if B else 0
    out = torch.empty((B, 8, 9), dtype=torch.int64, device=boards.device)
    rc = _hip.lib().slhip_alive_counts(_hip.ptr(boards), _hip.ptr(goals), B, hw, _hip.ptr(out),
                                       _hip.current_stream_ptr())
    _hip.check(rc)
    return out


def execute_actions_batch(boards, locs, actions):
    """In place.  boards [B,H,W]; locs int64 [B,A,2] (row, col); actions int64 [B,A] or [B,1]."""
    B, H, W = boards.shape
    A = locs.shape[1]
    if actions.shape[-1] == A and actions.dim() == 2:
        stride, bstride = 1, A
    elif actions.numel() == B:
        stride, bstride = 0, 1
    else:
        raise ValueError("Locations should be shape (n_agent, 2).")
    rc = _hip.lib().slhip_execute_actions(_hip.ptr(boards), B, H, W, _hip.ptr(locs), _hip.ptr(actions),
                                          A, stride, bstride, _hip.current_stream_ptr())
    _hip.check(rc, "Board must be at least 3x3.")


# --------------------------------------------------------------------------- reference-shaped API

def _run_with_global_rng(fn, board, spawn_prob):
    torch = _torch()
    bitgen = _current_bitgen()
    words = pcg64_words(bitgen)
    d_board = _to_device(board[None], np.uint16)
    d_rng = _to_device(words[None], np.uint64)
    d_p = torch.full((1,), float(np.float32(spawn_prob)), dtype=torch.float32, device=d_board.device)
    result = fn(d_board, d_p, d_rng)
    pcg64_set_words(bitgen, _to_host(d_rng, np.uint64)[0])
    return result


def advance_board(board, spawn_prob=0.3, n_step=1):
    """Advance `board` by `n_step` steps; returns a new uint16 array, input untouched."""
    b = _coerce_board(board)
    out = _run_with_global_rng(
        lambda d_b, d_p, d_rng: advance_board_batch(d_b, d_p, d_rng, n_step), b, spawn_prob)
    return _to_host(out, np.uint16)[0]


def life_occupancy(board, spawn_prob=0.3, n_step=1000):
    """int32 [H,W,8]: how often each cell held life of each colour over `n_step` steps."""
    b = _coerce_board(board)
    out = _run_with_global_rng(
        lambda d_b, d_p, d_rng: life_occupancy_batch(d_b, d_p, d_rng, n_step), b, spawn_prob)
    return _to_host(out, np.int32)[0]


def alive_counts(board, goals):
    """int64 [8,9]: rows = goal colour, columns = cell colour (k r g y b m c w) + empty."""
    b = np.ascontiguousarray(np.asarray(board).astype(np.uint16, copy=False))
    g = np.ascontiguousarray(np.asarray(goals).astype(np.uint16, copy=False))
    if b.size != g.size:
        raise ValueError("Board and goals must have same size.")
    out = alive_counts_batch(_to_device(b.reshape(1, -1), np.uint16), _to_device(g.reshape(1, -1), np.uint16))
    return _to_host(out, np.int64)[0]


def execute_actions(board, locations, actions):
    """Perform an action for each agent, in order; `board` and `locations` are updated in place."""
    if not isinstance(board, np.ndarray) or not isinstance(locations, np.ndarray):
        raise TypeError("board and locations must be numpy arrays (they are updated in place)")
    if board.ndim != 2:
        raise ValueError("Board should be 2-dimensional.")
    if board.shape[0] < 3 or board.shape[1] < 3:
        raise ValueError("Board must be at least 3x3.")
    acts = np.ascontiguousarray(np.asarray(actions), dtype=np.int64).reshape(-1)
    n_agents = locations.size // 2
    if acts.size != n_agents and acts.size != 1:
        raise ValueError("Locations should be shape (n_agent, 2).")
    if n_agents == 0:
        return None
    d_board = _to_device(board[None], np.uint16)
    d_locs = _to_device(locations.reshape(1, n_agents, 2), np.int64)
    d_acts = _to_device(acts.reshape(1, -1), np.int64)
    B, H, W = d_board.shape
    stride = 1 if acts.size == n_agents else 0
    rc = _hip.lib().slhip_execute_actions(_hip.ptr(d_board), 1, H, W, _hip.ptr(d_locs), _hip.ptr(d_acts),
                                          n_agents, stride, acts.size, _hip.current_stream_ptr())
    _hip.check(rc, "Board must be at least 3x3.")
    np.copyto(board, _to_host(d_board, np.uint16)[0], casting="unsafe")
    np.copyto(locations, _to_host(d_locs, np.int64)[0].reshape(locations.shape), casting="unsafe")
    return None


def _render_board(board, goals, sprites):
    """uint8 [..., H*14, W*14, 3] RGB frames of uint16 boards [..., H, W] over their goals; ``sprites``: the float32
    sheet, 70*70*4 values (module.c:438-512; safelife_amd.render has the arithmetic)."""
    from . import render
    b = np.ascontiguousarray(np.asarray(board).astype(np.uint16, copy=False))
    g = np.ascontiguousarray(np.asarray(goals).astype(np.uint16, copy=False))
    s = np.ascontiguousarray(np.asarray(sprites).astype(np.float32, copy=False))
    if b.ndim < 2:
        raise ValueError("Board must have at least two dimensions.")
    if b.size != g.size:
        raise ValueError("Board and goals must have same size.")
    if s.size != 70 * 70 * 4:
        raise ValueError("Sprites should have shape (70, 70, 4).")
    return render.render_board(b, g.reshape(b.shape), None, s)


# --------------------------------------------------------------------------- pattern generation

class BoardGenException(Exception):
    """module.c:580-581"""


class MaxIterException(BoardGenException):
    pass


class BadProbabilityException(BoardGenException):
    pass


class InsufficientAreaException(BoardGenException):
    pass


GEN_PATTERN_MAX_SIDE, GEN_PATTERN_MAX_PERIOD = _hip.GEN_PATTERN_MAX_SIDE, _hip.GEN_PATTERN_MAX_PERIOD


def _pair(value, name):
    try:
        a, b = value
        return float(a), float(b)
    except (TypeError, ValueError):
        raise TypeError("%s must be a pair of numbers: (penalty at density 0, penalty at density 1)" % name)


def gen_pattern_params(max_iter=40, min_fill=0.2, temperature=0.5, osc_bonus=0.3, alive=(0, 0), wall=(100, 100),
                       tree=(100, 100)):
    """The keywords of ``gen_pattern`` -> float64 [12] as slhip_gen_pattern_batch takes them: rel_max_iter, rel_min_fill,
    temperature, osc_bonus, then (intercept, slope) per cell type EMPTY, WALL, ALIVE, TREE.  A keyword is (penalty at
    density 0, penalty at density 1); module.c:316-325 files ``alive`` under type 2, ``wall`` under 1, ``tree`` under 3 and
    turns the second value into a slope."""
    out = [float(max_iter), float(min_fill), float(temperature), float(osc_bonus), 0.0, 0.0]
    for name, value in (("wall", wall), ("alive", alive), ("tree", tree)):
        at0, at1 = _pair(value, name)
        out += [at0, at1 - at0]
    return np.array(out, dtype=np.float64)


def _check_gen_range(H, W, period):
    if period <= 0:
        raise ValueError("Pattern period must be larger than 0.")
    if H < 3 or W < 3:
        raise ValueError("Board must be at least 3x3.")
    if H > GEN_PATTERN_MAX_SIDE or W > GEN_PATTERN_MAX_SIDE or period > GEN_PATTERN_MAX_PERIOD:
        raise ValueError("gen_pattern on the device supports boards from 3x3 to %dx%d and periods 1 to %d (got %dx%d, "
                         "period %d)" % (GEN_PATTERN_MAX_SIDE, GEN_PATTERN_MAX_SIDE, GEN_PATTERN_MAX_PERIOD, H, W, period))


def gen_pattern_batch(boards, masks, period, seeds=None, params=None, rng=None, out=None):
    """N independent ``gen_pattern`` problems of one shape and period in one launch.

    boards uint16 [N,H,W]; masks int32 [N,H,W]; seeds int32 [N,H,W] or None (the masks stand in); params float64 [N,12]
    (``gen_pattern_params``; None: the defaults for every problem); rng uint64 [N,6] (``pcg64_words6``), advanced IN
    PLACE.  All numpy arrays, or all torch tensors on the device (uint16 / uint64 travelling as int16 / int64).
    Returns (boards, status, iterations) of the same kind: the new boards -- the input board where status is not 0 --,
    status int32 [N] (0, -1 = max-iter, -4 = refused: max_iter * area * period does not fit an int) and the iterations
    run int32 [N].  Raises nothing per problem.  ``out`` (device tensors only): caller-owned contiguous (boards int16
    [N,H,W], status int32 [N], iterations int32 [N]) to write into."""
    torch = _torch()
    if rng is None:
        raise ValueError("gen_pattern_batch needs the generators' words: rng uint64 [N,6]")
    host = isinstance(boards, np.ndarray)
    if boards.ndim != 3 or tuple(masks.shape) != tuple(boards.shape) or (seeds is not None
                                                                          and tuple(seeds.shape) != tuple(boards.shape)):
        raise ValueError("Board, mask, and seeds must all have the same shape.")
    N, H, W = (int(x) for x in boards.shape)
    period = int(period)
    _check_gen_range(H, W, period)
    if params is None:
        params = np.tile(gen_pattern_params(), (N, 1))
        if not host:
            params = torch.from_numpy(params).to(boards.device)
    if tuple(params.shape) != (N, _hip.GEN_PATTERN_PARAMS) or tuple(rng.shape) != (N, _hip.GEN_PATTERN_RNG_WORDS):
        raise ValueError("params must be [N,12] and rng [N,6]")
    if host:
        if rng.dtype != np.uint64:
            raise ValueError("rng must be uint64 [N,6]")
        d_boards, d_masks = _to_device(boards, np.uint16), _to_device(masks, np.int32)
        d_seeds = None if seeds is None else _to_device(seeds, np.int32)
        d_params, d_rng = _to_device(params, np.float64), _to_device(rng, np.uint64)
    else:
        d_boards, d_masks, d_params, d_rng = boards.contiguous(), masks.contiguous(), params.contiguous(), rng.contiguous()
        d_seeds = None if seeds is None else seeds.contiguous()
        if (d_boards.dtype != torch.int16 or d_masks.dtype != torch.int32 or d_params.dtype != torch.float64
                or d_rng.dtype != torch.int64 or (d_seeds is not None and d_seeds.dtype != torch.int32)):
            raise ValueError("device tensors: boards int16, masks / seeds int32, params float64, rng int64")
    dev = d_boards.device
    if out is not None:
        out, status, iters = out
        if host or not (out.is_contiguous() and status.is_contiguous() and iters.is_contiguous()
                        and out.dtype == torch.int16 and status.dtype == iters.dtype == torch.int32
                        and tuple(out.shape) == (N, H, W) and tuple(status.shape) == tuple(iters.shape) == (N,)):
            raise ValueError("out: contiguous device tensors (int16 [N,H,W], int32 [N], int32 [N]), with device inputs")
    else:
        out = torch.empty_like(d_boards)
        status = torch.empty((N,), dtype=torch.int32, device=dev)
        iters = torch.empty((N,), dtype=torch.int32, device=dev)
    if N:
        layers = [d_boards]
        if period > 1:          # module.c:374-378: the later layers by the full rule at spawn_prob 0 -- spawners still draw
            p0 = torch.zeros((N,), dtype=torch.float32, device=dev)
            rng4 = d_rng[:, :4].contiguous()
            for _ in range(1, period):
                layers.append(advance_board_batch(layers[-1], p0, rng4, 1))
            d_rng[:, :4] = rng4
        d_layers = d_boards if period == 1 else torch.stack(layers, dim=1).contiguous()
        need = _hip.lib().slhip_gen_pattern_workspace_bytes(N, H, W, period)
        work = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None
        rc = _hip.lib().slhip_gen_pattern_batch(_hip.ptr(d_layers), _hip.ptr(d_masks), _hip.ptr(d_seeds), _hip.ptr(d_params),
                                                _hip.ptr(d_rng), _hip.ptr(out), _hip.ptr(status), _hip.ptr(iters), N, H, W,
                                                period, _hip.ptr(work), need, _hip.current_stream_ptr())
        _hip.check(rc, "Board must be at least 3x3.")
    if host:
        np.copyto(rng, _to_host(d_rng, np.uint64))
        return _to_host(out, np.uint16), _to_host(status, np.int32), _to_host(iters, np.int32)
    if d_rng.data_ptr() != rng.data_ptr():
        rng.copy_(d_rng)
    return out, status, iters


def _as_2d(obj, dtype, what):
    try:
        return np.array(obj).astype(dtype)          # NPY_ARRAY_ENSURECOPY | NPY_ARRAY_FORCECAST
    except (TypeError, ValueError):
        raise ValueError("Board and/or mask and/or seeds are not arrays.")


def gen_pattern(board, mask, period, seeds=None, max_iter=40, min_fill=0.2, temperature=0.5, osc_bonus=0.3,
                alive=(0, 0), wall=(100, 100), tree=(100, 100)):
    """Generate a random (potentially oscillating) pattern in the part of `board` that `mask` opens (module.c:252-417):
    returns the new board, uint16, the input untouched; raises MaxIterException when the sampler runs out of iterations.
    Draws from the process-global generator, which ends where the reference's would."""
    if isinstance(period, float) or not hasattr(period, "__index__"):
        raise TypeError("period must be an integer")
    period = int(period)
    params = gen_pattern_params(max_iter, min_fill, temperature, osc_bonus, alive, wall, tree)
    b = _as_2d(board, np.uint16, "board")
    m = _as_2d(mask, np.int32, "mask")
    s = None if seeds is None else _as_2d(seeds, np.int32, "seeds")
    if period <= 0:
        raise ValueError("Pattern period must be larger than 0.")
    if b.ndim != 2 or m.ndim != 2 or (s is not None and s.ndim != 2):
        raise ValueError("Board, mask, and seeds must all be dimension 2.")
    if b.shape[0] < 3 or b.shape[1] < 3:
        raise ValueError("Board must be at least 3x3.")
    if b.shape != m.shape or (s is not None and s.shape != b.shape):
        raise ValueError("Board, mask, and seeds must all have the same shape.")
    _check_gen_range(b.shape[0], b.shape[1], period)
    bitgen = _current_bitgen()
    words = pcg64_words6(bitgen)[None].copy()
    out, status, _ = gen_pattern_batch(b[None], m[None], period, None if s is None else s[None], params[None], words)
    if status[0] == _hip.GEN_PATTERN_REFUSED:
        raise ValueError("max_iter * area * period does not fit an int")
    pcg64_set_words6(bitgen, words[0])
    if status[0] == _hip.GEN_PATTERN_MAX_ITER:
        raise MaxIterException("Max-iter hit. Aborting!")
    if status[0] != 0:
        raise BoardGenException("Miscellany error.")
    return out[0]


# --------------------------------------------------------------------------- the level generator's region partition

PARTITION_MAX_SIDE, PARTITION_MAX_REGIONS = _hip.PARTITION_MAX_SIDE, _hip.PARTITION_MAX_REGIONS


def partition_batch(words, shape, min_regions=2, max_regions=5, out=None):
    """N independent ``proc_gen.partition`` problems of one board shape in one launch.

    words uint64 [N,6] (``pcg64_words6``; read only); shape (H, W); min_regions / max_regions: scalars or int32 [N].  All
    numpy, or device tensors (words int64, bounds int32 or scalars).  Returns (labels int16 [N,H,W], words [N,6] afterwards,
    status int32 [N]) of the same kind.  Where status is 0, labels and words are bit-equal to ``proc_gen.partition`` on a
    Generator(PCG64) set to the problem's words.  Status -4: refused -- H or W outside 3 .. 64, or more than 8 regions after
    the host function's clamping (lo = max(1, min), hi = max(max, lo)); -5: a loop cap ended the problem.  Where status is not
    0 the labels are left as they were (zeros, or what ``out`` held) and the words are the input's: run the host function.
    Raises nothing per problem.  ``out`` (device tensors only): caller-owned contiguous (labels int16 [N,H,W], words int64
    [N,6], status int32 [N]) to write into."""
    torch = _torch()
    host = isinstance(words, np.ndarray)
    H, W = (int(x) for x in shape)
    if words.ndim != 2 or int(words.shape[1]) != 6:
        raise ValueError("words must be [N,6]")
    N = int(words.shape[0])
    if host:
        if words.dtype != np.uint64:
            raise ValueError("words must be uint64 [N,6]")
        d_in = _to_device(words, np.uint64)
    else:
        if words.dtype != torch.int64:
            raise ValueError("device tensors: words int64 [N,6]")
        d_in = words
    dev = d_in.device

    def bounds(value, name):
        if isinstance(value, torch.Tensor):
            t = value.to(device=dev, dtype=torch.int32).contiguous()
        elif isinstance(value, np.ndarray) and value.ndim:
            t = torch.from_numpy(np.ascontiguousarray(np.clip(value, -2 ** 31, 2 ** 31 - 1), dtype=np.int32)).to(dev)
        else:
            t = torch.full((N,), max(-2 ** 31, min(2 ** 31 - 1, int(value))), dtype=torch.int32, device=dev)
        if tuple(t.shape) != (N,):
            raise ValueError("%s must be a scalar or one value per problem" % name)
        return t

    d_lo, d_hi = bounds(min_regions, "min_regions"), bounds(max_regions, "max_regions")
    if out is not None:
        labels, d_words, status = out
        if host or not (labels.is_contiguous() and d_words.is_contiguous() and status.is_contiguous()
                        and labels.dtype == torch.int16 and d_words.dtype == torch.int64 and status.dtype == torch.int32
                        and tuple(labels.shape) == (N, H, W) and tuple(d_words.shape) == (N, 6)
                        and tuple(status.shape) == (N,)):
            raise ValueError("out: contiguous device tensors (int16 [N,H,W], int64 [N,6], int32 [N]), with device inputs")
        d_words.copy_(d_in)
    else:
        labels = torch.zeros((N, H, W), dtype=torch.int16, device=dev)
        d_words = d_in if host else d_in.clone().contiguous()
        status = torch.empty((N,), dtype=torch.int32, device=dev)
    if N:
        # room for as many regions as the largest clamped bound asks for, 8 at the most (the problems above are refused)
        room = int(torch.maximum(d_hi, d_lo.clamp(min=1)).max())
        room = max(1, min(PARTITION_MAX_REGIONS, room))
        need = _hip.lib().slhip_partition_workspace_bytes(N, H, W, room)
        work = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None
        rc = _hip.lib().slhip_partition_batch(_hip.ptr(d_words), _hip.ptr(d_lo), _hip.ptr(d_hi), _hip.ptr(labels),
                                              _hip.ptr(status), N, H, W, room, _hip.ptr(work), need,
                                              _hip.current_stream_ptr())
        _hip.check(rc)
    if host:
        return _to_host(labels, np.int16), _to_host(d_words, np.uint64), _to_host(status, np.int32)
    return labels, d_words, status
