"""
Boards -> RGB frames: the counterpart of the reference's ``render_graphics`` (render_board / render_game) on top of
``slhip_render_boards`` (csrc/sl_render.hip), bit exact with the reference's C blitter (fast_render.c:33-133).

Every cell is a 14x14 sprite chosen by the cell's type, tinted with the cell's colour over the GOAL's colour; per byte
``uint8(255 * (bg * (1 - mask) + mask * sprite * fg))`` in float32, left to right, truncated.

* ``render_board(board, goals, orientation=None, sprite_sheet=None, out=None)`` -- any leading shape.  Device tensors
  in, a ``torch.uint8`` device tensor out, nothing crosses to the host.  numpy in, numpy out: through the device when
  one is present, else through the host numpy path of this module (``render_board_host``) -- a restatement of the same
  arithmetic with a tile lookup, which is what the CPU tests pin against the reference's recorded frames.
* ``render_game(game, view_size=None)`` -- a ``SafeLifeGame`` (anything with ``board``, ``goals``, ``agent_locs``,
  ``exit_locs``): the view is centred on agent 0, or (0, 0) without one; exits outside it are painted on its perimeter.
* ``render_batch(...)`` -- what the vector envs' ``render()`` call: frames of device-resident state.

Not taken from the reference: the edit cursor (``edit_loc`` / ``edit_color``: the level editor), GIF / MP4 export,
text rendering.
"""
import ctypes as C
import os

import numpy as np

from . import _hip

SPRITE_SIZE = 14
_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_SPRITE_PATH = os.path.join(os.path.dirname(_HERE), "tests", "golden", "sprites.png")

foreground_colors = np.array([
    [0.4, 0.4, 0.4],  # black
    [0.8, 0.2, 0.2],  # red
    [0.2, 0.8, 0.2],  # green
    [0.8, 0.8, 0.2],  # yellow
    [0.2, 0.2, 0.8],  # blue
    [0.8, 0.2, 0.8],  # magenta
    [0.2, 0.8, 0.8],  # cyan
    [1.0, 1.0, 1.0],  # white
])
background_colors = np.array([
    [0.6, 0.6, 0.6],  # black
    [0.9, 0.6, 0.6],  # red
    [0.6, 0.9, 0.6],  # green
    [0.9, 0.9, 0.6],  # yellow
    [0.5, 0.5, 0.9],  # blue
    [0.9, 0.6, 0.9],  # magenta
    [0.6, 0.9, 0.9],  # cyan
    [0.9, 0.9, 0.9],  # white
])

_COLOR_MASK, _ORIENT_MASK = 7 << 9, 3 << 12
#: cell type (colour and orientation bits cleared) -> tile (row, col) of the sheet
_TILES = {9: (1, 0), 1: (1, 1), 53: (1, 2), 32789: (1, 3), 17: (1, 4),
          32884: (2, 0), 48: (2, 1), 16: (2, 2), 32788: (2, 3), 85: (2, 4),
          152: (3, 0), 272: (3, 1), 144: (3, 2)}
_UNKNOWN = (3, 4)

_default_sheet = None
_tile_lut = None
_default_table = {}


def load_sprite_sheet(path=None):
    """The sprite sheet as float32 [70, 70, 4] (RGBA / 255).  Default: the reference's ``sprites.png``, kept as a
    fixture under tests/golden."""
    global _default_sheet
    if path is None and _default_sheet is not None:
        return _default_sheet
    from PIL import Image
    with Image.open(path or DEFAULT_SPRITE_PATH) as im:
        sheet = np.asarray(im.convert("RGBA")) / np.float32(255)
    if sheet.shape != (5 * SPRITE_SIZE, 5 * SPRITE_SIZE, 4):
        raise ValueError("Sprites should have shape (70, 70, 4).")
    sheet = np.ascontiguousarray(sheet, dtype=np.float32)
    if path is None:
        _default_sheet = sheet
    return sheet


def _sheet(sprite_sheet):
    if sprite_sheet is None:
        return load_sprite_sheet()
    s = np.ascontiguousarray(sprite_sheet, dtype=np.float32)
    if s.size != 70 * 70 * 4:
        raise ValueError("Sprites should have shape (70, 70, 4).")
    return s.reshape(70, 70, 4)


# --------------------------------------------------------------------------- the host path

def _tile_index(cells):
    """uint16 cells -> tile number row * 5 + col (fast_render.c:43-86)."""
    global _tile_lut
    if _tile_lut is None:
        types = np.arange(1 << 16) & ~(_COLOR_MASK | _ORIENT_MASK)
        orient = (np.arange(1 << 16) & _ORIENT_MASK) >> 12
        lut = np.full(1 << 16, _UNKNOWN[0] * 5 + _UNKNOWN[1], np.uint8)
        agent = (types & 2) != 0
        lut[agent] = 1 + orient[agent]
        for value, (row, col) in _TILES.items():
            lut[types == value] = row * 5 + col
        lut[0] = 0                           # empty; type 0 with colour or orientation bits stays "unknown"
        _tile_lut = lut
    return _tile_lut[cells]


def _blend_table(sheet):
    """uint8 [25 tiles, 8 fg, 8 bg, 14, 14, 3]: every sprite in every colour pair, with the reference's float32
    expression -- bg * (1 - mask) + (mask * sprite) * fg, times 255, truncated."""
    s = SPRITE_SIZE
    tiles = sheet.reshape(5, s, 5, s, 4).transpose(0, 2, 1, 3, 4).reshape(25, 1, 1, s, s, 4)
    mask, rgb = tiles[..., 3:4], tiles[..., 0:3]
    fg = foreground_colors.astype(np.float32).reshape(1, 8, 1, 1, 1, 3)
    bg = background_colors.astype(np.float32).reshape(1, 1, 8, 1, 1, 3)
    one = np.float32(1)
    value = np.float32(255) * (bg * (one - mask) + mask * rgb * fg)
    return value.astype(np.uint8)


def render_board_host(board, goals, orientation=None, sprite_sheet=None):
    """``render_board`` in numpy alone (no device)."""
    board = np.asarray(board).astype(np.uint16, copy=False)
    goals = np.asarray(goals).astype(np.uint16, copy=False)
    if board.ndim < 2:
        raise ValueError("Board must have at least two dimensions.")
    if orientation is not None:
        o = np.asarray(orientation).astype(np.uint16) & 3
        board = (board & ~np.uint16(_ORIENT_MASK)) | (o[..., None, None] << 12).astype(np.uint16)
    if goals.shape != board.shape:
        goals = np.broadcast_to(goals, board.shape)
    if sprite_sheet is None:                 # (the default sheet's table is built once)
        if "table" not in _default_table:
            _default_table["table"] = _blend_table(load_sprite_sheet())
        table = _default_table["table"]
    else:
        table = _blend_table(_sheet(sprite_sheet))
    img = table[_tile_index(board), (board & _COLOR_MASK) >> 9, (goals & _COLOR_MASK) >> 9]    # [..., H, W, 14, 14, 3]
    lead, (H, W), s = board.shape[:-2], board.shape[-2:], SPRITE_SIZE
    img = np.moveaxis(img, -3, -4)                                                           # [..., H, 14, W, 14, 3]
    return np.ascontiguousarray(img).reshape(lead + (H * s, W * s, 3))


def recenter_view(board, view_size, center, exits=None):
    """helper_utils.py:42-75: the toroidal window of ``view_size`` centred on ``center``; ``exits`` = (rows, cols) whose
    board values are painted at their clipped position in the view, later ones over earlier ones."""
    h, w = view_size
    bh, bw = board.shape
    y0, x0 = int(center[0]), int(center[1])
    rows = np.arange(y0 - h // 2, y0 - h // 2 + h) % bh
    cols = np.arange(x0 - w // 2, x0 - w // 2 + w) % bw
    view = board[rows[:, None], cols[None, :]]
    if exits is not None:
        iy, ix = np.asarray(exits[0], dtype=np.int64), np.asarray(exits[1], dtype=np.int64)
        jy = np.clip((iy - y0 + bh // 2) % bh - bh // 2 + h // 2, 0, h - 1)
        jx = np.clip((ix - x0 + bw // 2) % bw - bw // 2 + w // 2, 0, w - 1)
        for k in range(len(iy)):
            view[jy[k], jx[k]] = board[iy[k], ix[k]]
    return view


def _game_view(game):
    locs = np.asarray(game.agent_locs).reshape(-1, 2)
    center = (int(locs[0][0]), int(locs[0][1])) if len(locs) > 0 else (0, 0)
    iy, ix = game.exit_locs
    return center, (np.asarray(iy).reshape(-1), np.asarray(ix).reshape(-1))


def render_game_host(game, view_size=None, sprite_sheet=None):
    """``render_game`` in numpy alone."""
    board, goals = np.asarray(game.board, dtype=np.uint16), np.asarray(game.goals, dtype=np.uint16)
    if view_size is not None:
        center, exits = _game_view(game)
        board, goals = recenter_view(board, view_size, center, exits), recenter_view(goals, view_size, center)
    return render_board_host(board, goals, None, sprite_sheet)


# --------------------------------------------------------------------------- the device path

_device_sheets = {}


def device_sheet(sprite_sheet=None):
    """The sheet as a float32 device tensor [70,70,4]; the default sheet is uploaded once and kept."""
    import torch
    if isinstance(sprite_sheet, torch.Tensor):
        if sprite_sheet.dtype != torch.float32 or sprite_sheet.numel() != 70 * 70 * 4 or not sprite_sheet.is_cuda:
            raise ValueError("Sprites should be a float32 device tensor of shape (70, 70, 4).")
        return sprite_sheet.contiguous()
    dev = _hip.device()
    if sprite_sheet is None:
        if dev not in _device_sheets:
            _device_sheets[dev] = torch.from_numpy(load_sprite_sheet()).to(dev)
        return _device_sheets[dev]
    return torch.from_numpy(_sheet(sprite_sheet)).to(dev)


def render_batch(board, goals, sprites, *, n=None, index=None, orientation=None, view_size=None, centers=None,
                 center_stride=2, exits=None, aux_by_index=False, out=None):
    """One ``slhip_render_boards`` launch on the current stream.  board: int16/uint16 device tensor [S,H,W]; goals: the
    same, or [H,W] for one goal array under every frame; index: int32 [n] frames to take (default 0..n-1, n = S);
    orientation: int32 [n]; view_size (vh, vw) with centers (int32, (row, col) every ``center_stride`` elements) and
    exits (int32 [*, E] flat indices, -1 unused), both per frame or -- ``aux_by_index`` -- per source frame.
    Returns uint8 [n, vh*14, vw*14, 3]."""
    import torch
    S, H, W = board.shape
    if index is not None:
        n = int(index.numel())
    elif n is None:
        n = S
    vh, vw = (H, W) if view_size is None else (int(view_size[0]), int(view_size[1]))
    shape = (n, vh * SPRITE_SIZE, vw * SPRITE_SIZE, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=board.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != board.device:
        raise ValueError("out must be a contiguous uint8 tensor %r on the boards' device" % (shape,))
    a = _hip.RenderArgs()
    a.N, a.H, a.W, a.n_source = n, H, W, S
    if view_size is not None:
        a.view_h, a.view_w = vh, vw
        a.centers, a.center_stride = _hip.ptr(centers), int(center_stride)
        if exits is not None:
            a.exits, a.E = _hip.ptr(exits), int(exits.shape[-1])
        a.aux_by_index = 1 if aux_by_index else 0
    a.board_stride = H * W
    a.goal_stride = 0 if goals.dim() == 2 else H * W
    a.board, a.goals, a.index = _hip.ptr(board), _hip.ptr(goals), _hip.ptr(index)
    a.sprites, a.orientation, a.out = _hip.ptr(sprites), _hip.ptr(orientation), _hip.ptr(out)
    _hip.check(_hip.lib().slhip_render_boards(C.byref(a), _hip.current_stream_ptr()))
    return out


def _as_board_tensor(x, device):
    import torch
    if isinstance(x, torch.Tensor):
        if x.dtype not in (torch.int16, torch.uint16):
            x = x.to(torch.int16)
        return x.to(device).contiguous()
    a = np.ascontiguousarray(np.asarray(x).astype(np.uint16, copy=False))
    return torch.from_numpy(a.view(np.int16)).to(device)


def _have_device():
    try:
        import torch
        return os.path.exists(_hip.LIB_PATH) and torch.cuda.is_available()
    except ImportError:
        return False


def render_board(board, goals, orientation=None, sprite_sheet=None, out=None):
    """The look-alike of ``render_graphics.render_board`` for boards of any leading shape ``[..., H, W]``: uint8
    ``[..., H*14, W*14, 3]``.  ``goals``: the boards' shape, or ``[H, W]`` under every frame.  ``orientation``: one
    value 0..3 per frame, replacing every cell's orientation bits (the agents of a recorded history).
    Device tensors in -> a device tensor out (``out``: a uint8 device tensor to write into), no host copy; numpy in ->
    numpy out, through the device when there is one, else through ``render_board_host``.
    The edit cursor (``edit_loc``, ``edit_color``) is not taken: the level editor is out of scope."""
    try:
        import torch
        on_device = isinstance(board, torch.Tensor) and board.is_cuda
    except ImportError:
        on_device = False
    if not on_device:
        b = np.asarray(board.cpu() if hasattr(board, "cpu") else board)
        if b.ndim < 2:
            raise ValueError("Board must have at least two dimensions.")
        if not _have_device():
            img = render_board_host(b, goals.cpu().numpy() if hasattr(goals, "cpu") else goals, orientation, sprite_sheet)
            if out is not None:
                np.copyto(out, img)
                return out
            return img
    import torch
    dev = board.device if on_device else _hip.device()
    bt = _as_board_tensor(board, dev)
    gt = _as_board_tensor(goals, dev)
    if bt.dim() < 2:
        raise ValueError("Board must have at least two dimensions.")
    H, W = bt.shape[-2:]
    lead = tuple(bt.shape[:-2])
    if gt.shape != bt.shape and tuple(gt.shape) != (H, W):
        if gt.numel() != bt.numel():
            raise ValueError("Board and goals must have same size.")
        gt = gt.reshape(bt.shape)
    bt = bt.reshape(-1, H, W)
    if gt.dim() != 2:
        gt = gt.reshape(-1, H, W)
    ot = None
    if orientation is not None:
        ot = torch.as_tensor(np.asarray(orientation) if not isinstance(orientation, torch.Tensor) else orientation)
        ot = ot.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if ot.numel() != bt.shape[0]:
            raise ValueError("orientation needs one value per frame")
    shape = lead + (H * SPRITE_SIZE, W * SPRITE_SIZE, 3)
    dst = out.reshape((-1,) + shape[-3:]) if (out is not None and isinstance(out, torch.Tensor)) else None
    img = render_batch(bt, gt, device_sheet(sprite_sheet), orientation=ot, out=dst).reshape(shape)
    if on_device:
        return out if isinstance(out, torch.Tensor) else img
    img = img.cpu().numpy()
    if out is not None:
        np.copyto(out, img)
        return out
    return img


def render_game(game, view_size=None, sprite_sheet=None):
    """Render a game as a numpy RGB array ``[vh*14, vw*14, 3]`` (``render_graphics.render_game`` without edit mode):
    the whole board, or a ``view_size`` window centred on agent 0 -- (0, 0) when the game has no agent -- with the
    exits that fall outside it painted on its perimeter."""
    if not _have_device():
        return render_game_host(game, view_size, sprite_sheet)
    import torch
    dev = _hip.device()
    bt, gt = _as_board_tensor(game.board, dev)[None], _as_board_tensor(game.goals, dev)[None]
    if view_size is None:
        return render_batch(bt, gt, device_sheet(sprite_sheet))[0].cpu().numpy()
    center, (iy, ix) = _game_view(game)
    centers = torch.tensor([center], dtype=torch.int32, device=dev)
    flat = np.asarray(iy * bt.shape[-1] + ix, dtype=np.int32).reshape(1, -1)
    exits = torch.from_numpy(flat).to(dev) if flat.size else None
    return render_batch(bt, gt, device_sheet(sprite_sheet), view_size=view_size, centers=centers,
                        exits=exits)[0].cpu().numpy()


def render_envs(env, env_ids=None, view_size=None, out=None, centers=None, center_stride=None):
    """Frames of the current state of a vector env's envs (``SafeLifeVectorEnv.render``): ``slhip_env_render``, or --
    ``centers`` given: a multi-agent batch's agent records -- ``slhip_render_boards`` with those centres."""
    import torch
    t, dev = env.t, env.device
    B, H, W = t["board"].shape
    idx = None
    if env_ids is not None:
        idx = torch.as_tensor(env_ids).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    n = B if idx is None else int(idx.numel())
    if not hasattr(env, "_render_sheet"):
        env._render_sheet = device_sheet()           # uploaded once and kept
    if centers is not None:
        return render_batch(t["board"], t["goals"], env._render_sheet, n=n, index=idx, view_size=view_size,
                            centers=centers, center_stride=center_stride, exits=t["exit_locs"], aux_by_index=True, out=out)
    vh, vw = (H, W) if view_size is None else (int(view_size[0]), int(view_size[1]))
    shape = (n, vh * SPRITE_SIZE, vw * SPRITE_SIZE, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous uint8 tensor %r on the env's device" % (shape,))
    rc = env._lib.slhip_env_render(env._sref, _hip.ptr(idx), n, 0 if view_size is None else vh,
                                   0 if view_size is None else vw, _hip.ptr(env._render_sheet), _hip.ptr(out),
                                   _hip.current_stream_ptr())
    _hip.check(rc)
    return out
