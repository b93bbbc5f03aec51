"""
Packs transport problems into the buffers slhip_emd_batch reads (an episode queue with records, the occupancy
counts, the keys and the type masks) and runs it: the helper of tests/test_emd.py and tests/test_emd_reference.py.

A problem is a dict with integer boards ``a``, ``b`` [H,W] and ``den``: den == 1 is a 0/1 mask problem (cell-type
slots 8..23 of an entry), any other den is an occupancy-count problem over the queue's num_samples (life-colour slots
0..7).  An entry holds up to 8 count problems and up to 16 mask problems.
"""
import ctypes as C

import numpy as np

CUT_SHORT_TYPES = 17          # a record's n_cell_types above SL_SE_MAX_KEYS - 8: the entry's keys were cut short


def dense_placement(problems, skip=()):
    """(entry, slot) per problem: count problems fill slots 0..7 and mask problems slots 8..23 of successive entries,
    both from entry 0 on, never an entry of `skip`."""
    from safelife_amd import _hip
    K = _hip.SL_SE_MAX_KEYS
    free = {}

    def take(kind, width, base):
        e, k = free.get(kind, (0, 0))
        while e in skip:
            e += 1
        free[kind] = (e, k + 1) if k + 1 < width else (e + 1, 0)
        return e, base + k
    return [take("mask", K - 8, 8) if c["den"] == 1 else take("count", 8, 0) for c in problems]


def run_queue(problems, shape, den, table=None, penalty=1.0, concurrency=None, repeat=1, placement=None,
              cut_short=(), n_entries=None, count=None, capacity=None):
    """slhip_emd_batch over a queue that holds `problems` at `placement` (default: dense_placement).  `cut_short`:
    entries whose record says the keys were cut short (they are given the first problem's data and a valid key all the
    same: only the record may stop the solver).  `n_entries`: valid entries (default: as many as the placement needs),
    `count`: what the queue's counter says (default n_entries), `capacity` (default n_entries + 3).
    Checked here: entries past min(count, capacity) are untouched, unused slots of a valid entry give NaN / 0,
    cut-short entries NaN / -1, and the solver reports no loop-bound error.
    Returns one (scores [P,2] = distance and mass, n_cells [P]) per repeat."""
    import torch
    from safelife_amd import _hip
    from safelife_amd.side_effects import ground_table
    lib, dev = _hip.lib(), _hip.device()
    H, W = shape
    K = _hip.SL_SE_MAX_KEYS
    cut_short = set(cut_short)
    if placement is None:
        placement = dense_placement(problems, cut_short)
    assert len(placement) == len(set(placement)) == len(problems) and not cut_short & {e for e, _ in placement}
    if n_entries is None:
        n_entries = max([e + 1 for e, _ in placement] + [e + 1 for e in cut_short] + [0])
    cap = n_entries + 3 if capacity is None else capacity
    count = n_entries if count is None else count
    valid = min(count, cap)
    assert all(e < cap for e, _ in placement) and cap >= 1
    counts = np.zeros((2, cap, H, W, 8), np.int32)
    masks = np.zeros((cap, 2, K - 8, H, W), np.uint8)
    keys = np.full((cap, K), 0xFFFF, np.uint16)
    records = np.zeros((cap, 8), np.int32)

    def put(c, e, k):
        a, b = np.asarray(c["a"]), np.asarray(c["b"])
        assert a.shape == (H, W) and b.shape == (H, W) and min(a.min(), b.min()) >= 0
        if c["den"] == 1:
            assert 8 <= k < K and max(a.max(), b.max()) <= 1
            masks[e, 0, k - 8], masks[e, 1, k - 8] = a, b
        else:
            assert 0 <= k < 8 and c["den"] == den
            counts[0, e, :, :, k], counts[1, e, :, :, k] = a, b
        keys[e, k] = 0x0100 + k

    for c, (e, k) in zip(problems, placement):
        put(c, e, k)
    for e in cut_short:
        records[e, 7] = CUT_SHORT_TYPES << 16
        if problems:
            put(problems[0], e, 8 if problems[0]["den"] == 1 else 0)
    t = dict(count=torch.tensor([count], dtype=torch.int32, device=dev), records=torch.from_numpy(records).to(dev),
             counts=torch.from_numpy(counts).to(dev), keys=torch.from_numpy(keys.view(np.int16)).to(dev),
             masks=torch.from_numpy(masks).to(dev))
    table = torch.from_numpy(np.ascontiguousarray(ground_table(shape) if table is None else table, np.float64)).to(dev)
    assert tuple(table.shape) == (2 * H - 1, 2 * W - 1)
    conc = concurrency or min(64, cap * K)
    size = lib.slhip_emd_workspace_bytes(H, W, cap, conc)
    assert size > 0
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    q = _hip.EpisodeQueue()
    q.capacity, q.env_base = cap, 0
    q.count, q.records, q.boards = t["count"].data_ptr(), t["records"].data_ptr(), None
    used = np.zeros((cap, K), bool)
    for e, k in placement:
        used[e, k] = True
    runs = []
    for _ in range(repeat):
        scores = torch.full((cap, K, 2), -7.0, dtype=torch.float64, device=dev)
        n_cells = torch.full((cap, K), -7, dtype=torch.int32, device=dev)
        _hip.check(lib.slhip_emd_batch(C.byref(q), H, W, den, _hip.ptr(t["counts"]), _hip.ptr(t["keys"]),
                                       _hip.ptr(t["masks"]), _hip.ptr(table), float(penalty), _hip.ptr(ws), size, conc,
                                       _hip.ptr(scores), _hip.ptr(n_cells), _hip.current_stream_ptr()))
        _hip.check(lib.slhip_emd_status(_hip.ptr(ws), _hip.current_stream_ptr()))
        s, m = scores.cpu().numpy(), n_cells.cpu().numpy()
        assert (s[valid:] == -7.0).all() and (m[valid:] == -7).all()                 # entries past the count: untouched
        for e in range(valid):
            if e in cut_short:
                assert np.isnan(s[e]).all() and (m[e] == -1).all()                   # cut-short entries
            else:
                assert np.isnan(s[e, ~used[e]]).all() and (m[e, ~used[e]] == 0).all()    # empty key slots
        runs.append((np.array([s[e, k] for e, k in placement]).reshape(-1, 2),
                     np.array([m[e, k] for e, k in placement], np.int32)))
    return runs
