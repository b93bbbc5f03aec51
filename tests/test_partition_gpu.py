"""GPU suite for the batched region partition: slhip_partition_batch through speedups.partition_batch against
``proc_gen.partition`` on a numpy generator set to the same words -- labels, the six words afterwards, status -- at every
shape, batch size and entry state of the generator, the refusals, the workspace switch, and whole levels with the device
partition against whole levels with the host's."""
import os

import numpy as np
import pytest

from safelife_amd import _hip, proc_gen, speedups
from tests import partition_cases as pc
from tests import util

pytestmark = pytest.mark.gpu

GUARD = 64          # poisoned elements in front of and behind every buffer the kernel writes
POISON16, POISON32, POISON64 = 0x5A5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
_host = {}


def host(words, shape, lo, hi):
    """proc_gen.partition, each distinct problem once"""
    key = (np.asarray(words).tobytes(), tuple(shape), int(lo), int(hi))
    if key not in _host:
        _host[key] = pc.host(words, shape, lo, hi)
    return _host[key]


def check_against_host(words, shape, lo, hi, labels, after, status, what=""):
    lo, hi = np.broadcast_to(lo, (len(words),)), np.broadcast_to(hi, (len(words),))
    for k in range(len(words)):
        want, want_words = host(words[k], shape, lo[k], hi[k])
        assert int(status[k]) == 0, (shape, k, what)
        assert np.array_equal(labels[k], want), (shape, k, what)
        assert np.array_equal(after[k], want_words), (shape, k, what)


@pytest.mark.parametrize("H,W,lo,hi", pc.SHAPES)
def test_labels_words_and_status_at_every_shape(H, W, lo, hi):
    n = 4 if H * W > 2000 else 8
    words = np.stack([pc.words_of(500 + 7 * s + H * W, buffered=bool(s % 2)) for s in range(n)])
    keep = words.copy()
    labels, after, status = speedups.partition_batch(words, (H, W), lo, hi)
    assert labels.dtype == np.int16 and labels.shape == (n, H, W) and after.dtype == np.uint64 and status.dtype == np.int32
    assert np.array_equal(words, keep)                                      # the input words are only read
    check_against_host(words, (H, W), lo, hi, labels, after, status)
    counts = {int(x.max()) for x in labels}
    if (H, W) == (5, 5):
        assert counts == {1}                                                # later seeds find no free cell
    if (H, W, hi) == (26, 26, 1):
        assert all(int((x != 0).sum()) == 540 for x in labels)              # the lone region's stop


def test_small_boards_run_out_of_seed_cells():
    """3x3 with (1,3): the 5x5 window wraps onto duplicates, and a board with one region has no free seed cell left"""
    words = np.stack([pc.words_of(s) for s in range(200)])
    labels, after, status = speedups.partition_batch(words, (3, 3), 1, 3)
    check_against_host(words, (3, 3), 1, 3, labels, after, status)
    drawn = np.array([1 + pc.Draws(w).integers(0, 3) for w in words])
    assert (labels.reshape(200, -1).max(axis=1) < drawn).sum() >= 100


def guarded(shape, dtype, poison, dev):
    import torch
    flat = torch.full((2 * GUARD + int(np.prod(shape)),), poison, dtype=dtype, device=dev)
    return flat, flat[GUARD:GUARD + int(np.prod(shape))].view(*shape)


def run_guarded(words, shape, lo, hi):
    """partition_batch on device tensors, the outputs between poisoned guards -> numpy (labels, words, status)"""
    import torch
    dev = _hip.device()
    N = len(words)
    lab_all, labels = guarded((N,) + tuple(shape), torch.int16, POISON16, dev)
    w_all, after = guarded((N, 6), torch.int64, POISON64, dev)
    st_all, status = guarded((N,), torch.int32, POISON32, dev)
    d_words = torch.from_numpy(words.view(np.int64)).to(dev)
    keep = d_words.clone()
    d_lo = torch.from_numpy(np.broadcast_to(lo, (N,)).astype(np.int32)).to(dev)
    d_hi = torch.from_numpy(np.broadcast_to(hi, (N,)).astype(np.int32)).to(dev)
    got = speedups.partition_batch(d_words, shape, d_lo, d_hi, out=(labels, after, status))
    torch.cuda.synchronize()
    assert got[0] is labels and got[1] is after and got[2] is status and torch.equal(d_words, keep)
    for flat, poison in ((lab_all, POISON16), (w_all, POISON64), (st_all, POISON32)):
        assert bool((flat[:GUARD] == poison).all()) and bool((flat[-GUARD:] == poison).all()), shape
    return labels.cpu().numpy(), after.cpu().numpy().view(np.uint64), status.cpu().numpy()


@pytest.mark.parametrize("n_problems", [1, 63, 64, 65, 257])
def test_batch_sizes_between_poisoned_guards(n_problems):
    """Distinct words and mixed per-problem bounds at 26x26; the same words give the same bytes at any position and in
    any batch size (the distinct problems are 24: the host runs each once)."""
    bounds = [(2, 3), (2, 5), (1, 1), (3, 8)]
    distinct = [(pc.words_of(900 + s, buffered=bool(s % 3 == 0)),) + bounds[s % 4] for s in range(24)]
    deal = [distinct[(5 * k + n_problems) % 24] for k in range(n_problems)]
    words = np.stack([d[0] for d in deal])
    lo, hi = np.array([d[1] for d in deal]), np.array([d[2] for d in deal])
    labels, after, status = run_guarded(words, (26, 26), lo, hi)
    check_against_host(words, (26, 26), lo, hi, labels, after, status, "x%d" % n_problems)


def test_redraw_cases():
    """Generators whose first 32-bit draw lands under Lemire's threshold for H * W: with min == max the seed-cell draw is the
    partition's first draw, and numpy redraws there (the host side asserts it does)."""
    found = pc.redraw_cases()
    assert len(found[(61, 59)]) == 19 and found[(61, 59)][0] == 4449616
    for (H, W), idx in found.items():
        idx = idx[:4]
        words = np.stack([pc.words_of(12345, advance=i) for i in idx])
        for w in words:
            bg = np.random.PCG64(0)
            speedups.pcg64_set_words6(bg, w)
            np.random.Generator(bg).integers(0, H * W)
            assert int(w[4]) == 0 and int(speedups.pcg64_words6(bg)[4]) == 0        # both halves of one output: it redrew
            model = pc.Draws(w)
            model.integers(0, H * W)
            assert model.redraws == 1
        labels, after, status = speedups.partition_batch(words, (H, W), 2, 2)
        check_against_host(words, (H, W), 2, 2, labels, after, status, "redraw")


def test_buffered_half_on_entry_and_on_exit():
    words = np.stack([pc.words_of(40 + s, buffered=True) for s in range(16)])
    assert (words[:, 4] == 1).all()
    labels, after, status = speedups.partition_batch(words, (13, 20), 2, 4)
    check_against_host(words, (13, 20), 2, 4, labels, after, status, "buffered")
    assert {int(x) for x in after[:, 4]} == {0, 1}                          # and cases that end with it set, and without


def test_refusals_leave_poison_and_words():
    words = np.stack([pc.words_of(60 + s, buffered=bool(s % 2)) for s in range(6)])
    for shape, lo, hi in (((26, 26), 9, 9), ((26, 26), 2, 9), ((2, 26), 2, 3), ((26, 65), 2, 3), ((65, 2), 1, 1)):
        labels, after, status = run_guarded(words, shape, lo, hi)
        assert (status == _hip.PARTITION_REFUSED).all(), shape
        assert (labels.view(np.uint16) == POISON16).all() and np.array_equal(after, words), shape
    # a mixed batch: -4 on the offending problems only
    lo = np.array([2, 9, 2, 1, 12, 2])
    hi = np.array([3, 9, 9, 1, 2, 8])
    labels, after, status = run_guarded(words, (26, 26), lo, hi)
    bad = np.array([False, True, True, False, True, False])
    assert (status[bad] == _hip.PARTITION_REFUSED).all() and (status[~bad] == 0).all()
    assert (labels[bad].view(np.uint16) == POISON16).all() and np.array_equal(after[bad], words[bad])
    check_against_host(words[~bad], (26, 26), lo[~bad], hi[~bad], labels[~bad], after[~bad], status[~bad], "mixed")
    # the numpy path hands refused problems back as zeros with the input's words
    labels, after, status = speedups.partition_batch(words, (26, 26), lo, hi)
    assert (status[bad] == -4).all() and not labels[bad].any() and np.array_equal(after[bad], words[bad])
    assert (status[~bad] == 0).all()
    # and the backend runs them on the host
    rqs = [proc_gen.PartitionRequest(words[k], (26, 26), int(lo[k]), int(hi[k])) for k in range(6)]
    rqs.append(proc_gen.PartitionRequest(words[0], (66, 5), 2, 3))
    for rq, (got, got_words) in zip(rqs, proc_gen.device_partition_backend(rqs)):
        want, want_words = pc.host(rq.words, rq.shape, rq.min_regions, rq.max_regions)
        assert np.array_equal(got, want) and np.array_equal(got_words, want_words)


def layout_bytes(H, W, room):
    cells = H * W
    return (64 + 8 * room * ((cells + 63) // 64) + 2 * room * cells + cells + 15) // 16 * 16


def test_workspace_sizing_agrees_with_the_switch():
    """64x64 with room for eight regions is the state above 64 KiB: the sizing function says so, and the problem runs out of
    the workspace to the host's result; with room for seven it fits LDS and needs none; both through the same code."""
    size = _hip.lib().slhip_partition_workspace_bytes
    assert size(4, 64, 64, 8) == 4 * layout_bytes(64, 64, 8) and layout_bytes(64, 64, 8) > 65536
    assert size(4, 64, 64, 7) == 0 and layout_bytes(64, 64, 7) <= 65536
    assert size(4, 63, 61, 8) == 4 * layout_bytes(63, 61, 8) and size(4, 63, 61, 5) == 0
    words = np.stack([pc.words_of(80 + s) for s in range(3)])
    for lo, hi in ((7, 7), (8, 8), (5, 8)):
        labels, after, status = speedups.partition_batch(words, (64, 64), lo, hi)
        check_against_host(words, (64, 64), lo, hi, labels, after, status, "room %d" % hi)
    # without the workspace the call is an error, not a launch
    import torch
    dev = _hip.device()
    d_words = torch.from_numpy(words.view(np.int64)).to(dev)
    bounds = torch.full((3,), 8, dtype=torch.int32, device=dev)
    labels = torch.zeros((3, 64, 64), dtype=torch.int16, device=dev)
    status = torch.zeros((3,), dtype=torch.int32, device=dev)
    rc = _hip.lib().slhip_partition_batch(_hip.ptr(d_words), _hip.ptr(bounds), _hip.ptr(bounds), _hip.ptr(labels),
                                          _hip.ptr(status), 3, 64, 64, 8, None, 0, _hip.current_stream_ptr())
    assert rc == _hip.SL_E_ARG


# ---- whole levels ------------------------------------------------------------------------------------------------------------------

SPECS = os.path.join(util.REPO, "tests", "golden", "procgen")


def spec(name):
    return proc_gen.load_params(os.path.join(SPECS, name + ".yaml"), defaults=os.path.join(SPECS, "_defaults.yaml"))


class Recording(object):
    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __call__(self, requests):
        self.calls.append(len(requests))
        return self.inner(requests)


@pytest.mark.parametrize("name,n_seeds", [("prune-still", 32), ("append-still-easy", 32), ("append-spawn", 32),
                                          ("multi-agent-build-coop", 8)])
def test_whole_levels_device_partition_against_host_partition(name, n_seeds):
    params = spec(name)
    seeds = list(range(4000, 4000 + n_seeds))
    device = Recording(proc_gen.device_partition_backend)
    got = proc_gen.gen_games(params, seeds, partition_backend=device)
    want = proc_gen.gen_games(params, seeds, partition_backend=proc_gen.host_partition_backend)
    default = proc_gen.gen_games(params, seeds[:4])                          # no backend given: the device's partition
    assert device.calls == [n_seeds]                                        # a round's partitions arrive in ONE call
    for s, a, b in zip(seeds, got, want):
        assert a.board.tobytes() == b.board.tobytes() and a.goals.tobytes() == b.goals.tobytes(), (name, s)
        assert a.regions.tobytes() == b.regions.tobytes() and a.regions.dtype == b.regions.dtype == np.int16, (name, s)
        assert np.array_equal(a.agent_locs, b.agent_locs), (name, s)
        assert np.array_equal(a.initial_rng_words(), b.initial_rng_words()), (name, s)
    for a, b in zip(default, want):
        assert a.board.tobytes() == b.board.tobytes() and a.regions.tobytes() == b.regions.tobytes()
    assert len({x.regions.tobytes() for x in got}) == n_seeds
