"""Checkpoints, the host side (no GPU): the digest's host model (tests/checkpoint_ref.py) against the known answers and its
sensitivity; the checkpoint schedule's model against what the reference's trainers saved (tests/golden/checkpoint_cases.npz)
and five wrong readings of it; and the file layer of safelife_amd/checkpoint.py on CPU tensors through stand-in state
holders."""
import itertools
import os
import types

import numpy as np
import pytest

from tests import checkpoint_ref as ref

CASES = ref.load_cases()
BY_NAME = {c["name"]: c for c in CASES}


# ------------------------------------------------------------------------------------------------------------- the digest

def test_known_answers():
    for data, salt, want in ref.KNOWN:
        assert ref.digest(data, salt) == want, (data, salt)
        assert ref.digest_slow(data, salt) == want
        assert ref.digest(np.frombuffer(data, np.uint8), salt) == want


def test_the_package_s_host_digest_is_the_model():
    from safelife_amd import checkpoint
    rng = np.random.default_rng(5)
    for n in (0, 1, 7, 8, 9, 20, 255, 4097):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for salt in (0, 7, 0xFEDCBA9876543210):
            assert checkpoint.digest_bytes(data, salt) == ref.digest(data, salt) == ref.digest_slow(data, salt)


@pytest.mark.parametrize("n", (1, 7, 8, 9, 255, 256, 257, 4097))
def test_every_single_bit_flip_changes_the_digest(n):
    rng = np.random.default_rng(n)
    data = rng.integers(0, 256, n, dtype=np.uint8)
    base = ref.digest(data)
    # every flip changes exactly one word: acc moves by mix(w' + k) - mix(w + k), which mix (a bijection) keeps non-zero
    with np.errstate(over="ignore"):
        padded = np.zeros((n + 7) // 8 * 8, np.uint8)
        padded[:n] = data
        words = padded.view("<u8").astype(np.uint64)
        k = np.uint64(ref.mix(0)) + np.arange(1, len(words) + 1, dtype=np.uint64) * np.uint64(ref.G)
        terms = ref.mix_array(words + k)
        acc = int(np.add.reduce(terms, dtype=np.uint64))
        tail = ref.mix((0 ^ n) + ref.G)
        assert ref.mix(acc + tail) == base
        seen = set()
        for bit in range(64):
            flipped = ref.mix_array((words ^ np.uint64(1 << bit)) + k)
            moved = (np.uint64(acc) - terms + flipped)              # acc with word i's term replaced, for every i at once
            for i, a in enumerate(moved.tolist()):
                if 8 * i + bit // 8 < n:                            # (a bit of the padding is not a bit of the input)
                    d = ref.mix(a + tail)
                    assert d != base, (i, bit)
                    seen.add(d)
    assert len(seen) == 8 * n                                       # ... and all the flips differ from one another
    # the vectorised walk above is the digest: spot checks through the model itself
    for at in sorted({0, n // 2, n - 1}):
        for bit in (0, 7):
            other = data.copy()
            other[at] ^= 1 << bit
            assert ref.digest(other) in seen and ref.digest(other) != base


def test_every_swap_of_two_words_changes_the_digest():
    rng = np.random.default_rng(64)
    words = rng.integers(0, 1 << 63, 64, dtype=np.uint64)
    base = ref.digest(words)
    seen = set()
    for i, j in itertools.combinations(range(64), 2):
        other = words.copy()
        other[i], other[j] = words[j], words[i]
        d = ref.digest(other)
        assert d != base, (i, j)
        seen.add(d)
    assert len(seen) == 64 * 63 // 2


def test_zero_buffers_of_different_lengths_differ():
    digests = [ref.digest(bytes(n)) for n in range(41)]
    assert len(set(digests)) == 41
    assert digests[0] == ref.KNOWN[0][2]


def test_the_salt_matters():
    data = bytes(range(20))
    salts = (0, 1, 7, 1 << 63, (1 << 64) - 1)
    assert len({ref.digest(data, s) for s in salts}) == len(salts)
    assert len({ref.digest(b"", s) for s in salts}) == len(salts)
    assert ref.digest(data, 1 << 64) == ref.digest(data, 0)         # the salt is a 64-bit word


def test_symbols_layout_and_the_chunk_prefix(tmp_path):
    """The three entry points, `struct sl_digest_segment` against gcc's, and the two host helpers: a segment of w words has
    w // 4096 + 1 chunks (chunks are cut at aligned addresses, so an odd start may need one more than the words fill), the
    workspace is the prefix table and one word per chunk."""
    import ctypes as C
    import subprocess
    from safelife_amd import _hip
    from tests import util
    lib = _hip.lib()
    header = open(os.path.join(util.REPO, "include", "safelife_hip.h")).read()
    for name in ("slhip_state_digest_workspace_bytes", "slhip_state_digest_prefix", "slhip_state_digest"):
        assert name in _hip.EXPORTS and hasattr(lib, name) and name + "(" in header
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safelife_hip.h"\nint main(void) {'
                   'printf("%zu %zu %zu\\n", sizeof(sl_digest_segment), offsetof(sl_digest_segment, ptr), '
                   'offsetof(sl_digest_segment, bytes)); return 0; }')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(util.REPO, "include"), str(src), "-o", exe])
    st = _hip.DigestSegment
    assert subprocess.check_output([exe]).decode().split() == [str(C.sizeof(st)), str(st.ptr.offset), str(st.bytes.offset)]
    assert C.sizeof(st) == 16
    sizes = [0, 1, 8, 4, 32768, 32769, 3 * 32768 + 1, (1 << 30) + 5]
    arr = (C.c_ulonglong * len(sizes))(*sizes)
    prefix = np.zeros(len(sizes) + 1, np.uint64)
    assert lib.slhip_state_digest_prefix(arr, len(sizes), prefix.ctypes.data_as(C.c_void_p)) == 0
    chunks = [((b + 7) // 8) // 4096 + 1 for b in sizes]
    assert prefix.tolist() == [0] + np.cumsum(chunks).tolist() and chunks[:5] == [1, 1, 1, 1, 2]
    assert lib.slhip_state_digest_workspace_bytes(arr, len(sizes)) == 8 * (len(sizes) + 1 + sum(chunks))
    assert lib.slhip_state_digest_workspace_bytes(arr, 0) == 0
    assert lib.slhip_state_digest_prefix(arr, -1, prefix.ctypes.data_as(C.c_void_p)) == _hip.SL_E_ARG
    assert lib.slhip_state_digest_prefix(arr, 2, None) == _hip.SL_E_ARG


# ----------------------------------------------------------------------------------------------------------- the schedule

def test_the_fixture_holds_the_schedules_the_issue_asks_for():
    assert len(CASES) >= 12
    ppo = [c for c in CASES if c["kind"] == "ppo"]
    batch = lambda c: c["num_envs"] * c["steps_per_env"]            # noqa: E731
    assert any(c["interval"] % batch(c) == 0 for c in ppo) and any(c["interval"] % batch(c) for c in ppo)
    assert any(c["interval"] < batch(c) for c in ppo)
    assert {c["keep"] for c in CASES} >= {1, 3}
    assert any(len(c["calls"]) > 1 and c["reload_after"] < 0 for c in CASES)
    assert any(c["reload_after"] >= 0 for c in ppo) and any(c["reload_after"] >= 0 for c in CASES if c["kind"] == "dqn")
    assert any(c["kind"] == "dqn" and 0 < c["replay_initial"] < sum(c["calls"]) for c in CASES)
    assert any(c["test_steps"] for c in CASES)
    assert any(any(not ref._NAME.match(n) for n in c["before"]) for c in CASES)


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_schedule_model_reproduces_the_reference(name):
    c = BY_NAME[name]
    saves, left, test_steps, test_eps = ref.schedule_model(c)
    assert saves == c["saves"]
    assert left == c["left"]
    assert test_steps == c["test_steps"] and test_eps == c["test_eps"]


@pytest.mark.parametrize("wrong", ref.WRONG)
def test_wrong_readings_fail_on_the_fixture(wrong):
    """`<=` for `<`, no first save, pruning by modification time instead of step, `keep` off by one, a load that leaves
    `last` at -1: each disagrees with the reference on at least one schedule."""
    failing = []
    for c in CASES:
        saves, left, _steps, _eps = ref.schedule_model(c, wrong=wrong)
        if saves != c["saves"] or left != c["left"]:
            failing.append(c["name"])
    print(wrong, failing)
    assert failing


def test_dqn_test_steps_and_epsilons():
    tested = [c for c in CASES if c["test_steps"]]
    assert len(tested) >= 2
    for c in tested:
        _saves, _left, steps, eps = ref.schedule_model(c)
        assert steps == c["test_steps"] and eps == c["test_eps"]
        assert set(c["test_eps"]) == {c["eps_testing"]} == {0.01}
        assert all(s >= c["replay_initial"] for s in steps)         # never in front of the replay gate


class _Recorder(object):
    """What checkpoint.save would be for Checkpointer: notes the calls and writes a small file."""

    def __init__(self, monkeypatch):
        from safelife_amd import checkpoint
        self.saved, self.loaded = [], []
        monkeypatch.setattr(checkpoint, "save", self.save)
        monkeypatch.setattr(checkpoint, "load", self.load)

    def save(self, path, root, model=None, optimizer=None, extra=None):
        self.saved.append(extra["num_steps"])
        with open(path, "wb") as f:
            f.write(b"%d" % extra["num_steps"])

    def load(self, path, root, model=None, optimizer=None):
        self.loaded.append(path)
        return {"num_steps": int(open(path, "rb").read())}


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_checkpointer_follows_the_reference(name, tmp_path, monkeypatch):
    """checkpoint.Checkpointer driven as the trainers drive it (save_if_needed per iteration past the gate, a save at the
    end of train()), the file layer replaced by a recorder: the steps saved and the files left are the reference's."""
    from safelife_amd import checkpoint
    c = BY_NAME[name]
    rec = _Recorder(monkeypatch)
    for k, old in enumerate(c["before"]):
        path = tmp_path / old
        path.write_bytes(b"old")
        os.utime(path, (1000 + k, 1000 + k))
    ck = checkpoint.Checkpointer(tmp_path, interval=c["interval"], keep=c["keep"], root=object())
    num_steps = pushed = 0
    for k, steps in enumerate(c["calls"]):
        max_steps = num_steps + steps
        while num_steps < max_steps:
            if c["kind"] == "ppo":
                num_steps += c["num_envs"] * c["steps_per_env"]
                ck.save_if_needed(num_steps)
                continue
            num_steps += c["num_envs"]
            pushed += c["num_envs"]
            if pushed >= c["replay_initial"]:
                ck.save_if_needed(num_steps)
        ck.save(num_steps)
        if k == c["reload_after"]:
            ck = checkpoint.Checkpointer(tmp_path, interval=c["interval"], keep=c["keep"], root=object())
            assert ck.last == -1
            num_steps, pushed = ck.load_latest(), 0
            assert ck.last == num_steps == c["saves"][len(rec.saved) - 1]
    assert rec.saved == c["saves"]
    assert sorted(os.listdir(tmp_path)) == c["left"]
    assert [s for s, _p in ck.files()] == sorted(int(ref._NAME.match(n).group(1)) for n in c["left"] if ref._NAME.match(n))


def test_checkpointer_load_by_name_and_an_empty_directory(tmp_path, monkeypatch):
    from safelife_amd import checkpoint
    rec = _Recorder(monkeypatch)
    ck = checkpoint.Checkpointer(tmp_path / "new", interval=10, keep=3, root=object())
    assert ck.load_latest() is None and ck.last == -1 and not rec.loaded
    ck.save(5), ck.save(20)
    other = checkpoint.Checkpointer(tmp_path / "new", interval=10, keep=3, root=object())
    assert other.load("checkpoint-5.data") == 5 and other.last == 5
    assert not other.save_if_needed(15) and other.save_if_needed(16)


def test_checkpointer_load_looks_in_its_directory_first(tmp_path, monkeypatch):
    """A file of the same name in the working directory does not win; a missing file and a file without a step are
    ValueErrors, and nothing is loaded from them."""
    import torch
    from safelife_amd import checkpoint
    rec = _Recorder(monkeypatch)
    ck = checkpoint.Checkpointer(tmp_path / "run", interval=10, keep=3, root=object())
    ck.save(7)
    elsewhere = tmp_path / "cwd"
    elsewhere.mkdir()
    (elsewhere / "checkpoint-7.data").write_bytes(b"999")
    monkeypatch.chdir(elsewhere)
    assert ck.load("checkpoint-7.data") == 7 and rec.loaded == [os.path.join(str(tmp_path / "run"), "checkpoint-7.data")]
    assert ck.load(os.path.join(str(elsewhere), "checkpoint-7.data")) == 999            # a complete path is taken as it is
    with pytest.raises(ValueError, match="there is no file"):
        ck.load("checkpoint-8.data")
    odd = tmp_path / "run" / "latest.data"
    torch.save({"format": checkpoint.FORMAT_VERSION, "abi": 13, "objects": {}, "models": {}, "optimizers": {}, "extra": None},
               odd)
    before = list(rec.loaded)
    with pytest.raises(ValueError, match="says nowhere at which step it was taken"):
        ck.load("latest.data")
    assert rec.loaded == before and ck.last == 999


def test_config_values_that_cannot_be_compared_are_refused(tmp_path):
    import torch
    from safelife_amd import checkpoint

    class Odd(Holder):
        def _checkpoint_state(self):
            config, scalars, tensors = Holder._checkpoint_state(self)
            return dict(config, thing=object()), scalars, tensors

    with pytest.raises(ValueError, match="value of type object cannot be stored and compared"):
        checkpoint.capture(Odd(torch))
    assert checkpoint.capture(Holder(torch))["root"]["config"]["dtype"] == "torch.int64"


def test_the_pool_s_digest_is_computed_once():
    from safelife_amd import checkpoint
    calls = []

    class Pool(object):
        refreshable = False

        def arrays(self):
            calls.append(1)
            return {"pool_board": np.arange(6, dtype=np.uint16).reshape(1, 2, 3), "pool_rng": np.ones((1, 4), np.uint64)}

    pool = Pool()
    first = checkpoint.pool_digest(pool)
    assert checkpoint.pool_digest(pool) == first and len(calls) == 1 and len(first) == 40
    other = Pool()
    other.arrays = lambda: {"pool_board": np.arange(6, dtype=np.uint16).reshape(1, 3, 2), "pool_rng": np.ones((1, 4), np.uint64)}
    assert checkpoint.pool_digest(other) != first


# --------------------------------------------------------------------------------------------------------- the file layer

class Holder(object):
    """A stand-in state holder on the host."""
    _checkpoint_children = ("child", "other")

    def __init__(self, torch, size=4, child=None, other=None, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.size, self.child, self.other = size, child, other
        self.ring = torch.randint(0, 1 << 30, (size, 3), generator=g, dtype=torch.int64)
        self.flags = torch.randint(0, 255, (5,), generator=g, dtype=torch.uint8)
        self.value = torch.rand(size, generator=g, dtype=torch.float64)
        self.counter, self.gate, self.rate = 3 + seed, False, 0.5
        self.hooked = 0

    def _checkpoint_state(self):
        return (dict(size=self.size, shape=(self.size, 3), dtype=self.ring.dtype),
                dict(counter=self.counter, gate=self.gate, rate=self.rate),
                dict(ring=self.ring, flags=self.flags, value=self.value))

    def _checkpoint_loaded(self):
        self.hooked += 1


def _run(h, torch):
    """Something that moves every piece of state."""
    h.ring += 7
    h.flags ^= 0x55
    h.value *= 1.25
    h.counter += 10
    h.gate = True
    h.rate /= 3


def test_file_round_trip(tmp_path):
    import torch
    from safelife_amd import checkpoint
    shared = Holder(torch, seed=9)
    a = Holder(torch, child=Holder(torch, 6, child=shared, seed=1), other=shared, seed=2)
    model = torch.nn.Linear(3, 2)
    opt = torch.optim.Adam(model.parameters(), lr=0.1)
    model(torch.ones(1, 3)).sum().backward()
    opt.step()
    for h in (a, a.child, shared):
        _run(h, torch)
    path = tmp_path / "a.data"
    digests = checkpoint.save(path, a, model=model, optimizer=opt, extra={"note": 5})
    assert sorted(os.listdir(tmp_path)) == ["a.data"]                       # no temporary file is left
    assert digests == checkpoint.state_digest(a)
    assert digests["root/ring"] == ref.digest(a.ring.numpy()) and digests["root.other/value"] == ref.digest(shared.value.numpy())
    assert checkpoint.state_digest(a, salt=3)["root/ring"] == ref.digest(a.ring.numpy(), 3)

    # a shared object is stored once, under the path that reaches it first
    captured = checkpoint.capture(a)
    assert sorted(captured) == ["root", "root.child", "root.other"]
    assert captured["root.other"]["tensors"]["ring"] is shared.ring
    blob = torch.load(path, weights_only=True)
    assert sorted(blob["objects"]) == sorted(captured) and blob["format"] == checkpoint.FORMAT_VERSION
    assert blob["objects"]["root"]["class"] == "Holder" and blob["objects"]["root"]["scalars"]["counter"] == 15

    shared2 = Holder(torch, seed=9)
    b = Holder(torch, child=Holder(torch, 6, child=shared2, seed=1), other=shared2, seed=2)
    model2 = torch.nn.Linear(3, 2)
    opt2 = torch.optim.Adam(model2.parameters(), lr=0.1)
    ptrs = {k: t.data_ptr() for k, t in checkpoint._flat(checkpoint._states(b)).items()}
    assert checkpoint.load(path, b, model=model2, optimizer=opt2) == {"note": 5}
    assert {k: t.data_ptr() for k, t in checkpoint._flat(checkpoint._states(b)).items()} == ptrs
    for x, y in ((a, b), (a.child, b.child), (shared, shared2)):
        assert torch.equal(x.ring, y.ring) and torch.equal(x.flags, y.flags) and torch.equal(x.value, y.value)
        assert (x.counter, x.gate, x.rate) == (y.counter, y.gate, y.rate) and y.hooked == 1
        assert type(y.counter) is int and type(y.gate) is bool
    assert checkpoint.state_digest(b) == digests
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), model2.parameters()))
    s1, s2 = opt.state_dict()["state"], opt2.state_dict()["state"]
    assert all(torch.equal(s1[k]["exp_avg"], s2[k]["exp_avg"]) for k in s1)

    # going on from either ends in the same bits
    for h in (a, b):
        _run(h, torch)
    assert checkpoint.state_digest(a) == checkpoint.state_digest(b)


def _pair(torch, tmp_path, **kw):
    from safelife_amd import checkpoint
    a = Holder(torch, child=Holder(torch, 6, seed=1), seed=2)
    path = tmp_path / "a.data"
    checkpoint.save(path, a)
    return a, path, Holder(torch, child=Holder(torch, kw.get("child_size", 6), seed=1), seed=2)


def test_a_config_mismatch_names_the_object_and_the_field(tmp_path):
    import torch
    from safelife_amd import checkpoint
    a, path, b = _pair(torch, tmp_path, child_size=7)
    before = b.child.ring.clone(), b.ring.clone()
    with pytest.raises(ValueError, match=r"root\.child: shape is \[7, 3\] here and \[6, 3\] in the file"):
        checkpoint.load(path, b)
    assert torch.equal(b.child.ring, before[0]) and torch.equal(b.ring, before[1]) and b.hooked == 0    # nothing was touched
    with pytest.raises(ValueError, match="root.child.*no counterpart"):
        checkpoint.load(path, Holder(torch, seed=2))
    with pytest.raises(ValueError, match="holds no object of that name"):
        checkpoint.load(path, Holder(torch, child=Holder(torch, 6, child=Holder(torch), seed=1), seed=2))

    class Other(Holder):
        pass

    with pytest.raises(ValueError, match="root: class is Other here and Holder in the file"):
        checkpoint.load(path, Other(torch, child=Holder(torch, 6, seed=1), seed=2))
    with pytest.raises(ValueError, match="the models"):
        checkpoint.load(path, b, model=torch.nn.Linear(2, 2))


def test_a_flipped_byte_in_a_saved_tensor_names_the_tensor(tmp_path):
    import torch
    from safelife_amd import checkpoint
    a, path, b = _pair(torch, tmp_path)
    checkpoint.load(path, b)                                        # the file is good
    blob = torch.load(path, weights_only=True)
    blob["objects"]["root.child"]["tensors"]["flags"][2] ^= 0x10
    torch.save(blob, path)
    with pytest.raises(ValueError, match=r"root\.child/flags does not match its digest"):
        checkpoint.load(path, b)


def test_an_unknown_format_version_is_refused(tmp_path):
    import torch
    from safelife_amd import checkpoint
    a, path, b = _pair(torch, tmp_path)
    blob = torch.load(path, weights_only=True)
    blob["format"] = checkpoint.FORMAT_VERSION + 1
    torch.save(blob, path)
    with pytest.raises(ValueError, match="format version %d" % (checkpoint.FORMAT_VERSION + 1)):
        checkpoint.load(path, b)
    blob["format"], blob["abi"] = checkpoint.FORMAT_VERSION, 12
    torch.save(blob, path)
    with pytest.raises(ValueError, match="ABI version 12"):
        checkpoint.load(path, b)


def test_a_failing_save_leaves_the_previous_file(tmp_path, monkeypatch):
    import torch
    from safelife_amd import checkpoint
    a, path, b = _pair(torch, tmp_path)
    good = path.read_bytes()
    _run(a, torch)
    real = torch.save

    def failing(blob, f, *args, **kw):
        f.write(b"half a file")
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", failing)
    with pytest.raises(OSError, match="disk full"):
        checkpoint.save(path, a)
    monkeypatch.setattr(torch, "save", real)
    assert path.read_bytes() == good and sorted(os.listdir(tmp_path)) == ["a.data"]
    checkpoint.load(path, b)
    assert b.counter == 5


def test_a_tensor_that_is_not_contiguous_is_refused(tmp_path):
    import torch
    from safelife_amd import checkpoint
    a = Holder(torch)
    a.ring = a.ring.t()
    with pytest.raises(ValueError, match="root/ring is not contiguous"):
        checkpoint.save(tmp_path / "a.data", a)
    with pytest.raises(ValueError, match="names no state"):
        checkpoint.capture(object())


# --------------------------------------------------------------------------------------------------------- the refusals

def test_each_refusal_has_its_message():
    from safelife_amd import checkpoint
    ns = types.SimpleNamespace
    pool = ns(refreshable=False)
    checkpoint.refuse_env(ns(pool=pool, _se=None, _pool_refresh=None))
    checkpoint.refuse_env(ns(pool=pool, _se={"deferred": None, "last_done": None}, _pool_refresh=None))
    event = object()
    checkpoint.refuse_env(ns(pool=pool, _se={"deferred": None, "last_done": event, "joined": event}, _pool_refresh=None))
    with pytest.raises(ValueError, match="not joined"):        # (a batch launched behind the one that was joined)
        checkpoint.refuse_env(ns(pool=pool, _se={"last_done": object(), "joined": event}, _pool_refresh=None))
    with pytest.raises(ValueError, match=r"launched .* and not joined: call env.side_effects_join\(\) first"):
        checkpoint.refuse_env(ns(pool=pool, _se={"deferred": None, "last_done": object()}, _pool_refresh=None))
    with pytest.raises(ValueError, match=r"not joined"):
        checkpoint.refuse_env(ns(pool=pool, _se={"deferred": lambda: None}, _pool_refresh=None))
    with pytest.raises(ValueError, match=r"a pool write is staged: call env.pool_commit\(\) first"):
        checkpoint.refuse_env(ns(pool=pool, _se=None, _pool_refresh={"staged": object()}))
    with pytest.raises(ValueError, match=r"LevelPool\(refreshable=True\) is not checkpointed.*without refreshable=True"):
        checkpoint.refuse_env(ns(pool=ns(refreshable=True), _se=None, _pool_refresh={"staged": None}))
    checkpoint.refuse_run(ns(_live=False))
    with pytest.raises(ValueError, match=r"EpisodeRun is live \(mid test\): let run_episodes\(\) finish first"):
        checkpoint.refuse_run(ns(_live=True))
    checkpoint.refuse_runner(ns(generator=None, seed=5))
    with pytest.raises(ValueError, match=r"VectorRunner\(seed=None\) draws from torch's global generator.*build it with seed="):
        checkpoint.refuse_runner(ns(generator=None, seed=None))
    PipelinedRunner = type("PipelinedRunner", (), {})
    with pytest.raises(ValueError, match="PipelinedRunner is not checkpointed.*use a VectorRunner"):
        checkpoint.refuse_runner(PipelinedRunner())
    with pytest.raises(ValueError, match="PipelinedRunner is not checkpointed"):
        checkpoint.capture(PipelinedRunner())


# ------------------------------------------------------------------------------------------------- DQNTrainer without tests

class _Runner(object):
    def __init__(self, B):
        self.num_steps, self.B, self.epsilons = 0, B, []

    def collect(self, steps, epsilon, replay):
        assert steps == 1
        self.epsilons.append(epsilon)
        replay.rows += self.B
        self.num_steps += self.B


class _Replay(object):
    rows, gamma, multi_step = 0, 0.97, 2

    def __len__(self):
        return self.rows


def _trainer(**kw):
    from safelife_amd import dqn
    t = dqn.DQNTrainer(_Runner(5), _Replay(), None, None, None, optimize_interval=10, target_update_interval=35,
                       report_interval=25, replay_initial=60, epsilon_schedule=lambda n: 1.0 - n / 1000.0, record_events=True,
                       **kw)
    t.optimized = []
    t.optimize = lambda report: t.optimized.append(report)
    t.update_target = lambda: None
    return t


def test_events_without_a_test_runner_are_today_s():
    """The five-tuples of the events, by the schedule model of the existing DQN train fixture's tests."""
    from tests import dqn_loss_ref
    t = _trainer()
    t.train(200), t.train(100)
    case = dict(num_envs=5, start=0, capacity=10 ** 6, train_calls=[200, 100], pushes=[5] * 60, optimize_interval=10,
                target_update_interval=35, report_interval=25, replay_initial=60)
    assert t.events == dqn_loss_ref.schedule_model(case, t.epsilon_schedule)
    assert t.tests_run == [] and t.test_runner is None and t.checkpointer is None
    assert all(len(e) == 5 for e in t.events)


def test_dqn_tests_and_checkpoints_follow_the_fixture(tmp_path, monkeypatch):
    """DQNTrainer over stand-ins, with a recording checkpointer and test runner: the saves, the test steps and the epsilon
    the test runner saw are the reference's; the events are those of the run without either."""
    from safelife_amd import checkpoint
    for c in (c for c in CASES if c["kind"] == "dqn" and c["reload_after"] < 0):
        rec = _Recorder(monkeypatch)
        directory = tmp_path / c["name"]
        ck = checkpoint.Checkpointer(directory, interval=c["interval"], keep=c["keep"])
        seen = []
        kw = {}
        if c["test_interval"]:
            kw = dict(test_interval=c["test_interval"], epsilon_testing=c["eps_testing"],
                      test_runner=types.SimpleNamespace(run_episodes=lambda epsilon: seen.append((t.num_steps, epsilon, t.epsilon))))
        t = _trainer(checkpointer=ck, **kw)
        t.replay_initial = c["replay_initial"]
        assert ck.root is t and sorted(ck.model) == ["target_model", "training_model"]
        plain = _trainer()
        plain.replay_initial = c["replay_initial"]
        for steps in c["calls"]:
            t.train(steps), plain.train(steps)
        assert rec.saved == c["saves"] == ck.saved, c["name"]
        assert sorted(os.listdir(directory)) == c["left"]
        assert t.tests_run == c["test_steps"] and [s[0] for s in seen] == c["test_steps"]
        assert [s[1] for s in seen] == c["test_eps"] and [s[2] for s in seen] == c["test_eps"]
        assert t.events == plain.events and t.runner.epsilons == plain.runner.epsilons
        if c["test_steps"] and c["test_steps"][-1] == t.num_steps:
            assert t.epsilon == c["eps_testing"]                    # it stays there until the next iteration sets it
