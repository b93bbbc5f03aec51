"""
Checkpoints of device training runs: a run that is saved, rebuilt from nothing and resumed ends in the same bits as the run
that never stopped.

The reference checkpoints every 100 000 steps (training/base_algo.py:74-139: ``checkpoint_attribs`` -- the models', the
optimiser's ``state_dict()`` and ``num_steps`` -- into ``checkpoint-<num_steps>.data``, the newest few kept).  Its envs are
Python objects that simply start fresh episodes after a restart.  Here a run is far more than its models: the env batch with
its per-env PCG64 words, the wrapper state, the finished-episode queue, a level schedule's rings and successor table, the
episode log's rows and Polyak weights, the history slots, the draw counters, the agent state of the multi-agent runners,
DQN's replay ring and n-step window.  All of it lives in device tensors whose ``data_ptr()`` a C struct took at construction.

This module is the ONE mechanism.  A stateful class only NAMES its state:

    ``_checkpoint_state()``   -> ``(config, scalars, tensors)``: ``config`` is what must match for a load to make sense
                              (shapes, counts, dtypes, capacities, construction seeds, the pool's digest), ``scalars`` the
                              Python numbers that move during a run, keyed by ATTRIBUTE name (``load`` puts them back with
                              ``setattr``), ``tensors`` name -> contiguous tensor.  It raises ValueError where the object
                              cannot be checkpointed now (the refusals below).
    ``_checkpoint_children``  attribute names of the state holders attached to it (None values are skipped)
    ``_checkpoint_loaded()``  optional: rebuild what is DERIVED from the state just loaded

What is state: whatever the next step reads and the constructor does not rebuild from its arguments -- the observation the
runner will hand the model, ``pool_scalars`` under a level schedule (it rewrites the required points), the successor table.
What is derived and left out: the pool's boards, ``pool_ready``, ``score_lut``, the movement table, the goal-word cache (a
load invalidates it).

``load`` copies IN PLACE (``tensor.copy_``): no tensor is rebound, so every struct keeps pointing at live memory.

``state_digest`` fingerprints every state tensor on the device in ONE ``slhip_state_digest`` call (sl_digest.hip: a 64-bit
integrity checksum, NOT a cryptographic hash); ``save`` stores the digests, ``load`` digests what it uploaded and compares.
Tensors on the host (a holder that keeps none on the device) are digested by the same definition in numpy.

Refusals, each a ValueError that says what to do first: a side-effect batch launched and not joined, a staged pool write, a
live ``EpisodeRun``, a ``VectorRunner(seed=None)``, a ``LevelPool(refreshable=True)``, a ``PipelinedRunner``.

A checkpoint is ONE rank's: ``env_offset`` is part of the config check.
"""
import ctypes as C
import hashlib
import os
import re

import numpy as np

from . import _hip

FORMAT_VERSION = 1

_M64 = (1 << 64) - 1
_G = 0x9E3779B97F4A7C15


# ------------------------------------------------------------------------------------------------------------- the digest

def _mix(z):
    """splitmix64's finaliser on a numpy uint64 array."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _mix_int(z):
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def digest_bytes(data, salt=0):
    """The digest of host bytes (``bytes`` or a numpy array, read as its bytes): the definition in include/safelife_hip.h
    next to ``slhip_state_digest``, in numpy."""
    raw = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    n = int(raw.size)
    words = np.zeros((n + 7) // 8 * 8, np.uint8)
    words[:n] = raw
    w = words.view("<u8").astype(np.uint64)
    salt = int(salt) & _M64
    with np.errstate(over="ignore"):
        k = np.uint64(_mix_int(salt)) + np.arange(1, len(w) + 1, dtype=np.uint64) * np.uint64(_G)
        acc = int(_mix(w + k).sum(dtype=np.uint64)) if len(w) else 0
    return _mix_int(acc + _mix_int((salt ^ n) + _G))


def digest_segments(segments, salt=0, device=None):
    """``slhip_state_digest`` over ``[(device pointer, bytes), ...]`` -> the list of digests: one upload (the segment table
    and the chunk prefix), the chunk pass and its finish, one read-back.  The pointers may have any byte alignment."""
    import torch
    n = len(segments)
    if n == 0:
        return []
    lib = _hip.lib()
    dev = _hip.device() if device is None else device
    sizes = (C.c_ulonglong * n)(*[int(b) for _, b in segments])
    ws_words = int(lib.slhip_state_digest_workspace_bytes(sizes, n)) // 8
    # one buffer: segment table [n, 2] | workspace (prefix [n + 1], then the kernels' slab) | out [n]
    host = np.zeros(3 * n + 1, np.uint64)
    host[0:2 * n:2] = [int(p) for p, _ in segments]
    host[1:2 * n:2] = [int(b) for _, b in segments]
    _hip.check(lib.slhip_state_digest_prefix(sizes, n, host[2 * n:].ctypes.data_as(C.c_void_p)))
    buf = torch.empty(2 * n + ws_words + n, dtype=torch.int64, device=dev)
    buf[:3 * n + 1].copy_(torch.from_numpy(host.view(np.int64)))
    base = buf.data_ptr()
    out = buf[2 * n + ws_words:]
    _hip.check(lib.slhip_state_digest(C.c_void_p(base), n, int(salt) & _M64, C.c_void_p(out.data_ptr()),
                                      C.c_void_p(base + 16 * n), _hip.current_stream_ptr()))
    return [int(v) for v in out.cpu().numpy().view(np.uint64)]


def _digest_tensors(tensors, salt=0):
    """name -> digest for name -> tensor: the device tensors in ONE ``slhip_state_digest`` call, host tensors in numpy."""
    import torch
    out, names, segments, dev = {}, [], [], None
    for name, t in tensors.items():
        if t.is_cuda:
            names.append(name)
            segments.append((t.data_ptr() if t.numel() else 0, t.numel() * t.element_size()))
            dev = t.device
        else:
            out[name] = digest_bytes(t.detach().view(-1).view(torch.uint8).numpy(), salt)
    if names:
        out.update(zip(names, digest_segments(segments, salt, dev)))
    return {name: out[name] for name in tensors}


# ------------------------------------------------------------------------------------------------------------- refusals

def pool_digest(pool):
    """A fingerprint of a ``LevelPool``'s level arrays (part of an env's config: a checkpoint resumes on the SAME levels)."""
    cached = getattr(pool, "_checkpoint_digest", None)     # (a pool that can be checkpointed never changes: refuse_pool)
    if cached is not None:
        return cached
    h = hashlib.sha1()
    arrays = pool.arrays()
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        h.update(("%s %s %s;" % (k, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    if not getattr(pool, "refreshable", False):
        pool._checkpoint_digest = h.hexdigest()
    return h.hexdigest()


def refuse_pool(pool):
    if getattr(pool, "refreshable", False):
        raise ValueError("checkpoint: a LevelPool(refreshable=True) is not checkpointed -- its contents are the caller's "
                         "(replace / pool_stage): build the pool without refreshable=True, or save the levels yourself")


def refuse_env(env):
    """What keeps a ``SafeLifeVectorEnv`` from being saved or loaded now."""
    se = getattr(env, "_se", None)
    if se is not None and (se.get("deferred") is not None or se.get("last_done") is not se.get("joined")):
        raise ValueError("checkpoint: a side-effect batch was launched (side_effects_flush(overlap=True)) and not joined: "
                         "call env.side_effects_join() first")
    rf = getattr(env, "_pool_refresh", None)
    if rf is not None and rf.get("staged") is not None:
        raise ValueError("checkpoint: a pool write is staged: call env.pool_commit() first")
    refuse_pool(env.pool)


def refuse_run(run):
    """A run that was started and still has tickets to play (one 4-byte read of its counters when it was ever started)."""
    if getattr(run, "_live", False) and not getattr(run, "finished", lambda: False)():
        raise ValueError("checkpoint: an EpisodeRun is live (mid test): let run_episodes() finish first -- a checkpoint "
                         "is taken between tests, as the reference's is")


def refuse_runner(runner):
    name = type(runner).__name__
    if name == "PipelinedRunner":
        raise ValueError("checkpoint: a PipelinedRunner is not checkpointed (its groups run on streams of their own): "
                         "use a VectorRunner")
    if hasattr(runner, "generator") and getattr(runner, "seed", None) is None:
        raise ValueError("checkpoint: VectorRunner(seed=None) draws from torch's global generator, which is not part of "
                         "a checkpoint: build it with seed=")


# ------------------------------------------------------------------------------------------------------------- the walk

def _walk(root, name="root"):
    """Every state holder reachable from ``root`` through ``_checkpoint_children``, shared objects once, under the
    shortest attribute path that reaches them (breadth first: an object's direct children before their own)."""
    found, seen, queue = {}, set(), [(name, root)]
    while queue:
        name, obj = queue.pop(0)
        if id(obj) in seen:
            continue
        seen.add(id(obj))
        if type(obj).__name__ == "PipelinedRunner":
            refuse_runner(obj)
        if not hasattr(obj, "_checkpoint_state"):
            raise ValueError("checkpoint: %s (%s) names no state (_checkpoint_state)" % (name, type(obj).__name__))
        found[name] = obj
        for attr in getattr(obj, "_checkpoint_children", ()):
            child = getattr(obj, attr, None)
            if child is not None:
                queue.append(("%s.%s" % (name, attr.lstrip("_")), child))
    return found


def _plain(v):
    """A config or scalar value as what ``torch.load(weights_only=True)`` hands back: tuples become lists."""
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (bool, int, float, str)) or v is None:
        return v
    if isinstance(v, (np.integer, np.bool_)):
        return int(v)
    if isinstance(v, np.floating):
        return float(v)
    if type(v).__module__ == "torch" and type(v).__name__ == "dtype":
        return str(v)
    raise ValueError("checkpoint: a config or scalar value of type %s cannot be stored and compared: name it as numbers, "
                     "strings, lists or dicts of those" % type(v).__name__)


def _states(root):
    """name -> (object, config, scalars, tensors), the tensors checked."""
    out = {}
    for name, obj in _walk(root).items():
        config, scalars, tensors = obj._checkpoint_state()
        for k, t in tensors.items():
            if not t.is_contiguous():
                raise ValueError("checkpoint: %s/%s is not contiguous: name the tensor that owns the memory" % (name, k))
        out[name] = (obj, _plain(config), _plain(scalars), dict(tensors))
    return out


def capture(root):
    """Walks from a trainer, runner or env to everything attached -- the env's schedule, log, run and history, the trainer's
    replay, ``test_runner`` and its env -- and returns ``{name: {"class", "config", "scalars", "tensors"}}`` under stable
    names (attribute paths from ``root``); shared objects appear once.  The tensors are the LIVE device tensors."""
    return {name: {"class": type(obj).__name__, "config": config, "scalars": scalars, "tensors": tensors}
            for name, (obj, config, scalars, tensors) in _states(root).items()}


def _flat(states):
    return {"%s/%s" % (name, k): t for name, (_, _, _, tensors) in states.items() for k, t in tensors.items()}


def state_digest(root, salt=0):
    """``{"<object>/<tensor>": int}`` of every state tensor reachable from ``root``, in one launch: the public way to compare
    two runs (resumed against straight, rank against rank, today against yesterday).  An integrity checksum, not a
    cryptographic hash."""
    return _digest_tensors(_flat(_states(root)), salt)


# ------------------------------------------------------------------------------------------------------------- files

def _named(what, default):
    """``model=`` / ``optimizer=``: None, one object with ``state_dict()``, or a dict of them -> a dict."""
    if what is None:
        return {}
    if isinstance(what, dict):
        return dict(what)
    return {default: what}


def save(path, root, model=None, optimizer=None, extra=None):
    """Writes one checkpoint of ``root`` and everything attached (``capture``) to ``path``: the env is settled (each holder's
    ``_checkpoint_state`` does it), every tensor is digested on the device in one call and copied to the host, and ONE dict
    goes through ``torch.save`` -- format and ABI version, per object its class name, config, scalars, tensors and digests,
    and the ``state_dict()`` of the models and the optimiser (one, or a dict of them by name), as the reference's
    ``checkpoint_attribs``.  ``extra``: anything ``torch.load(weights_only=True)`` reads back.  The file is written under a
    temporary name and moved over ``path`` with ``os.replace``: a failing save leaves the previous file.  Returns the
    digests."""
    import torch
    states = _states(root)
    digests = _digest_tensors(_flat(states), 0)
    objects = {}
    for name, (obj, config, scalars, tensors) in states.items():
        objects[name] = {"class": type(obj).__name__, "config": config, "scalars": scalars,
                         "tensors": {k: t.detach().cpu() for k, t in tensors.items()},
                         "digests": {k: "%016x" % digests["%s/%s" % (name, k)] for k in tensors}}
    blob = {"format": FORMAT_VERSION, "abi": _hip.SL_ABI_VERSION, "objects": objects,
            "models": {k: m.state_dict() for k, m in _named(model, "model").items()},
            "optimizers": {k: o.state_dict() for k, o in _named(optimizer, "optimizer").items()},
            "extra": extra}
    path = os.fspath(path)
    tmp = "%s.tmp-%d" % (path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            torch.save(blob, f)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return digests


def _read(path):
    import torch
    blob = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    if not isinstance(blob, dict) or blob.get("format") != FORMAT_VERSION:
        raise ValueError("checkpoint: %s has format version %r, this package reads %d"
                         % (path, blob.get("format") if isinstance(blob, dict) else None, FORMAT_VERSION))
    if blob.get("abi") != _hip.SL_ABI_VERSION:
        raise ValueError("checkpoint: %s was written under ABI version %r, this package is %d: the state structs differ"
                         % (path, blob.get("abi"), _hip.SL_ABI_VERSION))
    return blob


def load(path, root, model=None, optimizer=None):
    """Reads ``path`` (``weights_only=True``) into ``root`` and everything attached.  The caller has REBUILT the objects with
    the same arguments and the same pool; nothing here constructs anything.  In this order: every object's class and config
    are compared with the file's (ValueError naming the object and the field that differs -- nothing has been touched yet);
    the tensors are copied IN PLACE (``tensor.copy_``: no tensor is rebound, every ``data_ptr()`` stays); the scalars are
    put back; the ``_checkpoint_loaded()`` hooks rebuild what is derived; the models and optimisers take their
    ``state_dict``; the device tensors are digested again and compared with the file's digests (ValueError naming the
    tensor).  Returns the file's ``extra``."""
    import torch
    blob = _read(path)
    states = _states(root)
    objects = blob["objects"]
    for name in states:
        if name not in objects:
            raise ValueError("checkpoint: %s: the file holds no object of that name (it holds %s)" % (name, sorted(objects)))
    for name in objects:
        if name not in states:
            raise ValueError("checkpoint: the file's object %s (%s) has no counterpart: rebuild the run as it was saved"
                             % (name, objects[name]["class"]))
    models, optimizers = _named(model, "model"), _named(optimizer, "optimizer")
    for kind, have, want in (("model", models, blob["models"]), ("optimizer", optimizers, blob["optimizers"])):
        if sorted(have) != sorted(want):
            raise ValueError("checkpoint: the file holds the %ss %s, load() was given %s" % (kind, sorted(want), sorted(have)))
    for name, (obj, config, scalars, tensors) in states.items():
        rec = objects[name]
        if rec["class"] != type(obj).__name__:
            raise ValueError("checkpoint: %s: class is %s here and %s in the file" % (name, type(obj).__name__, rec["class"]))
        for k in sorted(set(config) | set(rec["config"])):
            if k not in config or k not in rec["config"] or config[k] != rec["config"][k]:
                raise ValueError("checkpoint: %s: %s is %r here and %r in the file" % (name, k, config.get(k, "(absent)"),
                                                                                      rec["config"].get(k, "(absent)")))
        if sorted(tensors) != sorted(rec["tensors"]):
            odd = sorted(set(tensors) ^ set(rec["tensors"]))
            raise ValueError("checkpoint: %s: the state tensors differ from the file's: %s" % (name, odd))
        for k, t in tensors.items():
            src = rec["tensors"][k]
            if tuple(src.shape) != tuple(t.shape) or src.dtype != t.dtype:
                raise ValueError("checkpoint: %s/%s is %s %s here and %s %s in the file"
                                 % (name, k, t.dtype, tuple(t.shape), src.dtype, tuple(src.shape)))
    with torch.no_grad():
        for name, (obj, config, scalars, tensors) in states.items():
            rec = objects[name]
            for k, t in tensors.items():
                at = t.data_ptr()
                t.copy_(rec["tensors"][k])
                assert t.data_ptr() == at
            for k, v in rec["scalars"].items():
                setattr(obj, k, v)
    for name, (obj, _, _, _) in states.items():
        hook = getattr(obj, "_checkpoint_loaded", None)
        if hook is not None:
            hook()
    for k, m in models.items():
        m.load_state_dict(blob["models"][k])
    for k, o in optimizers.items():
        o.load_state_dict(blob["optimizers"][k])
    digests = _digest_tensors(_flat(states), 0)
    for name in states:
        for k, d in objects[name]["digests"].items():
            if "%016x" % digests["%s/%s" % (name, k)] != d:
                raise ValueError("checkpoint: %s/%s does not match its digest in %s (0x%016x here, 0x%s in the file): the "
                                 "file is damaged" % (name, k, path, digests["%s/%s" % (name, k)], d))
    return blob.get("extra")


# ------------------------------------------------------------------------------------------------------------- the schedule

class Checkpointer(object):
    """
    The reference's checkpoint schedule (``BaseAlgo``, training/base_algo.py:74-139) over ``save`` / ``load``.

    directory : where ``checkpoint-<num_steps>.data`` files live (created if missing)
    interval  : ``checkpoint_interval`` (100 000)
    keep      : ``max_checkpoints`` (3)
    root, model, optimizer : what ``save`` and ``load`` are given; the trainers fill in ``root`` (themselves) when it is None

    Files are sorted by the step parsed from their name; names that do not parse are ignored.  ``save_if_needed(num_steps)``
    saves when nothing was saved yet, or when ``last + interval < num_steps`` (strictly); after a save all but the newest
    ``keep`` files are deleted.  ``load_latest()`` / ``load(name)`` set ``last`` to the loaded file's step, as
    ``load_checkpoint`` does, so the first ``save_if_needed`` behind a load does not save.  ``saved`` lists the steps saved
    by this object, in order.
    """

    _NAME = re.compile(r"^checkpoint-(\d+)\.data$")

    def __init__(self, directory, interval=100000, keep=3, root=None, model=None, optimizer=None):
        self.directory, self.interval, self.keep = os.fspath(directory), int(interval), int(keep)
        self.root, self.model, self.optimizer = root, model, optimizer
        self.last = -1
        self.saved = []
        os.makedirs(self.directory, exist_ok=True)

    def files(self):
        """``[(num_steps, path), ...]`` in step order."""
        found = []
        for name in os.listdir(self.directory):
            m = self._NAME.match(name)
            if m:
                found.append((int(m.group(1)), os.path.join(self.directory, name)))
        return sorted(found)

    def due(self, num_steps):
        """``save_checkpoint_if_needed``'s condition: two integer comparisons.  The trainers ask it where the reference
        asks, and write the file at the end of the same iteration (see ``PPOTrainer`` / ``DQNTrainer``)."""
        return self.last < 0 or self.last + self.interval < num_steps

    def save_if_needed(self, num_steps):
        if self.due(num_steps):
            self.save(num_steps)
            return True
        return False

    def save(self, num_steps):
        num_steps = int(num_steps)
        path = os.path.join(self.directory, "checkpoint-%d.data" % num_steps)
        save(path, self.root, model=self.model, optimizer=self.optimizer, extra={"num_steps": num_steps})
        self.last = num_steps
        self.saved.append(num_steps)
        files = self.files()
        for _, old in files[:-self.keep]:          # (the reference's slice, old_checkpoints[:-max_checkpoints])
            os.remove(old)
        return path

    def load(self, name):
        """``name``: a file name, looked up inside the directory, or -- when it has a directory part -- a complete path
        (``load_checkpoint``'s rule, training/base_algo.py:110-115).  Returns ``num_steps``: the file's own, else the step
        in its name; a file that has neither is refused before anything is loaded."""
        name = os.fspath(name)
        path = name if os.path.dirname(name) else os.path.join(self.directory, name)
        if not os.path.exists(path):
            raise ValueError("checkpoint: there is no file %s" % path)
        m = self._NAME.match(os.path.basename(path))
        if m is None:       # (only then is the file read twice: the step must be known before anything is loaded)
            extra = _read(path).get("extra")
            if not (isinstance(extra, dict) and "num_steps" in extra):
                raise ValueError("checkpoint: %s says nowhere at which step it was taken (no num_steps inside, and its name "
                                 "is not checkpoint-<num_steps>.data)" % path)
        extra = load(path, self.root, model=self.model, optimizer=self.optimizer)
        self.last = int(extra["num_steps"]) if isinstance(extra, dict) and "num_steps" in extra else int(m.group(1))
        return self.last

    def load_latest(self):
        """Loads the file with the largest step; None (and nothing happens) when the directory holds none."""
        files = self.files()
        if not files:
            return None
        return self.load(files[-1][1])
