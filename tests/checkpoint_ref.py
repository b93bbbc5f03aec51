"""Host models for safelife_amd/checkpoint.py, written from the issue's definitions and the reference's BaseAlgo
(training/base_algo.py:56-139, ppo.py:184-219, dqn.py:177-214).  Nothing here is shared with checkpoint.py.

``digest``           the state digest in numpy uint64 arithmetic (sl_digest.hip is held to it bit for bit)
``load_cases``       tests/golden/checkpoint_cases.npz: what the REFERENCE's trainers saved, kept and tested
``schedule_model``   the checkpoint schedule of a fixture case: the steps saved in order, the files left, DQN's test steps;
                     ``wrong=`` turns on one of five wrong readings, each of which must fail on the fixture
"""
import os
import re

import numpy as np

from tests import util

PATH = os.path.join(util.GOLDEN, "checkpoint_cases.npz")

MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
KNOWN = ((b"", 0, 0x48218226ff3cd4bf), (bytes(range(20)), 0, 0x0c817c4bd668decf), (bytes(range(20)), 7, 0x510af6e63ac50e25))


def mix(z):
    """splitmix64's finaliser on Python ints."""
    z &= MASK
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & MASK
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & MASK
    return z ^ (z >> 31)


def mix_array(z):
    z = z.copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def digest(data, salt=0):
    """data: bytes, or a numpy array read as its bytes in memory order."""
    if not isinstance(data, (bytes, bytearray)):
        data = np.ascontiguousarray(data).tobytes()
    n = len(data)
    padded = bytes(data) + b"\0" * (-n % 8)
    w = np.frombuffer(padded, dtype="<u8").astype(np.uint64)
    salt &= MASK
    acc = 0
    if len(w):
        with np.errstate(over="ignore"):
            index = np.arange(1, len(w) + 1, dtype=np.uint64)
            terms = mix_array(w + np.uint64(mix(salt)) + index * np.uint64(G))
            acc = int(np.add.reduce(terms, dtype=np.uint64))
    return mix(acc + mix((salt ^ n) + G))


def digest_slow(data, salt=0):
    """The same, word by word in Python ints (for short inputs): no numpy arithmetic at all."""
    n = len(data)
    acc = 0
    for i in range((n + 7) // 8):
        w = int.from_bytes(data[8 * i:8 * i + 8], "little")
        acc = (acc + mix(w + mix(salt) + (i + 1) * G)) & MASK
    return mix(acc + mix(((salt & MASK) ^ n) + G))


# ------------------------------------------------------------------------------------------------------------ the fixture

KINDS = ("ppo", "dqn")
PARAMS = ("kind", "num_envs", "steps_per_env", "interval", "keep", "reload_after", "replay_initial", "test_interval")


def load_cases():
    """One dict per schedule: ``name``, the PARAMS, ``calls`` (the `steps` of consecutive train() calls; a fresh object
    loads the newest checkpoint behind call ``reload_after``, -1: never), ``before`` (file names in the directory at the
    start, oldest first), ``saves`` (num_steps of every save in order), ``left`` (file names at the end, sorted),
    ``test_steps`` / ``test_eps`` (DQN: the steps at which run_episodes ran and the epsilon it saw), ``eps_testing``."""
    z = np.load(PATH)
    cases = []
    cut = lambda key, off, i: z[key][z[off][i]:z[off][i + 1]]      # noqa: E731
    for i, name in enumerate(z["name"]):
        c = dict(zip(PARAMS, (int(v) for v in z["params"][i])), name=str(name))
        c["kind"] = KINDS[c["kind"]]
        c["calls"] = [int(v) for v in cut("calls", "call_offsets", i)]
        c["saves"] = [int(v) for v in cut("saves", "save_offsets", i)]
        c["before"] = [str(v) for v in cut("before", "before_offsets", i)]
        c["left"] = sorted(str(v) for v in cut("left", "left_offsets", i))
        c["test_steps"] = [int(v) for v in cut("test_steps", "test_offsets", i)]
        c["test_eps"] = [float(v) for v in cut("test_eps", "test_offsets", i)]
        c["eps_testing"] = float(z["eps_testing"][i])
        cases.append(c)
    return cases


WRONG = ("le", "no_first_save", "prune_by_mtime", "keep_off_by_one", "load_leaves_last")
_NAME = re.compile(r"^checkpoint-(\d+)\.data$")


def round_up(x, r):
    return x + r - x % r


class _Directory(object):
    """File names with the order they were (last) written in."""

    def __init__(self, names):
        self.names = list(names)            # oldest first

    def write(self, name):
        if name in self.names:
            self.names.remove(name)
        self.names.append(name)

    def checkpoints(self, by_mtime):
        found = [(int(_NAME.match(n).group(1)), n) for n in self.names if _NAME.match(n)]
        return [n for _, n in (found if by_mtime else sorted(found))]


def schedule_model(case, wrong=None, replay_restored=False):
    """-> (saves, files left sorted, test steps, test epsilons).  ``replay_restored``: what a reload does to the replay
    buffer -- the reference does not checkpoint it, so its resumed run fills an empty buffer up to ``replay_initial`` again
    (False); this library's checkpoint holds the ring (True)."""
    assert wrong is None or wrong in WRONG
    directory = _Directory(case["before"])
    B, interval, keep = case["num_envs"], case["interval"], case["keep"]
    if wrong == "keep_off_by_one":
        keep += 1
    saves, test_steps, test_eps = [], [], []
    state = dict(num_steps=0, last=-1, pushed=0)
    pushes = iter(case["pushes"]) if "pushes" in case else None     # (rows pushed per step; default: one per env)
    capacity = case.get("capacity", 1 << 62)

    def save():
        directory.write("checkpoint-%d.data" % state["num_steps"])
        saves.append(state["num_steps"])
        files = directory.checkpoints(wrong == "prune_by_mtime")
        for old in files[:-keep]:
            directory.names.remove(old)
        state["last"] = state["num_steps"]

    def save_if_needed():
        if state["last"] < 0 and wrong != "no_first_save":
            save()
        elif state["last"] + interval < state["num_steps"] or (wrong == "le" and state["last"] + interval == state["num_steps"]):
            save()

    for k, steps in enumerate(case["calls"]):
        max_steps = state["num_steps"] + steps
        while state["num_steps"] < max_steps:
            before = state["num_steps"]
            if case["kind"] == "ppo":
                state["num_steps"] += B * case["steps_per_env"]
                save_if_needed()
                continue
            next_test = round_up(before, case["test_interval"]) if case["test_interval"] else None
            state["num_steps"] += B
            state["pushed"] += B if pushes is None else next(pushes)
            if min(state["pushed"], capacity) < case["replay_initial"]:
                continue
            save_if_needed()
            if next_test is not None and state["num_steps"] >= next_test:
                test_steps.append(state["num_steps"])
                test_eps.append(case["eps_testing"])
        save()
        if k == case["reload_after"]:
            # a fresh object: num_steps and the replay come back from the newest file, and `last` is set to its step
            newest = directory.checkpoints(False)[-1]
            state = dict(num_steps=int(_NAME.match(newest).group(1)), last=-1,
                         pushed=state["pushed"] if replay_restored else 0)
            if wrong != "load_leaves_last":
                state["last"] = state["num_steps"]
    return saves, sorted(directory.names), test_steps, test_eps
