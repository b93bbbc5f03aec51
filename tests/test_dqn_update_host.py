"""The DQN update, the part that needs no GPU: the numpy restatement of the TD loss and its hand-written gradient
(tests/dqn_loss_ref.py) against what the reference's DQN.optimize and torch's autograd computed
(tests/golden/dqn_update_cases.npz), six deliberately wrong readings of the rule that the fixture must tell apart, the
schedule of DQN.train -- a pure-Python model and DQNTrainer itself, driven with stubs -- against the reference's recorded
events, sync_target against load_state_dict on CPU modules, and the C ABI: symbols, struct layout, argument errors (all
refused before anything touches a device).

Bounds of the float64 comparison -- measured; the bound is twice that, and never below four ulps of the value.  Over the
fixture's 29 cases the float64 restatement deviates from the reference's float64 run by at most 3.6e-16 relative in the loss
(the squares are added in numpy's order here and in torch's there) and not at all in the four report scalars, in td or in
the gradient.  In float32 td and the gradient are the reference's bit for bit."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from safelife_amd import _hip
from tests import dqn_loss_ref as ref
from tests import util

HAVE = os.path.exists(os.path.join(util.GOLDEN, "dqn_update_cases.npz"))
CASES = ref.load_cases() if HAVE else []
TRAIN = ref.load_train_cases() if HAVE else []
IDS = [c["id"] for c in CASES]

#: measured maximal deviation of the float64 restatement from the fixture's float64 run (the loss relative, the rest absolute)
MEASURED = dict(loss=3.6e-16, scalars=0.0, td=0.0, dq=0.0)


def within(got, want, measured, relative=False):
    """|got - want| <= max(2 * measured, 4 ulp of want), elementwise; what is not finite must be the same."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    finite = np.isfinite(want)
    if not np.array_equal(finite, np.isfinite(got)) or not ref.same_values(got[~finite], want[~finite]):
        return False
    got, want = got[finite], want[finite]
    floor = 4 * np.spacing(np.abs(want))
    bound = np.maximum(2 * measured * (np.abs(want) if relative else 1.0), floor)
    return bool(np.all(np.abs(got - want) <= bound))


def reproduces32(case, out):
    return ref.same_values(out["td"], case["td32"]) and ref.same_values(out["dq"], ref.full_gradient(case, "32"))


def test_fixture_covers_the_issue():
    assert os.path.getsize(os.path.join(util.GOLDEN, "dqn_update_cases.npz")) < 1024 * 1024
    plain = [c for c in CASES if not c["edge"]]
    assert {c["n"] for c in plain} == {1, 63, 64, 65, 257, 4099}
    assert {c["n_actions"] for c in plain} == {2, 9, 32}
    assert {(c["gamma"], c["multi_step"]) for c in plain} == {(0.97, 5), (0.9, 1), (0.99, 16)}
    for n in (1, 63, 64, 65, 257, 4099):
        assert {c["ring"] for c in plain if c["n"] == n} == {True, False}
    for hyper in ((0.97, 5), (0.9, 1), (0.99, 16)):
        assert {c["ring"] for c in plain if (c["gamma"], c["multi_step"]) == hyper} == {True, False}
    for c in plain:
        if c["ring"] and c["n"] > 1:        # n-step sums that float32 cannot hold
            assert np.any(c["reward"].astype(np.float32).astype(np.float64) != c["reward"])
    edges = {c["id"]: c for c in CASES if c["edge"]}
    for tag in ("ring", "batch"):
        assert edges["edge-all-done-" + tag]["done"].all() and not edges["edge-none-done-" + tag]["done"].any()
        assert edges["edge-n1-" + tag]["n"] == 1
        mixed = edges["edge-mixed-" + tag]
        top = mixed["next_q_values"].max(axis=1, keepdims=True)
        assert ((mixed["next_q_values"] == top).sum(axis=1) == 2).any()                     # a tied maximum
        assert (mixed["action"] != mixed["q_values"].argmax(axis=1)).any()                  # not the greedy column
        assert (mixed["td32"] == 0).any() and (mixed["td64"] == 0).any()
        assert np.isposinf(edges["edge-inf-" + tag]["next_q_values"]).any()
        assert np.isinf(edges["edge-inf-" + tag]["scalars32"][0])
        nan = edges["edge-nan-" + tag]
        assert np.isnan(nan["next_q_values"]).any() and np.isnan(nan["scalars32"][0])
        assert np.isnan(nan["td32"][nan["done"] == 1]).any() and np.isnan(nan["td32"][nan["done"] == 0]).any()
    for c in edges.values():                # dyadic: multiples of 2^-6 and a discount of 1/4
        assert c["gamma"] ** c["multi_step"] == 0.25
        for k in ("q_values", "next_q_values", "reward"):
            x = c[k][np.isfinite(c[k])]
            assert np.array_equal(x * 64, np.round(x * 64))
    for c in CASES:                         # no maximum that is a zero of both signs
        for k in ("q_values", "next_q_values"):
            x = c[k]
            at_top = (x == 0) & (np.nanmax(x, axis=1, keepdims=True) == 0)
            assert not np.any((at_top & np.signbit(x)).any(axis=1) & (at_top & ~np.signbit(x)).any(axis=1))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float64_restatement_reproduces_the_reference(case):
    out = ref.restate(case, np.float64)
    want = dict(td=case["td64"], dq=ref.full_gradient(case, "64"), loss=case["scalars64"][0], scalars=case["scalars64"][1:])
    got = dict(td=out["td"], dq=out["dq"], loss=out["scalars"][0], scalars=out["scalars"][1:])
    for name in ("td", "dq", "loss", "scalars"):
        with np.errstate(invalid="ignore"):
            dev = np.abs(np.asarray(got[name], np.float64) - want[name])
        dev = dev[np.isfinite(dev)]
        if name == "loss" and dev.size:
            dev = dev / abs(want[name])
        print("%s %s: max deviation %.3g" % (case["id"], name, dev.max() if dev.size else 0.0))
        assert within(got[name], want[name], MEASURED[name], relative=(name == "loss")), name


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float32_restatement_is_the_reference_bit_for_bit(case):
    out = ref.restate(case, np.float32)
    assert out["td"].dtype == out["dq"].dtype == np.float32
    assert ref.same_values(out["td"], case["td32"])
    assert ref.same_values(out["dq"], ref.full_gradient(case, "32"))


@pytest.mark.parametrize("variant", ref.WRONG_VARIANTS)
def test_fixture_tells_a_wrong_reading_apart(variant):
    failing = []
    with np.errstate(all="ignore"):
        for c in CASES:
            if not reproduces32(c, ref.restate(c, np.float32, **{variant: True})):
                failing.append(c["id"])
            assert reproduces32(c, ref.restate(c, np.float32))
    print(variant, "fails on", failing)
    assert failing, variant


def test_fma_and_late_rounding_change_rows_of_the_fixture():
    """What the generator verified when it wrote the fixture, once more on the fixture as it is."""
    with np.errstate(all="ignore"):
        for variant, only_ring in (("fused_multiply_add", False), ("late_reward_rounding", True)):
            rows = 0
            for c in CASES:
                td = ref.restate(c, np.float32, **{variant: True})["td"]
                changed = ~((td == c["td32"]) | (np.isnan(td) & np.isnan(c["td32"])))
                assert not (only_ring and not c["ring"] and changed.any())
                rows += int(changed.sum())
            print(variant, "changes", rows, "rows")
            assert rows > 0


def test_grad_loss_and_grad_td_in_the_restatement():
    c = next(c for c in CASES if c["id"].startswith("n65-a9"))
    one, half = ref.restate(c, np.float64), ref.restate(c, np.float64, grad_loss=0.5)
    assert np.array_equal(half["dq"], 0.5 * one["dq"])
    w = np.linspace(-1.0, 1.0, c["n"])
    both = ref.restate(c, np.float64, grad_td=w)
    want = np.zeros_like(one["dq"])
    want[np.arange(c["n"]), c["action"]] = w
    assert np.allclose(both["dq"] - one["dq"], want, rtol=0, atol=1e-15)


# --------------------------------------------------------------------------------------------------------- the schedule

def reference_spline():
    """The reference's epsilon spline: FITPACK's fit of the three points leaves every coefficient one ulp above its datum
    (dqn.EPSILON_COEFFICIENTS says why); LinearSchedule evaluates the spline those coefficients define."""
    from safelife_amd.schedule import LinearSchedule
    return LinearSchedule([5e4, 5e5, 4e6], [1.0000000000000002, 0.5000000000000001, 0.030000000000000002])


def test_the_data_points_themselves_are_told_apart():
    """A schedule through the data points instead of the fitted coefficients differs from the reference in the last bit."""
    from safelife_amd.schedule import LinearSchedule
    plain = LinearSchedule([5e4, 5e5, 4e6], [1, 0.5, 0.03])
    assert any(ref.schedule_model(c, plain) != c["events"] for c in TRAIN)
    assert all(abs(plain(e[0]) - e[1]) < 1e-4 for c in TRAIN for e in c["events"])


def test_train_fixture_covers_the_issue():
    assert {c["num_envs"] for c in TRAIN} == {1, 5, 16, 96}
    assert any(c["optimize_interval"] % c["num_envs"] and c["num_envs"] % c["optimize_interval"] for c in TRAIN)
    assert any(c["optimize_interval"] < c["num_envs"] for c in TRAIN)
    assert any(len(c["train_calls"]) == 2 for c in TRAIN)
    crossed = [c for c in TRAIN if c["replay_initial"] > 0 and any(e[2] for e in c["events"])]
    assert crossed and all(not c["events"][0][2] for c in crossed)
    assert any(c["capacity"] < c["replay_initial"] and not any(e[2] for e in c["events"]) for c in TRAIN)
    for knot in (50000, 500000, 4000000):   # epsilon was evaluated at num_steps BEFORE the step: below, on and above the knot
        before = {e[0] - c["num_envs"] for c in TRAIN for e in c["events"]}
        assert knot in before and any(knot - 20 < b < knot for b in before) and any(knot < b < knot + 20 for b in before)


@pytest.mark.parametrize("case", TRAIN, ids=[c["id"] for c in TRAIN])
def test_schedule_model_reproduces_the_reference(case):
    assert ref.schedule_model(case, reference_spline()) == case["events"]


@pytest.mark.parametrize("wrong", ("round_up_after_the_step", "report_flag_per_call_only"))
def test_schedule_model_tells_wrong_readings_apart(wrong):
    failing = [c["id"] for c in TRAIN if ref.schedule_model(c, reference_spline(), **{wrong: True}) != c["events"]]
    print(wrong, "fails on", failing)
    assert failing


class StubReplay(object):
    gamma, multi_step = 0.97, 5

    def __init__(self, case):
        self.case, self.pushed, self.k, self.reads = case, 0, 0, 0

    def add_step(self):
        self.pushed += self.case["pushes"][self.k]
        self.k += 1

    def __len__(self):
        self.reads += 1
        return min(self.pushed, self.case["capacity"])


class StubRunner(object):
    def __init__(self, case):
        self.num_steps = case["start"]
        self.env = types.SimpleNamespace(num_envs=case["num_envs"])
        self.epsilons = []

    def collect(self, steps, epsilon, replay):
        assert steps == 1
        self.epsilons.append(epsilon)
        replay.add_step()
        self.num_steps += self.env.num_envs


def stub_trainer(case, **kw):
    from safelife_amd import dqn
    calls = []

    class Recording(dqn.DQNTrainer):
        def optimize(self, report):
            calls.append(("optimize", self.num_steps, bool(report)))
            return "sums of %d" % self.num_steps

        def update_target(self):
            calls.append(("update", self.num_steps))

    replay, runner = StubReplay(case), StubRunner(case)
    trainer = Recording(runner, replay, None, None, None, optimize_interval=case["optimize_interval"],
                        target_update_interval=case["target_update_interval"], report_interval=case["report_interval"],
                        replay_initial=case["replay_initial"], record_events=True, **kw)
    return trainer, replay, runner, calls


@pytest.mark.parametrize("case", TRAIN, ids=[c["id"] for c in TRAIN])
def test_trainer_schedule_reproduces_the_reference(case):
    """DQNTrainer.train over a stub runner, replay and models: no device API is touched."""
    reports = []
    trainer, replay, runner, calls = stub_trainer(case, on_report=lambda *a: reports.append(a))
    for steps in case["train_calls"]:
        trainer.train(steps)
    assert trainer.events == case["events"]
    assert runner.epsilons == [e[1] for e in case["events"]]
    assert [c for c in calls if c[0] == "optimize"] == [("optimize", e[0], e[3]) for e in case["events"] if e[2]]
    assert [c for c in calls if c[0] == "update"] == [("update", e[0]) for e in case["events"] if e[4]]
    assert reports == [(e[0], e[1], "sums of %d" % e[0]) for e in case["events"] if e[3]]
    # the gate: one exact len() per step until it opens, none afterwards
    opened = [k for k, e in enumerate(case["events"])
              if min(sum(case["pushes"][:k + 1]), case["capacity"]) >= case["replay_initial"]]
    want_reads = (opened[0] + 1) if opened else len(case["events"])
    assert trainer.host_visits == replay.reads == want_reads


def test_trainer_without_record_events_keeps_no_list():
    case = TRAIN[0]
    trainer, _replay, _runner, calls = stub_trainer(case)
    trainer.record_events = False
    trainer.train(case["train_calls"][0])
    assert trainer.events == [] and calls


def test_default_epsilon_schedule_is_the_reference_spline():
    from safelife_amd import dqn
    case = next(c for c in TRAIN if c["id"] == "envs16-knot-500000")
    trainer = dqn.DQNTrainer(StubRunner(case), StubReplay(case), None, None, None)
    assert (trainer.training_batch_size, trainer.optimize_interval, trainer.target_update_interval,
            trainer.report_interval, trainer.replay_initial) == (96, 32, 10000, 256, 40000)
    for c in TRAIN:
        for steps, eps, *_ in c["events"]:
            assert trainer.epsilon_schedule(steps - c["num_envs"]) == eps
    assert dqn.round_up(64, 32) == 96 and dqn.round_up(65, 32) == 96 and dqn.round_up(0, 7) == 7
    with pytest.raises(ValueError):
        dqn.DQNTrainer(StubRunner(case), StubReplay(case), None, None, None, optimize_interval=0)


# ---------------------------------------------------------------------------------------------------------- sync_target

def _models(torch):
    def make(seed):
        torch.manual_seed(seed)
        m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(), torch.nn.Linear(36, 9))
        m(torch.randn(5, 3, 5, 5))          # moves the batch norm's running statistics and its step counter
        return m
    return make(1), make(2), make(2)


def test_sync_target_equals_load_state_dict_on_cpu():
    import torch
    from safelife_amd import dqn
    training, target, twin = _models(torch)
    training(torch.randn(7, 3, 5, 5))
    assert not all(torch.equal(a, b) for a, b in zip(training.state_dict().values(), target.state_dict().values()))
    before = {k: v.data_ptr() for k, v in target.state_dict().items()}
    dqn.sync_target(training, target)
    twin.load_state_dict(training.state_dict())
    got, want = target.state_dict(), twin.state_dict()
    assert list(got) == list(want) and any("num_batches_tracked" in k for k in got)
    for k in got:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
        assert got[k].data_ptr() == before[k]           # in place
        assert got[k].data_ptr() != training.state_dict()[k].data_ptr()
    assert all(p.requires_grad for p in target.parameters())
    x = torch.randn(3, 3, 5, 5)
    assert torch.equal(target.eval()(x), training.eval()(x))


def test_sync_target_refuses_models_that_differ():
    import torch
    from safelife_amd import dqn
    a = torch.nn.Linear(4, 3)
    with pytest.raises(ValueError, match="keys"):
        dqn.sync_target(a, torch.nn.Linear(4, 3, bias=False))
    with pytest.raises(ValueError, match="weight"):
        dqn.sync_target(a, torch.nn.Linear(5, 3))
    with pytest.raises(ValueError, match="keys"):
        dqn.sync_target(torch.nn.Sequential(a), a)


# ------------------------------------------------------------------------------------------------------ dqn_loss refusals

def test_dqn_loss_refuses_bad_arguments_before_any_launch():
    """CPU tensors stand in for every argument: each call is refused by the checks, in the order they are made."""
    import torch
    from safelife_amd import dqn
    from safelife_amd.replay import ReplayBatch
    q = torch.zeros(4, 9)
    batch = ReplayBatch(None, torch.zeros(4, dtype=torch.int64), torch.zeros(4), None, torch.zeros(4))
    with pytest.raises(ValueError, match="q_values must be a float32 tensor"):
        dqn.dqn_loss(q, q, batch)
    with pytest.raises(ValueError, match="q_values"):
        dqn.dqn_loss(np.zeros((4, 9), np.float32), q, batch)
    with pytest.raises(ValueError, match="q_values"):
        dqn.dqn_loss(q.double(), q, batch)
    assert dqn.dqn_loss.sums is None or torch.is_tensor(dqn.dqn_loss.sums)


# ------------------------------------------------------------------------------------------------------------- the ABI

NEW = ("slhip_dqn_workspace_bytes", "slhip_dqn_loss_forward", "slhip_dqn_loss_backward")


def test_symbols_and_version():
    lib = _hip.lib()
    header = open(os.path.join(util.REPO, "include", "safelife_hip.h")).read()
    for name in NEW:
        assert name in _hip.EXPORTS and hasattr(lib, name) and name + "(" in header
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13
    assert lib.slhip_dqn_workspace_bytes(1) == 40 and lib.slhip_dqn_workspace_bytes(256) == 40
    assert lib.slhip_dqn_workspace_bytes(257) == 80 and lib.slhip_dqn_workspace_bytes(0) == 0


def test_dqn_loss_layout_matches_header(tmp_path):
    """ctypes mirror of struct sl_dqn_loss against gcc's offsetof / sizeof, and the constants."""
    st = _hip.DqnLoss
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "safelife_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(sl_dqn_loss));',
             'printf("consts %d %d %d %d %d %d\\n", SL_DQN_BAD_ACTION, SL_DQN_BAD_INDEX, SL_DQN_FROM_RING, SL_DQN_FROM_BATCH, '
             'SL_DQN_SUMS, SL_DQN_SUM_LOSS_F32);',
             'printf("sums %d %d %d %d %d %d %d\\n", SL_DQN_SUM_LOSS, SL_DQN_SUM_Q_MODEL_MEAN, SL_DQN_SUM_Q_MODEL_MAX, '
             'SL_DQN_SUM_Q_TARGET_MEAN, SL_DQN_SUM_Q_TARGET_MAX, SL_DQN_SUM_N, SL_DQN_SUM_RESERVED);']
    want = ["size %d" % C.sizeof(st),
            "consts %d %d %d %d 8 %d" % (_hip.DQN_BAD_ACTION, _hip.DQN_BAD_INDEX, _hip.DQN_FROM_RING, _hip.DQN_FROM_BATCH,
                                         _hip.DQN_SUM_LOSS_F32),
            "sums " + " ".join(str(i) for i in range(len(_hip.DQN_SUMS)))]
    for name, ctype in st._fields_:
        lines.append('printf("%s %%zu %%zu\\n", offsetof(sl_dqn_loss, %s), sizeof(((sl_dqn_loss *)0)->%s));'
                     % (name, name, name))
        want.append("%s %d %d" % (name, getattr(st, name).offset, C.sizeof(ctype)))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(util.REPO, "include"), str(src), "-o", exe])
    got = [g for g in subprocess.check_output([exe]).decode().split("\n") if g]
    assert got == want
    assert C.sizeof(st) == 88
    assert _hip.DQN_SUMS == ("loss", "q_model_mean", "q_model_max", "q_target_mean", "q_target_max", "n", "reserved")


def _loss(**kw):
    """A description whose pointers are non-null but never dereferenced: every call below is refused first."""
    s = _hip.DqnLoss()
    s.n, s.N, s.n_actions, s.source, s.discount = 8, 32, 9, _hip.DQN_FROM_RING, 0.97 ** 5
    for name in ("q_values", "next_q_values", "action", "reward", "done", "index", "status"):
        setattr(s, name, 0x1000)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


BAD = [dict(n=0), dict(N=0), dict(n_actions=1), dict(n_actions=33), dict(source=2), dict(source=-1), dict(index=None),
       dict(q_values=None), dict(next_q_values=None), dict(action=None), dict(reward=None), dict(done=None),
       dict(status=None)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_bad_descriptions_are_refused_by_both(bad):
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    s = _loss(**bad)
    assert lib.slhip_dqn_loss_forward(C.byref(s), p, p, p, None) == _hip.SL_E_ARG
    assert b"dqn_loss" in lib.slhip_last_error()
    assert lib.slhip_dqn_loss_backward(C.byref(s), p, None, p, p, None) == _hip.SL_E_ARG
    assert b"dqn_loss" in lib.slhip_last_error()


def test_argument_errors():
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    s = _loss()
    assert lib.slhip_dqn_loss_forward(None, p, p, p, None) == _hip.SL_E_ARG
    for k in range(3):
        args = [p] * 3
        args[k] = None
        assert lib.slhip_dqn_loss_forward(C.byref(s), *args, None) == _hip.SL_E_ARG
        assert b"null pointer" in lib.slhip_last_error()
    assert lib.slhip_dqn_loss_forward(C.byref(s), p, C.c_void_p(0x1004), p, None) == _hip.SL_E_ARG
    assert b"aligned" in lib.slhip_last_error()
    for k in (0, 2, 3):                         # grad_td (1) may be null
        args = [p] * 4
        args[k] = None
        assert lib.slhip_dqn_loss_backward(C.byref(s), *args, None) == _hip.SL_E_ARG
        assert b"null pointer" in lib.slhip_last_error()
