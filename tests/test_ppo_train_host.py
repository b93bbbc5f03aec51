"""The PPO train loop and its report, the part that needs no GPU: the pure-Python model of PPO.train's schedule and the numpy
restatement of its report (tests/ppo_train_ref.py) against what the reference's own PPO.train did and logged
(tests/golden/ppo_train_cases.npz), five deliberately wrong readings that the fixture must tell apart, PPOTrainer itself
driven with stubs against the same events, and the C ABI of the report pass: symbols, workspace sizes, refusals (all made
before anything touches a device).

Bounds of the float64 comparison -- measured; the bound is twice that, and never below four ulps of the value.  Over the
fixture's 28 report cases the float64 restatement deviates from the reference's float64 run by at most 2.2e-16 relative in
the loss and 3.7e-16 relative in the entropy (the rows are added in numpy's order here and in torch's there), and not at all
in the means of values and advantages."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from safelife_amd import _hip
from tests import ppo_train_ref as ref
from tests import util

HAVE = os.path.exists(ref.PATH)
TRAIN = ref.load_train_cases() if HAVE else []
REPORTS = ref.load_report_cases() if HAVE else []

#: measured maximal relative deviation of the float64 restatement from the fixture's float64 run, per scalar
MEASURED = dict(loss=2.2e-16, entropy=3.7e-16, values=0.0, advantages=0.0)


def within(got, want, measured):
    """|got - want| <= max(2 * measured * |want|, 4 ulp of want)."""
    return abs(got - want) <= max(2 * measured * abs(want), 4 * np.spacing(abs(want)))


def test_fixture_covers_the_issue():
    assert os.path.getsize(ref.PATH) < 1024 * 1024
    assert {c["num_envs"] for c in TRAIN} == {1, 5, 16, 96} and {c["steps_per_env"] for c in TRAIN} == {1, 7, 20}
    per_batch = lambda c: c["num_envs"] * c["steps_per_env"]                                                # noqa: E731
    assert any(c["report_interval"] % per_batch(c) and per_batch(c) % c["report_interval"] for c in TRAIN)
    assert any(c["test_interval"] % per_batch(c) and per_batch(c) % c["test_interval"] for c in TRAIN)
    # num_steps lands ON a multiple of the interval: the "strictly above" case of round_up
    assert any(c["report_interval"] % per_batch(c) == 0 and c["start"] % per_batch(c) == 0 for c in TRAIN)
    assert any(c["test_interval"] % per_batch(c) == 0 and c["start"] % per_batch(c) == 0 for c in TRAIN)
    assert any(c["start"] % c["report_interval"] for c in TRAIN)
    assert any(c["start"] and c["start"] % c["report_interval"] == 0 for c in TRAIN)
    assert any(len(c["train_calls"]) == 2 for c in TRAIN)
    assert any(not c["has_logger"] for c in TRAIN) and any(not c["has_testing"] for c in TRAIN)
    for c in TRAIN:                     # every kind of iteration somewhere: a report, a test, both, neither
        assert c["has_logger"] == any(e[1] for e in c["events"])
    kinds = {(e[1], e[2]) for c in TRAIN for e in c["events"]}
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    plain = [c for c in REPORTS if not c["edge"]]
    assert {(c["n"], c["n_actions"]) for c in plain} == {(n, A) for n in (1, 63, 64, 65, 255, 256, 257, 4099)
                                                         for A in (2, 9, 32)}
    edges = {c["id"]: c for c in REPORTS if c["edge"]}
    at, over = edges["edge-entropy-at-clip"], edges["edge-entropy-over-clip"]
    assert at["scalars32"][1] == 0.0 == at["hyper"][4]
    assert 0 < over["scalars32"][1] - over["hyper"][4] < 1e-6 and 0 < over["scalars64"][1] - over["hyper"][4] < 1e-6
    assert not edges["edge-advantages-zero"]["advantages"].any() and edges["edge-advantages-zero"]["scalars32"][3] == 0
    cancel = edges["edge-values-cancel"]
    assert cancel["scalars64"][2] == 0.5 and cancel["scalars32"][2] != 0.5         # float32 lost the ones
    for c in edges.values():            # dyadic: multiples of 2^-6
        for k in ("values", "old_values", "returns", "advantages", "action_prob", "policy"):
            assert np.array_equal(c[k] * 64, np.round(c[k] * 64)), (c["id"], k)


@pytest.mark.parametrize("case", TRAIN, ids=[c["id"] for c in TRAIN])
def test_schedule_model_reproduces_the_reference(case):
    assert ref.schedule_model(case) == case["events"]


@pytest.mark.parametrize("case", REPORTS, ids=[c["id"] for c in REPORTS])
def test_float64_report_reproduces_the_reference(case):
    got = ref.report(case, np.float64)
    for k, name in enumerate(ref.SCALARS):
        want = case["scalars64"][k]
        print("%s %s: deviation %.3g (relative %.3g)" % (case["id"], name, abs(got[k] - want),
                                                         abs(got[k] - want) / abs(want) if want else 0.0))
        assert within(got[k], want, MEASURED[name]), name


@pytest.mark.parametrize("wrong", ref.WRONG_SCHEDULES)
def test_fixture_tells_a_wrong_schedule_apart(wrong):
    """round_up taken after the batch; `>` instead of `>=`; a round_up that leaves an exact multiple where it is; the report
    made without a logger."""
    failing = [c["id"] for c in TRAIN if ref.schedule_model(c, **{wrong: True}) != c["events"]]
    print(wrong, "fails on", failing)
    assert failing


def test_fixture_tells_means_over_the_last_minibatch_apart():
    """The report is calculate_loss over the WHOLE batch, not what train_batch's last minibatch left behind."""
    failing = []
    for c in REPORTS:
        got = ref.report(c, np.float64, means_over_the_last_minibatch=True)
        if not all(within(got[k], c["scalars64"][k], MEASURED[name]) for k, name in enumerate(ref.SCALARS)):
            failing.append(c["id"])
    print("fails on", failing)
    assert len(failing) >= len(REPORTS) - 6         # (one row is its own last minibatch; the dyadic cases may coincide)


# ------------------------------------------------------------------------------------------------------- PPOTrainer, stubbed

class StubRunner(object):
    def __init__(self, case, multi=False):
        self.case, self.num_steps, self._multi_agent, self.calls = case, case["start"], multi, []

    def gen_training_batch(self, steps_per_env, gamma, lmda):
        self.calls.append((steps_per_env, gamma, lmda))
        self.num_steps += steps_per_env * self.case["num_envs"]
        return types.SimpleNamespace(actions=np.zeros(7 + len(self.calls) % 2), at=self.num_steps)


def stub_trainer(case, multi=False, **kw):
    from safelife_amd import ppo
    log = []

    class Recording(ppo.PPOTrainer):
        def train_batch(self, batch):
            log.append(("train_batch", batch.at, self.batches_done))
            return "sums of %d" % batch.at

        def report(self, batch):
            log.append(("report", batch.at))
            return "report of %d" % batch.at

    tests = []
    test_runner = types.SimpleNamespace(run_episodes=lambda: tests.append(runner.num_steps)) if case["has_testing"] else None
    reports = []
    runner = StubRunner(case, multi)
    trainer = Recording(runner, None, None, steps_per_env=case["steps_per_env"], report_interval=case["report_interval"],
                        test_interval=case["test_interval"], test_runner=test_runner,
                        on_report=(lambda *a: reports.append(a)) if case["has_logger"] else None, record_events=True, **kw)
    return trainer, runner, log, reports, tests


@pytest.mark.parametrize("case", TRAIN, ids=[c["id"] for c in TRAIN])
def test_trainer_schedule_reproduces_the_reference(case):
    """PPOTrainer.train over a stub runner and stubbed train_batch / report: no device API is touched."""
    batches = []
    trainer, runner, log, reports, tests = stub_trainer(case, on_batch=batches.append, gamma=0.9, lmda=0.8)
    for steps in case["train_calls"]:
        trainer.train(steps)
    events = case["events"]
    assert trainer.events == events and trainer.num_steps == events[-1][0]
    assert runner.calls == [(case["steps_per_env"], 0.9, 0.8)] * len(events)
    assert batches == [e[0] for e in events]
    assert [x for x in log if x[0] == "train_batch"] == [("train_batch", e[0], k) for k, e in enumerate(events)]
    # the model is not called for a report nobody takes
    assert [x for x in log if x[0] == "report"] == [("report", e[0]) for e in events if e[1]]
    assert reports == [(e[0], "report of %d" % e[0]) for e in events if e[1]]
    assert tests == [e[0] for e in events if e[2]]
    assert trainer.batches_done == len(events) and trainer.host_visits == 0 and trainer.sums == "sums of %d" % events[-1][0]


def test_trainer_counts_one_host_visit_per_multi_agent_window_and_checkpoints():
    case = next(c for c in TRAIN if c["id"] == "envs5-T20-two-calls")
    trainer, runner, _log, _reports, _tests = stub_trainer(case, multi=True, seed=5)
    trainer.train(case["train_calls"][0])
    first = len(trainer.events)
    assert trainer.host_visits == first
    state = trainer.state_dict()
    assert state == dict(num_steps=runner.num_steps, batches_done=first, seed=5)
    # a fresh trainer picks the run up where the state says: the events of the second call and the epoch counter go on
    again, runner2, log2, _r, _t = stub_trainer(dict(case, start=0), multi=True, seed=0)
    again.load_state_dict(state)
    assert runner2.num_steps == state["num_steps"] and again.seed == 5
    again.train(case["train_calls"][1])
    assert again.events == case["events"][first:] and log2[0] == ("train_batch", case["events"][first][0], first)
    trainer.record_events = False
    trainer.train(case["train_calls"][1])
    assert len(trainer.events) == first and trainer.batches_done == len(case["events"])


def test_trainer_arguments():
    from safelife_amd import ppo
    case = TRAIN[0]
    t = ppo.PPOTrainer(StubRunner(case), None, None)
    assert (t.steps_per_env, t.num_minibatches, t.epochs_per_batch, t.gamma, t.lmda, t.report_interval, t.test_interval,
            t.seed, t.report_chunk_rows) == (20, 4, 3, 0.97, 0.95, 960, 500000, 0, 8192)
    for bad in (dict(steps_per_env=0), dict(report_interval=0), dict(test_interval=0), dict(num_minibatches=0),
                dict(epochs_per_batch=0), dict(report_chunk_rows=100), dict(report_chunk_rows=0)):
        with pytest.raises(ValueError):
            ppo.PPOTrainer(StubRunner(case), None, None, **bad)
    with pytest.raises(TypeError):
        ppo.PPOTrainer(StubRunner(case), None, None, eps_polcy=0.1)
    assert ppo.PPOTrainer(StubRunner(case), None, None, eps_policy=0.1).loss_kwargs == dict(eps_policy=0.1)


def test_ppo_report_refuses_a_bad_chunk_before_anything_else():
    from safelife_amd import ppo
    for bad in (100, 0, -256, 257):
        with pytest.raises(ValueError, match="multiple of 256"):
            ppo.ppo_report(None, None, chunk_rows=bad)
    assert callable(ppo.ppo_report.scalars)


# ------------------------------------------------------------------------------------------------------------- the ABI

NEW = ("slhip_ppo_report_workspace_bytes", "slhip_ppo_report_rows", "slhip_ppo_report_finish")


def test_symbols_and_constants(tmp_path):
    import subprocess
    lib = _hip.lib()
    header = open(os.path.join(util.REPO, "include", "safelife_hip.h")).read()
    for name in NEW:
        assert name in _hip.EXPORTS and hasattr(lib, name) and name + "(" in header
    assert lib.slhip_abi_version() == _hip.SL_ABI_VERSION == 13
    assert [lib.slhip_ppo_report_workspace_bytes(n) for n in (0, 1, 256, 257)] == [0, 40, 40, 80]
    assert lib.slhip_ppo_report_workspace_bytes(-5) == 0
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "safelife_hip.h"\nint main(void) { printf("%d %d %d %d %d %d %d %d %d\\n", '
                   'SL_PPO_REPORT_PARTIALS, SL_PPO_REPORT_DOUBLES, SL_PPO_REPORT_VALUES, SL_PPO_REPORT_ADVANTAGES, '
                   'SL_PPO_REPORT_F32, SL_PPO_REPORT_F32_LOSS, SL_PPO_REPORT_F32_ENTROPY, SL_PPO_REPORT_F32_VALUES, '
                   'SL_PPO_REPORT_F32_ADVANTAGES); return 0; }\n')
    exe = str(tmp_path / "consts")
    subprocess.check_call(["gcc", "-I", os.path.join(util.REPO, "include"), str(src), "-o", exe])
    want = (_hip.PPO_REPORT_PARTIALS, _hip.PPO_REPORT_DOUBLES, _hip.PPO_REPORT_VALUES, _hip.PPO_REPORT_ADVANTAGES,
            _hip.PPO_REPORT_F32) + tuple(_hip.PPO_REPORT_SCALARS.index(k) for k in ("loss", "entropy", "values", "advantages"))
    assert subprocess.check_output([exe]).decode().split() == [str(x) for x in want]
    assert _hip.PPO_REPORT_VALUES == len(_hip.PPO_SUMS) and _hip.PPO_REPORT_F32 + 2 == _hip.PPO_REPORT_DOUBLES


def _loss(**kw):
    """A description whose pointers are non-null but never dereferenced: every call below is refused first."""
    s = _hip.PpoLoss()
    s.n, s.N, s.n_actions = 256, 1024, 9
    for name in ("values", "policy", "actions", "action_prob", "old_values", "returns", "advantages", "status"):
        setattr(s, name, 0x1000)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_first_row_must_be_a_multiple_of_256():
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    for first_row in (128, 1, 255, -256):
        assert lib.slhip_ppo_report_rows(C.byref(_loss()), first_row, p, None) == _hip.SL_E_ARG
        assert b"multiple of 256" in lib.slhip_last_error()


BAD = [dict(n=0), dict(N=0), dict(n_actions=1), dict(n_actions=33), dict(n=2048), dict(n=100), dict(values=None),
       dict(policy=None), dict(actions=None), dict(action_prob=None), dict(old_values=None), dict(returns=None),
       dict(advantages=None), dict(status=None)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_bad_descriptions_are_refused(bad):
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    assert lib.slhip_ppo_report_rows(C.byref(_loss(**bad)), 256, p, None) == _hip.SL_E_ARG
    assert b"ppo_report_rows" in lib.slhip_last_error()


def test_argument_errors():
    lib, p = _hip.lib(), C.c_void_p(0x1000)
    s = _loss()
    assert lib.slhip_ppo_report_rows(None, 0, p, None) == _hip.SL_E_ARG
    assert lib.slhip_ppo_report_rows(C.byref(s), 0, None, None) == _hip.SL_E_ARG
    assert lib.slhip_ppo_report_rows(C.byref(s), 0, C.c_void_p(0x1004), None) == _hip.SL_E_ARG
    assert lib.slhip_ppo_report_rows(C.byref(s), 1024, p, None) == _hip.SL_E_ARG           # the chunk ends beyond the batch
    assert b"beyond" in lib.slhip_last_error()
    # a chunk of 100 rows is fine where it ends the batch and nowhere else
    assert lib.slhip_ppo_report_rows(C.byref(_loss(n=100, N=612)), 256, p, None) == _hip.SL_E_ARG
    assert b"does not end the batch" in lib.slhip_last_error()
    for args in ((None, p, 4, p), (C.byref(s), None, 4, p), (C.byref(s), p, 4, None), (C.byref(s), p, 3, p), (C.byref(s), p, 5, p),
                 (C.byref(s), C.c_void_p(0x1004), 4, p), (C.byref(_loss(N=0)), p, 0, p)):
        assert lib.slhip_ppo_report_finish(*args, None) == _hip.SL_E_ARG
        assert b"ppo_report_finish" in lib.slhip_last_error()
