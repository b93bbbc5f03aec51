"""
The DQN update on the device: what the reference does with a replay sample (training/dqn.py:136-214).

``dqn_loss`` is ``DQN.optimize`` between the two model calls and ``backward`` -- the Q-value of the action taken, the
n-step target from the target model's maximum, the mean squared TD error and its gradient, with the four scalars the
reference reports -- fused into one pass forward (one launch up to 256 rows, the row pass plus a one-workgroup finish
beyond) and one backward (``slhip_dqn_loss_forward`` / ``_backward``, sl_dqn.hip).  It reads action, reward and done
straight from a ``ReplayBuffer``'s ring through the sampled index, or from a gathered ``ReplayBatch``.  ``sync_target``
is ``target_model.load_state_dict(training_model.state_dict())`` without leaving the device, ``optimize`` is
``DQN.optimize`` over these pieces and ``DQNTrainer.train`` the schedule of ``DQN.train``: when to optimise, when to
report, when to copy the training model into the target.

The per-row arithmetic is the reference's float32 arithmetic operation for operation, so ``td`` and the gradient equal the
reference's bit for bit; the loss and the report scalars are float64 sums of the float32 terms, better than the
reference's float32 means.
"""
import ctypes as C

from . import _hip
from .replay import ReplayBatch

_function = None

#: The reference's epsilon schedule, ``UnivariateSpline([5e4, 5e5, 4e6], [1, 0.5, 0.03], s=0, k=1, ext='const')``
#: (training/dqn.py:51-53), as knots and B-spline coefficients.  FITPACK FITS the coefficients, and with three data points
#: its Givens rotations leave each of them one ulp above the datum (a two-point spline, as in env_factory.py, comes out
#: exact); ``LinearSchedule`` evaluates a spline from its coefficients, so these are what it is given.
EPSILON_KNOTS = (5e4, 5e5, 4e6)
EPSILON_COEFFICIENTS = (1.0000000000000002, 0.5000000000000001, 0.030000000000000002)


def _loss_function():
    """The autograd.Function, made on first use (torch is imported late everywhere in this package)."""
    global _function
    if _function is not None:
        return _function
    import torch

    class DqnLossFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, q_values, next_q_values, action, reward, done, index, status, meta, hold):
            lib = _hip.lib()
            q_values = q_values.detach()
            n, A = q_values.shape
            s = _hip.DqnLoss()
            s.n, s.N, s.n_actions = n, action.numel(), A
            s.source, s.discount = meta
            for name, t in (("q_values", q_values), ("next_q_values", next_q_values), ("action", action), ("reward", reward),
                            ("done", done), ("index", index), ("status", status)):
                setattr(s, name, None if t is None else t.data_ptr())
            dev = q_values.device
            td = torch.empty(n, dtype=torch.float32, device=dev)
            sums = torch.empty(8, dtype=torch.float64, device=dev)
            work = torch.empty(lib.slhip_dqn_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
            rc = lib.slhip_dqn_loss_forward(C.byref(s), _hip.ptr(td), _hip.ptr(sums), _hip.ptr(work),
                                            _hip.current_stream_ptr())
            if rc:
                _hip.check(rc)
            ctx.struct = s
            ctx.shape = (n, A)
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(td, action, index, status)
            hold.append(sums)
            return td, sums.view(torch.float32)[2 * _hip.DQN_SUM_LOSS_F32]      # a view: the kernel wrote the float

        @staticmethod
        def backward(ctx, grad_td, grad_loss):
            lib = _hip.lib()
            td = ctx.saved_tensors[0]
            dev = td.device
            if grad_loss is None:
                grad_loss = torch.zeros((), dtype=torch.float32, device=dev)
            grad_loss = grad_loss.to(torch.float32).contiguous()
            if grad_td is not None:
                grad_td = grad_td.to(torch.float32).contiguous()
            d_q = torch.empty(ctx.shape, dtype=torch.float32, device=dev)
            rc = lib.slhip_dqn_loss_backward(C.byref(ctx.struct), _hip.ptr(grad_loss), _hip.ptr(grad_td), _hip.ptr(td),
                                             _hip.ptr(d_q), _hip.current_stream_ptr())
            if rc:
                _hip.check(rc)
            return (d_q,) + (None,) * 8

    _function = DqnLossFunction
    return _function


def _q_rows(x, torch, name):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2):
        raise ValueError("dqn_loss: %s must be a float32 tensor [n, n_actions] on the device" % name)
    return x if x.is_contiguous() else x.contiguous()


def _flat(x, torch, name, dtype, dev):
    if not (torch.is_tensor(x) and x.device == dev and x.dtype == dtype and x.dim() == 1):
        raise ValueError("dqn_loss: %s must be a flat %s tensor on the Q-values' device" % (name, dtype))
    return x if x.is_contiguous() else x.contiguous()


def dqn_loss(q_values, next_q_values, source, index=None, *, gamma=0.97, multi_step=5, status=None):
    """
    ``DQN.optimize`` between the model calls and ``backward`` (training/dqn.py:152-157) -> ``(td [n], loss)``.

    q_values : float32 ``[n, n_actions]`` (2 to 32 actions), the training model's output for the minibatch's
    observations; ``loss.backward()`` reaches it and nothing else.  next_q_values : the target model's output for the next
    observations, same shape; it gets no gradient (one that requires grad is detached, as the reference detaches it).
    source : where action, reward and done come from --

    * a ``ReplayBuffer`` / ``MultiAgentReplayBuffer``: the ring's own storage (int32 actions, float64 n-step rewards,
      uint8 done) is read THROUGH ``index`` (int64 ``[n]`` ring rows, what ``sample_indices`` returned); no copy of the
      three scalars is made.  The float64 reward is rounded to float32 once, as ``gather`` rounds it.
    * a ``ReplayBatch`` (``gather`` / ``sample``): int64 actions, float32 rewards and done of the n rows in order;
      ``index`` must be None.

    ``gamma ** multi_step`` is computed here in Python floats, as the reference computes it.  The defaults are the
    reference's hyper-parameters.

    ``td`` is the per-row TD error ``q_values[i][a_i] - (reward_i + gamma ** n * (1 - done_i) * max_k next_q_values[i][k])``,
    a differentiable output; ``loss`` is ``mean(td ** 2)``.  ``dqn_loss.sums`` is, after every call, that call's float64
    device tensor ``[8]``: loss, q_model_mean, q_model_max, q_target_mean, q_target_max, n (``_hip.DQN_SUMS``; the last
    slot carries the float32 ``loss``) -- what training/dqn.py:163-171 logs, without another launch.

    No host visit.  An index outside the source or an action outside ``[0, n_actions)`` raises a bit in ``status`` (int64
    ``[1]``; ``dqn_loss.status`` when None is passed -- one word per device), contributes zero and gets zero gradients;
    ``check_status()`` reads it.
    """
    import torch
    q_values = _q_rows(q_values, torch, "q_values")
    next_q_values = _q_rows(next_q_values, torch, "next_q_values")
    n, A = q_values.shape
    dev = q_values.device
    if next_q_values.shape != q_values.shape or next_q_values.device != dev:
        raise ValueError("dqn_loss: next_q_values must have the shape and device of q_values")
    if not 2 <= A <= 32:
        raise ValueError("dqn_loss: n_actions outside 2..32")
    if n < 1:
        raise ValueError("dqn_loss: an empty minibatch")
    if next_q_values.requires_grad:
        next_q_values = next_q_values.detach()
    if isinstance(source, ReplayBatch):
        if index is not None:
            raise ValueError("dqn_loss: a ReplayBatch holds the minibatch's rows in order: index must be None")
        form, kinds = _hip.DQN_FROM_BATCH, (torch.int64, torch.float32, torch.float32)
    elif all(hasattr(source, k) for k in ("action", "reward", "done", "capacity")):
        form, kinds = _hip.DQN_FROM_RING, (torch.int32, torch.float64, torch.uint8)
    else:
        raise ValueError("dqn_loss: source must be a ReplayBuffer, a MultiAgentReplayBuffer or a ReplayBatch")
    action, reward, done = (_flat(getattr(source, k), torch, "source." + k, kind, dev)
                            for k, kind in zip(("action", "reward", "done"), kinds))
    N = action.numel()
    if reward.numel() != N or done.numel() != N:
        raise ValueError("dqn_loss: the source's fields differ in length")
    if index is None:
        if n != N:
            raise ValueError("dqn_loss: without index the Q-values must cover the whole source (%d rows, not %d)" % (N, n))
    else:
        if not (torch.is_tensor(index) and index.device == dev and index.dtype == torch.int64 and index.numel() == n):
            raise ValueError("dqn_loss: index must be an int64 tensor of n source rows on the Q-values' device")
        index = index if index.is_contiguous() else index.contiguous()
    if status is None:
        status = _status_word(dev)
    elif not (torch.is_tensor(status) and status.device == dev and status.dtype == torch.int64 and status.numel() >= 1):
        raise ValueError("dqn_loss: status must be an int64 tensor [1] on the Q-values' device")
    meta = (form, float(gamma) ** int(multi_step))
    hold = []
    td, loss = _loss_function().apply(q_values, next_q_values, action, reward, done, index, status, meta, hold)
    dqn_loss.sums = hold[0]
    return td, loss


dqn_loss.sums = None
dqn_loss.status = {}


def _status_word(dev):
    import torch
    word = dqn_loss.status.get(dev)
    if word is None:
        word = dqn_loss.status[dev] = torch.zeros(1, dtype=torch.int64, device=dev)
    return word


def check_status(status=None):
    """Read a status word (a host visit; None: every word ``dqn_loss`` / ``optimize`` made) and raise on a bad index or
    action."""
    for word in (list(dqn_loss.status.values()) if status is None else [status]):
        bits = int(word.item())
        if bits & _hip.DQN_BAD_INDEX:
            raise ValueError("dqn: an index outside the source was used (the row was skipped)")
        if bits & _hip.DQN_BAD_ACTION:
            raise ValueError("dqn: an action outside [0, n_actions) was met (the row was skipped)")


def sync_target(training_model, target_model):
    """``target_model.load_state_dict(training_model.state_dict())`` (training/dqn.py:90-91, :206) as one batched copy:
    parameters and buffers of the training model over the target's, in place, no host visit.  Raises ValueError if the two
    state dicts differ in their keys or in a tensor's shape."""
    import torch
    src, dst = training_model.state_dict(), target_model.state_dict()
    if list(src.keys()) != list(dst.keys()):
        odd = sorted(set(src.keys()) ^ set(dst.keys()))
        raise ValueError("sync_target: the models' state dicts differ in their keys: %s" % (odd or "(their order)"))
    for k in dst:
        if src[k].shape != dst[k].shape:
            raise ValueError("sync_target: %s is %s in the training model and %s in the target"
                             % (k, tuple(src[k].shape), tuple(dst[k].shape)))
    if dst:
        with torch.no_grad():
            torch._foreach_copy_(list(dst.values()), [src[k] for k in dst])


def _float_obs(store, index, status):
    from . import ppo
    import torch
    if store.dtype in (torch.uint8, torch.float32):
        return ppo.minibatch_obs(store, index, float32=True, status=status)
    return ppo.minibatch_obs(store, index, float32=False, status=status).to(torch.float32)


def optimize(training_model, target_model, optimizer, replay, batch_size=96, *, gamma, multi_step, report=False):
    """
    ``DQN.optimize`` (training/dqn.py:136-175) after its length check: ``batch_size`` distinct ring rows
    (``replay.sample_indices``), their observations and next observations as float32 (``ppo.minibatch_obs``, widened in the
    same pass), both models, ``dqn_loss`` through the index -- action, reward and done are never gathered -- then
    ``zero_grad``, ``backward``, ``step``.  No host visit.

    -> ``dqn_loss.sums`` of this update, a device tensor: what the reference logs when ``report`` is set.  Nothing is read
    back either way; ``report`` says whether the caller means to keep the sums (``DQNTrainer`` hands them to ``on_report``).
    """
    import torch
    index = replay.sample_indices(batch_size)
    status = _status_word(index.device)
    obs = _float_obs(replay.obs, index, status)
    next_obs = _float_obs(replay.next_obs, index, status)
    q_values = training_model(obs)
    with torch.no_grad():
        next_q_values = target_model(next_obs)
    _td, loss = dqn_loss(q_values, next_q_values, replay, index, gamma=gamma, multi_step=multi_step, status=status)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return dqn_loss.sums


def round_up(x, r):
    """training/utils.py: the next multiple of r STRICTLY above x when x is one itself."""
    return x + r - x % r


class DQNTrainer(object):
    """
    The loop of ``DQN.train`` (training/dqn.py:177-214) over a ``DQNRunner`` or a ``MultiAgentDQNRunner`` and its replay
    buffer.

    Per iteration: ``round_up(num_steps, interval)`` for the three intervals BEFORE the step, epsilon from the schedule at
    that ``num_steps``, one ``runner.collect(1, epsilon, replay)`` (which adds ``env.num_envs`` to ``runner.num_steps``),
    and then, once the replay holds ``replay_initial`` rows, the reference's three ``>=`` tests in the reference's order:
    report due, optimise (with the pending report flag, which every optimise clears), target update.  ``needs_report``
    starts True at every ``train()`` call.

    The replay-length gate uses the exact ``len(replay)``, as the reference does: ONE host visit per step while the ring
    is filling.  ``idx`` never decreases, so the gate stays open once it has passed and no ``.item()`` is made in steady
    state; ``host_visits`` counts the visits made.

    Parameters: ``gamma`` and ``multi_step`` are the replay buffer's.  ``epsilon_schedule``: a function of ``num_steps``
    (None: the reference's spline, ``LinearSchedule(EPSILON_KNOTS, EPSILON_COEFFICIENTS)`` -- 1 until 5e4 steps, 0.5 at 5e5,
    0.03 from 4e6 on, to the last bit what the reference's ``epsilon_schedule`` returns).  ``on_report(num_steps, epsilon,
    sums)`` gets the device tensor of the optimise that carried the report flag.  ``record_events``: keep, per iteration,
    ``(num_steps after the step, epsilon, optimized, reported, target_updated)`` in ``events``.

    ``checkpointer``: a ``checkpoint.Checkpointer`` (None: nothing is saved and nothing is computed).  Whether a save is
    due is asked past the replay gate only, behind the target update, where the reference calls
    ``save_checkpoint_if_needed`` (training/dqn.py:208), so the files carry the reference's steps; the file itself is
    written at the END of that iteration, behind the test run and the event, with the loop's report flag, so that it is a
    whole iteration: a ``train()`` call on a trainer loaded from it goes on where the interrupted call stood and owes
    nothing (the reference's file, taken in front of ``run_episodes``, loses the test that was due, and its resumed
    ``train()`` raises the report flag anew).  ``train()`` ends with a save (:214), behind which the next call starts as
    the reference's does.  A checkpointer without a
    ``root`` gets this trainer, both models (``training_model``, ``target_model``) and the optimiser.

    ``test_runner``: a second ``DQNRunner`` / ``MultiAgentDQNRunner`` over an env with an ``EpisodeRun`` (None: no tests).
    ``next_test = round_up(num_steps, test_interval)`` is taken with the other three intervals; past the replay gate and
    behind the checkpoint, when ``num_steps >= next_test``, ``self.epsilon`` becomes ``epsilon_testing`` and
    ``test_runner.run_episodes(epsilon=epsilon_testing)`` runs (training/dqn.py:210-212).  ``self.epsilon`` stays there
    until the next iteration sets it, as in the reference; ``runner.num_steps`` is untouched; the tuples in ``events`` do
    not change; the steps at which a test ran go to ``tests_run``.
    """

    _checkpoint_children = ("runner", "replay", "test_runner")

    def __init__(self, runner, replay, training_model, target_model, optimizer, *, training_batch_size=96,
                 optimize_interval=32, target_update_interval=10000, report_interval=256, replay_initial=40000,
                 epsilon_schedule=None, on_report=None, record_events=False, checkpointer=None, test_runner=None,
                 test_interval=100000, epsilon_testing=0.01):
        if epsilon_schedule is None:
            from .schedule import LinearSchedule
            epsilon_schedule = LinearSchedule(EPSILON_KNOTS, EPSILON_COEFFICIENTS)
        for name, v in (("training_batch_size", training_batch_size), ("optimize_interval", optimize_interval),
                        ("target_update_interval", target_update_interval), ("report_interval", report_interval),
                        ("test_interval", test_interval)):
            if int(v) < 1:
                raise ValueError("DQNTrainer: %s must be at least 1" % name)
        self.runner, self.replay = runner, replay
        self.training_model, self.target_model, self.optimizer = training_model, target_model, optimizer
        self.training_batch_size = int(training_batch_size)
        self.optimize_interval, self.target_update_interval = int(optimize_interval), int(target_update_interval)
        self.report_interval, self.replay_initial = int(report_interval), int(replay_initial)
        self.epsilon_schedule, self.on_report = epsilon_schedule, on_report
        self.record_events = bool(record_events)
        self.events = []
        self.epsilon = None
        self.sums = None                # dqn_loss.sums of the last optimise
        self.host_visits = 0            # exact len(replay) reads: .item() calls made by train()
        self._gate_open = False
        self._needs_report, self._in_train = True, False    # the loop's report flag, as a checkpoint inside train() finds it
        self.test_runner, self.test_interval = test_runner, int(test_interval)
        self.epsilon_testing = float(epsilon_testing)
        self.tests_run = []             # num_steps at which test episodes ran
        self.checkpointer = checkpointer
        if checkpointer is not None and checkpointer.root is None:
            checkpointer.root, checkpointer.optimizer = self, optimizer
            checkpointer.model = {"training_model": training_model, "target_model": target_model}

    @property
    def num_steps(self):
        return self.runner.num_steps

    def optimize(self, report):
        """One update (``dqn.optimize`` with the replay buffer's gamma and multi_step)."""
        return optimize(self.training_model, self.target_model, self.optimizer, self.replay, self.training_batch_size,
                        gamma=self.replay.gamma, multi_step=self.replay.multi_step, report=report)

    def update_target(self):
        sync_target(self.training_model, self.target_model)

    def _replay_ready(self):
        if not self._gate_open:
            self.host_visits += 1
            self._gate_open = len(self.replay) >= self.replay_initial
        return self._gate_open

    def train(self, steps):
        """``DQN.train(steps)``: iterations until ``num_steps`` has grown by at least ``steps``."""
        runner = self.runner
        # (a trainer loaded from a file that was written inside a train() call goes on with that call's report flag)
        needs_report = self._needs_report if self._in_train else True
        self._in_train = False
        max_steps = runner.num_steps + int(steps)
        while runner.num_steps < max_steps:
            before = runner.num_steps
            next_opt = round_up(before, self.optimize_interval)
            next_update = round_up(before, self.target_update_interval)
            next_report = round_up(before, self.report_interval)
            next_test = round_up(before, self.test_interval)
            self.epsilon = epsilon = float(self.epsilon_schedule(before))
            runner.collect(1, epsilon, self.replay)
            num_steps = runner.num_steps
            optimized = reported = updated = save_due = False
            if self._replay_ready():
                if num_steps >= next_report:
                    needs_report = True
                if num_steps >= next_opt:
                    optimized, reported = True, needs_report
                    self.sums = self.optimize(needs_report)
                    if needs_report and self.on_report is not None:
                        self.on_report(num_steps, epsilon, self.sums)
                    needs_report = False
                if num_steps >= next_update:
                    updated = True
                    self.update_target()
                save_due = self.checkpointer is not None and self.checkpointer.due(num_steps)
                if self.test_runner is not None and num_steps >= next_test:
                    self.epsilon = self.epsilon_testing
                    self.test()
                    self.tests_run.append(num_steps)
            if self.record_events:
                self.events.append((num_steps, epsilon, optimized, reported, updated))
            if save_due:
                self._needs_report, self._in_train = needs_report, True
                self.checkpointer.save(num_steps)
        self._needs_report, self._in_train = needs_report, False
        if self.checkpointer is not None:
            self.checkpointer.save(runner.num_steps)

    def test(self):
        """``run_episodes`` of the test runner at ``epsilon_testing`` (training/dqn.py:211-212)."""
        return self.test_runner.run_episodes(epsilon=self.epsilon_testing)

    def _checkpoint_state(self):
        """``checkpoint.py``: whether the replay gate has opened, and the events so far; the runner, the replay buffer and
        the test runner carry the rest."""
        config = dict(training_batch_size=self.training_batch_size, optimize_interval=self.optimize_interval,
                      target_update_interval=self.target_update_interval, report_interval=self.report_interval,
                      replay_initial=self.replay_initial, test_interval=self.test_interval,
                      epsilon_testing=self.epsilon_testing)
        scalars = dict(_gate_open=self._gate_open, _needs_report=self._needs_report, _in_train=self._in_train,
                       host_visits=self.host_visits, epsilon=self.epsilon,
                       events=self.events, tests_run=self.tests_run)
        return config, scalars, {}

    def _checkpoint_loaded(self):
        self.events = [tuple(e) for e in self.events]
