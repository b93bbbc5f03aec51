"""
The PPO update on the device: what the reference does with a training batch (training/ppo.py:145-182).

``ppo_loss`` is ``PPO.calculate_loss`` after the model call -- the clipped policy term, the clipped value term and the
entropy bonus with their gradients, fused into one pass forward (plus a one-workgroup finish) and one backward
(``slhip_ppo_loss_forward`` / ``_backward``, sl_ppo.hip).  ``MinibatchDeal`` cuts an epoch's rows into the reference's
minibatches, ``minibatch_obs`` fetches a minibatch's observations, widened to float32 in the same pass, and
``train_batch`` is the loop of ``PPO.train_batch`` over these pieces.  ``ppo_report`` is the report of ``PPO.train``
(:199-205) over a batch too large for one model call, evaluated chunk by chunk with the same bits however it is cut
(``slhip_ppo_report_rows`` / ``_finish``), and ``PPOTrainer.train`` the loop of ``PPO.train`` (:184-219): when to report,
when to test.  Nothing here visits the host but ``check_status`` and ``ppo_report.scalars``.

The reference's rule has four details a textbook PPO does not: the policy clamp is ONE-sided (``max(pd, -eps)`` on
``pd = sign(A) * (1 - pi / pi_old)``), the value term is the MAXIMUM of the clipped and the unclipped squared error, the
entropy bonus switches off when the minibatch's MEAN entropy exceeds ``entropy_clip``, and ``train_batch`` cuts
``num_minibatches + 1`` pieces.  All four are kept.
"""
import ctypes as C

import numpy as np

from . import _hip

_FIELDS = ("actions", "action_prob", "returns", "advantages", "values")
_function = None


def _float_rows(x, torch, name, n=None):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
        raise ValueError("ppo_loss: %s must be a float32 tensor on the device" % name)
    if n is not None and x.numel() != n:
        raise ValueError("ppo_loss: %s has %d elements, %d expected" % (name, x.numel(), n))
    return x if x.is_contiguous() else x.contiguous()


def _batch_fields(batch, dev, torch, who):
    """The five per-row scalars of a training batch, checked: flat, contiguous, on ``dev``, of one length."""
    fixed = []
    for name in _FIELDS:
        x = getattr(batch, name)
        want = torch.int64 if name == "actions" else torch.float32
        if not (torch.is_tensor(x) and x.device == dev and x.dtype == want and x.dim() == 1):
            raise ValueError("%s: batch.%s must be a flat %s tensor on the policy's device" % (who, name, want))
        fixed.append(x if x.is_contiguous() else x.contiguous())
    if any(x.numel() != fixed[0].numel() for x in fixed):
        raise ValueError("%s: the batch's fields differ in length" % who)
    return fixed


def _loss_function():
    """The autograd.Function, made on first use (torch is imported late everywhere in this package)."""
    global _function
    if _function is not None:
        return _function
    import torch

    class PpoLossFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, values, policy, actions, action_prob, old_values, returns, advantages, rows, status, hyper, hold):
            lib = _hip.lib()
            values, policy = values.detach(), policy.detach()
            n, A = policy.shape
            s = _hip.PpoLoss()
            s.n, s.N, s.n_actions = n, actions.numel(), A
            s.eps_policy, s.eps_value, s.vf_coef, s.entropy_reg, s.entropy_clip = hyper
            for name, t in (("values", values), ("policy", policy), ("actions", actions), ("action_prob", action_prob),
                            ("old_values", old_values), ("returns", returns), ("advantages", advantages),
                            ("rows", rows), ("status", status)):
                setattr(s, name, None if t is None else t.data_ptr())
            dev = policy.device
            entropy = torch.empty(n, dtype=torch.float32, device=dev)
            sums = torch.empty(8, dtype=torch.float64, device=dev)
            work = torch.empty(lib.slhip_ppo_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
            rc = lib.slhip_ppo_loss_forward(C.byref(s), _hip.ptr(entropy), _hip.ptr(sums), _hip.ptr(work),
                                            _hip.current_stream_ptr())
            if rc:
                _hip.check(rc)
            ctx.struct = s
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(values, policy, actions, action_prob, old_values, returns, advantages, rows, status, sums)
            hold.append(sums)
            return entropy, sums.view(torch.float32)[2 * _hip.PPO_SUM_LOSS_F32]     # a view: the finish kernel wrote the float

        @staticmethod
        def backward(ctx, grad_entropy, grad_loss):
            lib = _hip.lib()
            values, policy, sums = ctx.saved_tensors[0], ctx.saved_tensors[1], ctx.saved_tensors[-1]
            dev = policy.device
            if grad_loss is None:
                grad_loss = torch.zeros((), dtype=torch.float32, device=dev)
            grad_loss = grad_loss.to(torch.float32).contiguous()
            if grad_entropy is not None:
                grad_entropy = grad_entropy.to(torch.float32).contiguous()
            d_values = torch.empty_like(values)
            d_policy = torch.empty_like(policy)
            rc = lib.slhip_ppo_loss_backward(C.byref(ctx.struct), _hip.ptr(grad_loss), _hip.ptr(grad_entropy),
                                             _hip.ptr(sums), _hip.ptr(d_values), _hip.ptr(d_policy),
                                             _hip.current_stream_ptr())
            if rc:
                _hip.check(rc)
            return (d_values, d_policy) + (None,) * 9

    _function = PpoLossFunction
    return _function


def ppo_loss(values, policy, batch, rows=None, *, eps_policy=0.2, eps_value=0.2, vf_coef=0.5, entropy_reg=0.01,
             entropy_clip=1.0, status=None):
    """
    ``PPO.calculate_loss`` (training/ppo.py:145-166) for the model outputs of one minibatch -> ``(entropy [n], loss)``.

    values : float32 ``[n]`` (or ``[n, 1]``) and policy : float32 ``[n, n_actions]`` (probabilities, 2 to 32 actions) are
    what ``model(obs)`` returned for the minibatch; ``loss.backward()`` reaches both.  batch : a ``TrainingBatch`` or any
    object with its fields (``obs`` is not looked at); rows : int64 ``[n]``, the batch row behind every minibatch row --
    the five per-row scalars are read THROUGH it, no minibatch copy of them is made -- or None: the whole batch in order.
    The defaults are the reference's hyper-parameters.

    ``ppo_loss.sums`` is, after every call, that call's float64 device tensor ``[8]``: mean policy loss, mean value loss,
    mean entropy, the entropy term, the total, the flag "the bonus has a gradient", n (``_hip.PPO_SUMS``; the last slot
    carries the float32 ``loss``) -- what training/ppo.py:198-214 logs, without another launch.

    No host visit.  A row id outside the batch or an action outside ``[0, n_actions)`` raises a bit in ``status`` (int64
    ``[1]``; ``ppo_loss.status`` when None is passed -- one word per device), contributes zero and gets zero gradients;
    ``check_status()`` reads it.
    """
    import torch
    if policy.dim() != 2:
        raise ValueError("ppo_loss: policy must be [n, n_actions]")
    n = policy.shape[0]
    policy = _float_rows(policy, torch, "policy")
    values = _float_rows(values, torch, "values", n).reshape(n)
    dev = policy.device
    actions, action_prob, returns, advantages, old_values = _batch_fields(batch, dev, torch, "ppo_loss")
    N = actions.numel()
    if rows is None:
        if n != N:
            raise ValueError("ppo_loss: without rows the model outputs must cover the whole batch (%d rows, not %d)" % (N, n))
    else:
        if not (torch.is_tensor(rows) and rows.device == dev and rows.dtype == torch.int64 and rows.numel() == n):
            raise ValueError("ppo_loss: rows must be an int64 tensor of n row ids on the policy's device")
        rows = rows if rows.is_contiguous() else rows.contiguous()
    if status is None:
        status = _status_word(dev)
    hyper = (float(eps_policy), float(eps_value), float(vf_coef), float(entropy_reg), float(entropy_clip))
    hold = []
    entropy, loss = _loss_function().apply(values, policy, actions, action_prob, old_values, returns, advantages, rows,
                                           status, hyper, hold)
    ppo_loss.sums = hold[0]
    return entropy, loss


ppo_loss.sums = None
ppo_loss.status = {}


def _status_word(dev):
    import torch
    word = ppo_loss.status.get(dev)
    if word is None:
        word = ppo_loss.status[dev] = torch.zeros(1, dtype=torch.int64, device=dev)
    return word


def check_status(status=None):
    """Read a status word (a host visit; None: every word ``ppo_loss`` / ``minibatch_obs`` made) and raise on a bad row
    id or action."""
    for word in (list(ppo_loss.status.values()) if status is None else [status]):
        bits = int(word.item())
        if bits & _hip.PPO_BAD_INDEX:
            raise ValueError("ppo: a row id outside the batch was used (the row was skipped)")
        if bits & _hip.PPO_BAD_ACTION:
            raise ValueError("ppo: an action outside [0, n_actions) was met (the row was skipped)")


# ---------------------------------------------------------------------------------------------------------------- the deal

_G64, _MIX, _M64 = 0x9E3779B97F4A7C15, 0x100000001B3, (1 << 64) - 1


def deal_keys_host(num_rows, seed, epoch):
    """The host model of ``slhip_minibatch_keys``: uint64 ``[num_rows]``."""
    i = np.arange(num_rows, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & _M64) + np.uint64(_G64) * (np.uint64((epoch * _MIX) & _M64) + i + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def split_points(num_rows, num_minibatches):
    """Where the reference's ``train_batch`` cuts: ``np.linspace(0, N, num_minibatches + 2, dtype=int)[1:-1]``, in integer
    arithmetic (linspace's step is N / (m + 1) in float64 and ``k * step`` truncates to ``k * N // (m + 1)`` only up to
    rounding, so the reference's own expression is what is evaluated)."""
    return [int(x) for x in np.linspace(0, num_rows, num_minibatches + 2, dtype=int)[1:-1]]


def deal_host(num_rows, num_minibatches, seed, epoch):
    """The exact host model of ``MinibatchDeal.epoch``: a list of int64 arrays (zero-row pieces left out)."""
    keys = deal_keys_host(num_rows, seed, epoch).view(np.int64)
    perm = np.argsort(keys, kind="stable").astype(np.int64)
    return [p for p in np.split(perm, split_points(num_rows, num_minibatches)) if len(p)]


class MinibatchDeal(object):
    """
    The minibatches of ``PPO.train_batch`` (training/ppo.py:168-176), dealt on the device.

    ``epoch(e)`` -> the list of int64 row-id tensors of epoch ``e``, views of one permutation of ``range(num_rows)``.
    The permutation is the stable argsort of the epoch's keys -- key ``i`` is the splitmix64 mix of ``(seed, e, i)``
    (``slhip_minibatch_keys``; the generator of ``slhip_sample_actions``), compared as two's-complement int64, which is
    how ``torch.sort`` reads them -- so it is a function of ``(seed, e)`` alone and ``deal_host`` reproduces it exactly.
    It is NOT numpy's ``Generator.shuffle``, which the reference calls: that is a sequential Fisher-Yates over one random
    stream and cannot be dealt in parallel; nothing downstream depends on which permutation it is.

    The permutation is cut where the reference cuts, at ``np.linspace(0, N, num_minibatches + 2, dtype=int)[1:-1]``:
    that is ``num_minibatches + 1`` pieces, not ``num_minibatches`` -- the reference's rule, kept.  A piece of zero rows
    (``N < num_minibatches + 1``) is skipped; the reference would take the mean of nothing and train on NaN.
    """

    def __init__(self, num_rows, num_minibatches=4, seed=0, device=None):
        import torch
        self.torch = torch
        self.num_rows, self.num_minibatches, self.seed = int(num_rows), int(num_minibatches), int(seed) & _M64
        if self.num_rows < 1 or self.num_minibatches < 1:
            raise ValueError("MinibatchDeal needs num_rows >= 1 and num_minibatches >= 1")
        self.device = _hip.device() if device is None else torch.device(device)
        self.splits = split_points(self.num_rows, self.num_minibatches)
        self._lib = _hip.lib()
        self.keys = torch.empty(self.num_rows, dtype=torch.int64, device=self.device)
        self.permutation = None

    def epoch(self, e):
        rc = self._lib.slhip_minibatch_keys(self.num_rows, self.seed, int(e) & _M64, _hip.ptr(self.keys),
                                            _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)
        self.permutation = perm = self.torch.sort(self.keys, stable=True).indices
        bounds = [0] + self.splits + [self.num_rows]
        return [perm[lo:hi] for lo, hi in zip(bounds[:-1], bounds[1:]) if hi > lo]


def minibatch_obs(batch_obs, rows, float32=True, out=None, status=None):
    """Rows ``rows`` (int64 ``[n]``) of the batch's observation store ``[N, ...]`` -> ``[n, ...]``, one kernel
    (``slhip_minibatch_obs``).  With ``float32`` a uint8 store comes out as float32, widened in the same pass -- what
    ``batch.obs[k]`` and the model's float cast do in two; a float32 store is moved as it is.  ``out``: where to write
    (contiguous, of the result's shape and dtype).  A row id outside the store raises PPO_BAD_INDEX in ``status`` and
    leaves its output row as it was."""
    import torch
    if not (torch.is_tensor(batch_obs) and batch_obs.is_cuda and batch_obs.dim() >= 1):
        raise ValueError("minibatch_obs: the observation store must be a device tensor [N, ...]")
    src = batch_obs if batch_obs.is_contiguous() else batch_obs.contiguous()
    dev = src.device
    if not (torch.is_tensor(rows) and rows.device == dev and rows.dtype == torch.int64 and rows.dim() == 1):
        raise ValueError("minibatch_obs: rows must be a flat int64 tensor on the store's device")
    rows = rows if rows.is_contiguous() else rows.contiguous()
    N, n = src.shape[0], rows.numel()
    widen = bool(float32) and src.dtype == torch.uint8
    if float32 and src.dtype not in (torch.uint8, torch.float32):
        raise ValueError("minibatch_obs: float32=True serves uint8 and float32 stores, not %s" % src.dtype)
    dtype = torch.float32 if widen else src.dtype
    shape = (n,) + tuple(src.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    elif not (out.is_contiguous() and tuple(out.shape) == shape and out.dtype == dtype and out.device == dev):
        raise ValueError("minibatch_obs: out must be a contiguous %s tensor of shape %s" % (dtype, shape))
    if N == 0 or n == 0:
        return out
    per_row = src[0].numel()
    obs_bytes = per_row * src.element_size()
    if status is None:
        status = _status_word(dev)
    rc = _hip.lib().slhip_minibatch_obs(_hip.ptr(src), obs_bytes, N, _hip.ptr(rows), n, _hip.ptr(out), 1 if widen else 0,
                                        _hip.ptr(status), _hip.current_stream_ptr())
    if rc:
        _hip.check(rc)
    return out


def train_batch(model, optimizer, batch, deal, first_epoch, epochs_per_batch=3, **loss_kwargs):
    """
    ``PPO.train_batch`` (training/ppo.py:168-182): ``epochs_per_batch`` passes over the batch, epoch ``first_epoch + k``
    of ``deal`` (a ``MinibatchDeal`` over ``len(batch.actions)`` rows) cut into minibatches; per minibatch
    ``model(obs) -> (values, policy)`` on the gathered float32 observations, ``ppo_loss``, ``zero_grad``, ``backward``,
    ``step``.  No host visit.  -> the last minibatch's ``ppo_loss.sums``.
    """
    sums = None
    for k in range(int(epochs_per_batch)):
        for rows in deal.epoch(first_epoch + k):
            obs = minibatch_obs(batch.obs, rows, float32=True)
            values, policy = model(obs)
            _entropy, loss = ppo_loss(values, policy, batch, rows, **loss_kwargs)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            sums = ppo_loss.sums
    return sums


# -------------------------------------------------------------------------------------------------------------- the report

def ppo_report(model, batch, *, chunk_rows=8192, eps_policy=0.2, eps_value=0.2, vf_coef=0.5, entropy_reg=0.01,
               entropy_clip=1.0, status=None):
    """
    The report of ``PPO.train`` (training/ppo.py:199-205) -- ``calculate_loss`` on the WHOLE batch, its loss, the mean
    entropy and the means of ``batch.values`` and ``batch.advantages`` -- without a host visit and without one model call on
    the whole batch: under ``torch.no_grad()`` the model is called on ``chunk_rows`` rows of ``batch.obs`` at a time (a uint8
    store is widened to float32, as ``minibatch_obs`` widens it) and every chunk's outputs go through
    ``slhip_ppo_report_rows``; one ``slhip_ppo_report_finish`` follows.  The loss clips the entropy bonus at the batch's mean
    entropy, so the chunks leave float64 partial sums per 256 rows, each at its place in the batch, and the finish adds them
    in order: the result does not depend on ``chunk_rows``, bit for bit, and its first seven doubles are ``ppo_loss.sums``
    of one ``ppo_loss(values, policy, batch)`` over the whole batch.

    ``chunk_rows`` must be a positive multiple of 256 (ValueError).  -> the float64 device tensor ``[PPO_REPORT_DOUBLES]``:
    ``_hip.PPO_SUMS``, the mean of ``batch.values``, the mean of ``batch.advantages``, and in the last two slots the four
    scalars the reference logs as float32 (``_hip.PPO_REPORT_SCALARS``).  ``ppo_report.scalars(t)`` reads those four back.
    A bad action raises ``PPO_BAD_ACTION`` in ``status`` (``ppo_loss.status`` when None) and its row adds nothing.
    """
    import torch
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1 or chunk_rows % 256:
        raise ValueError("ppo_report: chunk_rows must be a positive multiple of 256, not %d" % chunk_rows)
    obs = batch.obs
    if not (torch.is_tensor(obs) and obs.is_cuda):
        raise ValueError("ppo_report: batch.obs must be a device tensor [N, ...]")
    dev = obs.device
    actions, action_prob, returns, advantages, old_values = _batch_fields(batch, dev, torch, "ppo_report")
    N = actions.numel()
    if N < 1 or obs.shape[0] != N:
        raise ValueError("ppo_report: batch.obs has %d rows, the batch %d" % (obs.shape[0], N))
    if status is None:
        status = _status_word(dev)
    lib = _hip.lib()
    s = _hip.PpoLoss()
    s.N = N
    s.eps_policy, s.eps_value, s.vf_coef, s.entropy_reg, s.entropy_clip = (
        float(eps_policy), float(eps_value), float(vf_coef), float(entropy_reg), float(entropy_clip))
    for name, t in (("actions", actions), ("action_prob", action_prob), ("old_values", old_values), ("returns", returns),
                    ("advantages", advantages), ("status", status)):
        setattr(s, name, t.data_ptr())
    work = torch.empty(lib.slhip_ppo_report_workspace_bytes(N) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(_hip.PPO_REPORT_DOUBLES, dtype=torch.float64, device=dev)
    stream = _hip.current_stream_ptr()
    with torch.no_grad():
        for lo in range(0, N, chunk_rows):
            x = obs[lo:lo + chunk_rows]
            values, policy = model(x.to(torch.float32) if x.dtype == torch.uint8 else x)
            n = x.shape[0]
            if policy.dim() != 2 or policy.shape[0] != n:
                raise ValueError("ppo_report: the model must return a policy [n, n_actions] for n rows")
            policy = _float_rows(policy, torch, "policy")
            values = _float_rows(values, torch, "values", n)
            s.n, s.n_actions, s.values, s.policy = n, policy.shape[1], values.data_ptr(), policy.data_ptr()
            rc = lib.slhip_ppo_report_rows(C.byref(s), lo, _hip.ptr(work), stream)
            if rc:
                _hip.check(rc)
    rc = lib.slhip_ppo_report_finish(C.byref(s), _hip.ptr(work), work.numel() // _hip.PPO_REPORT_PARTIALS, _hip.ptr(out),
                                     stream)
    if rc:
        _hip.check(rc)
    return out


def _report_scalars(report):
    """The four values the reference logs, read back from a ``ppo_report`` tensor (ONE host visit): a dict of Python
    floats keyed ``loss``, ``entropy``, ``values``, ``advantages`` -- float32 numbers, the precision the reference logs."""
    import torch
    four = report[_hip.PPO_REPORT_F32:_hip.PPO_REPORT_F32 + 2].view(torch.float32).cpu().tolist()
    return dict(zip(_hip.PPO_REPORT_SCALARS, four))


ppo_report.scalars = _report_scalars


# ------------------------------------------------------------------------------------------------------------- the trainer

class PPOTrainer(object):
    """
    The loop of ``PPO.train`` (training/ppo.py:184-219) over a ``VectorRunner`` or a ``MultiAgentRunner``.

    Per iteration: ``round_up(num_steps, interval)`` for the report and the test interval BEFORE the batch,
    ``runner.gen_training_batch(steps_per_env, gamma, lmda)``, ``train_batch`` over epochs ``batches_done *
    epochs_per_batch ...`` of the ``MinibatchDeal`` of the batch's row count (one deal per distinct row count: a
    multi-agent window's varies; the epoch counter runs on across windows and ``train()`` calls), ``on_batch(num_steps)``
    where the reference checkpoints, then the reference's two ``>=`` tests: ``on_report(num_steps, ppo_report(...))`` when
    the report is due and ``on_report`` was given -- without it the model is not called, as the reference reports only with
    a logger -- and ``test_runner.run_episodes()`` when a test is due and ``test_runner`` was given (which leaves
    ``runner.num_steps`` alone: the test runner counts for itself).

    ``events`` (with ``record_events``) holds ``(num_steps after the batch, reported, tested)`` per iteration.
    ``host_visits`` counts the ``.item()`` calls made: none over a single-agent runner, one per window over a multi-agent
    runner (the row count its ``gen_training_batch`` reads).  ``loss_kwargs`` are ``ppo_loss``'s hyper-parameters, for the
    update and the report alike.

    ``checkpointer``: a ``checkpoint.Checkpointer`` (None: nothing is saved and nothing is computed).  Whether a save is
    due is asked right behind ``on_batch``, where the reference calls ``save_checkpoint_if_needed`` (training/ppo.py:194), so
    the files carry the reference's steps; the file itself is written at the END of that iteration, behind the report, the
    test run and the event, so that it is a whole iteration: a run resumed from it owes nothing (the reference's file, taken
    in front of ``run_episodes``, loses the test that was due).  ``train()`` ends with a save (:219).  A checkpointer without
    a ``root`` gets this trainer, its model and its optimiser.
    """

    _checkpoint_children = ("runner", "test_runner")

    def __init__(self, runner, model, optimizer, *, steps_per_env=20, num_minibatches=4, epochs_per_batch=3, gamma=0.97,
                 lmda=0.95, report_interval=960, test_interval=500000, seed=0, test_runner=None, on_report=None,
                 on_batch=None, report_chunk_rows=8192, record_events=False, checkpointer=None, **loss_kwargs):
        for name, v in (("steps_per_env", steps_per_env), ("num_minibatches", num_minibatches),
                        ("epochs_per_batch", epochs_per_batch), ("report_interval", report_interval),
                        ("test_interval", test_interval)):
            if int(v) < 1:
                raise ValueError("PPOTrainer: %s must be at least 1" % name)
        if int(report_chunk_rows) < 1 or int(report_chunk_rows) % 256:
            raise ValueError("PPOTrainer: report_chunk_rows must be a positive multiple of 256")
        unknown = set(loss_kwargs) - {"eps_policy", "eps_value", "vf_coef", "entropy_reg", "entropy_clip"}
        if unknown:
            raise TypeError("PPOTrainer: unknown arguments %s" % sorted(unknown))
        self.runner, self.model, self.optimizer = runner, model, optimizer
        self.steps_per_env, self.num_minibatches = int(steps_per_env), int(num_minibatches)
        self.epochs_per_batch, self.gamma, self.lmda = int(epochs_per_batch), float(gamma), float(lmda)
        self.report_interval, self.test_interval = int(report_interval), int(test_interval)
        self.seed, self.test_runner, self.on_report, self.on_batch = int(seed), test_runner, on_report, on_batch
        self.report_chunk_rows, self.record_events, self.loss_kwargs = int(report_chunk_rows), bool(record_events), loss_kwargs
        self.events = []
        self.batches_done = 0           # the deal's epoch is batches_done * epochs_per_batch + k
        self.host_visits = 0            # .item() calls made by train(): the row count of a multi-agent window
        self.sums = None                # ppo_loss.sums of the last minibatch
        self._deals = {}
        self.checkpointer = checkpointer
        if checkpointer is not None and checkpointer.root is None:
            checkpointer.root, checkpointer.model, checkpointer.optimizer = self, model, optimizer

    @property
    def num_steps(self):
        return self.runner.num_steps

    def deal(self, num_rows):
        """The ``MinibatchDeal`` of batches of ``num_rows`` rows, made on first use."""
        deal = self._deals.get(num_rows)
        if deal is None:
            deal = self._deals[num_rows] = MinibatchDeal(num_rows, self.num_minibatches, self.seed)
        return deal

    def train_batch(self, batch):
        """``train_batch`` on the next ``epochs_per_batch`` epochs of the batch's deal."""
        return train_batch(self.model, self.optimizer, batch, self.deal(int(batch.actions.shape[0])),
                           self.batches_done * self.epochs_per_batch, self.epochs_per_batch, **self.loss_kwargs)

    def report(self, batch):
        """``ppo_report`` of the batch -> the device tensor."""
        return ppo_report(self.model, batch, chunk_rows=self.report_chunk_rows, **self.loss_kwargs)

    def test(self):
        return self.test_runner.run_episodes()

    def train(self, steps):
        """``PPO.train(steps)``: iterations until ``num_steps`` has grown by at least ``steps``."""
        from .dqn import round_up
        runner = self.runner
        multi = bool(getattr(runner, "_multi_agent", False))
        max_steps = runner.num_steps + int(steps)
        while runner.num_steps < max_steps:
            next_report = round_up(runner.num_steps, self.report_interval)
            next_test = round_up(runner.num_steps, self.test_interval)
            batch = runner.gen_training_batch(self.steps_per_env, self.gamma, self.lmda)
            if multi:
                self.host_visits += 1
            self.sums = self.train_batch(batch)
            self.batches_done += 1
            num_steps = runner.num_steps
            if self.on_batch is not None:
                self.on_batch(num_steps)
            save_due = self.checkpointer is not None and self.checkpointer.due(num_steps)
            reported = num_steps >= next_report and self.on_report is not None
            if reported:
                self.on_report(num_steps, self.report(batch))
            tested = self.test_runner is not None and num_steps >= next_test
            if tested:
                self.test()
            if self.record_events:
                self.events.append((num_steps, reported, tested))
            if save_due:
                self.checkpointer.save(num_steps)
        if self.checkpointer is not None:
            self.checkpointer.save(runner.num_steps)

    def _checkpoint_state(self):
        """``checkpoint.py``: where the deal stands, and the events so far; the runner and the test runner carry the
        rest."""
        config = dict(steps_per_env=self.steps_per_env, num_minibatches=self.num_minibatches,
                      epochs_per_batch=self.epochs_per_batch, gamma=self.gamma, lmda=self.lmda,
                      report_interval=self.report_interval, test_interval=self.test_interval, seed=self.seed,
                      loss_kwargs=self.loss_kwargs)
        return config, dict(batches_done=self.batches_done, host_visits=self.host_visits, events=self.events), {}

    def _checkpoint_loaded(self):
        self.events = [tuple(e) for e in self.events]

    def state_dict(self):
        """What a checkpoint needs beside the model's and the optimiser's own: where the schedule and the deal stand."""
        return dict(num_steps=int(self.runner.num_steps), batches_done=int(self.batches_done), seed=int(self.seed))

    def load_state_dict(self, state):
        self.runner.num_steps = int(state["num_steps"])
        self.batches_done = int(state["batches_done"])
        if int(state["seed"]) != self.seed:
            self.seed = int(state["seed"])
            self._deals = {}
