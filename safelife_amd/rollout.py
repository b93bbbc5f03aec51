"""
``RolloutBuffer`` -- a window of ``VectorRunner`` steps kept on the device, and the PPO training batch made from it.

The reference's ``PPO.gen_training_batch`` (training/ppo.py:74-143) strings the tuples of ``take_one_step`` into
per-agent trajectories on the host, bootstraps the open ones with ``V(next_obs)``, computes discounted returns and GAE
advantages with numpy and flattens everything into the six tensors ``train_batch`` consumes.  Here the window is a set
of time-major ``[T, B]`` tensors: ``record`` writes one row per step with one kernel (``slhip_rollout_record``), and
``finish`` runs the returns / advantages of the whole window in one more (``slhip_training_batch``), bit exact with the
reference's numpy arithmetic -- including the float64 islands its ``np.append`` creates (closed trajectories and
trajectories of one step are computed in float64, open ones of two steps or more in the rewards' dtype; see
include/safelife_hip.h and DESIGN.md section 4.5).

Order of the flattened batch.  The reference concatenates trajectory after trajectory; ``finish`` flattens the window in
time-major order, row ``t * B + b`` being step ``t`` of env ``b``.  ``train_batch`` shuffles the rows before it cuts
minibatches, so the order carries no meaning; whoever needs the reference's segmentation takes ``traj_start`` (1 where a
row starts a trajectory) and regroups.

``MultiAgentRolloutBuffer`` is the same for ``SafeLifeMultiAgentVectorEnv``: the window is ``[T, B * A]`` plus ``active``
(who took part in which step), and ``finish`` hands out the ACTIVE rows only, as the reference does (a finished agent
gets no row until its env reloads: training/base_algo.py:152-244).
"""
import collections
import ctypes as C

from . import _hip

TrainingBatch = collections.namedtuple("TrainingBatch", "obs actions action_prob returns advantages values")
DenseTrainingBatch = collections.namedtuple("DenseTrainingBatch", TrainingBatch._fields + ("valid",))


class _Window(object):
    """What the two buffers share: the time-major ``[T, N]`` tensors of a window of N columns, ``struct sl_rollout`` filled
    from them, the conversion of a step's fields into what the record kernels read, their call, and the status word."""

    _bad_action = None                  # check_status()'s message for ROLLOUT_BAD_ACTION

    def _allocate(self, struct, T, N, obs_shape, obs_dtype, reward_dtype, device, traj_start=True):
        """The window's tensors as attributes, and ``struct`` (the ``sl_rollout`` to fill) pointing at them."""
        import torch
        self.torch = torch
        reward_dtype = torch.float32 if reward_dtype is None else reward_dtype
        if reward_dtype not in (torch.float32, torch.float64):
            raise ValueError("reward_dtype must be torch.float32 or torch.float64")
        self.device = dev = _hip.device() if device is None else torch.device(device)
        self.steps, self.reward_dtype = T, reward_dtype
        self.obs = None
        if obs_shape is not None:
            self.obs = torch.zeros((T, N) + tuple(obs_shape), dtype=obs_dtype or torch.float32, device=dev)
        self.actions = torch.zeros((T, N), dtype=torch.int32, device=dev)
        self.action_prob = torch.zeros((T, N), dtype=torch.float32, device=dev)
        self.rewards = torch.zeros((T, N), dtype=reward_dtype, device=dev)
        self.values = torch.zeros((T, N), dtype=torch.float32, device=dev)
        self.done = torch.zeros((T, N), dtype=torch.uint8, device=dev)
        self.returns = torch.zeros((T, N), dtype=torch.float32, device=dev)
        self.advantages = torch.zeros((T, N), dtype=torch.float32, device=dev)
        self.traj_start = torch.zeros((T, N), dtype=torch.uint8, device=dev) if traj_start else None
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._lib = _hip.lib()
        struct.T, struct.B = T, N
        struct.reward_dtype = _hip.REWARD_F64 if reward_dtype == torch.float64 else _hip.REWARD_F32
        struct.row_stride = struct.out_stride = N
        for name in ("actions", "action_prob", "rewards", "values", "done", "status"):
            setattr(struct, name, getattr(self, name).data_ptr())

    def _as(self, x, dtype, shape):
        torch = self.torch
        if not torch.is_tensor(x):
            x = torch.as_tensor(x)
        elif x.dtype == dtype and x.device == self.device and x.is_contiguous() and (
                tuple(x.shape) == shape or (shape[-1] == -1 and x.dim() == len(shape) and x.shape[0] == shape[0])):
            return x                            # what VectorRunner hands over, but for the int64 actions
        x = x.to(device=self.device, dtype=dtype).reshape(shape)
        return x if x.is_contiguous() else x.contiguous()

    def _step_tensors(self, t, step, N):
        """``t`` and the step's reward dtype checked; its actions, policies, rewards, values and done over the N columns
        as the record kernels read them."""
        torch = self.torch
        if not 0 <= t < self.steps:
            raise ValueError("t outside [0, steps)")
        if step.rewards.dtype != self.reward_dtype:
            raise ValueError("rewards are %s, the buffer was built for %s" % (step.rewards.dtype, self.reward_dtype))
        done = step.done
        if torch.is_tensor(done) and done.dtype == torch.bool:
            done = done.view(torch.uint8)       # (a bool tensor is one byte of 0 / 1 per element)
        return (self._as(step.actions, torch.int32, (N,)), self._as(step.policies, torch.float32, (N, -1)),
                self._as(step.rewards, self.reward_dtype, (N,)), self._as(step.values, torch.float32, (N,)),
                self._as(done, torch.uint8, (N,)))

    def _record(self, entry, t, tensors, *more):
        """One of the record entry points on row ``t``, on the current stream."""
        actions, probs, rewards, values, done = tensors
        rc = entry(self._sref, int(t), _hip.ptr(actions), _hip.ptr(probs), probs.shape[1], _hip.ptr(rewards),
                   _hip.ptr(values), _hip.ptr(done), *more, _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)

    def check_status(self):
        """Read the status word (a host visit) and raise on a recorded action outside the policy's range or, where rows
        are gathered by id, a bad row id."""
        word = int(self.status.item())
        if word & _hip.ROLLOUT_BAD_ACTION:
            raise ValueError(self._bad_action)
        if word & _hip.ROLLOUT_BAD_INDEX:
            raise ValueError("%s: a row id outside the window was gathered" % type(self).__name__)


class RolloutBuffer(_Window):
    """
    Parameters
    ----------
    num_envs, steps : int        B and T of the window
    obs_shape, obs_dtype         shape of ONE env's observation and its torch dtype: ``obs`` is ``[T, B, *obs_shape]``
                                 (None: no observation store, ``finish().obs`` is None)
    reward_dtype                 torch.float32 (``env.reward``) or torch.float64 (``env.shaped_reward`` under wrappers)
    device                       the torch device
    traj_start : bool            also keep ``traj_start`` uint8 [T, B] (written by ``finish``)

    ``status`` is a device word: bit ROLLOUT_BAD_ACTION is raised by a recorded action outside [0, n_actions).
    """

    _bad_action = "RolloutBuffer: an action outside [0, n_actions) was recorded (its probability reads 0)"

    def __init__(self, num_envs, steps, obs_shape=None, obs_dtype=None, reward_dtype=None, device=None, traj_start=True):
        T, B = int(steps), int(num_envs)
        if T < 1 or B < 1:
            raise ValueError("RolloutBuffer needs steps >= 1 and num_envs >= 1")
        self.num_envs = B
        self.struct = _hip.Rollout()
        self._allocate(self.struct, T, B, obs_shape, obs_dtype, reward_dtype, device, traj_start)
        self._sref = C.byref(self.struct)

    def record(self, t, step):
        """Row ``t`` of the window from a ``StepResult`` (or any object with obs, actions, rewards, done, policies,
        values): the observation with ``copy_``, the rest -- the action's own probability included -- with one kernel on
        the current stream."""
        tensors = self._step_tensors(t, step, self.num_envs)
        if self.obs is not None:
            self.obs[t].copy_(step.obs)
        self._record(self._lib.slhip_rollout_record, t, tensors)

    def finish(self, final_values, gamma=0.97, lmda=0.95):
        """Returns and advantages of the recorded window; the reference's ``named_output`` of ``gen_training_batch``:
        ``obs actions action_prob returns advantages values``, each ``[T * B, ...]`` in time-major order (views of the
        buffer's tensors; ``actions`` an int64 copy).  final_values: float32 [B], ``V(next_obs)`` of the last step (the
        kernel ignores it where that step has ``done``).  No host visit: ``check_status()`` is the caller's to make."""
        torch, T, B = self.torch, self.steps, self.num_envs
        fv = self._as(final_values, torch.float32, (B,))
        rc = self._lib.slhip_training_batch(self._sref, _hip.ptr(fv), float(gamma), float(lmda), _hip.ptr(self.returns),
                                            _hip.ptr(self.advantages), _hip.ptr(self.traj_start),
                                            _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)
        obs = None if self.obs is None else self.obs.view((T * B,) + tuple(self.obs.shape[2:]))
        return TrainingBatch(obs, self.actions.view(T * B).to(torch.int64), self.action_prob.view(T * B),
                             self.returns.view(T * B), self.advantages.view(T * B), self.values.view(T * B))


class MultiAgentRolloutBuffer(_Window):
    """
    A window of ``MultiAgentRunner`` steps: ``[T, B * A]`` columns, column ``b * A + a`` being agent ``a`` of env ``b``,
    with ``active`` uint8 ``[T, B * A]`` next to the arrays of ``RolloutBuffer``.  The state the reference carries from
    step to step -- and from window to window -- is ``active_now`` uint8 ``[B, A]`` (its ``~last_done``) and
    ``num_resets`` int64 ``[B]``; ``record`` moves both on (``slhip_rollout_record_multi``, one launch).  Every buffer
    has a pair of its own, for whoever records windows by hand; a runner, whose windows come and go, keeps the pair of
    a one-step buffer for its whole life and names it to ``record``.

    Parameters
    ----------
    num_envs, n_agents, steps : int     B, A and T
    obs_shape, obs_dtype                shape of ONE agent's observation and its torch dtype: ``obs`` is
                                        ``[T, B * A, *obs_shape]`` (None: no observation store)
    reward_dtype                        torch.float32 (the multi-agent env's ``reward`` and ``shaped_reward``) or float64
    device                              the torch device

    ``status`` is a device word: ROLLOUT_BAD_ACTION (an active agent's action outside [0, n_actions)), ROLLOUT_BAD_INDEX.
    """

    _bad_action = "MultiAgentRolloutBuffer: an active agent's action lay outside [0, n_actions)"

    def __init__(self, num_envs, n_agents, steps, obs_shape=None, obs_dtype=None, reward_dtype=None, device=None):
        T, B, A = int(steps), int(num_envs), int(n_agents)
        if T < 1 or B < 1 or not 1 <= A <= _hip.SL_MAX_AGENTS:
            raise ValueError("MultiAgentRolloutBuffer needs steps >= 1, num_envs >= 1 and 1 <= n_agents <= %d"
                             % _hip.SL_MAX_AGENTS)
        self.num_envs, self.n_agents = B, A
        N = self.columns = B * A
        m = self.struct = _hip.RolloutMulti()
        self._allocate(m.w, T, N, obs_shape, obs_dtype, reward_dtype, device)
        torch, dev = self.torch, self.device
        self.active = torch.zeros((T, N), dtype=torch.uint8, device=dev)
        #: num_resets of every env DURING step t (the middle entry of the reference's agent ids)
        self.resets_at = torch.zeros((T, B), dtype=torch.int64, device=dev)
        self.active_now = torch.ones((B, A), dtype=torch.uint8, device=dev)
        self.num_resets = torch.zeros(B, dtype=torch.int64, device=dev)
        self.rows_all = torch.zeros(T * N, dtype=torch.int64, device=dev)
        self.count = torch.zeros(1, dtype=torch.int64, device=dev)
        m.n_agents, m.active = A, self.active.data_ptr()
        self._sref = C.byref(m)
        self._scan = torch.zeros(self._lib.slhip_rollout_compact_chunks(self._sref), dtype=torch.int32, device=dev)
        self.rows = self.agent_ids = None

    def record(self, t, step, state=None):
        """Row ``t`` of the window from a step of all ``B * A`` agents (an object with obs, actions, rewards, done,
        policies, values shaped ``[B, A, ...]`` or ``[B * A, ...]``).  What ``active_now`` says decides which columns are
        kept -- the others record zeros, whatever the step holds for them -- and then ``active_now`` / ``num_resets``
        move on to the next step.  They are those of ``state``, another ``MultiAgentRolloutBuffer`` of the same B and A,
        or the window's own.  The observation goes with ``copy_``, everything else with one kernel."""
        state = self if state is None else state
        if state.active_now.shape != self.active_now.shape:
            raise ValueError("state is for another number of envs or agents")
        tensors = self._step_tensors(t, step, self.columns)
        if self.obs is not None:
            self.obs[t].copy_(step.obs.reshape(self.obs.shape[1:]))
        self.resets_at[t].copy_(state.num_resets)
        self._record(self._lib.slhip_rollout_record_multi, t, tensors, _hip.ptr(state.active_now), _hip.ptr(state.num_resets))

    def finish(self, final_values, gamma=0.97, lmda=0.95, gather_obs=True, dense=False):
        """Returns and advantages of the recorded window (``slhip_training_batch_multi``), then the reference's
        ``named_output`` of ``gen_training_batch`` -- ``obs actions action_prob returns advantages values`` -- for the
        ACTIVE rows only, in ``(t, b, a)`` order: ``slhip_rollout_compact`` numbers them, ``slhip_rollout_gather`` moves
        them.  ``self.rows`` then holds their dense ids ``(t * B + b) * A + a`` and ``self.agent_ids`` ``[N, 3]`` the
        reference's ``(env index, resets so far, agent)`` per row; ``self.traj_start`` stays ``[T, B * A]``.

        The outputs have N rows and N is only known on the device: reading it (``count.item()``) is the ONE host visit of
        a window.  ``dense=True`` makes none: it returns a ``DenseTrainingBatch``, the ``[T * B * A]`` views of the buffer's tensors
        plus ``valid`` (uint8, 1 for an active row); rows with ``valid == 0`` hold zeros in the recorded tensors and
        whatever they held before in returns / advantages.

        final_values: float32 ``[B, A]``, ``V(next_obs)`` of the last step (ignored for an agent that is gone or done
        there).  ``gather_obs=False`` leaves ``obs`` None."""
        torch, T, N = self.torch, self.steps, self.columns
        fv = self._as(final_values, torch.float32, (N,))
        stream = _hip.current_stream_ptr()
        rc = self._lib.slhip_training_batch_multi(self._sref, _hip.ptr(fv), float(gamma), float(lmda),
                                                  _hip.ptr(self.returns), _hip.ptr(self.advantages),
                                                  _hip.ptr(self.traj_start), stream)
        if rc:
            _hip.check(rc)
        if dense:
            obs = None if self.obs is None or not gather_obs else self.obs.view((T * N,) + tuple(self.obs.shape[2:]))
            return DenseTrainingBatch(obs, self.actions.view(T * N).to(torch.int64), self.action_prob.view(T * N),
                                      self.returns.view(T * N), self.advantages.view(T * N), self.values.view(T * N),
                                      self.active.view(T * N))
        rc = self._lib.slhip_rollout_compact(self._sref, _hip.ptr(self.rows_all), _hip.ptr(self.count), _hip.ptr(self._scan),
                                             stream)
        if rc:
            _hip.check(rc)
        n = int(self.count.item())              # the window's one host visit: the outputs' size
        dev = self.device
        rows = self.rows = self.rows_all[:n]
        obs = src = None
        obs_bytes = 0
        if self.obs is not None and gather_obs:
            src = self.obs
            obs = torch.empty((n,) + tuple(src.shape[2:]), dtype=src.dtype, device=dev)
            obs_bytes = src[0, 0].numel() * src.element_size()
        actions = torch.empty(n, dtype=torch.int64, device=dev)
        prob, ret, adv, val = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4))
        rc = self._lib.slhip_rollout_gather(self._sref, _hip.ptr(rows), n, _hip.ptr(self.returns), _hip.ptr(self.advantages),
                                            _hip.ptr(src), obs_bytes, _hip.ptr(obs), _hip.ptr(actions), _hip.ptr(prob),
                                            _hip.ptr(ret), _hip.ptr(adv), _hip.ptr(val), stream)
        if rc:
            _hip.check(rc)
        A = self.n_agents
        env = torch.div(rows, A, rounding_mode="floor")
        t, b = torch.div(env, self.num_envs, rounding_mode="floor"), env % self.num_envs
        self.agent_ids = torch.stack([b, self.resets_at[t, b], rows % A], dim=1)
        return TrainingBatch(obs, actions, prob, ret, adv, val)
