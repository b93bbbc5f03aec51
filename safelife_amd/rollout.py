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
"""
import collections
import ctypes as C

from . import _hip

TrainingBatch = collections.namedtuple("TrainingBatch", "obs actions action_prob returns advantages values")


class RolloutBuffer(object):
    """
    Parameters
    ----------
    num_envs, steps : int        B and T of the window
    obs_shape, obs_dtype         shape of ONE env's observation and its torch dtype: ``obs`` is ``[T, B, *obs_shape]``
                                 (None: no observation store, ``finish().obs`` is None)
    reward_dtype                 torch.float32 (``env.reward``) or torch.float64 (``env.shaped_reward`` under wrappers)
    device                       the torch device
    traj_start : bool            also keep ``traj_start`` uint8 [T, B] (written by ``finish``)
    """

    def __init__(self, num_envs, steps, obs_shape=None, obs_dtype=None, reward_dtype=None, device=None, traj_start=True):
        import torch
        self.torch = torch
        T, B = int(steps), int(num_envs)
        if T < 1 or B < 1:
            raise ValueError("RolloutBuffer needs steps >= 1 and num_envs >= 1")
        reward_dtype = torch.float32 if reward_dtype is None else reward_dtype
        if reward_dtype not in (torch.float32, torch.float64):
            raise ValueError("reward_dtype must be torch.float32 or torch.float64")
        self.device = dev = _hip.device() if device is None else torch.device(device)
        self.num_envs, self.steps, self.reward_dtype = B, T, reward_dtype
        self.obs = None
        if obs_shape is not None:
            self.obs = torch.zeros((T, B) + tuple(obs_shape), dtype=obs_dtype or torch.float32, device=dev)
        self.actions = torch.zeros((T, B), dtype=torch.int32, device=dev)
        self.action_prob = torch.zeros((T, B), dtype=torch.float32, device=dev)
        self.rewards = torch.zeros((T, B), dtype=reward_dtype, device=dev)
        self.values = torch.zeros((T, B), dtype=torch.float32, device=dev)
        self.done = torch.zeros((T, B), dtype=torch.uint8, device=dev)
        self.returns = torch.zeros((T, B), dtype=torch.float32, device=dev)
        self.advantages = torch.zeros((T, B), dtype=torch.float32, device=dev)
        self.traj_start = torch.zeros((T, B), dtype=torch.uint8, device=dev) if traj_start else None
        #: device word: bit ROLLOUT_BAD_ACTION is raised by a recorded action outside [0, n_actions)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._lib = _hip.lib()
        s = self.struct = _hip.Rollout()
        s.T, s.B = T, B
        s.reward_dtype = _hip.REWARD_F64 if reward_dtype == torch.float64 else _hip.REWARD_F32
        s.row_stride = s.out_stride = B
        for name in ("actions", "action_prob", "rewards", "values", "done", "status"):
            setattr(s, name, getattr(self, name).data_ptr())
        self._sref = C.byref(s)

    def _as(self, x, dtype, shape):
        torch = self.torch
        if not torch.is_tensor(x):
            x = torch.as_tensor(x)
        elif x.dtype == dtype and x.device == self.device and x.is_contiguous() and (
                tuple(x.shape) == shape or (shape[-1] == -1 and x.dim() == len(shape) and x.shape[0] == shape[0])):
            return x                            # what VectorRunner hands over, but for the int64 actions
        x = x.to(device=self.device, dtype=dtype).reshape(shape)
        return x if x.is_contiguous() else x.contiguous()

    def record(self, t, step):
        """Row ``t`` of the window from a ``StepResult`` (or any object with obs, actions, rewards, done, policies,
        values): the observation with ``copy_``, the rest -- the action's own probability included -- with one kernel on
        the current stream."""
        torch, B = self.torch, self.num_envs
        if not 0 <= t < self.steps:
            raise ValueError("t outside [0, steps)")
        if step.rewards.dtype != self.reward_dtype:
            raise ValueError("rewards are %s, the buffer was built for %s" % (step.rewards.dtype, self.reward_dtype))
        if self.obs is not None:
            self.obs[t].copy_(step.obs)
        actions = self._as(step.actions, torch.int32, (B,))
        probs = self._as(step.policies, torch.float32, (B, -1))
        rewards = self._as(step.rewards, self.reward_dtype, (B,))
        values = self._as(step.values, torch.float32, (B,))
        done = step.done
        if torch.is_tensor(done) and done.dtype == torch.bool:
            done = done.view(torch.uint8)       # (a bool tensor is one byte of 0 / 1 per element)
        done = self._as(done, torch.uint8, (B,))
        rc = self._lib.slhip_rollout_record(self._sref, int(t), _hip.ptr(actions), _hip.ptr(probs), probs.shape[1],
                                            _hip.ptr(rewards), _hip.ptr(values), _hip.ptr(done),
                                            _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)

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

    def check_status(self):
        """Read the status word (a host visit) and raise if a recorded action lay outside the policy's range."""
        if int(self.status.item()) & _hip.ROLLOUT_BAD_ACTION:
            raise ValueError("RolloutBuffer: an action outside [0, n_actions) was recorded (its probability reads 0)")
