"""
``VectorRunner`` -- the driver loop of the reference's trainers, batched and device-resident.

The reference steps a Python list of environments one by one: ``obs_for_envs`` collects the observations of
the active agents, the algorithm's ``take_one_step`` runs the model on them and samples an action per agent
with numpy on the host, ``act_on_envs`` steps every env, resets the ones that finished and remembers their
last observation (training/base_algo.py:152-244, training/ppo.py:61-73).  Here the envs are one
``SafeLifeVectorEnv``: the observation arrives from the step kernel already in the layout the policy network
convolves (``policy_layout``), actions are sampled on the device, finished envs are reloaded inside the step
kernel (``auto_reset``), and nothing visits the host.

What carries over from the reference, per step and per agent (= per env for ``VectorRunner``, ``DQNRunner`` and
``PipelinedRunner``; ``MultiAgentRunner`` and ``MultiAgentDQNRunner`` at the end of the file drive envs with several
agents):
``obs, actions, rewards, done, next_obs, agent_ids, policies, values`` with the reference's meaning --
``done`` describes the step that was just taken, ``next_obs`` of a finished env is already the first
observation of its next episode, and an agent id changes when its env resets (``(env index, resets so far)``
instead of ``(id(env), env.num_resets, k)``), so trajectories are strung together exactly as
``gen_training_batch`` does.
"""
import collections

StepResult = collections.namedtuple("StepResult", "obs actions rewards done next_obs agent_ids policies values")
DQNStep = collections.namedtuple("DQNStep", "obs actions rewards done next_obs agent_ids")
MultiAgentStep = collections.namedtuple("MultiAgentStep", StepResult._fields + ("active",))
MultiAgentDQNStep = collections.namedtuple("MultiAgentDQNStep", DQNStep._fields + ("active",))

_SPLITMIX_G = 0x9E3779B97F4A7C15        # the increment of the draw kernel's splitmix64 (slhip_sample_actions)


def _set_training_steps(env, num_steps):
    """An env with a level schedule (schedule.LevelSchedule) evaluates its schedules at the runner's step count, as the
    reference's LinearSchedule reads the logger's ``training_steps``."""
    sched = getattr(env, "level_schedule", None)
    if sched is not None:
        sched.training_steps = int(num_steps)


def _model_in(obs, cast_obs):
    """What the model is handed: float32 (training/ppo.py:64, dqn.py:97), or with ``cast_obs=False`` the env's tensor as
    it is (a uint8 policy tensor stays uint8)."""
    import torch
    return obs if (obs.dtype == torch.float32 or not cast_obs) else obs.to(torch.float32)


class VectorRunner(object):
    """
    Parameters
    ----------
    env : SafeLifeVectorEnv      built with ``policy_layout="float32"`` (or "uint8") and ``auto_reset=True``
    policy : callable            ``policy(obs [B,C,W,H]) -> (values [B], action probabilities [B,9])`` on the
                                 device -- the interface of ``SafeLifePolicyNetwork.forward`` after its transpose
                                 (training/models.py:99-109); a torch module or any function
    generator : torch.Generator  for the action draws (device generator); None = torch's default
    copy_obs : bool              ``obs`` / ``next_obs`` of a result are views of the env's tensor, which the next
                                 step overwrites; True returns an own copy of ``obs`` (what a replay buffer needs)
    cast_obs : bool              True: the policy gets float32 (training/ppo.py:64); False: the env's tensor as it is
    """

    def __init__(self, env, policy, generator=None, copy_obs=True, cast_obs=True):
        import torch
        self.torch = torch
        if env.policy_tensor is None:
            raise ValueError("VectorRunner needs SafeLifeVectorEnv(policy_layout=...)")
        if not env.auto_reset:
            raise ValueError("VectorRunner needs auto_reset=True (finished envs reload inside the step kernel)")
        self.env, self.policy, self.generator, self.copy_obs, self.cast_obs = env, policy, generator, copy_obs, cast_obs
        B = env.num_envs
        self.env_ids = torch.arange(B, device=env.device, dtype=torch.int64)
        self.num_resets = torch.zeros(B, device=env.device, dtype=torch.int64)       # env.num_resets of the reference
        self.num_steps = 0
        self._started = False

    def obs_for_envs(self):
        """Current observation of every env and its agent id ``(env index, resets so far)``; the first call
        resets the envs (training/base_algo.py:166-171)."""
        if not self._started:
            self.env.reset()
            self._started = True
        return self.env.policy_tensor, (self.env_ids, self.num_resets.clone())

    def act_on_envs(self, actions):
        """Step every env with its action; returns ``(next_obs, rewards, done)`` -- ``rewards`` is the wrapped
        (float64) reward when the env was built with ``wrappers=``, the game's float32 reward otherwise; the raw one
        stays available as ``env.reward``.  An env whose episode ended has
        already been reset: its ``next_obs`` row is the new episode's first observation and its reset counter is
        bumped (training/base_algo.py:231-238)."""
        torch = self.torch
        a = actions.to(device=self.env.device, dtype=torch.int32).contiguous()
        _set_training_steps(self.env, self.num_steps)
        self.env.step(a)
        # what the reference's trainers see is the reward as the wrapper stack hands it on (movement bonus, exit
        # bonus, side-effect penalty: env_factory.py:277-283 wraps the env before base_algo steps it)
        shaped = getattr(self.env, "shaped_reward", None)
        rewards = shaped.clone() if shaped is not None else self.env.reward.clone()
        done = self.env.done.to(torch.bool)
        self.num_resets += done.to(torch.int64)
        self.num_steps += 1
        return self.env.policy_tensor, rewards, done

    def take_one_step(self):
        """training/ppo.py:61-73 without the host: model forward, one categorical draw per env on the device,
        the fused step."""
        torch = self.torch
        obs, agent_ids = self.obs_for_envs()
        with torch.no_grad():
            values, policies = self.policy(_model_in(obs, self.cast_obs))
        actions = torch.multinomial(policies, 1, generator=self.generator).squeeze(1)
        kept = obs.clone() if self.copy_obs else obs
        next_obs, rewards, done = self.act_on_envs(actions)
        return StepResult(kept, actions, rewards, done, next_obs, agent_ids, policies, values)

    def run_steps(self, n):
        """n steps; yields each StepResult (a generator, so that a learner can consume them as they come)."""
        for _ in range(n):
            yield self.take_one_step()

    def gen_training_batch(self, steps_per_env, gamma=0.97, lmda=0.95):
        """training/ppo.py:74-143 without the host: ``steps_per_env`` steps of ``take_one_step`` recorded into a
        device-resident ``RolloutBuffer`` (one kernel per step), the policy once more on the last ``next_obs`` for the
        open trajectories' bootstrap, and one kernel for the returns and GAE advantages, bit exact with the reference's
        numpy arithmetic.  Returns the reference's ``obs actions action_prob returns advantages values``, flattened in
        time-major order (``rollout.py`` says how that differs from the reference's trajectory order); the buffer, with
        ``traj_start``, stays available as ``self.rollout`` and is overwritten by the next call."""
        torch = self.torch
        from .rollout import RolloutBuffer
        T = int(steps_per_env)
        assert T > 0
        steps_before, copy_obs = self.num_steps, self.copy_obs
        self.copy_obs = True        # the step overwrites the env's tensor before the row is recorded
        try:
            step = self.take_one_step()
            buf = getattr(self, "rollout", None)
            if (buf is None or buf.steps != T or buf.reward_dtype != step.rewards.dtype
                    or buf.obs.shape[2:] != step.obs.shape[1:] or buf.obs.dtype != step.obs.dtype):
                buf = self.rollout = RolloutBuffer(self.env.num_envs, T, tuple(step.obs.shape[1:]), step.obs.dtype,
                                                   step.rewards.dtype, self.env.device)
            buf.record(0, step)
            for t in range(1, T):
                step = self.take_one_step()
                buf.record(t, step)
        finally:
            self.copy_obs = copy_obs
        with torch.no_grad():
            final_values = self.policy(_model_in(step.next_obs, self.cast_obs))[0]
        # training/ppo.py:134 counts agent steps: steps_per_env * len(training_envs)
        self.num_steps = steps_before + T * self.env.num_envs
        # (envs whose last step has `done` take 0.0 instead: the kernel looks at the flag itself)
        return buf.finish(final_values, gamma, lmda)


class DQNRunner(object):
    """The driver loop of the reference's DQN (training/dqn.py:93-108, 177-191) without the host: Q-values from the
    model, the epsilon-greedy draw on the device (``slhip_sample_actions_eps``: ``argmax`` taking the first maximum, or a
    uniform action with probability epsilon, straight into the int32 tensor the step kernel reads), the fused step, and
    ``collect`` feeding every step to a ``replay.ReplayBuffer``.  The action of env e at step c is a function of
    ``(seed, c, env.env_offset + e)``, its Q-values and epsilon alone.

    Parameters: `env` as for ``VectorRunner`` (``policy_layout=...``, ``auto_reset=True``);
    ``q_model(obs [B,C,W,H]) -> qvals [B,A]`` on the device; ``cast_obs``: True hands the model float32 (dqn.py:97),
    False the env's tensor as it is.
    """

    def __init__(self, env, q_model, seed=0, cast_obs=True):
        import torch
        from . import _hip
        self.torch, self._hip = torch, _hip
        if env.policy_tensor is None:
            raise ValueError("DQNRunner needs SafeLifeVectorEnv(policy_layout=...)")
        if not env.auto_reset:
            raise ValueError("DQNRunner needs auto_reset=True (finished envs reload inside the step kernel)")
        self.env, self.q_model, self.cast_obs = env, q_model, cast_obs
        B = env.num_envs
        self.seed = (int(seed) + _SPLITMIX_G * int(env.env_offset)) & (2 ** 64 - 1)
        self.env_ids = torch.arange(B, device=env.device, dtype=torch.int64)
        self.num_resets = torch.zeros(B, device=env.device, dtype=torch.int64)
        self.actions = torch.zeros(B, dtype=torch.int32, device=env.device)
        self.num_steps = 0          # agent steps, as dqn.py:191 counts them
        self.draws = 0              # the draw counter: steps taken
        self._started = False
        self._lib = _hip.lib()

    def take_one_step(self, epsilon):
        """``obs actions rewards done next_obs agent_ids`` of one step of every env: ``obs`` is an own copy (the step
        overwrites the env's tensor), ``actions`` an own int32 copy, ``rewards`` the wrapped float64 reward when the env
        has ``wrappers=``, the game's float32 reward otherwise; ``next_obs`` is the env's tensor -- valid until the next
        step, and for a finished env already the first observation of its next episode."""
        torch, env, _hip = self.torch, self.env, self._hip
        if not self._started:
            env.reset()
            self._started = True
        obs = env.policy_tensor
        agent_ids = (self.env_ids, self.num_resets.clone())
        with torch.no_grad():
            qvals = self.q_model(_model_in(obs, self.cast_obs))
        if qvals.dtype != torch.float32 or not qvals.is_contiguous():
            qvals = qvals.to(torch.float32).contiguous()
        if qvals.dim() != 2 or qvals.shape[0] != env.num_envs:
            raise ValueError("q_model must return [num_envs, n_actions]")
        rc = self._lib.slhip_sample_actions_eps(_hip.ptr(qvals), env.num_envs, qvals.shape[1], float(epsilon), self.seed,
                                                self.draws, _hip.ptr(self.actions), _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)
        self.draws += 1
        kept = obs.clone()
        _set_training_steps(env, self.num_steps)
        env.step(self.actions)
        shaped = getattr(env, "shaped_reward", None)
        rewards = shaped.clone() if shaped is not None else env.reward.clone()
        done = env.done.to(torch.bool)
        self.num_resets += done.to(torch.int64)
        return DQNStep(kept, self.actions.clone(), rewards, done, env.policy_tensor, agent_ids)

    def collect(self, steps, epsilon, replay):
        """``steps`` steps of every env, each added to ``replay`` (``add_to_replay``); ``epsilon`` is a number or a
        function of ``num_steps`` (the reference's ``epsilon_schedule``).  Returns the last step."""
        step = None
        for _ in range(int(steps)):
            eps = epsilon(self.num_steps) if callable(epsilon) else epsilon
            step = self.take_one_step(float(eps))
            replay.add(step)
            self.num_steps += self.env.num_envs
        return step


class PipelinedRunner(object):
    """The same loop with the envs in GROUPS (the env's slices), each on a stream of its own: a group's observation ->
    policy -> action draw -> step all run on that stream, in that order, so nothing inside a group needs a fence, and the
    groups overlap -- one group's step kernel runs while another group's policy does (the reference's trainers walk their
    envs one after the other, training/base_algo.py:208-238; here the walk is over groups and the device does two things
    at once).  The draw is the library's own kernel (``slhip_sample_actions``: one thread per env, straight into the
    group's part of the ONE int32 action tensor the step kernel reads); ``sampler="torch"`` uses ``torch.multinomial``
    and a copy instead (20 times the device time at 8192 envs).

    With the device sampler the action of an env at a step is a function of ``(seed, step, global env index)`` and its
    probabilities alone, the global index being ``env.env_offset + e``: the same run cut into another number of slices,
    or dealt to shards with their own ``env_offset``, draws the same actions for the same envs.  (A group that holds
    envs ``[lo, hi)`` calls the kernel with ``seed + G * (env_offset + lo) mod 2**64``, ``G`` the kernel's splitmix64
    increment, and its own step count as the counter.)

    Parameters: `env` built with ``policy_layout=...``, ``auto_reset=True``, ``slices >= 2``.
    ``policy(obs [n,C,W,H]) -> (values, probs float32 [n,9])`` gets the env's policy tensor AS IT IS (uint8 or
    float32: a network casts its own input, a cheap policy need not pay for a float copy of the observation).
    ``on_step(group, lo, hi)`` (optional) is called, with the group's stream current, after each group step: the
    group's ``env.reward[lo:hi]`` / ``env.done[lo:hi]`` / ``env.policy_tensor[lo:hi]`` are valid on that stream there.
    """

    def __init__(self, env, policy, seed=0, on_step=None, sampler="device", generator=None):
        import torch
        from . import _hip
        self.torch, self._hip = torch, _hip
        if env.policy_tensor is None or not env.auto_reset or env.slices < 2:
            raise ValueError("PipelinedRunner needs SafeLifeVectorEnv(policy_layout=..., auto_reset=True, slices>=2)")
        if sampler not in ("device", "torch"):
            raise ValueError("sampler must be 'device' or 'torch'")
        self.env, self.policy, self.on_step, self.sampler, self.generator = env, policy, on_step, sampler, generator
        self.seed = int(seed) & (2 ** 64 - 1)
        offset = int(env.env_offset)
        self.actions = torch.zeros(env.num_envs, dtype=torch.int32, device=env.device)
        self.num_steps = 0
        self._group_steps = [0] * env.slices        # steps taken per group: the draw counter of the group's next step
        self._started = False
        self._lib = _hip.lib()
        self._groups = []
        for g in range(env.slices):
            lo, hi = env.slice_bounds[g], env.slice_bounds[g + 1]
            st = env.slice_stream(g)
            # (the kernel's env e of this group is env offset + lo + e of the whole run: see slhip_sample_actions)
            self._groups.append((g, lo, hi, st, torch.cuda.stream(st), env.policy_tensor[lo:hi],
                                 self.actions.data_ptr() + 4 * lo, st.cuda_stream,
                                 (self.seed + _SPLITMIX_G * (offset + lo)) & (2 ** 64 - 1)))

    def start(self):
        if not self._started:
            self.env.reset()
            self.env.fence()                    # the groups' streams wait for the reset once
            self._started = True

    def step_group(self, g):
        torch, env = self.torch, self.env
        g, lo, hi, st, ctx, obs, act_ptr, st_ptr, group_seed = self._groups[g]
        if hi <= lo:
            return
        # Work the caller put on ITS stream since the last fence (env.reset(mask), step(), a snapshot ...) is fenced HERE,
        # while the caller's stream is still the current one: inside the group's stream context env.fence() would take
        # the group's own stream for the caller's and order the slices against the wrong one.
        if env._queues_pending:
            env._settle()
        if env._caller_ahead:
            env.fence()
        draw = self._group_steps[g]
        self._group_steps[g] = draw + 1
        with ctx:
            with torch.no_grad():
                values, probs = self.policy(obs)
            if self.sampler == "device":
                if probs.dtype != torch.float32 or not probs.is_contiguous():
                    probs = probs.to(torch.float32).contiguous()
                rc = self._lib.slhip_sample_actions(probs.data_ptr(), hi - lo, probs.shape[1], group_seed, draw, act_ptr,
                                                    st_ptr)
                if rc:
                    self._hip.check(rc)
            else:
                drawn = torch.multinomial(probs, 1, generator=self.generator)
                self.actions[lo:hi].copy_(drawn.view(-1))       # int64 -> int32, into the step's buffer
            env.step_slice(g, self.actions)
            if self.on_step is not None:
                self.on_step(g, lo, hi)

    def run(self, n_steps):
        """n_steps steps of every env."""
        self.start()
        for _ in range(n_steps):
            for g in range(self.env.slices):
                self.step_group(g)
            self.num_steps = min(self._group_steps)

    def finish(self):
        """The caller's current stream waits for every group."""
        self.env.join()


class MultiAgentRunner(object):
    """The driver loop of the reference's trainers for envs with SEVERAL agents (training/base_algo.py:152-244 with
    training/ppo.py:61-143), without the host.  The agents of one env finish at different steps; a finished agent gets no
    action (the env is handed 0 for it) and no row in the training batch until its env reloads, which happens -- inside the
    step kernel -- once ALL its agents are done.  Who is active is kept on the device (``active`` uint8 ``[B, A]``, the
    reference's ``~last_done``; ``num_resets`` int64 ``[B]``) and carried from step to step and from one
    ``gen_training_batch`` to the next.

    The reference hands its model the active agents' observations only.  Here the policy is called on ALL ``B * A`` rows
    and what it returns for inactive rows is ignored (their action is 0 whatever the probabilities hold, NaN included):
    a compacted input would need the active count on the host every step.  The action of agent ``a`` of env ``e`` at step
    ``c`` is the draw of ``slhip_sample_actions`` for row ``(env_offset + e) * A + a`` under ``(seed, c)``.

    Parameters: ``env`` a ``SafeLifeMultiAgentVectorEnv(policy_layout=..., auto_reset=True)``;
    ``policy(obs [B*A, C, vw, vh]) -> (values [B*A], probs float32 [B*A, n_actions])`` on the device; ``cast_obs``: True
    hands the model float32 (training/ppo.py:64), False the env's tensor as it is.
    """

    def __init__(self, env, policy, seed=0, cast_obs=True):
        import torch
        from . import _hip
        from .rollout import MultiAgentRolloutBuffer
        self.torch, self._hip, self._buffer = torch, _hip, MultiAgentRolloutBuffer
        if getattr(env, "n_agents", None) is None or env.policy_tensor is None:
            raise ValueError("MultiAgentRunner needs SafeLifeMultiAgentVectorEnv(policy_layout=...)")
        if not env.base.auto_reset:
            raise ValueError("MultiAgentRunner needs auto_reset=True (an env reloads inside the step kernel once all its "
                             "agents are done)")
        self.env, self.policy, self.cast_obs = env, policy, cast_obs
        B, A = env.num_envs, env.n_agents
        self.seed = (int(seed) + _SPLITMIX_G * int(env.base.env_offset) * A) & (2 ** 64 - 1)
        self.env_ids = torch.arange(B, device=env.device, dtype=torch.int64)
        self.actions = torch.zeros((B, A), dtype=torch.int32, device=env.device)
        #: agent steps taken so far -- what ppo.py:134 would count with per-agent lists -- as a device tensor
        self.num_agent_steps = torch.zeros(1, dtype=torch.int64, device=env.device)
        self.num_steps = 0          # env steps * envs, as ppo.py:134 counts
        self.draws = 0              # the draw counter: steps taken
        self.rollout = None
        # the carried state lives in a one-step buffer until gen_training_batch makes the real one
        self._state = MultiAgentRolloutBuffer(B, A, 1, None, None, self._reward_dtype(), env.device)
        self._started = False
        self._lib = _hip.lib()

    def _reward_dtype(self):
        env = self.env
        return (env.shaped_reward if env.shaped_reward is not None else env.reward).dtype

    @property
    def active(self):
        """uint8 [B, A]: who takes part in the NEXT step."""
        return self._state.active_now

    @property
    def num_resets(self):
        """int64 [B]: reloads of every env so far (``env.num_resets`` of the reference)."""
        return self._state.num_resets

    def _model_in(self, obs):
        return _model_in(obs.view((-1,) + tuple(obs.shape[2:])), self.cast_obs)

    def _step(self):
        """Model, masked draw, fused step -- everything but the bookkeeping, which ``record_multi`` does."""
        torch, env, _hip = self.torch, self.env, self._hip
        if not self._started:
            env.reset()
            self._started = True
        B, A = env.num_envs, env.n_agents
        obs = env.policy_tensor
        with torch.no_grad():
            values, policies = self.policy(self._model_in(obs))
        if policies.dtype != torch.float32 or not policies.is_contiguous():
            policies = policies.to(torch.float32).contiguous()
        if policies.dim() != 2 or policies.shape[0] != B * A:
            raise ValueError("policy must return probabilities [num_envs * n_agents, n_actions]")
        state = self._state
        active = state.active_now.clone()
        agent_ids = (self.env_ids, state.num_resets.clone())
        rc = self._lib.slhip_sample_actions_masked(_hip.ptr(policies), _hip.ptr(active), B * A, policies.shape[1],
                                                   self.seed, self.draws, _hip.ptr(self.actions),
                                                   _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)
        self.draws += 1
        kept = obs.clone()
        _set_training_steps(env, self.num_steps)
        env.step(self.actions)
        rewards = (env.shaped_reward if env.shaped_reward is not None else env.reward).clone()
        done = env.done.to(torch.bool)
        self.num_agent_steps += active.sum()
        self.num_steps += B
        return MultiAgentStep(kept, self.actions.clone(), rewards, done, env.policy_tensor, agent_ids,
                              policies.view(B, A, -1), values.reshape(B, A), active)

    def take_one_step(self):
        """One step of every env: the ``StepResult`` fields shaped ``[B, A, ...]`` plus ``active`` uint8 ``[B, A]`` -- who
        took part; the rows of the others are to be ignored (their action is 0).  ``agent_ids`` is ``(env index [B],
        resets so far [B])``, the agent being the column.  ``rewards`` is ``env.shaped_reward`` when the env has
        ``wrappers=``, else ``env.reward``; ``next_obs`` is the env's tensor, valid until the next step.  (The bookkeeping
        runs through row 0 of the buffer that holds the carried state -- after a ``gen_training_batch`` that is
        ``self.rollout``, whose window is then no longer whole.)"""
        step = self._step()
        self._state.record(0, step)         # moves active / num_resets on (the one-step window itself is not used)
        return step

    def gen_training_batch(self, steps_per_env, gamma=0.97, lmda=0.95, gather_obs=True, dense=False):
        """training/ppo.py:74-143 for multi-agent envs without the host loop: ``steps_per_env`` steps recorded into a
        ``MultiAgentRolloutBuffer`` (``self.rollout``: ``rows``, ``agent_ids``, ``traj_start``, ``active``), the policy
        once more on the last ``next_obs`` for the bootstrap of the agents that go on, one kernel for returns and
        advantages, and the active rows gathered in ``(t, b, a)`` order -- bit exact with the reference's numpy
        arithmetic.  One host visit per window (the row count; none with ``dense=True``).  ``active`` and ``num_resets``
        persist: the next window starts with whoever is gone now."""
        torch, env = self.torch, self.env
        T = int(steps_per_env)
        assert T > 0
        step = self._step()
        buf = self.rollout
        if (buf is None or buf.steps != T or buf.reward_dtype != step.rewards.dtype
                or buf.obs.shape[2:] != step.obs.shape[2:] or buf.obs.dtype != step.obs.dtype):
            buf = self.rollout = self._buffer(env.num_envs, env.n_agents, T, tuple(step.obs.shape[2:]), step.obs.dtype,
                                              step.rewards.dtype, env.device)
        if buf is not self._state:           # the carried state moves into the window's buffer
            buf.active_now.copy_(self._state.active_now)
            buf.num_resets.copy_(self._state.num_resets)
            self._state = buf
        buf.record(0, step)
        for t in range(1, T):
            step = self._step()
            buf.record(t, step)
        with torch.no_grad():
            final_values = self.policy(self._model_in(step.next_obs))[0]
        return buf.finish(final_values.reshape(env.num_envs, env.n_agents), gamma, lmda, gather_obs=gather_obs, dense=dense)


class MultiAgentDQNRunner(object):
    """``DQNRunner`` for envs with SEVERAL agents: the reference's DQN (training/dqn.py:93-108, 177-191) over
    ``obs_for_envs`` / ``act_on_envs`` (training/base_algo.py:152-244), without the host.  A finished agent gets no action
    (the env is handed 0 for it) and no row in the replay buffer until its env reloads, which happens -- inside the step
    kernel -- once ALL its agents are done.  Who is active (``active`` uint8 ``[B, A]``, ``num_resets`` int64 ``[B]``) is
    kept on the device and moved on once per step by ``slhip_rollout_record_multi``, through a one-step
    ``MultiAgentRolloutBuffer`` as in ``MultiAgentRunner``: there is one implementation of that rule.

    ``q_model`` is called on ALL ``B * A`` rows and what it returns for inactive rows is ignored (NaN included): a
    compacted input would need the active count on the host every step.  The action of agent ``a`` of env ``e`` at step
    ``c`` is the draw of ``slhip_sample_actions_eps`` for row ``(env_offset + e) * A + a`` under ``(seed, c)``.

    Parameters: ``env`` a ``SafeLifeMultiAgentVectorEnv(policy_layout=..., auto_reset=True)``;
    ``q_model(obs [B*A, C, vw, vh]) -> qvals [B*A, n_actions]`` on the device; ``cast_obs``: True hands the model float32
    (dqn.py:97), False the env's tensor as it is.
    """

    _StateStep = collections.namedtuple("_StateStep", "obs actions rewards done policies values")

    def __init__(self, env, q_model, seed=0, cast_obs=True):
        import torch
        from . import _hip
        from .rollout import MultiAgentRolloutBuffer
        self.torch, self._hip = torch, _hip
        if getattr(env, "n_agents", None) is None or env.policy_tensor is None:
            raise ValueError("MultiAgentDQNRunner needs SafeLifeMultiAgentVectorEnv(policy_layout=...)")
        if not env.base.auto_reset:
            raise ValueError("MultiAgentDQNRunner needs auto_reset=True (an env reloads inside the step kernel once all "
                             "its agents are done)")
        self.env, self.q_model, self.cast_obs = env, q_model, cast_obs
        B, A = env.num_envs, env.n_agents
        self.seed = (int(seed) + _SPLITMIX_G * int(env.base.env_offset) * A) & (2 ** 64 - 1)
        self.env_ids = torch.arange(B, device=env.device, dtype=torch.int64)
        self.actions = torch.zeros((B, A), dtype=torch.int32, device=env.device)
        #: active agent steps taken so far, as a device tensor
        self.num_agent_steps = torch.zeros(1, dtype=torch.int64, device=env.device)
        self.num_steps = 0          # env steps * envs, as dqn.py:191 counts
        self.draws = 0              # the draw counter: steps taken
        reward = env.shaped_reward if env.shaped_reward is not None else env.reward
        # the carried state and the one kernel that moves it on (the one-step window itself is not used)
        self._state = MultiAgentRolloutBuffer(B, A, 1, None, None, reward.dtype, env.device)
        self._no_values = torch.zeros(B * A, dtype=torch.float32, device=env.device)
        self._started = False
        self._lib = _hip.lib()

    @property
    def active(self):
        """uint8 [B, A]: who takes part in the NEXT step."""
        return self._state.active_now

    @property
    def num_resets(self):
        """int64 [B]: reloads of every env so far (``env.num_resets`` of the reference)."""
        return self._state.num_resets

    def take_one_step(self, epsilon):
        """``obs actions rewards done next_obs agent_ids active`` of one step of every env, the fields shaped
        ``[B, A, ...]``: ``active`` uint8 ``[B, A]`` says who took part -- the rows of the others are to be ignored (their
        action is 0, their ``done`` stays 1 as the env reports it).  ``obs`` is an own copy, ``actions`` an own int32
        copy, ``rewards`` is ``env.shaped_reward`` when the env has ``wrappers=``, else ``env.reward``; ``next_obs`` is the
        env's tensor, valid until the next step; ``agent_ids`` is ``(env index [B], resets so far [B])``, the agent being
        the column."""
        torch, env, _hip = self.torch, self.env, self._hip
        if not self._started:
            env.reset()
            self._started = True
        B, A = env.num_envs, env.n_agents
        obs = env.policy_tensor
        with torch.no_grad():
            qvals = self.q_model(_model_in(obs.view((-1,) + tuple(obs.shape[2:])), self.cast_obs))
        if qvals.dtype != torch.float32 or not qvals.is_contiguous():
            qvals = qvals.to(torch.float32).contiguous()
        if qvals.dim() != 2 or qvals.shape[0] != B * A:
            raise ValueError("q_model must return [num_envs * n_agents, n_actions]")
        state = self._state
        active = state.active_now.clone()
        agent_ids = (self.env_ids, state.num_resets.clone())
        rc = self._lib.slhip_sample_actions_eps_masked(_hip.ptr(qvals), _hip.ptr(active), B * A, qvals.shape[1],
                                                       float(epsilon), self.seed, self.draws, _hip.ptr(self.actions),
                                                       _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)
        self.draws += 1
        kept = obs.clone()
        _set_training_steps(env, self.num_steps)
        env.step(self.actions)
        rewards = (env.shaped_reward if env.shaped_reward is not None else env.reward).clone()
        done = env.done.to(torch.bool)
        self.num_agent_steps += active.sum()
        step = MultiAgentDQNStep(kept, self.actions.clone(), rewards, done, env.policy_tensor, agent_ids, active)
        # active / num_resets move on (the Q-values stand in for the probabilities of the window nobody reads)
        state.record(0, self._StateStep(None, step.actions, rewards, done, qvals, self._no_values))
        return step

    def collect(self, steps, epsilon, replay):
        """``steps`` steps of every env, each added to ``replay`` (a ``MultiAgentReplayBuffer``); ``epsilon`` is a number
        or a function of ``num_steps`` (the reference's ``epsilon_schedule``).  ``num_steps`` counts env steps * envs,
        ``num_agent_steps`` the active agent steps.  Returns the last step."""
        step = None
        for _ in range(int(steps)):
            eps = epsilon(self.num_steps) if callable(epsilon) else epsilon
            step = self.take_one_step(float(eps))
            replay.add(step)
            self.num_steps += self.env.num_envs
        return step
