"""
The driver loops of the reference's trainers, batched and device-resident.

The reference steps a Python list of environments one by one: ``obs_for_envs`` collects the observations of
the active agents, the algorithm's ``take_one_step`` runs the model on them and samples an action per agent
with numpy on the host, ``act_on_envs`` steps every env, resets the ones that finished and remembers their
last observation (training/base_algo.py:152-244, training/ppo.py:61-73).  Here the envs are one
``SafeLifeVectorEnv``: the observation arrives from the step kernel already in the layout the policy network
convolves (``policy_layout``), actions are sampled on the device, finished envs are reloaded inside the step
kernel (``auto_reset``), and nothing visits the host.

What carries over from the reference, per step and per agent (= per env for ``VectorRunner``, ``DQNRunner`` and
``PipelinedRunner``; ``MultiAgentRunner`` and ``MultiAgentDQNRunner`` drive envs with several agents):
``obs, actions, rewards, done, next_obs, agent_ids, policies, values`` with the reference's meaning --
``done`` describes the step that was just taken, ``next_obs`` of a finished env is already the first
observation of its next episode, and an agent id changes when its env resets (``(env index, resets so far)``
instead of ``(id(env), env.num_resets, k)``), so trajectories are strung together exactly as
``gen_training_batch`` does.

``VectorRunner``, ``DQNRunner``, ``MultiAgentRunner`` and ``MultiAgentDQNRunner`` are one loop, ``_Runner``: it reads
the env's facts and holds every piece of a step that they share (first reset, model call, check of what the model
returned, device draw, env step).  A runner puts the pieces in its order and adds what is its own: its draw, what its
step result is made of, and ``gen_training_batch`` or ``collect``.  The two multi-agent runners keep who is active in an
``_AgentState`` each.  ``PipelinedRunner`` is another loop (groups of envs on streams of their own).

``run_episodes`` of the shared loop is the reference's evaluation (training/base_algo.py:278-318): exactly N episodes over
the env's ``episode_run.EpisodeRun``, every runner stepping with its own ``take_one_step``.
"""
import collections

from . import _hip

StepResult = collections.namedtuple("StepResult", "obs actions rewards done next_obs agent_ids policies values")
DQNStep = collections.namedtuple("DQNStep", "obs actions rewards done next_obs agent_ids")
MultiAgentStep = collections.namedtuple("MultiAgentStep", StepResult._fields + ("active",))
MultiAgentDQNStep = collections.namedtuple("MultiAgentDQNStep", DQNStep._fields + ("active",))

_SPLITMIX_G = 0x9E3779B97F4A7C15        # the increment of the draw kernel's splitmix64 (slhip_sample_actions)


def _shifted_seed(seed, first_row):
    """The seed for a draw kernel whose row 0 is row ``first_row`` of the whole run: a draw is then a function of
    ``(seed, counter, row of the whole run)`` however the rows are dealt to shards or groups."""
    return (int(seed) + _SPLITMIX_G * int(first_row)) & (2 ** 64 - 1)


def _float32_rows(torch, x):
    """What the draw kernels read: float32, contiguous."""
    return x if (x.dtype == torch.float32 and x.is_contiguous()) else x.to(torch.float32).contiguous()


class _Runner(object):
    """The loop under ``VectorRunner``, ``DQNRunner``, ``MultiAgentRunner`` and ``MultiAgentDQNRunner``: the checks of the
    env, its facts (the single-agent env underneath, agents per env, rows = agents in all, the reward the trainers see)
    and the pieces of a step.  A subclass says what only it knows in the class attributes below."""

    _env_class, _multi_agent = "SafeLifeVectorEnv", False
    _reloads = "finished envs reload inside the step kernel"
    _bad_output = None                  # the ValueError of _draw_input

    def __init__(self, env, cast_obs):
        import torch
        self.torch = torch
        A = getattr(env, "n_agents", None)
        if env.policy_tensor is None or (self._multi_agent and A is None):
            raise ValueError("%s needs %s(policy_layout=...)" % (type(self).__name__, self._env_class))
        self._base = getattr(env, "base", env)
        if not self._base.auto_reset:
            raise ValueError("%s needs auto_reset=True (%s)" % (type(self).__name__, self._reloads))
        self.env, self.cast_obs = env, cast_obs
        B = env.num_envs
        self._per_agent = (B,) if A is None else (B, A)         # the shape of one entry per agent
        self._rows = B * (1 if A is None else A)
        self.env_ids = torch.arange(B, device=env.device, dtype=torch.int64)
        self.num_steps = 0          # agent steps as ppo.py:134 / dqn.py:191 count them: env steps * envs
        self._started = False

    def _device_draws(self, seed):
        """For a runner that draws with the library's kernels: the action of row ``r`` (agent ``a`` of env ``e`` is row
        ``e * A + a``) at step ``c`` is a function of ``(seed, c, env_offset * A + r)`` and the model's output alone."""
        self.seed = _shifted_seed(seed, self._base.env_offset * (self._rows // self.env.num_envs))
        self.actions = self.torch.zeros(self._per_agent, dtype=self.torch.int32, device=self.env.device)
        self.draws = 0              # the draw counter: steps taken
        self._lib = _hip.lib()

    def _reward(self):
        """What the reference's trainers see is the reward as the wrapper stack hands it on (movement bonus, exit bonus,
        side-effect penalty: env_factory.py:277-283 wraps the env before base_algo steps it): the wrapped reward when the
        env was built with ``wrappers=``, the game's otherwise."""
        shaped = getattr(self.env, "shaped_reward", None)
        return shaped if shaped is not None else self.env.reward

    def _obs(self):
        """The env's observation tensor; the first call resets the envs (training/base_algo.py:166-171)."""
        if not self._started:
            self.env.reset()
            self._started = True
        return self.env.policy_tensor

    def _agent_rows(self, obs):
        """``obs`` with one row per agent."""
        return obs

    def _call(self, model, obs):
        """The model on one row per agent: float32 (training/ppo.py:64, dqn.py:97), or with ``cast_obs=False`` the env's
        tensor as it is (a uint8 policy tensor stays uint8)."""
        torch = self.torch
        x = self._agent_rows(obs)
        with torch.no_grad():
            return model(x if (x.dtype == torch.float32 or not self.cast_obs) else x.to(torch.float32))

    def _draw_input(self, x):
        """Probabilities or Q-values as the draw kernels read them: float32, contiguous, ``[rows, n]``."""
        x = _float32_rows(self.torch, x)
        if x.dim() != 2 or x.shape[0] != self._rows:
            raise ValueError(self._bad_output)
        return x

    def _draw(self, entry, *args):
        """One of the draw entry points into ``self.actions``, the int32 tensor the step kernel reads."""
        rc = entry(*args, self.seed, self.draws, _hip.ptr(self.actions), _hip.current_stream_ptr())
        if rc:
            _hip.check(rc)
        self.draws += 1

    def _env_step(self, actions):
        """The fused step -> own copies of ``rewards`` and ``done`` (bool).  An env with a level schedule
        (schedule.LevelSchedule) evaluates its schedules at the runner's step count, as the reference's LinearSchedule
        reads the logger's ``training_steps``."""
        sched = getattr(self.env, "level_schedule", None)
        if sched is not None:
            sched.training_steps = int(self.num_steps)
        self.env.step(actions)
        return self._reward().clone(), self.env.done.to(self.torch.bool)

    _checkpoint_children = ("env",)

    def _checkpoint_state(self):
        """``checkpoint.py``: the step and draw counters, the action tensor the step kernel reads, the reset counters --
        and, through the env, the observation the next model call gets."""
        from . import checkpoint
        checkpoint.refuse_runner(self)
        config = dict(rows=self._rows, per_agent=self._per_agent, seed=self.seed, cast_obs=bool(self.cast_obs))
        scalars = dict(num_steps=self.num_steps, _started=self._started, draws=self.draws)
        tensors = dict(actions=self.actions)
        if self._multi_agent:
            buf = self._state.buffer
            tensors.update(num_agent_steps=self.num_agent_steps, active=buf.active_now, num_resets=buf.num_resets)
        else:
            tensors.update(num_resets=self.num_resets)
        return config, scalars, tensors

    def _live_run(self):
        """The env's ``EpisodeRun`` while a run is on (started), else None."""
        run = getattr(self.env, "episode_run", None)
        return run if (run is not None and run._live) else None

    def _mask_retired(self, actions):
        """Retired envs of a live run get action 0 (in place; ``actions`` integers ``[B]``)."""
        run = self._live_run()
        if run is not None:
            actions.mul_(run.active)
        return actions

    def _run_begins(self):
        """What a runner carries from step to step starts over with the run's reset."""

    def run_episodes(self, num_episodes=None, poll_every=16, **how):
        """The reference's ``run_episodes`` (training/base_algo.py:278-318) over the env's ``EpisodeRun``: the log's
        ``reset_summary()`` if the env has a log, ``run.start()``, steps until every ticket has been played -- the run's
        counter is read once every ``poll_every`` steps; the steps past the end are harmless, every env is retired and masked
        by then -- and the log's ``flush()``, which is what ``log_summary`` reports.  Retired envs get action 0.
        ``num_episodes`` is the run's (None: that); ``num_steps`` is not advanced, as the reference's trainers do not count
        test steps.  Returns ``run.results()``, rows by ticket."""
        run = getattr(self.env, "episode_run", None)
        if run is None:
            raise ValueError("run_episodes() needs an env built with episode_run=EpisodeRun(...)")
        if num_episodes is not None and int(num_episodes) != run.num_episodes:
            raise ValueError("the env's EpisodeRun was built for %d episodes, not %d: its result table is sized by that"
                             % (run.num_episodes, int(num_episodes)))
        poll_every = max(1, int(poll_every))
        log = getattr(self.env, "episode_log", None)
        if log is not None:
            log.reset_summary()
        num_steps = self.num_steps
        run.start()
        self._started = True
        self._run_begins()
        steps = 0
        while True:
            self.take_one_step(**how)
            steps += 1
            if steps % poll_every == 0 and run.finished():
                break
        self.num_steps = num_steps
        if log is not None:
            log.flush()
        return run.results()


class _ReplayCollector(object):
    """``collect`` of the two DQN runners."""

    def collect(self, steps, epsilon, replay):
        """``steps`` steps of every env, each added to ``replay`` (``add_to_replay``: a ``ReplayBuffer``, or a
        ``MultiAgentReplayBuffer`` for a multi-agent env); ``epsilon`` is a number or a function of ``num_steps`` (the
        reference's ``epsilon_schedule``).  ``num_steps`` counts env steps * envs.  Returns the last step."""
        step = None
        for _ in range(int(steps)):
            eps = epsilon(self.num_steps) if callable(epsilon) else epsilon
            step = self.take_one_step(float(eps))
            replay.add(step)
            self.num_steps += self.env.num_envs
        return step


class VectorRunner(_Runner):
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
    seed : int or None           an int: the draw is the library's kernel (``slhip_sample_actions``), the action of env e
                                 at step c a function of ``(seed, c, env.env_offset + e)`` and its probabilities alone --
                                 the rule of the other runners; ``generator`` is then not used.  None: ``torch.multinomial``
    """

    _bad_output = "policy must return probabilities [num_envs, n_actions]"

    def __init__(self, env, policy, generator=None, copy_obs=True, cast_obs=True, seed=None):
        super(VectorRunner, self).__init__(env, cast_obs)
        self.policy, self.generator, self.copy_obs = policy, generator, copy_obs
        self.seed = None
        if seed is not None:
            self._device_draws(seed)
        # env.num_resets of the reference
        self.num_resets = self.torch.zeros(env.num_envs, device=env.device, dtype=self.torch.int64)

    def obs_for_envs(self):
        """Current observation of every env and its agent id ``(env index, resets so far)``; the first call
        resets the envs (training/base_algo.py:166-171)."""
        return self._obs(), (self.env_ids, self.num_resets.clone())

    def act_on_envs(self, actions):
        """Step every env with its action; returns ``(next_obs, rewards, done)`` -- ``rewards`` is the wrapped
        (float64) reward when the env was built with ``wrappers=``, the game's float32 reward otherwise; the raw one
        stays available as ``env.reward``.  An env whose episode ended has
        already been reset: its ``next_obs`` row is the new episode's first observation and its reset counter is
        bumped (training/base_algo.py:231-238).  ``num_steps`` counts the calls; ``gen_training_batch`` makes it the
        reference's count."""
        torch = self.torch
        rewards, done = self._env_step(actions.to(device=self.env.device, dtype=torch.int32).contiguous())
        self.num_resets += done.to(torch.int64)
        self.num_steps += 1
        return self.env.policy_tensor, rewards, done

    def take_one_step(self):
        """training/ppo.py:61-73 without the host: model forward, one categorical draw per env on the device,
        the fused step."""
        obs, agent_ids = self.obs_for_envs()
        values, policies = self._call(self.policy, obs)
        if self.seed is None:
            stepped = actions = self._mask_retired(self.torch.multinomial(policies, 1, generator=self.generator).squeeze(1))
        else:
            probs = self._draw_input(policies)
            self._draw(self._lib.slhip_sample_actions, _hip.ptr(probs), self._rows, probs.shape[1])
            stepped = self._mask_retired(self.actions)          # the int32 tensor the step kernel reads
            actions = stepped.to(self.torch.int64)              # an own copy, int64 as the multinomial's
        kept = obs.clone() if self.copy_obs else obs
        next_obs, rewards, done = self.act_on_envs(stepped)
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
        final_values = self._call(self.policy, step.next_obs)[0]
        # training/ppo.py:134 counts agent steps: steps_per_env * len(training_envs)
        self.num_steps = steps_before + T * self.env.num_envs
        # (envs whose last step has `done` take 0.0 instead: the kernel looks at the flag itself)
        return buf.finish(final_values, gamma, lmda)


class DQNRunner(_ReplayCollector, _Runner):
    """The driver loop of the reference's DQN (training/dqn.py:93-108, 177-191) without the host: Q-values from the
    model, the epsilon-greedy draw on the device (``slhip_sample_actions_eps``: ``argmax`` taking the first maximum, or a
    uniform action with probability epsilon, straight into the int32 tensor the step kernel reads), the fused step, and
    ``collect`` feeding every step to a ``replay.ReplayBuffer``.  The action of env e at step c is a function of
    ``(seed, c, env.env_offset + e)``, its Q-values and epsilon alone.

    Parameters: `env` as for ``VectorRunner`` (``policy_layout=...``, ``auto_reset=True``);
    ``q_model(obs [B,C,W,H]) -> qvals [B,A]`` on the device; ``cast_obs``: True hands the model float32 (dqn.py:97),
    False the env's tensor as it is.
    """

    _bad_output = "q_model must return [num_envs, n_actions]"

    def __init__(self, env, q_model, seed=0, cast_obs=True):
        super(DQNRunner, self).__init__(env, cast_obs)
        self.q_model = q_model
        self._device_draws(seed)
        self.num_resets = self.torch.zeros(env.num_envs, device=env.device, dtype=self.torch.int64)

    def take_one_step(self, epsilon):
        """``obs actions rewards done next_obs agent_ids`` of one step of every env: ``obs`` is an own copy (the step
        overwrites the env's tensor), ``actions`` an own int32 copy, ``rewards`` the wrapped float64 reward when the env
        has ``wrappers=``, the game's float32 reward otherwise; ``next_obs`` is the env's tensor -- valid until the next
        step, and for a finished env already the first observation of its next episode."""
        obs = self._obs()
        agent_ids = (self.env_ids, self.num_resets.clone())
        qvals = self._draw_input(self._call(self.q_model, obs))
        self._draw(self._lib.slhip_sample_actions_eps, _hip.ptr(qvals), self._rows, qvals.shape[1], float(epsilon))
        self._mask_retired(self.actions)
        kept = obs.clone()
        rewards, done = self._env_step(self.actions)
        self.num_resets += done.to(self.torch.int64)
        return DQNStep(kept, self.actions.clone(), rewards, done, self.env.policy_tensor, agent_ids)


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
                                 self.actions.data_ptr() + 4 * lo, st.cuda_stream, _shifted_seed(self.seed, offset + lo)))

    def _checkpoint_state(self):
        from . import checkpoint
        checkpoint.refuse_runner(self)

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
                probs = _float32_rows(torch, probs)
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


class _AgentState(object):
    """What a multi-agent run carries from step to step, owned by its runner for the runner's whole life: ``active``
    uint8 ``[B, A]`` (who takes part in the NEXT step; the reference's ``~last_done``) and ``num_resets`` int64 ``[B]``.
    They are ``active_now`` / ``num_resets`` of ``buffer``, a one-step ``MultiAgentRolloutBuffer``: one kernel holds the
    rule that moves them on (``k_rollout_record_multi``), one launch per step, whether the step goes into a window
    (``window.record(t, step, state.buffer)``) or into no window at all (``advance``)."""

    _Step = collections.namedtuple("_Step", "obs actions rewards done policies values")

    def __init__(self, num_envs, n_agents, reward_dtype, device):
        from .rollout import MultiAgentRolloutBuffer
        self.buffer = buf = MultiAgentRolloutBuffer(num_envs, n_agents, 1, None, None, reward_dtype, device)
        self.active, self.num_resets = buf.active_now, buf.num_resets
        self._zeros = buf.torch.zeros(num_envs * n_agents, dtype=buf.torch.float32, device=buf.device)

    def advance(self, step, policies=None):
        """Past ``step`` (its actions, rewards and done) outside a window: the row goes into the buffer's own one step,
        which nobody reads.  A step without policies and values, a DQN step, hands in what stands for its probabilities
        -- its Q-values ``[B * A, n]`` -- and zeros stand for its values."""
        if policies is not None:
            step = self._Step(None, step.actions, step.rewards, step.done, policies, self._zeros)
        self.buffer.record(0, step)


class _MultiAgentRunner(_Runner):
    """The two multi-agent runners: the agents of one env finish at different steps; a finished agent gets no action (the
    env is handed 0 for it) until its env reloads, which happens -- inside the step kernel -- once ALL its agents are done.
    Who is active is kept on the device, in an ``_AgentState``.  The model is called on ALL ``B * A`` rows and what it
    returns for inactive rows is ignored (their action is 0 whatever it holds, NaN included): a compacted input would need
    the active count on the host every step."""

    _env_class, _multi_agent = "SafeLifeMultiAgentVectorEnv", True
    _reloads = "an env reloads inside the step kernel once all its agents are done"

    def __init__(self, env, seed, cast_obs):
        super(_MultiAgentRunner, self).__init__(env, cast_obs)
        self._device_draws(seed)
        #: active agent steps taken so far -- what ppo.py:134 would count with per-agent lists -- as a device tensor
        self.num_agent_steps = self.torch.zeros(1, dtype=self.torch.int64, device=env.device)
        self._state = _AgentState(env.num_envs, env.n_agents, self._reward().dtype, env.device)

    @property
    def active(self):
        """uint8 [B, A]: who takes part in the NEXT step."""
        return self._state.active

    @property
    def num_resets(self):
        """int64 [B]: reloads of every env so far (``env.num_resets`` of the reference)."""
        return self._state.num_resets

    def _agent_rows(self, obs):
        return obs.view((self._rows,) + tuple(obs.shape[2:]))

    def _run_begins(self):
        self._state.active.fill_(1)         # (every env has just been reset)

    def _masked_step(self, obs, x, entry, *epsilon):
        """From the model's checked output ``x`` on: the masked draw, the fused step, the agent-step count -- everything
        but moving the state on.  -> ``obs actions rewards done next_obs agent_ids active``, the first two own copies.
        The agents of an env that a live ``EpisodeRun`` has retired are inactive: action 0, no rollout or replay row."""
        run = self._live_run()
        if run is not None:
            self._state.active.mul_(run.active[:, None])
        active = self._state.active.clone()
        agent_ids = (self.env_ids, self._state.num_resets.clone())
        self._draw(entry, _hip.ptr(x), _hip.ptr(active), self._rows, x.shape[1], *epsilon)
        kept = obs.clone()
        rewards, done = self._env_step(self.actions)
        self.num_agent_steps += active.sum()
        return kept, self.actions.clone(), rewards, done, self.env.policy_tensor, agent_ids, active


class MultiAgentRunner(_MultiAgentRunner):
    """The driver loop of the reference's trainers for envs with SEVERAL agents (training/base_algo.py:152-244 with
    training/ppo.py:61-143), without the host.  A finished agent gets no row in the training batch until its env
    reloads.  ``active`` and ``num_resets`` are carried from step to step and from one ``gen_training_batch`` to the next,
    whatever the windows' lengths and whatever single steps lie between them.

    The action of agent ``a`` of env ``e`` at step ``c`` is the draw of ``slhip_sample_actions`` for row
    ``(env_offset + e) * A + a`` under ``(seed, c)``.

    Parameters: ``env`` a ``SafeLifeMultiAgentVectorEnv(policy_layout=..., auto_reset=True)``;
    ``policy(obs [B*A, C, vw, vh]) -> (values [B*A], probs float32 [B*A, n_actions])`` on the device; ``cast_obs``: True
    hands the model float32 (training/ppo.py:64), False the env's tensor as it is.
    """

    _bad_output = "policy must return probabilities [num_envs * n_agents, n_actions]"

    def __init__(self, env, policy, seed=0, cast_obs=True):
        super(MultiAgentRunner, self).__init__(env, seed, cast_obs)
        self.policy = policy
        self.rollout = None

    def _step(self):
        """Model, masked draw, fused step; the caller moves the state on."""
        obs = self._obs()
        values, policies = self._call(self.policy, obs)
        policies = self._draw_input(policies)
        step = self._masked_step(obs, policies, self._lib.slhip_sample_actions_masked)
        self.num_steps += self.env.num_envs
        return MultiAgentStep(*step[:6], policies.view(self._per_agent + (-1,)), values.reshape(self._per_agent), step[6])

    def take_one_step(self):
        """One step of every env: the ``StepResult`` fields shaped ``[B, A, ...]`` plus ``active`` uint8 ``[B, A]`` -- who
        took part; the rows of the others are to be ignored (their action is 0).  ``agent_ids`` is ``(env index [B],
        resets so far [B])``, the agent being the column.  ``rewards`` is ``env.shaped_reward`` when the env has
        ``wrappers=``, else ``env.reward``; ``next_obs`` is the env's tensor, valid until the next step.  The step is
        recorded nowhere: ``self.rollout`` and the batch of the last ``gen_training_batch`` stay as they are."""
        step = self._step()
        self._state.advance(step)
        return step

    def gen_training_batch(self, steps_per_env, gamma=0.97, lmda=0.95, gather_obs=True, dense=False):
        """training/ppo.py:74-143 for multi-agent envs without the host loop: ``steps_per_env`` steps recorded into a
        ``MultiAgentRolloutBuffer`` (``self.rollout``: ``rows``, ``agent_ids``, ``traj_start``, ``active``), the policy
        once more on the last ``next_obs`` for the bootstrap of the agents that go on, one kernel for returns and
        advantages, and the active rows gathered in ``(t, b, a)`` order -- bit exact with the reference's numpy
        arithmetic.  One host visit per window (the row count; none with ``dense=True``).  ``active`` and ``num_resets``
        persist: the next window starts with whoever is gone now."""
        from .rollout import MultiAgentRolloutBuffer
        env = self.env
        T = int(steps_per_env)
        assert T > 0
        step = self._step()
        buf = self.rollout
        if (buf is None or buf.steps != T or buf.reward_dtype != step.rewards.dtype
                or buf.obs.shape[2:] != step.obs.shape[2:] or buf.obs.dtype != step.obs.dtype):
            buf = self.rollout = MultiAgentRolloutBuffer(env.num_envs, env.n_agents, T, tuple(step.obs.shape[2:]),
                                                         step.obs.dtype, step.rewards.dtype, env.device)
        buf.record(0, step, self._state.buffer)
        for t in range(1, T):
            step = self._step()
            buf.record(t, step, self._state.buffer)
        final_values = self._call(self.policy, step.next_obs)[0]
        return buf.finish(final_values.reshape(self._per_agent), gamma, lmda, gather_obs=gather_obs, dense=dense)


class MultiAgentDQNRunner(_ReplayCollector, _MultiAgentRunner):
    """``DQNRunner`` for envs with SEVERAL agents: the reference's DQN (training/dqn.py:93-108, 177-191) over
    ``obs_for_envs`` / ``act_on_envs`` (training/base_algo.py:152-244), without the host.  A finished agent gets no row in
    the replay buffer until its env reloads.  ``collect`` counts env steps * envs in ``num_steps`` and the active agent
    steps in ``num_agent_steps``.

    The action of agent ``a`` of env ``e`` at step ``c`` is the draw of ``slhip_sample_actions_eps`` for row
    ``(env_offset + e) * A + a`` under ``(seed, c)``.

    Parameters: ``env`` a ``SafeLifeMultiAgentVectorEnv(policy_layout=..., auto_reset=True)``;
    ``q_model(obs [B*A, C, vw, vh]) -> qvals [B*A, n_actions]`` on the device; ``cast_obs``: True hands the model float32
    (dqn.py:97), False the env's tensor as it is.
    """

    _bad_output = "q_model must return [num_envs * n_agents, n_actions]"

    def __init__(self, env, q_model, seed=0, cast_obs=True):
        super(MultiAgentDQNRunner, self).__init__(env, seed, cast_obs)
        self.q_model = q_model

    def take_one_step(self, epsilon):
        """``obs actions rewards done next_obs agent_ids active`` of one step of every env, the fields shaped
        ``[B, A, ...]``: ``active`` uint8 ``[B, A]`` says who took part -- the rows of the others are to be ignored (their
        action is 0, their ``done`` stays 1 as the env reports it).  ``obs`` is an own copy, ``actions`` an own int32
        copy, ``rewards`` is ``env.shaped_reward`` when the env has ``wrappers=``, else ``env.reward``; ``next_obs`` is the
        env's tensor, valid until the next step; ``agent_ids`` is ``(env index [B], resets so far [B])``, the agent being
        the column."""
        obs = self._obs()
        qvals = self._draw_input(self._call(self.q_model, obs))
        step = MultiAgentDQNStep(*self._masked_step(obs, qvals, self._lib.slhip_sample_actions_eps_masked, float(epsilon)))
        self._state.advance(step, qvals)
        return step
