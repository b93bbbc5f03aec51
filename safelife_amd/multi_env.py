"""
SafeLifeMultiAgentVectorEnv -- B device-resident envs with A agents each: the batched counterpart of the reference's
``SafeLifeEnv(single_agent=False)`` (safelife_env.py:148-218 with the unwrapping of :162-170 not taken).

Every agent has its own points table, exit condition, reward, done flag, episode accumulators and an observation centred
on itself; the agents' actions are applied in index order (advance_board.c:217-220) and the exits turn red when ANY of
them may leave (safelife_game.py:537-552).  One fused launch per step (``slhip_env_step_multi``: the size-generic kernel
family, one workgroup per board, any board shape); an env reloads its next pool level inside the step once ALL its
agents are done (training/base_algo.py:231-236).  Levels: the reference's ``levels/random/multi-agent`` specs, or any
level with A agents -- ``LevelPool(levels, n_agents=A)``.

With ``wrappers=``, ``side_effects=`` or ``policy_layout=`` the steps go through ``slhip_env_step_multi_ex`` /
``_reset_multi_ex``: the reference's multi-agent training stack (training/env_factory.py:277-283) fused into the step,
per agent (include/safelife_hip.h, sl_multi_extras).
"""
import ctypes as C

import numpy as np

from . import _hip
from .levels import LevelPool
from .vector_env import SafeLifeVectorEnv


class SafeLifeMultiAgentVectorEnv(object):
    """
    pool : LevelPool(levels, n_agents=A)
    num_envs, time_limit, remove_white_goals, view_shape, output_channels, auto_reset, first_level, level_stride,
    env_offset, episode_streams, points_on_level_exit : as SafeLifeVectorEnv.
    wrappers, side_effects, policy_layout : the keys and meaning of SafeLifeVectorEnv's, per agent:
        ``shaped_reward``  float32 [B, A]: what the outermost wrapper returns (each wrapper rounds to float32, as the
                           reference's in-place updates of its float32 reward array do); done agents keep being shaped
        ``policy_tensor``  [B, A, C, view_w, view_h] uint8 / float32
        ``side_effects_flush()``: a ``SideEffectBatch`` with one entry per env EPISODE (queued on the step where every
                           agent is done), whose ``agent_records()`` hold every agent's record of that step
    level_schedule : schedule.LevelSchedule (built on this pool) or None
        the reference's level iterators and exit-difficulty schedule on the device, as for SafeLifeVectorEnv: the env's
        first levels are the schedule's ``first_levels`` (unless ``first_level`` is given), every reload takes its successor
        from the schedule's table, an episode files one performance record -- the average over the env's agents, on the
        step where the last of them finishes -- and every agent's required points follow ``min_performance_fraction``.
        Two extra launches per step on the caller's stream, three in curriculum mode.
    episode_log : episode_log.MultiAgentEpisodeLog (built on this pool, for num_envs envs) or None
        the reference's ``SafeLifeLogger`` for arrays over the agents, on the device: one more launch per ``step()``, behind
        the schedule's harvest on the same stream, files a row for every env whose agents are all done; ``episode_log.flush()``
        joins the side-effect queue's totals in and folds the new rows into the per-name running summaries.  Needs
        ``auto_reset=True``.  None: no launch and no allocation.
    episode_run : episode_run.EpisodeRun (built on this pool with ``n_agents=A``) or None
        a bounded evaluation run, the reference's ``run_episodes(envs, num_episodes)``: build the env with
        ``**run.env_arguments()``; after ``run.start()`` one more launch per ``step()``, in front of the log's harvest, files
        the episodes whose agents are all done by ticket, retires the envs that have no ticket left and zeroes every
        record of a retired env.  Refuses ``level_schedule`` and ``wrappers``.  None: no launch and no allocation.
    episode_history : episode_history.MultiAgentEpisodeHistory (built on this pool, for num_envs envs) or None
        the board frames of selected episodes, the reference's ``SafeLifeLogWrapper`` history and ``SafeLifeLogger``'s
        ``video_interval`` rule: two launches behind every ``step()``, in front of the run's and the log's harvests, copy the
        watched envs' boards into frame slots; an episode ends where every agent is done.  Needs ``side_effects=`` (the last
        frame comes from the finished-episode queue), ``auto_reset=True`` and a pool with static goals.  None: no launch and
        no allocation.

    ``reset()`` -> obs;  ``step(actions)`` -> (obs, reward, done, info) with
        actions  int   [B, A]   0..8 (an agent that is done takes 0: training/base_algo.py:216-219)
        obs      uint8 [B, A, view_h, view_w, C]  (int32 [B, A, view_h, view_w] holding the uint32 view for
                 ``output_channels=None``)
        reward   float32 [B, A];  done uint8 [B, A]
        info     success, times_up uint8 [B, A]; episode_reward float32, episode_length int32 [B, A] (of the episode the
                 step belonged to, before any reload)
    all views of device tensors that the next step overwrites.
    """

    def __init__(self, pool, num_envs, *, time_limit=1000, remove_white_goals=True, view_shape=(15, 15),
                 output_channels=tuple(range(16)) + (25, 26, 27), auto_reset=True, first_level=None, level_stride=1,
                 env_offset=0, with_obs=True, points_on_level_exit=1, episode_streams=True, wrappers=None,
                 side_effects=None, policy_layout=None, level_schedule=None, episode_log=None, episode_run=None,
                 episode_history=None):
        import torch
        if not isinstance(pool, LevelPool) or getattr(pool, "n_agents", 1) < 1:
            raise TypeError("pool must be a LevelPool")
        if episode_log is not None and not auto_reset:      # (refused before anything is allocated)
            raise ValueError("an episode log needs auto_reset=True: an env that stays all-done would file a row on every "
                             "step where the reference logs the episode once")
        A = int(pool.n_agents)
        if A > _hip.SL_MAX_AGENTS:
            raise ValueError("at most %d agents per board" % _hip.SL_MAX_AGENTS)
        if episode_run is not None:         # (refused before anything is allocated)
            episode_run._check_env(pool, num_envs, A, auto_reset, first_level, level_stride, env_offset, level_schedule,
                                   wrappers)
        if episode_history is not None:     # (refused before anything is allocated)
            if not hasattr(episode_history, "n_agents"):
                raise ValueError("a multi-agent env takes an episode_history.MultiAgentEpisodeHistory")
            episode_history._check_env(pool, num_envs, time_limit, side_effects, torch, None, n_agents=A,
                                       auto_reset=auto_reset)
        if level_schedule is not None:
            level_schedule._check_env(pool, A)
            if first_level is None:
                first_level = level_schedule.first_levels(num_envs, env_offset)
        # the boards, goals, generators, exit tables, the pool and the view are the single-agent env's: built once there
        self.base = base = SafeLifeVectorEnv(pool, num_envs, time_limit=time_limit, remove_white_goals=remove_white_goals,
                                             view_shape=view_shape, output_channels=output_channels, auto_reset=auto_reset,
                                             first_level=first_level, level_stride=level_stride, env_offset=env_offset,
                                             with_obs=False, points_on_level_exit=points_on_level_exit,
                                             episode_streams=episode_streams, wrappers=wrappers, side_effects=side_effects)
        self.torch, self.pool, self.device = torch, pool, base.device
        self.num_envs, self.n_agents, self.time_limit = int(num_envs), A, base.time_limit
        B = self.num_envs
        base.struct.goal_cache = None       # (the multi-agent kernels keep no goal words: nothing to drop per launch)
        self.view_shape, self.output_channels = base.view_shape, base.output_channels
        self._lib = base._lib
        dev, t = self.device, {}
        L = pool.n_slots
        t["agents"] = torch.zeros((B, A, 12), dtype=torch.int32, device=dev)           # struct sl_agent_state
        la = np.zeros((L, A, 8), np.int32)                                              # struct sl_level_agent
        la[:, :, 0:2] = pool.pool_agent_locs if A > 1 else pool.pool_agent_loc[:, None, :]
        if A > 1:
            la[:, :, 2], la[:, :, 3] = pool.pool_agent_required_reset, pool.pool_agent_required_step
            la[:, :, 4], la[:, :, 5] = pool.pool_agent_initial_points, pool.pool_agent_table_idx
        else:
            la[:, 0, 2], la[:, 0, 3] = pool.pool_required_reset, pool.pool_required_step
            la[:, 0, 4], la[:, 0, 5] = pool.pool_initial_points, pool.pool_table_idx
        t["pool_agents"] = torch.from_numpy(la).to(dev)
        t["out"] = torch.zeros((B, A, 4), dtype=torch.int32, device=dev)               # struct sl_step_out
        vh, vw = self.view_shape
        chans = self.output_channels or ()
        if not with_obs:
            self.obs = None
        elif chans:
            self.obs = torch.zeros((B, A, vh, vw, len(chans)), dtype=torch.uint8, device=dev)
        else:
            self.obs = torch.zeros((B, A, vh, vw), dtype=torch.int32, device=dev)      # uint32 payload
        self.t = t
        m = self.struct = _hip.MultiAgent()
        m.n_agents = A
        m.agents, m.pool_agents, m.out = t["agents"].data_ptr(), t["pool_agents"].data_ptr(), t["out"].data_ptr()
        m.obs = None if self.obs is None else self.obs.data_ptr()
        self._mref = C.byref(m)
        out = t["out"]
        flags = out[:, :, 1:2].view(torch.uint8)                                        # done, success, times_up, pad
        self.reward = out[:, :, 0].view(torch.float32)
        self.done = flags[:, :, 0]
        self.info = {"success": flags[:, :, 1], "times_up": flags[:, :, 2],
                     "episode_reward": out[:, :, 2].view(torch.float32), "episode_length": out[:, :, 3]}
        self.shaped_reward = self.policy_tensor = None
        self._x = None
        if wrappers or side_effects or policy_layout is not None:
            self._setup_extras(wrappers, side_effects, policy_layout)
        self.level_schedule = level_schedule
        if level_schedule is not None:      # the schedule's own successor table: redrawn before every step
            base.struct.pool_next = level_schedule._attach(self).data_ptr()
            # (the base env's sliced and queue steppers and its rollout() refuse to run under a schedule)
            base.level_schedule = level_schedule
        self.episode_log = episode_log
        if episode_log is not None:         # one launch behind every step(): a row per episode whose agents are all done
            episode_log._attach(self)
            base.episode_log = episode_log  # (the base env's sliced and queue steppers and its rollout() refuse a log too)
        self.episode_run = episode_run
        if episode_run is not None:         # one launch behind every step() of a started run, in front of the log's
            episode_run._attach(self)
            base.episode_run = episode_run  # (... and a run)
        self.episode_history = episode_history
        if episode_history is not None:     # two launches behind every step(): the watched envs' frames
            episode_history._attach(self)
            # (... and a recorder; the flush's hook that tells it of a fresh queue hangs on this too)
            base.episode_history = episode_history

    def _setup_extras(self, wrappers, side_effects, policy_layout):
        torch, t, base, dev = self.torch, self.t, self.base, self.device
        B, A = self.num_envs, self.n_agents
        H, W = self.pool.shape
        x = self.extras = _hip.MultiExtras()
        w = base.struct.wrap
        if w.flags:
            # movement_bonus * speed**power with the reference's own array expression over the agents' integer distances
            # (env_wrappers.py:80-87: speed = dist / n elementwise), every reachable distance at once
            cfg = dict(wrappers)
            bonus, power = cfg.get("movement_bonus"), cfg.get("movement_bonus_power", 1e-100)
            table = np.zeros(w.move_table_len, np.float64)
            if bonus is not None:
                dist = np.arange(w.move_table_len)
                table = bonus * (dist / w.move_period) ** power
            t["move_table"] = torch.from_numpy(np.ascontiguousarray(table, np.float64)).to(dev)
            w.move_table = t["move_table"].data_ptr()
            t["wrap_state"] = torch.zeros((B, A, 12), dtype=torch.int32, device=dev)      # struct sl_wrap_state
            t["shaped_reward"] = torch.zeros((B, A), dtype=torch.float32, device=dev)
            x.wrap_state, x.shaped_reward = t["wrap_state"].data_ptr(), t["shaped_reward"].data_ptr()
            self.shaped_reward = t["shaped_reward"]
            if w.flags & _hip.WRAP_SIDE_EFFECT:
                t["baseline"] = torch.zeros((self.pool.n_slots, H, W), dtype=torch.int16, device=dev)
                x.baseline = t["baseline"].data_ptr()
        if side_effects:
            # the base env's queue and flush machinery, with every agent's record of the queued step next to each entry
            base._se["agent_records"] = A
            base._se["queue"] = base._new_queue()
            base.struct.finished = base._se["queue"][0]
            x.finished_agents = base._se["queue"][1]["agents"].data_ptr()
        if policy_layout is not None:
            chans = self.output_channels
            if policy_layout not in ("uint8", "float32") or not chans:
                raise ValueError("policy_layout must be 'uint8' or 'float32' and needs output_channels")
            vh, vw = self.view_shape
            self.policy_tensor = torch.zeros((B, A, len(chans), vw, vh), device=dev,
                                             dtype=torch.uint8 if policy_layout == "uint8" else torch.float32)
            x.policy_obs = self.policy_tensor.data_ptr()
            x.policy_dtype = 0 if policy_layout == "uint8" else 1
        self._x = C.byref(x)

    def reset(self, mask=None):
        """SafeLifeEnv.reset() for every env (or those with mask[e] != 0)."""
        mk = None
        if mask is not None:
            mk = self.torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8)).to(self.device)
        mp = None if mk is None else mk.data_ptr()
        sched = self.level_schedule
        if sched is not None:       # (envs that have played move on to a successor: drawn now, like a step's)
            sched._before_step()
        if self._x is not None:
            _hip.check(self._lib.slhip_env_reset_multi_ex(self.base._sref, self._mref, self._x, mp, _hip.current_stream_ptr()))
        else:
            _hip.check(self._lib.slhip_env_reset_multi(self.base._sref, self._mref, mp, _hip.current_stream_ptr()))
        if sched is not None:
            sched._rewind(mk)
        if self.episode_log is not None:
            self.episode_log._rewind(mk)
        if self.episode_history is not None:
            self.episode_history._rewind(mk)
        if mk is not None:
            self.torch.cuda.current_stream().synchronize()      # (the mask tensor is the call's own)
        return self.obs

    def step(self, actions):
        torch = self.torch
        a = torch.as_tensor(actions, device=self.device).to(torch.int32).contiguous()
        if tuple(a.shape) != (self.num_envs, self.n_agents):
            raise ValueError("actions must have shape [num_envs, n_agents]")
        self._actions = a                                       # (alive until the next step)
        sched = self.level_schedule
        if sched is not None:       # draw (and required points, if due) -> the step as ever -> harvest, all on this stream
            sched._before_step()
        if self._x is not None:
            _hip.check(self._lib.slhip_env_step_multi_ex(self.base._sref, self._mref, self._x, a.data_ptr(),
                                                         _hip.current_stream_ptr()))
        else:
            _hip.check(self._lib.slhip_env_step_multi(self.base._sref, self._mref, a.data_ptr(), _hip.current_stream_ptr()))
        if sched is not None:
            sched._after_step()
        if self.episode_history is not None:
            self.episode_history._after_step()
        if self.episode_run is not None:
            self.episode_run._after_step()
        if self.episode_log is not None:
            self.episode_log._after_step()
        self.base.steps_dispatched += 1
        return self.obs, self.reward, self.done, self.info

    def render(self, env_ids=None, view_size=None, out=None):
        """``SafeLifeVectorEnv.render`` for the boards of this batch; a view is centred on agent 0 (``render_game``
        takes ``agent_locs[0]``)."""
        from . import render
        self.base._settle()
        return render.render_envs(self.base, env_ids, view_size, out, centers=self.t["agents"],
                                  center_stride=self.n_agents * 12)

    def side_effects_flush(self, overlap=False, defer=False):
        """The base env's ``side_effects_flush()`` over the episodes this env queued (one entry per env episode; the
        returned batch's ``agent_records()`` has every agent's record of the step that ended it)."""
        batch = self.base.side_effects_flush(overlap=overlap, defer=defer)
        self.extras.finished_agents = self.base._se["queue"][1]["agents"].data_ptr()
        return batch

    def side_effects_launch(self):
        self.base.side_effects_launch()

    def side_effects_join(self):
        self.base.side_effects_join()

    # (the base env last: what both name -- schedule, log, run, history -- is then filed under this env)
    _checkpoint_children = ("level_schedule", "episode_log", "episode_run", "episode_history", "base")

    def _checkpoint_state(self):
        """``checkpoint.py``: the agents' records, the per-agent level records (a schedule rewrites their required points),
        the step's output and what the wrappers and the policy layout keep; boards, generators and the queue are the base
        env's."""
        config = dict(num_envs=self.num_envs, n_agents=self.n_agents, time_limit=self.time_limit,
                      view_shape=self.view_shape, output_channels=self.output_channels)
        tensors = {k: v for k, v in self.t.items() if k != "move_table"}
        if self.obs is not None:
            tensors["obs"] = self.obs
        if self.policy_tensor is not None:
            tensors["policy_tensor"] = self.policy_tensor
        return config, {}, tensors

    def numpy(self, name):
        """Host copy of a state array: the single-agent env's names for what the env owns (board, goals, rng, num_steps,
        level_idx, episode_idx, goals_static, exit_locs), and per agent [B, A(, 2)]: agent_locs, old_value,
        required_points, initial_points, table_idx, episode_length, episode_reward, is_active, reward, done, success,
        times_up; obs."""
        if name == "obs":
            a = self.obs.cpu().numpy()
            return a.view(np.uint32) if self.output_channels is None else a
        if name == "agent_locs":
            return self.t["agents"][:, :, 0:2].cpu().numpy()
        if name in _hip.AGENT_COLS:
            col = self.t["agents"][:, :, _hip.AGENT_COLS[name]].cpu().numpy()
            return col.view(np.float32) if name == "episode_reward" else col
        if name == "reward":
            return self.reward.cpu().numpy()
        if name == "shaped_reward":
            return self.shaped_reward.cpu().numpy()
        if name in ("wrap_state", "baseline"):
            a = self.t[name].cpu().numpy()
            return a.view(np.uint16) if name == "baseline" else a
        if name == "done":
            return self.done.cpu().numpy()
        if name in ("success", "times_up"):
            return self.info[name].cpu().numpy()
        return self.base.numpy(name)
