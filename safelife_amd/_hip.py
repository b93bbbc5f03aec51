"""
ctypes binding of ``libsafelife_hip.so`` (the C-ABI of include/safelife_hip.h).

This is the only way the package reaches the GPU kernels.  There is no CPU
fallback: if the library is missing, or no HIP device is visible when a compute
entry point is called, an exception is raised.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SAFELIFE_HIP_LIB selects another build of the same library (A/B runs of kernel variants)
LIB_PATH = os.environ.get("SAFELIFE_HIP_LIB") or os.path.join(_HERE, "libsafelife_hip.so")

SL_MAX_CELLS = 16384
SL_MAX_CHANNELS = 32
SL_E_SHAPE, SL_E_ARG, SL_E_HIP, SL_E_UNSUPPORTED = -1, -2, -3, -4

#: every symbol include/safelife_hip.h declares
EXPORTS = (
    "slhip_abi_version", "slhip_last_error", "slhip_device_count",
    "slhip_advance_board", "slhip_advance_board_each", "slhip_life_occupancy", "slhip_alive_counts", "slhip_execute_actions",
    "slhip_env_prepare", "slhip_pool_baseline", "slhip_pool_write", "slhip_goal_cache_bytes", "slhip_env_row_kernels", "slhip_env_reset", "slhip_env_step", "slhip_env_step_slices", "slhip_env_step_range", "slhip_env_rollout",
    "slhip_streams_concurrent", "slhip_streams_order",
    "slhip_env_obs", "slhip_env_step_multi", "slhip_env_reset_multi", "slhip_env_step_multi_ex", "slhip_env_reset_multi_ex",
    "slhip_obs_to_policy", "slhip_sample_actions", "slhip_side_effects",
    "slhip_emd_workspace_bytes", "slhip_emd_batch", "slhip_emd_status",
    "slhip_gather_unique_id", "slhip_gather_init", "slhip_gather_window", "slhip_gather_destroy",
    "slhip_gather_window_async", "slhip_gather_done", "slhip_gather_wait_streams",
    "slhip_gather_window_queued",
    "slhip_queues_open", "slhip_queues_open_on", "slhip_queues_stream_shares", "slhip_gather_stream_shares", "slhip_gather_poke", "slhip_queues_mode", "slhip_queues_steps", "slhip_queues_step", "slhip_queues_stage", "slhip_queues_go", "slhip_queues_marker",
    "slhip_queues_wait", "slhip_queues_sync", "slhip_queues_close", "slhip_queues_selftest",
    "slhip_render_boards", "slhip_env_render",
    "slhip_rollout_record", "slhip_training_batch",
    "slhip_replay_add", "slhip_replay_sample", "slhip_replay_gather", "slhip_sample_actions_eps",
    "slhip_replay_add_masked", "slhip_sample_actions_eps_masked",
    "slhip_sample_actions_masked", "slhip_rollout_record_multi", "slhip_training_batch_multi",
    "slhip_rollout_compact_chunks", "slhip_rollout_compact", "slhip_rollout_gather",
    "slhip_schedule_draw", "slhip_schedule_required", "slhip_schedule_harvest", "slhip_schedule_curriculum",
    "slhip_schedule_required_multi", "slhip_schedule_harvest_multi",
    "slhip_episode_log_harvest", "slhip_episode_log_join", "slhip_episode_log_summaries", "slhip_episode_log_run_summary",
    "slhip_episode_log_harvest_multi", "slhip_episode_log_join_multi", "slhip_episode_log_summaries_multi",
    "slhip_episode_log_run_summary_multi",
    "slhip_episode_run_start", "slhip_episode_run_harvest", "slhip_episode_run_harvest_multi", "slhip_episode_run_tickets",
    "slhip_history_capture", "slhip_history_rewind", "slhip_history_capture_multi",
    "slhip_ppo_workspace_bytes", "slhip_ppo_loss_forward", "slhip_ppo_loss_backward", "slhip_minibatch_obs",
    "slhip_minibatch_keys",
    "slhip_ppo_report_workspace_bytes", "slhip_ppo_report_rows", "slhip_ppo_report_finish",
    "slhip_dqn_workspace_bytes", "slhip_dqn_loss_forward", "slhip_dqn_loss_backward",
    "slhip_state_digest_workspace_bytes", "slhip_state_digest_prefix", "slhip_state_digest",
    "slhip_gen_pattern_workspace_bytes", "slhip_gen_pattern_batch",
    "slhip_partition_workspace_bytes", "slhip_partition_batch",
)
#: slhip_partition_batch: per-problem status, the supported range
PARTITION_REFUSED, PARTITION_CAPPED = -4, -5
PARTITION_MAX_SIDE, PARTITION_MAX_REGIONS = 64, 8
#: slhip_gen_pattern_batch: per-problem status, doubles per problem, generator words per problem, supported range
GEN_PATTERN_MAX_ITER, GEN_PATTERN_REFUSED = -1, -4
GEN_PATTERN_PARAMS, GEN_PATTERN_RNG_WORDS = 12, 6
GEN_PATTERN_MAX_SIDE, GEN_PATTERN_MAX_PERIOD = 64, 4
PPO_BAD_ACTION, PPO_BAD_INDEX = 1, 2
#: sums_out of slhip_ppo_loss_forward: the doubles' names in order; slot PPO_SUM_LOSS_F32 holds a float32, not a double
PPO_SUMS = ("policy", "value", "entropy", "entropy_term", "loss", "flag", "n")
PPO_SUM_LOSS_F32 = 7
#: out of slhip_ppo_report_finish: PPO_SUMS, then these two doubles, then four float32 in slots PPO_REPORT_F32 and the next
PPO_REPORT_PARTIALS, PPO_REPORT_DOUBLES = 5, 11
PPO_REPORT_VALUES, PPO_REPORT_ADVANTAGES, PPO_REPORT_F32 = 7, 8, 9
PPO_REPORT_SCALARS = ("loss", "entropy", "values", "advantages")       # the float32 in order
DQN_BAD_ACTION, DQN_BAD_INDEX = 1, 2
DQN_FROM_RING, DQN_FROM_BATCH = 0, 1
#: sums_out of slhip_dqn_loss_forward: the doubles' names in order; slot DQN_SUM_LOSS_F32 holds a float32, not a double
DQN_SUMS = ("loss", "q_model_mean", "q_model_max", "q_target_mean", "q_target_max", "n", "reserved")
DQN_SUM_LOSS_F32 = 7
HIST_LIVE, HIST_NO_FINAL = 1, 2
HIST_SLOT_FREE, HIST_SLOT_ENV, HIST_SLOT_ENTRY = 0, 1, 2
HIST_MAX_WATCH, HIST_MAX_SLOTS, HIST_ORDER_WORDS = 1024, 1024, 8
HIST_COUNTERS = ("episodes", "kept", "missed", "incomplete", "cursor", "reserved0", "reserved1", "reserved2")
RUN_WRITTEN, RUN_SCORED = 1, 2
RUN_COUNTERS = ("completed", "in_progress", "env_steps", "reserved")
LOG_JOINED, LOG_MAX_HOPS, LOG_RUN_SUMMARY = 1, 64, 12
LOG_MAX_NAMES, LOG_NO_NAME = 16, 0xFF
#: the per-name summaries' keys of a multi-agent log, in the reference's order
LOG_MULTI_KEYS = ("length", "reward", "success", "score")
#: the summaries' keys, in the reference's order
LOG_KEYS = ("side_effects", "length", "reward", "success", "score")
LOG_COUNTERS = ("n_rows", "steps", "episodes", "summarised", "unmatched")
SCHEDULE_MAX_GROUPS, SCHEDULE_MAX_LOOKBACK = 8, 1024
SCHEDULE_BAD_PROBS = 1
REWARD_F32, REWARD_F64 = 0, 1
ROLLOUT_BAD_ACTION, ROLLOUT_BAD_INDEX = 1, 2
ROLLOUT_SCAN_CHUNK = 4096
REPLAY_MAX_N, REPLAY_MAX_K = 16, 4096
REPLAY_SHORT, REPLAY_BAD_INDEX = 1, 2
QUEUES_RELEASE_FREE = 1
QUEUES_STAGE_MAX = 48
QUEUES_SELFTEST_PLANT, QUEUES_SELFTEST_SWAP = 1, 2
SL_GATHER_ID_BYTES = 128
SL_SE_MAX_KEYS = 24


class SafeLifeHipError(RuntimeError):
    pass


class Pcg64(C.Structure):
    _fields_ = [("state_hi", C.c_uint64), ("state_lo", C.c_uint64),
                ("inc_hi", C.c_uint64), ("inc_lo", C.c_uint64)]


_p = C.c_void_p

#: field names of `struct sl_env_batch`, in order
ENV_SCALARS_HEAD = ("B", "H", "W", "E", "time_limit", "exit_points", "n_tables", "auto_reset",
                    "remove_white_goals", "view_h", "view_w", "n_channels")
ENV_STATE_PTRS = ("board", "goals", "exit_locs", "rng", "scalars", "points_table")
ENV_POOL_PTRS = ("pool_board", "pool_goals", "pool_exit_locs", "pool_rng", "pool_scalars")
ENV_POOL_TAIL = ("pool_next",)      # (optional: set by SafeLifeVectorEnv for refreshable pools)
ENV_OUT_PTRS = ("out", "obs", "score_lut")
SL_ABI_VERSION = 13

#: int32 column of each field inside `struct sl_env_scalars` (64 bytes = 16 columns)
SCALAR_COLS = {"agent_row": 0, "agent_col": 1, "num_steps": 2, "old_value": 3, "required_points": 4,
               "initial_points": 5, "table_idx": 6, "level_idx": 7, "episode_idx": 8, "episode_length": 9,
               "episode_reward": 10, "spawn_prob": 11, "goals_static": 12, "is_active": 13,
               "exit_open_at_reset": 14, "loaded": 15}
SCALAR_FLOATS = ("episode_reward", "spawn_prob")
#: `struct sl_level_scalars` (32 bytes = 8 columns)
LEVEL_COLS = {"agent_row": 0, "agent_col": 1, "required_reset": 2, "required_step": 3, "initial_points": 4,
              "table_idx": 5, "spawn_prob": 6}


WRAP_MOVEMENT, WRAP_AS_PENALTY, WRAP_EXIT_BONUS, WRAP_SIDE_EFFECT, WRAP_IGNORE_REWARD_CELLS, WRAP_INACTION = 1, 2, 4, 8, 16, 32
WRAP_MAX_PERIOD = 8


class WrapState(C.Structure):
    """`struct sl_wrap_state` (48 bytes)."""
    _fields_ = [("n_prior", C.c_int32), ("last_side_effect", C.c_int32),
                ("prior", C.c_int16 * (2 * WRAP_MAX_PERIOD)), ("reserved", C.c_int32 * 2)]


class Wrappers(C.Structure):
    """`struct sl_wrappers`."""
    _fields_ = [("flags", C.c_int32), ("move_period", C.c_int32), ("move_table_len", C.c_int32),
                ("reserved", C.c_int32),
                ("move_bonus", C.c_double), ("exit_bonus", C.c_double), ("penalty_coef", C.c_double),
                ("move_table", _p), ("state", _p), ("shaped_reward", _p), ("shaped_reward_t", _p),
                ("pool_baseline", _p), ("inaction_board", _p), ("inaction_rng", _p), ("inaction_rows", _p)]


class EpisodeRecord(C.Structure):
    """`struct sl_episode_record` (32 bytes)."""
    _fields_ = [("env", C.c_int32), ("level", C.c_int32), ("num_steps", C.c_int32), ("episode_idx", C.c_int32),
                ("spawn_prob", C.c_float), ("episode_reward", C.c_float), ("episode_length", C.c_int32),
                ("success", C.c_uint8), ("times_up", C.c_uint8), ("n_cell_types", C.c_uint8), ("reserved", C.c_uint8)]


class PoolRows(C.Structure):
    """``struct sl_pool_rows`` (slhip_pool_write)."""
    _fields_ = [("n", C.c_int32), ("slot", C.c_void_p), ("board", C.c_void_p), ("goals", C.c_void_p),
                ("exit_locs", C.c_void_p), ("rng", C.c_void_p), ("scalars", C.c_void_p), ("next", C.c_void_p),
                ("next_dst", C.c_void_p)]


class EpisodeQueue(C.Structure):
    """`struct sl_episode_queue`."""
    _fields_ = [("capacity", C.c_int32), ("env_base", C.c_int32), ("count", _p), ("records", _p), ("boards", _p)]


class AgentState(C.Structure):
    """struct sl_agent_state (48 bytes = 12 int32 columns)"""
    _fields_ = [("row", C.c_int32), ("col", C.c_int32), ("old_value", C.c_int32), ("required_points", C.c_int32),
                ("initial_points", C.c_int32), ("table_idx", C.c_int32), ("episode_length", C.c_int32),
                ("episode_reward", C.c_float), ("is_active", C.c_int32), ("reserved", C.c_int32 * 3)]


AGENT_COLS = {"row": 0, "col": 1, "old_value": 2, "required_points": 3, "initial_points": 4, "table_idx": 5,
              "episode_length": 6, "episode_reward": 7, "is_active": 8}
LEVEL_AGENT_COLS = {"row": 0, "col": 1, "required_reset": 2, "required_step": 3, "initial_points": 4, "table_idx": 5}
SL_MAX_AGENTS = 8


class MultiAgent(C.Structure):
    """struct sl_multi_agent"""
    _fields_ = [("n_agents", C.c_int32), ("reserved", C.c_int32), ("agents", C.c_void_p), ("pool_agents", C.c_void_p),
                ("out", C.c_void_p), ("obs", C.c_void_p)]


class MultiExtras(C.Structure):
    """struct sl_multi_extras"""
    _fields_ = [("wrap_state", C.c_void_p), ("shaped_reward", C.c_void_p), ("baseline", C.c_void_p),
                ("finished_agents", C.c_void_p), ("policy_obs", C.c_void_p), ("policy_dtype", C.c_int32),
                ("reserved", C.c_int32)]


class RenderArgs(C.Structure):
    """struct sl_render_args"""
    _fields_ = ([(n, C.c_int32) for n in ("N", "H", "W", "n_source", "view_h", "view_w", "E", "aux_by_index")]
                + [(n, C.c_longlong) for n in ("board_stride", "goal_stride", "center_stride")]
                + [(n, C.c_void_p) for n in ("board", "goals", "index", "sprites", "orientation", "centers", "exits", "out")])


class Rollout(C.Structure):
    """struct sl_rollout (80 bytes)"""
    _fields_ = ([(n, C.c_int32) for n in ("T", "B", "reward_dtype", "reserved")]
                + [(n, C.c_longlong) for n in ("row_stride", "out_stride")]
                + [(n, C.c_void_p) for n in ("actions", "action_prob", "rewards", "values", "done", "status")])


class RolloutMulti(C.Structure):
    """struct sl_rollout_multi (96 bytes)"""
    _fields_ = [("w", Rollout), ("n_agents", C.c_int32), ("reserved", C.c_int32), ("active", C.c_void_p)]


class Replay(C.Structure):
    """struct sl_replay (264 bytes)"""
    _fields_ = ([(n, C.c_longlong) for n in ("capacity", "obs_bytes")]
                + [(n, C.c_int32) for n in ("B", "n", "reward_dtype", "reserved")]
                + [("gamma_pow", C.c_double * (REPLAY_MAX_N - 1))]
                + [(n, C.c_void_p) for n in ("obs", "next_obs", "action", "reward", "done", "win_obs", "win_action",
                                             "win_reward", "fill", "head", "idx", "status", "plan_base", "plan_code")])


class LevelSchedule(C.Structure):
    """struct sl_level_schedule (168 bytes)"""
    _fields_ = ([(n, C.c_int32) for n in ("G", "lookback", "L", "reserved")]
                + [("start", C.c_int32 * SCHEDULE_MAX_GROUPS), ("len", C.c_int32 * SCHEDULE_MAX_GROUPS)]
                + [(n, C.c_void_p) for n in ("min_performance", "available", "reward_possible", "cur_slot", "ring", "count",
                                             "episodes", "pos", "best", "mean", "status")])


class LevelScheduleMulti(C.Structure):
    """struct sl_level_schedule_multi (208 bytes)"""
    _fields_ = ([("s", LevelSchedule), ("n_agents", C.c_int32), ("reserved", C.c_int32)]
                + [(n, C.c_void_p) for n in ("available", "reward_possible", "pool_agents", "out")])


class EpisodeLogRow(C.Structure):
    """struct sl_episode_log_row (96 bytes)"""
    _fields_ = ([(n, C.c_int64) for n in ("index", "training_steps", "prev")]
                + [(n, C.c_int32) for n in ("env", "level", "episode_idx", "length")]
                + [("reward", C.c_float), ("reward_possible", C.c_int32), ("reward_needed", C.c_int32)]
                + [(n, C.c_uint8) for n in ("success", "times_up", "flags", "reserved")]
                + [("reward_frac", C.c_double), ("side_effects", C.c_double * 2), ("side_effects_frac", C.c_double),
                   ("score", C.c_double)])


class EpisodeLog(C.Structure):
    """struct sl_episode_log (104 bytes)"""
    _fields_ = ([("capacity", C.c_int64), ("B", C.c_int32), ("L", C.c_int32), ("polyak", C.c_double)]
                + [(n, C.c_void_p) for n in ("rows", "counters", "cur_slot", "cur_required", "cur_episode", "last_row",
                                             "reward_possible", "value", "count", "weight")])


class EpisodeLogMulti(C.Structure):
    """struct sl_episode_log_multi (120 bytes)"""
    _fields_ = ([("capacity", C.c_int64), ("B", C.c_int32), ("L", C.c_int32), ("n_agents", C.c_int32),
                 ("n_names", C.c_int32), ("polyak", C.c_double)]
                + [(n, C.c_void_p) for n in ("rows", "counters", "cur_slot", "cur_required", "cur_episode", "last_row",
                                             "reward_possible", "name_id", "value", "count", "weight")])


class EpisodeHistory(C.Structure):
    """struct sl_episode_history (112 bytes)"""
    _fields_ = ([(n, C.c_int32) for n in ("B", "n_watch", "n_slots", "T", "H", "W", "interval", "reserved")]
                + [(n, C.c_void_p) for n in ("watch", "owner", "cur_level", "cur_episode", "slot_state",
                                             "entries", "counters", "goals", "frames", "orders")])


class PpoLoss(C.Structure):
    """struct sl_ppo_loss (136 bytes)"""
    _fields_ = ([("n", C.c_longlong), ("N", C.c_longlong), ("n_actions", C.c_int32), ("reserved", C.c_int32)]
                + [(n, C.c_double) for n in ("eps_policy", "eps_value", "vf_coef", "entropy_reg", "entropy_clip")]
                + [(n, C.c_void_p) for n in ("values", "policy", "actions", "action_prob", "old_values", "returns",
                                             "advantages", "rows", "status")])


class DqnLoss(C.Structure):
    """struct sl_dqn_loss (88 bytes)"""
    _fields_ = ([("n", C.c_longlong), ("N", C.c_longlong), ("n_actions", C.c_int32), ("source", C.c_int32),
                 ("discount", C.c_double)]
                + [(n, C.c_void_p) for n in ("q_values", "next_q_values", "action", "reward", "done", "index", "status")])


class DigestSegment(C.Structure):
    """struct sl_digest_segment (16 bytes)"""
    _fields_ = [("ptr", C.c_void_p), ("bytes", C.c_ulonglong)]


class EpisodeRun(C.Structure):
    """struct sl_episode_run (80 bytes)"""
    _fields_ = ([(n, C.c_int32) for n in ("B", "G", "env_offset", "N", "L", "n_agents")]
                + [(n, C.c_void_p) for n in ("active", "played", "base_episode", "counters", "results", "agent_results",
                                             "side_effects")])


def log_row_multi_bytes(n_agents):
    """SL_LOG_ROW_MULTI_BYTES(A): a 64-byte header and 40 bytes per agent."""
    return 64 + 40 * int(n_agents)


class LogWeights(C.Structure):
    """struct sl_log_weights (248 bytes)"""
    _fields_ = [("n", C.c_int32), ("reserved", C.c_int32), ("cell", C.c_uint16 * SL_SE_MAX_KEYS),
                ("weight", C.c_double * SL_SE_MAX_KEYS)]


class EnvBatch(C.Structure):
    _fields_ = (
        [(n, C.c_int32) for n in ENV_SCALARS_HEAD]
        + [("channels", C.c_int32 * SL_MAX_CHANNELS), ("spawner_free", C.c_int32), ("stream_salt", C.c_int32)]
        + [(n, _p) for n in ENV_STATE_PTRS]
        + [("L", C.c_int32), ("level_stride", C.c_int32)]
        + [(n, _p) for n in ENV_POOL_PTRS + ENV_POOL_TAIL]
        + [("out", _p), ("obs", _p), ("policy_obs", _p), ("policy_dtype", C.c_int32), ("out_compact", C.c_int32),
           ("score_lut", _p), ("goal_cache", _p), ("pool_ready", _p)]
        + [("wrap", Wrappers), ("finished", EpisodeQueue)]
    )


_lib = None


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SafeLifeHipError(
                "safelife_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        # One HIP runtime per process: torch ships its own libamdhip64.so.7 and must be loaded
        # first so that this library binds to the same runtime (same SONAME) instead of pulling a
        # second copy from /opt/rocm, which would then see no device.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        L.slhip_abi_version.restype = C.c_int
        L.slhip_last_error.restype = C.c_char_p
        L.slhip_device_count.restype = C.c_int
        L.slhip_advance_board.argtypes = [_p, _p, C.c_int, C.c_int, C.c_int, _p, C.c_int, _p, _p]
        L.slhip_advance_board_each.argtypes = [_p, _p, C.c_int, C.c_int, C.c_int, _p, _p, _p, _p]
        L.slhip_life_occupancy.argtypes = [_p, _p, C.c_int, C.c_int, C.c_int, _p, C.c_int, _p, _p]
        L.slhip_alive_counts.argtypes = [_p, _p, C.c_int, C.c_int, _p, _p]
        L.slhip_execute_actions.argtypes = [_p, C.c_int, C.c_int, C.c_int, _p, _p, C.c_int, C.c_int,
                                            C.c_int, _p]
        L.slhip_env_prepare.argtypes = [C.POINTER(EnvBatch), _p]
        if hasattr(L, "slhip_pool_baseline"):
            L.slhip_pool_baseline.argtypes = [C.POINTER(EnvBatch), _p]
        if hasattr(L, "slhip_pool_write"):
            L.slhip_pool_write.argtypes = [C.POINTER(EnvBatch), C.POINTER(PoolRows), _p]
        if hasattr(L, "slhip_goal_cache_bytes"):
            L.slhip_goal_cache_bytes.argtypes = [C.POINTER(EnvBatch), C.POINTER(C.c_int)]
            L.slhip_goal_cache_bytes.restype = C.c_size_t
        if hasattr(L, "slhip_env_row_kernels"):
            L.slhip_env_row_kernels.argtypes = [C.POINTER(EnvBatch)]
        L.slhip_env_reset.argtypes = [C.POINTER(EnvBatch), _p, _p]
        L.slhip_env_step.argtypes = [C.POINTER(EnvBatch), _p, _p]
        L.slhip_env_step_slices.argtypes = [C.POINTER(EnvBatch), C.c_int, _p, _p, _p]
        if hasattr(L, "slhip_env_step_range"):
            L.slhip_env_step_range.argtypes = [C.POINTER(EnvBatch), C.c_int, C.c_int, _p, _p]
        L.slhip_streams_concurrent.argtypes = [_p, _p, C.POINTER(C.c_int)]
        L.slhip_streams_order.argtypes = [_p, C.c_int, _p, C.c_int]
        L.slhip_env_rollout.argtypes = [C.POINTER(EnvBatch), _p, C.c_int, _p, _p, _p]
        L.slhip_env_obs.argtypes = [C.POINTER(EnvBatch), _p]
        if hasattr(L, "slhip_env_step_multi"):
            L.slhip_env_step_multi.argtypes = [C.POINTER(EnvBatch), C.POINTER(MultiAgent), _p, _p]
            L.slhip_env_reset_multi.argtypes = [C.POINTER(EnvBatch), C.POINTER(MultiAgent), _p, _p]
        if hasattr(L, "slhip_env_step_multi_ex"):
            L.slhip_env_step_multi_ex.argtypes = [C.POINTER(EnvBatch), C.POINTER(MultiAgent), C.POINTER(MultiExtras), _p, _p]
            L.slhip_env_reset_multi_ex.argtypes = [C.POINTER(EnvBatch), C.POINTER(MultiAgent), C.POINTER(MultiExtras), _p, _p]
        if hasattr(L, "slhip_queues_step"):
            L.slhip_queues_open.argtypes = [C.POINTER(EnvBatch), C.c_int, _p, C.c_int, C.POINTER(C.c_void_p)]
            L.slhip_queues_step.argtypes = [C.c_void_p, C.POINTER(EnvBatch), _p, C.c_int]
            if hasattr(L, "slhip_queues_open_on"):
                L.slhip_queues_open_on.argtypes = [C.POINTER(EnvBatch), C.c_int, _p, _p, C.c_int, C.POINTER(C.c_void_p)]
                L.slhip_queues_stream_shares.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_int)]
                L.slhip_gather_stream_shares.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
                L.slhip_gather_poke.argtypes = [C.c_void_p]
            L.slhip_queues_sync.argtypes = [C.c_void_p]
            L.slhip_queues_close.argtypes = [C.c_void_p]
        if hasattr(L, "slhip_queues_steps"):
            L.slhip_queues_mode.argtypes = [C.c_void_p, C.POINTER(C.c_char_p)]
            L.slhip_queues_steps.argtypes = [C.c_void_p, C.POINTER(EnvBatch), _p, C.c_longlong, C.c_longlong, C.c_int, C.c_int]
            if hasattr(L, "slhip_queues_stage"):
                L.slhip_queues_stage.argtypes = L.slhip_queues_steps.argtypes
                L.slhip_queues_go.argtypes = [C.c_void_p]
            L.slhip_queues_marker.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
            L.slhip_queues_wait.argtypes = [C.c_void_p, C.c_longlong]
            L.slhip_queues_selftest.argtypes = [C.c_void_p, C.c_int, C.c_int]
            L.slhip_gather_window_queued.argtypes = [_p, _p, _p, C.c_size_t, C.c_void_p, _p, C.POINTER(C.c_longlong)]
        L.slhip_side_effects.argtypes = [C.POINTER(EnvBatch), C.POINTER(EpisodeQueue), C.c_int, C.c_int] + [_p] * 9
        if hasattr(L, "slhip_emd_batch"):
            L.slhip_emd_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
            L.slhip_emd_workspace_bytes.restype = C.c_size_t
            L.slhip_emd_batch.argtypes = [C.POINTER(EpisodeQueue), C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, C.c_double,
                                          _p, C.c_size_t, C.c_int, _p, _p, _p]
            L.slhip_emd_status.argtypes = [_p, _p]
        if hasattr(L, "slhip_sample_actions"):
            L.slhip_sample_actions.argtypes = [_p, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong, _p, _p]
        L.slhip_render_boards.argtypes = [C.POINTER(RenderArgs), _p]
        L.slhip_env_render.argtypes = [C.POINTER(EnvBatch), _p, C.c_int, C.c_int, C.c_int, _p, _p, _p]
        L.slhip_rollout_record.argtypes = [C.POINTER(Rollout), C.c_int, _p, _p, C.c_int, _p, _p, _p, _p]
        L.slhip_training_batch.argtypes = [C.POINTER(Rollout), _p, C.c_double, C.c_double, _p, _p, _p, _p]
        L.slhip_replay_add.argtypes = [C.POINTER(Replay), _p, _p, _p, _p, _p, _p]
        L.slhip_replay_sample.argtypes = [C.POINTER(Replay), C.c_int, C.c_ulonglong, C.c_ulonglong, _p, _p]
        L.slhip_replay_gather.argtypes = [C.POINTER(Replay), _p, C.c_int, _p, _p, C.c_int, _p, _p, _p, _p]
        L.slhip_sample_actions_eps.argtypes = [_p, C.c_int, C.c_int, C.c_double, C.c_ulonglong, C.c_ulonglong, _p, _p]
        L.slhip_replay_add_masked.argtypes = [C.POINTER(Replay), _p, _p, _p, _p, _p, _p, _p]
        L.slhip_sample_actions_eps_masked.argtypes = [_p, _p, C.c_int, C.c_int, C.c_double, C.c_ulonglong, C.c_ulonglong,
                                                      _p, _p]
        L.slhip_sample_actions_masked.argtypes = [_p, _p, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong, _p, _p]
        L.slhip_rollout_record_multi.argtypes = [C.POINTER(RolloutMulti), C.c_int, _p, _p, C.c_int, _p, _p, _p, _p, _p, _p]
        L.slhip_training_batch_multi.argtypes = [C.POINTER(RolloutMulti), _p, C.c_double, C.c_double, _p, _p, _p, _p]
        L.slhip_rollout_compact_chunks.argtypes = [C.POINTER(RolloutMulti)]
        L.slhip_rollout_compact.argtypes = [C.POINTER(RolloutMulti), _p, _p, _p, _p]
        L.slhip_rollout_gather.argtypes = [C.POINTER(RolloutMulti), _p, C.c_longlong, _p, _p, _p, C.c_longlong, _p,
                                           _p, _p, _p, _p, _p, _p]
        L.slhip_schedule_draw.argtypes = [C.POINTER(LevelSchedule), C.POINTER(C.c_double), _p, C.c_ulonglong, C.c_ulonglong,
                                          _p, C.c_int, _p]
        L.slhip_schedule_required.argtypes = [C.POINTER(LevelSchedule), C.c_double, _p, C.c_int, _p]
        L.slhip_schedule_harvest.argtypes = [C.POINTER(LevelSchedule), _p, _p, C.c_int, _p]
        L.slhip_schedule_curriculum.argtypes = [C.POINTER(LevelSchedule), _p, _p]
        L.slhip_schedule_required_multi.argtypes = [C.POINTER(LevelScheduleMulti), C.c_double, _p]
        L.slhip_schedule_harvest_multi.argtypes = [C.POINTER(LevelScheduleMulti), _p, C.c_int, _p]
        L.slhip_episode_log_harvest.argtypes = [C.POINTER(EpisodeLog), _p, _p, C.c_int, _p]
        L.slhip_episode_log_join.argtypes = [C.POINTER(EpisodeLog), C.POINTER(EpisodeQueue), _p, _p, _p,
                                             C.POINTER(LogWeights), _p]
        L.slhip_episode_log_summaries.argtypes = [C.POINTER(EpisodeLog), _p]
        L.slhip_episode_log_run_summary.argtypes = [C.POINTER(EpisodeLog), C.c_longlong, _p, _p]
        L.slhip_episode_log_harvest_multi.argtypes = [C.POINTER(EpisodeLogMulti), _p, _p, _p, C.c_int, _p]
        L.slhip_episode_log_join_multi.argtypes = [C.POINTER(EpisodeLogMulti), C.POINTER(EpisodeQueue), _p, _p, _p,
                                                   C.POINTER(LogWeights), _p]
        L.slhip_episode_log_summaries_multi.argtypes = [C.POINTER(EpisodeLogMulti), _p]
        L.slhip_episode_log_run_summary_multi.argtypes = [C.POINTER(EpisodeLogMulti), C.c_longlong, _p, _p]
        L.slhip_episode_run_start.argtypes = [C.POINTER(EpisodeRun), _p, _p]
        L.slhip_episode_run_harvest.argtypes = [C.POINTER(EpisodeRun), _p, C.c_int, _p]
        L.slhip_episode_run_harvest_multi.argtypes = [C.POINTER(EpisodeRun), _p, C.c_int, _p]
        L.slhip_episode_run_tickets.argtypes = [C.POINTER(EpisodeRun), C.POINTER(EpisodeQueue), _p, _p, _p, _p,
                                                C.POINTER(LogWeights), _p]
        L.slhip_history_capture.argtypes = [C.POINTER(EpisodeHistory), _p, _p, _p, _p, C.POINTER(EpisodeQueue), _p, _p]
        L.slhip_history_rewind.argtypes = [C.POINTER(EpisodeHistory), _p, _p, _p, _p]
        L.slhip_history_capture_multi.argtypes = [C.POINTER(EpisodeHistory), _p, _p, _p, _p, C.c_int, C.POINTER(EpisodeQueue),
                                                  _p, _p]
        L.slhip_ppo_workspace_bytes.argtypes = [C.c_longlong]
        L.slhip_ppo_workspace_bytes.restype = C.c_size_t
        L.slhip_ppo_loss_forward.argtypes = [C.POINTER(PpoLoss), _p, _p, _p, _p]
        L.slhip_ppo_loss_backward.argtypes = [C.POINTER(PpoLoss), _p, _p, _p, _p, _p, _p]
        L.slhip_minibatch_obs.argtypes = [_p, C.c_longlong, C.c_longlong, _p, C.c_longlong, _p, C.c_int, _p, _p]
        L.slhip_minibatch_keys.argtypes = [C.c_longlong, C.c_ulonglong, C.c_ulonglong, _p, _p]
        L.slhip_ppo_report_workspace_bytes.argtypes = [C.c_longlong]
        L.slhip_ppo_report_workspace_bytes.restype = C.c_size_t
        L.slhip_ppo_report_rows.argtypes = [C.POINTER(PpoLoss), C.c_longlong, _p, _p]
        L.slhip_ppo_report_finish.argtypes = [C.POINTER(PpoLoss), _p, C.c_longlong, _p, _p]
        L.slhip_dqn_workspace_bytes.argtypes = [C.c_longlong]
        L.slhip_dqn_workspace_bytes.restype = C.c_size_t
        L.slhip_dqn_loss_forward.argtypes = [C.POINTER(DqnLoss), _p, _p, _p, _p]
        L.slhip_dqn_loss_backward.argtypes = [C.POINTER(DqnLoss), _p, _p, _p, _p, _p]
        L.slhip_state_digest_workspace_bytes.argtypes = [_p, C.c_int]
        L.slhip_state_digest_workspace_bytes.restype = C.c_size_t
        L.slhip_state_digest_prefix.argtypes = [_p, C.c_int, _p]
        L.slhip_state_digest.argtypes = [_p, C.c_int, C.c_ulonglong, _p, _p, _p]
        L.slhip_gen_pattern_workspace_bytes.argtypes = [C.c_int] * 4
        L.slhip_gen_pattern_workspace_bytes.restype = C.c_size_t
        L.slhip_gen_pattern_batch.argtypes = [_p] * 8 + [C.c_int] * 4 + [_p, C.c_size_t, _p]
        L.slhip_partition_workspace_bytes.argtypes = [C.c_int] * 4
        L.slhip_partition_workspace_bytes.restype = C.c_size_t
        L.slhip_partition_batch.argtypes = [_p] * 5 + [C.c_int] * 4 + [_p, C.c_size_t, _p]
        L.slhip_obs_to_policy.argtypes = [_p, C.c_int, C.c_int, C.c_int, _p, C.c_int, _p, C.c_int, _p]
        L.slhip_gather_unique_id.argtypes = [_p]
        L.slhip_gather_init.argtypes = [_p, C.c_int, C.c_int, C.POINTER(_p)]
        L.slhip_gather_window.argtypes = [_p, _p, _p, C.c_size_t, _p]
        L.slhip_gather_destroy.argtypes = [_p]
        L.slhip_gather_window_async.argtypes = [_p, _p, _p, C.c_size_t, _p, C.c_int, _p, C.POINTER(C.c_longlong)]
        L.slhip_gather_done.argtypes = [_p, C.c_longlong, C.c_int, C.POINTER(C.c_int)]
        L.slhip_gather_wait_streams.argtypes = [_p, C.c_longlong, _p, C.c_int]
        foreign = bool(os.environ.get("SAFELIFE_HIP_LIB")) and os.environ.get("SAFELIFE_HIP_LIB_ANY_ABI") == "1"
        for name in EXPORTS:
            if not foreign or hasattr(L, name):      # (A/B runs against an older build: tools/ab_libs.sh)
                getattr(L, name)  # AttributeError here means the .so is stale
        if L.slhip_abi_version() != SL_ABI_VERSION and not foreign:
            raise SafeLifeHipError("%s has ABI version %d, this package needs %d: rebuild it"
                                   % (LIB_PATH, L.slhip_abi_version(), SL_ABI_VERSION))
        _lib = L
    return _lib


def check(rc, shape_message=None):
    """Translate a status code into the exception the reference's wrapper would raise."""
    if rc == 0:
        return
    msg = (lib().slhip_last_error() or b"").decode()
    if rc == SL_E_SHAPE:
        raise ValueError(shape_message or msg)
    if rc == SL_E_ARG:
        raise ValueError(msg)
    raise SafeLifeHipError("libsafelife_hip: %s (status %d)" % (msg, rc))


_device = None


def device():
    """The torch device this process computes on (cuda:LOCAL_RANK).  Raises without a GPU."""
    global _device
    if _device is None:
        import torch
        if not torch.cuda.is_available():
            raise SafeLifeHipError(
                "safelife_amd needs a HIP device (torch.cuda.is_available() is False); "
                "there is no CPU fallback.")
        idx = int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count()
        torch.cuda.set_device(idx)
        _device = torch.device("cuda", idx)
    return _device


def current_stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())
