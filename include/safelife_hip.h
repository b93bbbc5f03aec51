/*
 * safelife_hip.h -- C-ABI of libsafelife_hip.so: the MI355X (gfx950) implementation of the
 * SafeLife per-step hot path.  This is the drop-in boundary: every entry point replaces one
 * prototype of the reference's native layer (safelife/speedups_src/advance_board.h:3-16) or one
 * method of its Python step surface, batched over B independent boards.
 *
 * Conventions (all entry points)
 *   - Plain pointers and sizes only; no torch / Python types.  Every array pointer is a DEVICE
 *     pointer (HBM) unless the parameter is documented as "host".  The library allocates nothing
 *     per call and retains no pointer; the caller owns every buffer.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls only enqueue work.
 *   - Return value: 0 on success, negative on failure (SL_E_*); slhip_last_error() gives a
 *     thread-local message.  The Python shim turns SL_E_SHAPE into the reference's ValueError text.
 *   - Boards are C-contiguous uint16 [B,H,W], the cell bit layout of constants.h:4-33
 *     (== safelife_game.py:75-123).  3 <= H, W; H*W <= SL_MAX_CELLS.
 *   - Random numbers: one numpy-compatible PCG64 (XSL-RR 128/64) stream per board replaces the
 *     reference's process-global bit generator (random.c:21-22,76-83).  Draws are consumed exactly
 *     as advance_board.c:115 consumes them (eligible cells only, row-major), so a board stepped
 *     here with the state of numpy generator G equals the reference stepped under G, and the
 *     state written back equals G's state afterwards.
 */
#ifndef SAFELIFE_HIP_H
#define SAFELIFE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SL_ABI_VERSION 13       /* 13: slhip_queues_stage / slhip_queues_go, sl_env_batch.pool_ready / out_compact, sl_level_scalars.ready, slhip_env_step_multi / _reset_multi; 12: slhip_pool_write; 11: sl_env_batch.goal_cache, slhip_goal_cache_bytes; 10: slhip_queues_open_on, slhip_queues_stream_shares, slhip_gather_stream_shares, slhip_gather_poke */
#define SL_MAX_CELLS 16384        /* H*W limit of one board */
#define SL_MAX_CHANNELS 32

enum sl_status {
    SL_OK = 0,
    SL_E_SHAPE = -1,      /* bad board shape / sizes (module.c:32-35,112-114,170-179) */
    SL_E_ARG = -2,        /* null pointer or inconsistent argument */
    SL_E_HIP = -3,        /* HIP runtime error, see slhip_last_error() */
    SL_E_UNSUPPORTED = -4
};

/* numpy.random.PCG64 state as four 64-bit words (state = hi:lo, inc = hi:lo). */
typedef struct sl_pcg64 {
    uint64_t state_hi, state_lo, inc_hi, inc_lo;
} sl_pcg64;

int slhip_abi_version(void);
const char *slhip_last_error(void);
/* Number of HIP devices visible, or a negative sl_status. */
int slhip_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Batched primitives == the five prototypes of advance_board.h, one launch for B boards.
 * ------------------------------------------------------------------------------------------ */

/* advance_board_nstep (advance_board.h:6-7; Python advance_board(board, spawn_prob, n_step),
 * module.c:20-49).  out may alias in.  spawn_prob: [B] float (the reference parses a C float,
 * module.c:26, and compares the draw against it promoted to double, advance_board.c:35,115).
 * rng: [B], read and written back advanced by the number of draws consumed. */
int slhip_advance_board(const uint16_t *in, uint16_t *out, int B, int H, int W,
                        const float *spawn_prob, int n_steps, sl_pcg64 *rng, void *stream);

/* The same with one step count per board (n_steps: int32 [B]): side_effect_score rolls every
 * finished episode's starting board forward by that episode's length (side_effects.py:108). */
int slhip_advance_board_each(const uint16_t *in, uint16_t *out, int B, int H, int W,
                             const float *spawn_prob, const int32_t *n_steps, sl_pcg64 *rng, void *stream);

/* life_occupancy (advance_board.h:9-10, module.c:52-81).  counts: int32 [B,H,W,8], overwritten
 * (the reference accumulates into a zeroed array): per cell and colour, the number of steps
 * 1..n_steps after which the cell is ALIVE and not AGENT|EXIT|FROZEN (advance_board.c:153-161). */
int slhip_life_occupancy(const uint16_t *in, int32_t *counts, int B, int H, int W,
                         const float *spawn_prob, int n_steps, sl_pcg64 *rng, void *stream);

/* alive_counts (advance_board.h:12, module.c:99-132).  out: int64 [B,8,9], overwritten.
 * HW = cells per board (any shape, flat, as the reference). */
int slhip_alive_counts(const uint16_t *board, const uint16_t *goals, int B, int HW,
                       int64_t *out, void *stream);

/* execute_actions (advance_board.h:14-16, module.c:155-202).  board and locs are updated in
 * place; locs: int64 [B,A,2] as (row, col); actions: int64, element (b,k) at
 * actions[b*action_batch_stride + k*action_stride] (action_stride 0 broadcasts one action to all
 * agents of a board, module.c:185).  Agents of one board act in index order. */
int slhip_execute_actions(uint16_t *board, int B, int H, int W, int64_t *locs,
                          const int64_t *actions, int A, int action_stride,
                          int action_batch_stride, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused single-agent SafeLifeEnv.step()/reset() over B device-resident environments
 * (safelife_env.py:148-218 with the game glue of safelife_game.py:505-552,657-719,746-761 and
 * the observation of safelife_env.py:105-146 / helper_utils.py:42-75).
 * The struct lives on the HOST; every pointer inside is a device pointer.
 * ------------------------------------------------------------------------------------------ */
/* Per-env scalar state: one 64-byte record per env (a single wide load/store per step instead of a
 * dozen strided ones).  Field <-> reference attribute: */
typedef struct sl_env_scalars {
    int32_t agent_row, agent_col; /* SafeLifeGame.agent_locs[0] (row, col); row < 0 => no agent */
    int32_t num_steps;            /* GameState.num_steps */
    int32_t old_value;            /* SafeLifeEnv._old_game_value */
    int32_t required_points;      /* GameWithGoals.required_points() */
    int32_t initial_points;       /* sum(points_table * initial_counts) */
    int32_t table_idx;            /* row of points_table used by this env */
    int32_t level_idx;            /* pool level currently loaded */
    int32_t episode_idx;          /* episodes finished by this env */
    int32_t episode_length;       /* SafeLifeEnv.episode_length */
    float episode_reward;         /* SafeLifeEnv.episode_reward */
    float spawn_prob;             /* GameState.spawn_prob */
    int32_t goals_static;         /* SafeLifeGame._static_goals: 0 None, 1 True, 2 False */
    int32_t is_active;            /* SafeLifeEnv._is_active */
    int32_t exit_open_at_reset;   /* can_exit() during the reset's update_exit_colors (the exit paint of
                                     SimpleSideEffectPenalty's starting-state baseline) */
    int32_t loaded;               /* != 0 once a level has been loaded into this slot: slhip_env_reset() then moves on
                                     to the next level (level_idx += level_stride, episode_idx += 1), as
                                     SafeLifeEnv.reset() takes next(level_iterator) (safelife_env.py:204) */
} sl_env_scalars;

/* What one step() returns per env besides the observation (16 bytes). */
typedef struct sl_step_out {
    float reward;                 /* np.float32 reward of safelife_env.py:157,172 */
    uint8_t done;
    uint8_t success;              /* info['episode']['success'] */
    uint8_t times_up;             /* info['times_up'] */
    uint8_t reserved;
    float episode_reward;         /* info['episode']['reward'] (before any auto-reset) */
    int32_t episode_length;       /* info['episode']['length'] */
} sl_step_out;

/* Per-level constants of the pool (32 bytes). */
typedef struct sl_level_scalars {
    int32_t agent_row, agent_col;
    int32_t required_reset;       /* required_points while resetting (first observation) */
    int32_t required_step;        /* required_points for the steps that follow (differs under
                                     MinPerformanceScheduler, env_wrappers.py:142-145) */
    int32_t initial_points;
    int32_t table_idx;
    float spawn_prob;
    int32_t ready;                /* written by the library where sl_env_batch.pool_ready is kept (round 6), else unused:
                                     (old_value << 1) | exit_open -- what SafeLifeEnv.reset() computes on this level
                                     (safelife_env.py:203-218: the score of the fresh board + the exit bonus if the agent
                                     stands on an open exit; whether update_exit_colors opened the exits) */
} sl_level_scalars;

/* Training-wrapper math of safelife/env_wrappers.py, applied per env inside the step in the order
 * of training/env_factory.py:277-283:
 *   MovementBonusWrapper   :32-98   reward += movement_bonus * speed**power [- movement_bonus]
 *   ExtraExitBonus         :120-128 reward += done * bonus * episode_reward   (unless times_up)
 *   SimpleSideEffectPenalty:150-213 reward -= penalty_coef * (side_effect - last_side_effect),
 *                                   baseline = "starting-state" (the board right after reset) or, with
 *                                   SL_WRAP_INACTION, "inaction" (:179-180: that board advanced once per step)
 * (MinPerformanceScheduler :131-147 has no per-step arithmetic: sl_level_scalars.required_step.)
 * The wrapped reward is float64, as in the reference (np.float32 + np.float64), evaluated with the
 * same operations in the same order; speed**power comes from a host-built table so no pow() runs on
 * the device.  flags == 0 switches all of it off.
 * "inaction": the reference advances the baseline board outside any game method, so its spawners draw from the
 * process-wide generator (safelife/random.py:13).  With many envs that is one generator per env, inaction_rng[e];
 * an env whose generator starts in the state the process-wide one had reproduces the reference run exactly
 * (tests/golden/trace_wrap_inaction_*).  The baselines are advanced inside the step kernels (row-kernel shapes: a
 * third pass of the kernel's CA loop, every step of a T-step launch, through streams and queues alike; other shapes: a
 * launch of its own in front of each step, T = 1 only); an env whose num_steps is 0 takes its current board as the
 * baseline first, which is what the wrapper's reset() does. */
#define SL_WRAP_MOVEMENT 1
#define SL_WRAP_AS_PENALTY 2            /* MovementBonusWrapper.as_penalty */
#define SL_WRAP_EXIT_BONUS 4
#define SL_WRAP_SIDE_EFFECT 8
#define SL_WRAP_IGNORE_REWARD_CELLS 16  /* SimpleSideEffectPenalty.ignore_reward_cells */
#define SL_WRAP_INACTION 32             /* SimpleSideEffectPenalty.baseline == "inaction" (with SL_WRAP_SIDE_EFFECT) */
#define SL_WRAP_MAX_PERIOD 8

typedef struct sl_wrap_state {    /* per env, 48 bytes */
    int32_t n_prior;              /* positions held by MovementBonusWrapper's deque (<= period) */
    int32_t last_side_effect;     /* SimpleSideEffectPenalty.last_side_effect */
    int16_t prior[SL_WRAP_MAX_PERIOD][2];   /* (row, col), oldest first */
    int32_t reserved[2];
} sl_wrap_state;

typedef struct sl_wrappers {
    int32_t flags;                /* SL_WRAP_* */
    int32_t move_period;          /* movement_bonus_period, 1..SL_WRAP_MAX_PERIOD */
    int32_t move_table_len;       /* >= H + W + move_period */
    int32_t reserved;
    double move_bonus;            /* movement_bonus */
    double exit_bonus;            /* ExtraExitBonus.bonus */
    double penalty_coef;          /* SimpleSideEffectPenalty.penalty_coef */
    const double *move_table;     /* [move_table_len]: movement_bonus * (d / period) ** power, d = 0.. */
    sl_wrap_state *state;         /* [B] */
    double *shaped_reward;        /* [B] out: what the outermost wrapper's step() returns as reward */
    double *shaped_reward_t;      /* [T,B] per-step copy for slhip_env_rollout, or NULL */
    uint32_t *pool_baseline;      /* workspace [L, H, (W+1)/2]: every pool level as it stands right after
                                     reset, player bits cleared, in the row kernels' register layout;
                                     filled by slhip_env_prepare() (needed with SL_WRAP_SIDE_EFFECT) */
    uint16_t *inaction_board;     /* SL_WRAP_INACTION: [B,H,W] the baseline boards (state; 16-byte aligned) */
    sl_pcg64 *inaction_rng;       /* SL_WRAP_INACTION: [B] the baselines' generators (state) */
    uint32_t *inaction_rows;      /* (unused since ABI 9: the row kernels lay the advanced baselines out in LDS) */
} sl_wrappers;

/* Finished episodes, queued on the device by the step kernels for the side-effect pass (safelife_env.py:183-192
 * runs side_effect_score() inside the step that ends an episode; with thousands of envs the episode-end work
 * is batched instead).  The step that ends an env's episode -- done while the env was still active -- takes
 * slot = atomic_add(count, 1) and, if slot < capacity, writes a record and a copy of the board as the agent
 * left it (after update_exit_colors, before any auto-reset reloads the slot).  capacity == 0 switches the
 * queue off.  The consumer (slhip_side_effects) reads min(*count, capacity) entries; it never resets *count:
 * the caller alternates two queues and clears the idle one (hipMemsetAsync) before handing it back. */
typedef struct sl_episode_record {    /* 32 bytes */
    int32_t env;                  /* index of the env in the batch */
    int32_t level;                /* pool level the episode was played on: its starting board */
    int32_t num_steps;            /* GameState.num_steps when it ended */
    int32_t episode_idx;          /* the env's episode counter during that episode */
    float spawn_prob;
    float episode_reward;
    int32_t episode_length;
    uint8_t success, times_up;
    uint8_t n_cell_types;         /* written by slhip_side_effects: frozen movable / destructible cell types on the
                                     starting board (saturating); more than SL_SE_MAX_KEYS - 8 means keys and
                                     type_masks of this entry are cut short (rebuild them from `counts` on the host) */
    uint8_t reserved;
} sl_episode_record;

typedef struct sl_episode_queue {
    int32_t capacity;             /* slots; 0 = no queue */
    int32_t env_base;             /* added to the env index written into records (slices of a batch) */
    int32_t *count;               /* device int32: episodes pushed so far (beyond capacity: dropped) */
    sl_episode_record *records;   /* [capacity] */
    uint16_t *boards;             /* [capacity,H,W] */
} sl_episode_queue;

typedef struct sl_env_batch {
    int32_t B, H, W, E;          /* envs; board dims; exit slots per env (>= 1) */
    int32_t time_limit;          /* SafeLifeEnv.time_limit (safelife_env.py:65) */
    int32_t exit_points;         /* GameState.points_on_level_exit (safelife_game.py:156) */
    int32_t n_tables;
    int32_t auto_reset;          /* !=0: an env whose episode ends reloads its next pool level */
    int32_t remove_white_goals;  /* safelife_env.py:66,125-126 */
    int32_t view_h, view_w;      /* SafeLifeEnv.view_shape */
    int32_t n_channels;          /* len(output_channels); 0 => raw uint32 view */
    int32_t channels[SL_MAX_CHANNELS];
    int32_t spawner_free;        /* !=0: the caller guarantees that no board or goal array of the batch and
                                    of the pool holds a SPAWNING cell (the rules never create one), which
                                    lets the kernels drop the random-draw machinery; 0 = no promise */
    int32_t stream_salt;         /* 0: an env that loads pool level l starts from pool_rng[l] exactly (what replaying
                                    the reference's traces needs: every recorded level carries its own generator).
                                    != 0: the episode's generator is pool_rng[l] moved to a state derived from
                                    (stream_salt + env index, episode_idx), so envs that replay one pool level --
                                    and successive replays by one env -- see different random streams, as the
                                    reference's per-game SeedSequence children do (level_iterator.py:218).
                                    Use 1 + (global index of env 0) so that shards of one run do not collide */
    /* per-env state */
    uint16_t *board;             /* [B,H,W] */
    uint16_t *goals;             /* [B,H,W] */
    int32_t *exit_locs;          /* [B,E] flat cell index of GameState.exit_locs, -1 = unused */
    sl_pcg64 *rng;               /* [B] SafeLifeGame._rng */
    sl_env_scalars *scalars;     /* [B] */
    const int32_t *points_table; /* [n_tables,8,9] (safelife_game.py:595-605) */
    /* level pool: the device-resident counterpart of SafeLifeLevelIterator */
    int32_t L;
    int32_t level_stride;        /* next level of an env = (level_idx + level_stride) % L */
    const uint16_t *pool_board;  /* [L,H,W] as loaded (before update_exit_colors) */
    const uint16_t *pool_goals;  /* [L,H,W] */
    const int32_t *pool_exit_locs;      /* [L,E] */
    const sl_pcg64 *pool_rng;           /* [L] */
    const sl_level_scalars *pool_scalars; /* [L] */
    const int32_t *pool_next;    /* optional [L]: an env on slot s loads slot pool_next[s] at its next reset instead of
                                    (s + level_stride) % L.  What a pool that is REFRESHED while the envs step needs
                                    (safelife_amd.levels.LevelPool.stage / commit: new levels go into spare slots and the
                                    table is switched between two steps -- the device-resident counterpart of
                                    level_iterator.py:200-223 handing every reset a fresh level).  Read at launch time:
                                    the queue launcher patches the pointer into every dispatch.  NULL = the rule above */
    /* per-step outputs */
    sl_step_out *out;            /* [B] */
    uint8_t *obs;                /* [B,vh,vw,C] uint8, or uint32 [B,vh,vw] if n_channels == 0; NULL = skip */
    void *policy_obs;            /* the same observation as the policy network takes it (training/models.py:100-103
                                    transposes (h,w,c) -> (c,w,h); training/ppo.py:64 casts to float32), written by
                                    the step / reset kernels themselves: [B,C,vw,vh], policy_obs[b][c][x][y] = bit
                                    channels[c] of the view word at (y,x); uint8 or float32 (policy_dtype).  Needs
                                    n_channels >= 1.  NULL = skip */
    int32_t policy_dtype;        /* 0 = uint8, 1 = float32 */
    int32_t out_compact;         /* != 0: `out` takes 8-byte records -- the first half of sl_step_out: reward, done, success,
                                    times_up -- instead of 16-byte ones (what a learner on another rank needs of every
                                    step: half the bytes a gather window carries; sharding.RewardGather(record="compact")) */
    /* workspace */
    int8_t *score_lut;           /* [n_tables,4096+65536] per-cell score tables derived from points_table by
                                    slhip_env_prepare(); NULL => the size-generic kernels are used */
    uint32_t *goal_cache;        /* optional workspace of slhip_goal_cache_bytes() bytes, 16-byte aligned, ZEROED by the
                                    caller: the fused step kernels keep the goal colours of boards whose goals are
                                    static (safelife_game.py:753-760) in the form their lanes use, and a launch whose
                                    boards all have them there moves no goal array at all.  The kernels maintain it
                                    across steps, resets and slices; whoever writes `goals`, `scalars.goals_static` or
                                    `scalars.level_idx` from OUTSIDE the library zeroes it again.  Only batches without
                                    observation and wrappers use it (with a finished-episode queue: the wide board shapes).
                                    The kernels that keep it hold no goal image in LDS at all: WITHOUT the workspace
                                    (NULL) they fetch every lane's goal row from global memory at every step -- correct,
                                    and slower; give such batches their cache */
    uint16_t *pool_ready;        /* optional workspace [L,H,W] (round 6): every pool level as an episode STARTS on it --
                                    pool_board after the reset's update_exit_colors (safelife_game.py:537-552) -- kept by
                                    slhip_env_prepare() and slhip_pool_write() together with pool_scalars[l].ready.
                                    What a reset computes on a level depends on the level alone, so an env whose episode
                                    ends inside a step kernel COPIES its next level from here instead of scoring and
                                    repainting it (one pass over the board, the leaders' exit walk and a workgroup
                                    barrier less on the chain of the one workgroup its whole launch waits for).
                                    NULL: the step kernels work it out at every reset, as before */
    sl_wrappers wrap;            /* training wrappers; wrap.flags == 0 => none */
    sl_episode_queue finished;   /* episodes that ended, for the side-effect pass; finished.capacity == 0 => none */
} sl_env_batch;

/* Derive env->score_lut from env->points_table, and env->wrap.pool_baseline / env->pool_ready from the level pool
 * (call once, and again whenever points_table or the pool changes).
 * Synchronises the stream.  Returns SL_E_UNSUPPORTED when a table entry does not fit int8; the
 * caller then passes score_lut = NULL and every shape runs on the size-generic kernels. */
int slhip_env_prepare(const sl_env_batch *env, void *stream);

/* Rebuild env->wrap.pool_baseline from the level pool as it stands now, asynchronously on `stream` (what
 * slhip_env_prepare does once, synchronously): after pool slots have been rewritten. */
int slhip_pool_baseline(const sl_env_batch *env, void *stream);

/* New levels for pool slots no env can load at present (the spare bank of a refreshable pool: pool_next, above), in one
 * kernel on `stream`: the level iterator's hand-over (level_iterator.py:200-223) for a device-resident pool.  Every
 * source may be host memory the device can read (pinned): the kernel fetches it when it runs, so it stays untouched
 * until the stream has passed the launch. */
typedef struct sl_pool_rows {
    int32_t n;                   /* levels */
    const int32_t *slot;         /* [n] pool slots to write, distinct, < env->L */
    const uint16_t *board;       /* [n,H,W] */
    const uint16_t *goals;       /* [n,H,W] */
    const int32_t *exit_locs;    /* [n,E] */
    const sl_pcg64 *rng;         /* [n] */
    const sl_level_scalars *scalars; /* [n] */
    const int32_t *next;         /* optional [L]: a successor table, copied to next_dst by the same launch */
    int32_t *next_dst;
} sl_pool_rows;
int slhip_pool_write(const sl_env_batch *env, const sl_pool_rows *rows, void *stream);

/* Bytes of env->goal_cache for this batch as described by *env -- call it with the observation, wrapper and queue fields
 * already set (0: no step kernel of this batch keeps a cache -- leave goal_cache NULL).
 * *boards_per_block (optional): the cache is one block of bytes / ceil(B / boards_per_block) bytes per group of that many
 * consecutive envs; a block's first 32-bit word is its flag (1: the group steps on cached goal words). */
size_t slhip_goal_cache_bytes(const sl_env_batch *env, int *boards_per_block);

/* Which kernel family steps and resets this batch as described by *env: 1 = the row kernels, 0 = the size-generic kernels
 * (no row kernel for the board shape, points outside int8 -- score_lut NULL --, more than 8 exit slots, a view too large
 * for the fused policy-layout observation, unaligned arrays), < 0 = an error.  The answer is the whole batch's (launches
 * that start at env 0 or at a multiple of 64 envs); nothing is launched. */
int slhip_env_row_kernels(const sl_env_batch *env);

/* SafeLifeEnv.reset() for the envs with mask[e] != 0 (mask NULL = all): an env that has never been loaded
 * takes pool level level_idx[e]; any other moves on to (level_idx[e] + level_stride) % L and counts an
 * episode, exactly as the in-kernel auto-reset does.  Writes the first observation. */
int slhip_env_reset(const sl_env_batch *env, const uint8_t *mask, void *stream);

/* One SafeLifeEnv.step() for every env.  actions: int32 [B] in 0..8. */
int slhip_env_step(const sl_env_batch *env, const int32_t *actions, void *stream);

/* T consecutive steps in ONE launch (boards stay on chip between steps).  actions: int32 [T,B].
 * reward_t / done_t: optional [T,B] per-step outputs (NULL = only the last step's outputs in
 * env->reward/done are kept).  Observations are produced for the final state only. */
int slhip_env_rollout(const sl_env_batch *env, const int32_t *actions, int T,
                      float *reward_t, uint8_t *done_t, void *stream);

/* Do kernels on stream_a and stream_b overlap on the device?  HIP multiplexes streams onto a few hardware queues
 * (four by default); two streams that share one run their kernels one after the other, which silently turns sliced
 * stepping into serial stepping (measured: 24 instead of 13.5 us per step).  Which streams collide depends on what
 * else the process has created (RCCL, other envs).  The probe runs two idle 100 us one-wavefront kernels, one per
 * stream, and compares the wall time with one; *concurrent = 1 if they overlapped.  Synchronises both streams. */
int slhip_streams_concurrent(void *stream_a, void *stream_b, int *concurrent);

/* Stream ordering without a host wait: every stream of `after` waits for what has been enqueued so far on every
 * stream of `before` (HOST arrays of hipStream_t; a stream that appears on both sides is skipped).  The fence and join
 * of sliced stepping: order({caller}, slices) before a step whose actions the caller's stream produced, and
 * order(slices, {caller}) before the caller's stream reads the outputs.  Events come from a ring inside the library. */
int slhip_streams_order(void *const *before, int n_before, void *const *after, int n_after);

/* One step for every env, issued as n_slices launches: slice i = envs [bounds[i], bounds[i+1]) on
 * streams[i] (bounds: HOST int32 [n_slices+1], bounds[0] = 0, bounds[n_slices] = B; streams: HOST array of
 * hipStream_t).  Envs are independent, so the slices need no ordering among themselves: on distinct
 * streams the load / compute / store phases and the launch boundaries of one slice overlap those of the
 * others, step after step (a single launch per step leaves the chip idle at both ends of every launch).
 * The caller orders each stream against whoever produces `actions` and consumes the outputs.
 * actions: int32 [B].  Slice bounds should be multiples of 64
 * envs so that every slice keeps the 16-byte alignment the row kernels' DMA needs. */
int slhip_env_step_slices(const sl_env_batch *env, int n_slices, const int32_t *bounds, const int32_t *actions,
                          void *const *streams);

/* One step for the envs [first, first + count) only, one launch on `stream` (actions: int32 [B], indexed by the env's
 * index in the batch; `first` a multiple of 64 keeps the row kernels' alignment).  What a pipelined driver uses: the
 * policy of one group of envs runs while another group steps (training/base_algo.py:208-238 walks its envs one by one);
 * with a group's policy, action draw and step all on the group's own stream nothing needs a fence
 * (safelife_amd/runner.py: PipelinedRunner). */
int slhip_env_step_range(const sl_env_batch *env, int first, int count, const int32_t *actions, void *stream);

/* Sliced stepping WITHOUT HIP's launch path: slhip_env_step_slices hides one slice's kernel boundary under the other
 * slices' kernels, but a launch through a HIP stream costs the host 2.4-3 us, so one stepping thread feeds two slices per
 * ~8 us step and no more.  These entry points issue the SAME kernel from HSA queues of the library's own, one per slice
 * (csrc/sl_aql.hip): a dispatch is a 64-byte packet and a doorbell, and the packets and argument blocks of MANY steps
 * are written by one call.  Ordering is a stream's: every dispatch waits for its queue's previous one (barrier bit) with
 * agent-scope acquire / release fences -- independent of where workgroups run.
 *   open   : slices as in slhip_env_step_slices (1 to 8); row-kernel shapes only
 *            (SL_E_UNSUPPORTED otherwise, or when the HSA runtime offers no queue -- callers then keep to streams).
 *   steps  : n_steps consecutive steps of every env, all enqueued by this call (the queue rings give back-pressure: the
 *            call blocks while they are full).  Step t takes its actions from actions + t * action_stride (int32
 *            elements; device int32 [B] each, complete when the call is made) and writes its sl_step_out records to
 *            env->out + t * out_stride (records; 0: every step overwrites env->out).  head != 0 for the first step
 *            after anything OUTSIDE the queues wrote the envs' state or the actions through a HIP stream: the caller
 *            has synchronised those streams, and step 0 is dispatched with a system-scope acquire.
 *   step   : steps(handle, env, actions, 0, 0, 1, head).
 *   marker : a system-scope release behind every step dispatched so far, with a completion signal; returns at once
 *            (*ticket = -1: nothing was outstanding).  wait: the calling thread -- any thread -- waits for it.  Only then
 *            may HIP streams or the host read what the steps in front of the marker wrote.
 *   sync   : marker + wait.
 *   mode   : the flags in effect (why_not, optional: why SL_QUEUES_RELEASE_FREE was asked for and not granted, or NULL).
 *
 * SL_QUEUES_RELEASE_FREE (open's flags; OPT-IN, never the default): the steps of a queue go without the RELEASE fence
 * (it alone costs ~0.9 us of a 7.5 us step of 8192 25x25 envs: the write-back of the XCDs' L2s).  What a step wrote then
 * stays in the L2 of the XCD its workgroups ran on, and the next step's workgroup of the same index reads it there --
 * which is valid ONLY while a workgroup index of a QUEUE keeps running on the same XCD.  MI355X runs workgroup i of
 * every dispatch of a queue on XCD (q + i) mod 8, q a constant of the queue (tools/ubench/xcd_place.hip,
 * profiles/round4_a_xcd_placement.txt: whatever the grid, the kernel, the queue's history and the other queues are
 * doing), but no programming guide promises it, so
 *   - open probes it (a probe kernel, three dispatches per queue: q of every queue, and that every workgroup follows
 *     the formula) and falls back to the fenced mode where it does not hold (slhip_queues_mode reports that), and
 *   - EVERY step verifies it: every workgroup compares the XCD it runs on with (q + i) mod 8 of its slice's queue --
 *     scalar code, no memory access -- and raises a host-visible flag if it finds itself anywhere else; wait / sync
 *     then -- and from then on -- return SL_E_HIP: the envs' state since the queues were opened is not valid, and the
 *     caller starts over without the flag.  Use it where losing a run to that is acceptable (benchmarks, restartable
 *     roll-outs).
 *
 * selftest (tests only): SL_QUEUES_SELFTEST_PLANT tells slice 0 to expect its workgroups one XCD further on than they run;
 * SL_QUEUES_SELFTEST_SWAP (arg 1 / 0: on / off) dispatches step t's slice i on queue (i + t) mod n behind a host-side
 * drain of all queues that carries no release, so that every env is stepped -- in order -- by a workgroup of another
 * QUEUE than the step before, which on MI355X means another XCD -- harmless with a stream's fences, a real misplacement
 * for release-free stepping (tests/test_hip_parity.py shows both). */
#define SL_QUEUES_RELEASE_FREE 1
#define SL_QUEUES_SELFTEST_PLANT 1
#define SL_QUEUES_SELFTEST_SWAP 2
int slhip_queues_open(const sl_env_batch *env, int n_slices, const int32_t *bounds, int flags, void **handle);
/* The same with slice i on queue queue_ids[i] (distinct, 0 to 7; NULL: slice i on queue i) -- for callers that leave
 * out a queue another kernel of theirs would hold up (slhip_gather_stream_shares).
 * SL_E_UNSUPPORTED also for a batch whose step kernel the queues cannot dispatch -- one that keeps private memory (it
 * spills: the single-step kernels of 32x32 spawner pools), which these packets do not set up: found out here, when the
 * queues are opened, never by a step.  The message then starts "AQL queues cannot dispatch this batch", where a runtime
 * without queues to give says "AQL queues unavailable". */
int slhip_queues_open_on(const sl_env_batch *env, int n_slices, const int32_t *bounds, const int32_t *queue_ids, int flags,
                         void **handle);
/* Which of the queues 0 .. n_queues - 1 does a long one-wavefront kernel on HIP `stream` hold up (bit q of *mask)?
 * (On MI355X: none -- a kernel that fits next to the steps runs beside them whatever its queue.) */
int slhip_queues_stream_shares(int n_queues, void *stream, int *mask);
int slhip_queues_mode(void *handle, const char **why_not);
int slhip_queues_steps(void *handle, const sl_env_batch *env, const int32_t *actions, long long action_stride,
                       long long out_stride, int n_steps, int head);
int slhip_queues_step(void *handle, const sl_env_batch *env, const int32_t *actions, int head);
/* steps() split in two (round 6): stage() writes the argument blocks and packets of all n_steps (<= SL_QUEUES_STAGE_MAX)
 * WITHOUT handing anything to the device; go() makes them valid and rings one doorbell per queue.  The action buffers must
 * exist when the region is staged, their contents when it goes -- a caller stages the next region while it still waits
 * for the last one's results, and starts it with a few hundred nanoseconds of host work.  Nothing else is dispatched on
 * the handle in between (a marker or a steps() call hands the staged packets over early: harmless, just not deferred). */
#define SL_QUEUES_STAGE_MAX 48
int slhip_queues_stage(void *handle, const sl_env_batch *env, const int32_t *actions, long long action_stride,
                       long long out_stride, int n_steps, int head);
int slhip_queues_go(void *handle);
int slhip_queues_marker(void *handle, long long *ticket);
int slhip_queues_wait(void *handle, long long ticket);
int slhip_queues_sync(void *handle);
int slhip_queues_close(void *handle);
int slhip_queues_selftest(void *handle, int what, int arg);

/* The episode-end pass of side_effect_score() (side_effects.py:103-130) for every episode in `queue` (what
 * safelife_env.py:183-192 runs inside the step that ends an episode), all on the device and without a host
 * read: every stage is launched over queue->capacity entries and stops at min(*queue->count, capacity).
 *   1. b0 = pool_board[record.level]; b1 = advance_board(b0, spawn_prob, record.num_steps)       (:108)
 *   2. counts[:,0] = life_occupancy(b1, p, num_samples); counts[:,1] = life_occupancy(queue board, ...)  (:109-110)
 *   3. the distributions of :111-130: keys / life_dist / type_masks below.
 * Random draws: the reference takes them from its process-wide generator (side_effects.py runs outside
 * use_rng), so there is nothing to be stream-compatible with; every entry gets its own PCG64 stream derived
 * from its level's generator, env index and episode index, consumed in the reference's order (roll-forward,
 * inaction tensor, action tensor); derive_streams == 0 takes the caller's work_rng [C] as they are instead (how
 * the reference's recorded generator states are replayed).  The earth-mover distances: slhip_emd_batch below.
 * All buffers are caller-owned device memory sized by the queue's capacity C:
 *   work_boards  uint16 [2C,H,W]     run 0: b0 (rolled forward in place when derive_streams == 0); run 1: copies of
 *                                    the final boards (derive_streams != 0: both runs are worked on by ONE fused
 *                                    launch, roll-forward and sampling in the same kernel)
 *   work_prob    float  [2C],  work_steps int32 [2C],  work_rng sl_pcg64 [2C]  (derive_streams == 0: the first C)
 *   counts       int32  [2,C,H,W,8]  out: the occupancy tensors, counts[0] = inaction, counts[1] = action
 *   keys         uint16 [C,SL_SE_MAX_KEYS] out: slots 0-7 = CellTypes.life | colour i where total_counts[i] > 0,
 *                else 0xFFFF; slots 8.. = the frozen, movable-or-destructible, non-agent cell values of b0 in
 *                ascending order (np.unique), 0xFFFF-padded (more than SL_SE_MAX_KEYS-8 of them: the rest are cut)
 *   life_dist    double [C,2,8,H,W]  out: counts / num_samples as float64 (num_runs = 1), colour-major
 *   type_masks   uint8  [C,2,SL_SE_MAX_KEYS-8,H,W] out: (b0 == key), (final board == key) for slots 8..
 * Any board of 3 <= H, W with H*W <= 4096 cells (so every shape up to 64x64): the row kernels where the shape has
 * them and work_boards / queue->boards are 16-byte aligned, else (other shapes, unaligned boards,
 * SAFELIFE_HIP_FORCE_GENERIC=1) the size-generic kernels, with bit-identical results.  Larger boards:
 * SL_E_UNSUPPORTED (use the primitives). */
#define SL_SE_MAX_KEYS 24
int slhip_side_effects(const sl_env_batch *env, const sl_episode_queue *queue, int num_samples, int derive_streams,
                       uint16_t *work_boards, float *work_prob, int32_t *work_steps, sl_pcg64 *work_rng,
                       int32_t *counts, uint16_t *keys, double *life_dist, uint8_t *type_masks, void *stream);

/* The earth-mover distances of side_effect_score() (side_effects.py:13-57,132-154) for every entry of `queue` and
 * every key slot, from the outputs of slhip_side_effects (counts, keys, type_masks; the record's n_cell_types), on
 * the device and without a host read; stops at min(*queue->count, capacity) like the other stages.  Per (entry, key):
 * a, b = the inaction / action distribution; the cells with |a - b| > 1e-3 * max|a - b| take part; the result is the
 * EMD-hat of Pele & Werman over them -- the minimum-cost flow of min(sum a, sum b) under the ground distance, plus
 * extra_mass_penalty * |sum a - sum b| -- solved EXACTLY (successive shortest paths on integer flows; only the final
 * sum(flow * cost) is floating point, in a fixed order: the result is deterministic).  Any H, W <= 64.
 *   ground       double [(2H-1),(2W-1)]: ground[dr + H-1][dc + W-1] = distance from a cell to the cell dr rows and
 *                dc columns before it (row_i - row_j, col_i - col_j: the reference's rule is asymmetric); built by the
 *                host (safelife_amd.side_effects.ground_table) so that both sides price arcs with the same bits.
 *                Must be a quasi-metric: 0 at (0,0) and obeying the triangle inequality (sl_emd.hip says why).
 *   extra_mass_penalty  >= 0 (the reference's default: 1.0)
 *   workspace    device memory, 256-byte aligned, slhip_emd_workspace_bytes(H, W, capacity, concurrency) bytes:
 *                256 + concurrency * (align256(2 * M * M) + align256(36 * (H*W + 2))), M = H*W/2 + 1
 *                (`concurrency` workgroups each solve one problem at a time and take the next off a device counter)
 *   scores       double [C,SL_SE_MAX_KEYS,2] out: distance, inaction mass (sum a over the board); NaN, NaN for an
 *                empty key slot, and for every slot of an entry whose keys were cut short (n_cell_types >
 *                SL_SE_MAX_KEYS - 8: evaluate those on the host).  Entries past the count are not written.
 *   n_cells      int32 [C,SL_SE_MAX_KEYS] out: participating cells (0 for an empty slot, -1 for a cut-short entry)
 * Every loop of the solver is bounded by the problem's size; a problem that runs over a bound gets NaN scores and
 * slhip_emd_status(workspace, stream) -- which synchronises the stream -- returns SL_E_HIP naming it. */
size_t slhip_emd_workspace_bytes(int H, int W, int capacity, int concurrency);
int slhip_emd_batch(const sl_episode_queue *queue, int H, int W, int num_samples, const int32_t *counts,
                    const uint16_t *keys, const uint8_t *type_masks, const double *ground, double extra_mass_penalty,
                    void *workspace, size_t workspace_bytes, int concurrency, double *scores, int32_t *n_cells,
                    void *stream);
int slhip_emd_status(const void *workspace, void *stream);

/* ---- multi-GPU: the per-step records of every rank's envs -> rank 0 ----------------------------
 * Boards never cross GPUs; the only exchange of the path is what a learner on rank 0 needs from the other ranks:
 * their sl_step_out records.  A rank's step kernels write the records of a WINDOW of consecutive steps straight
 * into one device buffer; these entry points move a window to rank 0 with RCCL point-to-point calls
 * (ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd: xGMI is point-to-point, the seven peers' windows arrive over
 * seven links at once) on a stream of the caller's choosing, so the exchange overlaps the following steps.  RCCL is
 * loaded on first use (dlopen of librccl.so.1 -- the copy the process already has, if any); a process that never
 * gathers never touches it.  Replaces, for this path, what training/base_algo.py does with Python lists of
 * per-env results (there is one process and no exchange in the reference).
 *
 *   slhip_gather_unique_id   rank 0: a fresh ncclUniqueId (SL_GATHER_ID_BYTES bytes, host memory) for the caller to
 *                            broadcast over whatever it has (the existing torch.distributed process group)
 *   slhip_gather_init        every rank, same id: ncclCommInitRank on the current device; *comm is an opaque handle
 *   slhip_gather_window      one window: rank r sends `bytes` from `send` to rank 0; rank 0 receives rank r's window
 *                            at recv + r * bytes (its own included), all inside one RCCL group, enqueued on `stream`.
 *                            recv is ignored on the other ranks.  Returns once the calls are enqueued.
 *   slhip_gather_destroy     releases the communicator */
#define SL_GATHER_ID_BYTES 128
int slhip_gather_unique_id(void *id_out);
int slhip_gather_init(const void *id, int world, int rank, void **comm);
int slhip_gather_window(void *comm, const void *send, void *recv, size_t bytes, void *stream);
int slhip_gather_destroy(void *comm);

/* Which of the library's step queues 0 .. n_queues - 1 (slhip_queues_*) does the exchange hold up when it runs on
 * `stream` (bit q of *mask)?  RCCL's kernel is dispatched from one of HIP's hardware queues; the step queue that takes
 * turns with it stands still for the length of the exchange (~40 us per window next to a running step loop) while the
 * others step on.  Measured with a real 8 MiB exchange per queue -- COLLECTIVE: every rank calls it, with the same
 * n_queues.  A caller that steps through queues then opens them with slhip_queues_open_on, leaving the marked queue out. */
int slhip_gather_stream_shares(void *comm, int n_queues, void *stream, int *mask);

/* The same hand-off off the caller's thread: the request is queued and a worker thread of the library issues the
 * stream ordering (the exchange's `stream` waits for what is enqueued on the window's `writers`, HOST array of up to 8
 * hipStream_t, at the time the WORKER gets to it -- later than the call, never earlier, which is safe because the
 * writers' later launches fill the OTHER window), the RCCL group, and an event behind it.  The stepping thread pays
 * for a queue push (~1 us) instead of the runtime calls (20 us, 35-80 us with busy queues).  *ticket identifies the
 * window: slhip_gather_done (is it finished?  block != 0 waits on the host) and slhip_gather_wait_streams (make streams
 * wait for it, e.g. before its buffers are written or read again; waits on the host only until the worker has
 * enqueued the group).  At most 8 windows may be outstanding. */
int slhip_gather_window_async(void *comm, const void *send, void *recv, size_t bytes, void *const *writers, int n_writers,
                              void *stream, long long *ticket);
/* A window will be handed over within the next few milliseconds: the worker thread, if it sleeps, wakes up now and polls
 * for the request (a wake-up at the hand-over itself costs tens of microseconds, milliseconds on a busy host). */
int slhip_gather_poke(void *comm);
int slhip_gather_done(void *comm, long long ticket, int block, int *done);
int slhip_gather_wait_streams(void *comm, long long ticket, void *const *streams, int n_streams);
/* A window that was written from the library's AQL queues (slhip_queues_steps): the call puts a marker behind the steps
 * dispatched so far on `queues` (the handle of slhip_queues_open) and returns; the worker thread waits for the marker
 * -- not the stepping thread, which goes on enqueuing the next window's steps -- and then issues the RCCL group on
 * `stream`.  Tickets as above. */
int slhip_gather_window_queued(void *comm, const void *send, void *recv, size_t bytes, void *queues, void *stream,
                               long long *ticket);

/* SafeLifeEnv.get_obs() for the current state. */
int slhip_env_obs(const sl_env_batch *env, void *stream);

/* ---- multi-agent batches (round 6): SafeLifeEnv(single_agent=False), safelife_env.py:148-218 with :162-170 NOT taken --
 * every board carries n_agents agents (advance_board.c:217-220: their actions in index order), each with its own points
 * table, exit condition, reward, done flag and episode accumulators (safelife_game.py:505-552,657-719 evaluated per
 * agent; the exits turn red when ANY agent may leave), and an observation centred on itself.  The fused step is the
 * size-generic family's (one workgroup per board, any shape).  `env` supplies the boards, goals, generators, exit tables,
 * the level pool, the points tables and the view; of sl_env_scalars only num_steps, level_idx, episode_idx, spawn_prob,
 * goals_static and loaded are used (the per-agent words live in `agents`).  env->obs and env->out are ignored: the
 * per-agent outputs are `multi`'s.  An env whose agents are ALL done reloads its next pool level inside the step when
 * env->auto_reset is set (training/base_algo.py:231-236 resets on np.all(done)).  These two entry points refuse
 * wrappers, the finished-episode queue and the policy layout (SL_E_UNSUPPORTED): the _ex pair below takes them, with
 * the per-agent buffers they need in sl_multi_extras. */
typedef struct sl_agent_state {   /* per env and agent (48 bytes) */
    int32_t row, col;             /* where the agent is -- or was when it left the board (GameState.agent_locs) */
    int32_t old_value;            /* SafeLifeEnv._old_game_value[a] */
    int32_t required_points;      /* SafeLifeGame.required_points()[a] */
    int32_t initial_points;       /* sum(points_table[a] * initial_counts) */
    int32_t table_idx;            /* the agent's table in env->points_table */
    int32_t episode_length;
    float episode_reward;
    int32_t is_active;            /* SafeLifeEnv._is_active[a] */
    int32_t reserved[3];
} sl_agent_state;
typedef struct sl_level_agent {   /* per pool level and agent (32 bytes); every level of the pool has exactly n_agents agents */
    int32_t row, col, required_reset, required_step, initial_points, table_idx, reserved[2];
} sl_level_agent;
typedef struct sl_multi_agent {
    int32_t n_agents;             /* A, 1 to SL_MAX_AGENTS */
    int32_t reserved;
    sl_agent_state *agents;       /* [B, A] */
    const sl_level_agent *pool_agents;   /* [L, A] */
    sl_step_out *out;             /* [B, A]: one record per agent and step */
    uint8_t *obs;                 /* [B, A, view_h, view_w, n_channels] uint8, or uint32 [B, A, view_h, view_w]; NULL = skip */
} sl_multi_agent;
#define SL_MAX_AGENTS 8
/* actions: int32 [B, A] in 0..8 (an agent that is done takes 0, as training/base_algo.py:216-219 feeds it). */
int slhip_env_step_multi(const sl_env_batch *env, const sl_multi_agent *multi, const int32_t *actions, void *stream);
/* SafeLifeEnv.reset() for the envs with mask[e] != 0 (NULL: all), as slhip_env_reset. */
int slhip_env_reset_multi(const sl_env_batch *env, const sl_multi_agent *multi, const uint8_t *mask, void *stream);

/* ---- multi-agent batches with the training wrappers, the finished-episode queue and the policy layout ----------------
 * The reference's multi-agent training stack: SafeLifeEnv(single_agent=False) under MovementBonusWrapper(as_penalty),
 * ExtraExitBonus, SimpleSideEffectPenalty and MinPerformanceScheduler (training/env_factory.py:277-283), and the
 * episode-end side-effect pass of safelife_env.py:183-192.  env->wrap configures the wrappers as for single-agent
 * batches (flags, coefficients, move_table, inaction_board / inaction_rng; wrap.state, wrap.shaped_reward and
 * wrap.pool_baseline are not used: the per-agent buffers are below).  What differs per agent:
 *   - the shaped reward is float32 per agent: the reference's reward is a float32 array that every wrapper updates in
 *     place, so each wrapper rounds once -- f32(f64(r) + movement term), then r - f32(move_bonus) (as_penalty), then
 *     f32(f64(r) + done * exit_bonus * episode_reward) unless times_up, then f32(f64(r) - delta * penalty_coef);
 *   - an agent that is done keeps being shaped until the env resets (its done flag stays set, its location stays put);
 *   - one side-effect count per env, against the board as the multi-agent reset leaves it (every agent's cell carries
 *     the EXIT bit iff THAT agent could leave: `baseline` below) or the inaction board, subtracted from every agent;
 *     CellTypes.player does not clear colour or exit bits, so a coloured agent that moves counts at both cells.
 * An episode is queued (env->finished) once, on the step where every agent is done and at least one was active before
 * it: one sl_episode_record (agent 0's accumulators, success and times_up in its own fields) plus one sl_step_out per
 * agent in `finished_agents`, and the board as the agents left it; slhip_side_effects consumes the queue as it does
 * a single-agent one (env->H x W must be a row-kernel board shape). */
typedef struct sl_multi_extras {
    sl_wrap_state *wrap_state;    /* [B, A]: each agent's MovementBonusWrapper trail; last_side_effect (the env's count,
                                     the same in every agent's record); reserved[0] = can_exit() of the agent at reset */
    float *shaped_reward;         /* [B, A] out: what the outermost wrapper's step() returns, per agent */
    uint16_t *baseline;           /* workspace [L, H, W]: every pool level as the multi-agent reset leaves it (the
                                     starting-state baseline); written by slhip_env_reset_multi_ex, read by the step.
                                     Needed with SL_WRAP_SIDE_EFFECT */
    sl_step_out *finished_agents; /* [env->finished.capacity, A]: each agent's record of the step that queued an entry */
    void *policy_obs;             /* [B, A, C, view_w, view_h] uint8 or float32 (policy_dtype): sl_env_batch.policy_obs
                                     per agent; NULL = skip.  env->policy_obs must be NULL */
    int32_t policy_dtype;         /* 0 = uint8, 1 = float32 */
    int32_t reserved;
} sl_multi_extras;
/* slhip_env_step_multi with env->wrap, env->finished and extras.  An inaction baseline advances in a launch of its own
 * in front of the step. */
int slhip_env_step_multi_ex(const sl_env_batch *env, const sl_multi_agent *multi, const sl_multi_extras *extras,
                            const int32_t *actions, void *stream);
/* slhip_env_reset_multi, and the wrappers' reset(); also (re)writes extras->baseline for every pool level.  Call it
 * before the first step. */
int slhip_env_reset_multi_ex(const sl_env_batch *env, const sl_multi_agent *multi, const sl_multi_extras *extras,
                             const uint8_t *mask, void *stream);

/* The raw uint32 view (output_channels=None, safelife_env.py:141) -> the tensor the policy network
 * convolves: channel-first with the spatial axes swapped, out[b][c][x][y] = (view[b][y][x] >> channels[c]) & 1,
 * i.e. what training/models.py:100-103 (obs.transpose(-1, -3)) and the float cast of training/ppo.py:64
 * produce from the (h, w, c) uint8 observation.  dtype: 0 = uint8, 1 = float32.  view: [B,vh,vw],
 * out: [B,C,vw,vh].  The step then only writes 4 bytes per view cell instead of C.
 * `channels` is a HOST pointer (C int32 values, copied into the launch); view and out are device pointers.
 * (sl_env_batch.policy_obs makes the step kernel write this layout itself.) */
int slhip_obs_to_policy(const uint32_t *view, int B, int vh, int vw, const int32_t *channels, int C,
                        void *out, int dtype, void *stream);

/* One categorical draw per env from policy probabilities, on the device, written as the int32 action the step kernels
 * read (training/ppo.py:66-69 draws on the host with numpy; there is no random stream to be compatible with).
 * probs: float32 [B, n_actions] (rows sum to 1), n_actions in 1..64; the draw of env e in call `counter` of a run
 * seeded `seed` is a function of (seed, counter, e) alone, so runs are reproducible:
 *   z = seed + G * (counter * 0x100000001B3 + e + 1) mod 2^64, G = 0x9E3779B97F4A7C15, through splitmix64's finalizer;
 *   u = (z >> 40) * 2^-24, a 24-bit uniform in [0, 1 - 2^-24];
 *   cum_k = the fp32 running sum p_0 + ... + p_k over all n_actions entries, in index order;
 *   the action is the first k with u < cum_k; if there is none, the largest k with p_k > 0; if no entry is positive,
 *   n_actions - 1.
 * An action with p_k == 0 is therefore never returned while any entry is positive (a row whose fp32 sum stays below 1
 * gives what rounding leaves to its last POSITIVE action), and the result lies in [0, n_actions) for rows with NaN,
 * inf or negative entries as well (which action they get is otherwise unspecified).
 * A caller that holds envs [lo, lo + B) of a larger batch passes seed + G * lo (mod 2^64) and draws exactly what envs
 * lo + e of the whole batch draw under `seed`; seed + lo does NOT do that. */
int slhip_sample_actions(const float *probs, int B, int n_actions, unsigned long long seed, unsigned long long counter,
                         int32_t *actions, void *stream);

/* ---- rendering: boards -> RGB frames (additive to ABI 13: two new symbols and one new struct, nothing existing changes,
 * so SL_ABI_VERSION stays where it is) ---------------------------------------------------------------------------------
 * The reference's render_board (fast_render.c:33-133; Python speedups._render_board, module.c:438-512) and the view of
 * render_graphics.render_game (helper_utils.py:42-75), for N frames in one launch, bit exact with the reference: per
 * output byte (uint8)(255.f * (bg * (1.f - mask) + mask * sprite * fg)) in fp32, left to right, nothing fused, truncated;
 * the tile comes from the cell's type (colour and orientation bits masked off; 13 named types, empty, the agent's four
 * orientations, anything else -- an empty cell that carries a colour included -- the "unknown" tile), fg from the cell's
 * colour bits, bg from the GOAL's.  The edit cursor of render_graphics.render_board is not drawn.
 *   frame n shows source frame f = index ? index[n] : n (f outside [0, n_source): an empty frame):
 *     board + f * board_stride, goals + f * goal_stride (strides in cells; goal_stride 0: one goal array for all frames)
 *   sprites      float32 [70,70,4], 16-byte aligned: the sheet, RGBA / 255
 *   orientation  optional int32 [N]: replaces bits 12-13 of every cell of frame n (values 0..3)
 *   view_h, view_w  both 0: the whole board, [N, H*14, W*14, 3].  Both > 0: a view_h x view_w window centred on
 *     centers[s * center_stride + 0..1] (row, col; a negative row: no agent, the centre is (0,0)), toroidal -- a view
 *     larger than the board tiles it; every entry >= 0 of exits[s * E + 0..E) (flat cell indices) has its BOARD value
 *     painted at its position relative to the centre, clipped to the view's perimeter, later entries over earlier ones;
 *     goals are not repainted.  s = n, or f where aux_by_index != 0 (centres and exits live with the source frames).
 *     exits may be NULL (E is then ignored).
 *   out          uint8 [N, vh*14, vw*14, 3] contiguous, 4-byte aligned (16-byte aligned: wide stores) */
typedef struct sl_render_args {
    int32_t N, H, W, n_source;
    int32_t view_h, view_w, E, aux_by_index;
    long long board_stride, goal_stride, center_stride;
    const uint16_t *board, *goals;
    const int32_t *index;
    const float *sprites;
    const int32_t *orientation;
    const int32_t *centers;
    const int32_t *exits;
    uint8_t *out;
} sl_render_args;
int slhip_render_boards(const sl_render_args *args, void *stream);
/* The current state of the envs env_ids[0..n) (device int32; NULL: envs 0..n-1, n = env->B for all of them), the view
 * centred on the env's agent (sl_env_scalars.agent_row / agent_col) with the env's exit_locs; view 0 x 0: whole boards.
 * Of *env only B, H, W, E, board, goals, exit_locs and scalars are read.  A multi-agent batch keeps its agents'
 * locations in sl_agent_state: its caller passes agent 0's (row, col) through slhip_render_boards' centers with
 * center_stride = n_agents * 12 (render_game centres on agent_locs[0]). */
int slhip_env_render(const sl_env_batch *env, const int32_t *env_ids, int n, int view_h, int view_w,
                     const float *sprites, uint8_t *out, void *stream);

/* ---- PPO training batches: the rollout buffer and its returns / GAE advantages (additive to ABI 13: two new symbols and
 * one new struct, nothing existing changes, so SL_ABI_VERSION stays where it is) ---------------------------------------
 * What the reference's PPO.gen_training_batch (training/ppo.py:74-143) does with the tuples of take_one_step, on the
 * device: a window of T steps of B envs is kept TIME-MAJOR ([T,B]: row t holds step t of every env), and one kernel
 * turns it into discounted returns and GAE advantages, bit exact with numpy's arithmetic in the reference.
 * The struct lives on the HOST; every pointer inside is a device pointer the caller owns.
 *
 * The arithmetic (numpy 2 promotion rules; g, l = gamma, lmda as doubles; f32(x) = x rounded to float32):
 *   - a trajectory is the run of steps of one env between resets: it ends at a step with done != 0 and at the window's
 *     last row.  It is CLOSED if its last step has done != 0 -- its final_value is then the Python float 0.0 -- else OPEN,
 *     with final_value = final_values[b], float32 V(next_obs) of the window's last step;
 *   - a trajectory is WIDE if it is closed or has one step (np.append(values[1:], final_value) is float64 then: a Python
 *     float joins a float32 array, or anything joins an empty one), else NARROW;
 *   - wide:    adv[i] = (f64(r[i]) + g * f64(v[i+1])) - f64(v[i]);  adv[i] += l * adv[i+1]; all float64, v[last+1] =
 *              final_value;
 *   - narrow, float32 rewards:  adv[i] = (r[i] + f32(g) * v[i+1]) - v[i];  adv[i] += f32(l) * adv[i+1]; all float32;
 *   - narrow, float64 rewards:  adv[i] = (r[i] + f64(f32(g) * v[i+1])) - f64(v[i]);  adv[i] += l * adv[i+1]: the product
 *              is still float32 (v is a float32 array), the rest float64;
 *   - returns, in the rewards' dtype R: ret[last] = r[last] + R(f32(g) * final_value) (a float32 product even for float64
 *     rewards; a closed trajectory adds 0.0);  ret[i] = r[i] + R(g) * ret[i+1];
 *   - nothing is fused, and everything is rounded to float32 once, at the end. */
#define SL_REWARD_F32 0
#define SL_REWARD_F64 1
#define SL_ROLLOUT_BAD_ACTION 1   /* bit of *status: a recorded action lay outside [0, n_actions) */
typedef struct sl_rollout {       /* 80 bytes */
    int32_t T, B;                 /* steps of the window, envs; both >= 1 */
    int32_t reward_dtype;         /* SL_REWARD_F32 or SL_REWARD_F64: what `rewards` holds and the recorded rewards are */
    int32_t reserved;
    long long row_stride;         /* elements between rows t and t + 1 of the five arrays below, >= B */
    long long out_stride;         /* the same for returns / advantages / traj_start of slhip_training_batch, >= B */
    int32_t *actions;             /* [T, row_stride] */
    float *action_prob;           /* [T, row_stride] probability the policy gave the action taken */
    void *rewards;                /* [T, row_stride] float32 or float64 */
    float *values;                /* [T, row_stride] V(obs) */
    uint8_t *done;                /* [T, row_stride] != 0: the step ended the env's episode */
    int32_t *status;              /* one device word, zeroed by the caller; the kernels only ever set bits (SL_ROLLOUT_*) */
} sl_rollout;

/* Step t of the window: row t of the five arrays takes actions[b], probs[b * n_actions + actions[b]], rewards[b]
 * (buf->reward_dtype), values[b], done[b] -- one launch where a gather and four copies would run.  actions: int32 [B];
 * probs: float32 [B, n_actions]; values: float32 [B]; done: uint8 [B].  An action outside [0, n_actions) reads no
 * probability: 0 is recorded and SL_ROLLOUT_BAD_ACTION is raised in *buf->status (the action itself is kept). */
int slhip_rollout_record(const sl_rollout *buf, int t, const int32_t *actions, const float *probs, int n_actions,
                         const void *rewards, const float *values, const uint8_t *done, void *stream);

/* Returns and advantages of the whole window by the rules above, from buf->rewards / values / done (the other pointers
 * of *buf are not used).  final_values: float32 [B], V(next_obs) of the last step -- envs whose last step has `done` do
 * not read theirs.  returns, advantages: float32 [T, out_stride]; traj_start: optional uint8 [T, out_stride] (NULL:
 * skipped), 1 where step t is the first of its trajectory (t == 0 or done[t-1]) -- with it a caller can regroup the rows
 * in the reference's trajectory order. */
int slhip_training_batch(const sl_rollout *buf, const float *final_values, double gamma, double lmda, float *returns,
                         float *advantages, uint8_t *traj_start, void *stream);

/* ---- DQN replay: the n-step window, the ring, sampling and the epsilon-greedy draw (additive to ABI 13: four new symbols
 * and one new struct, nothing existing changes, so SL_ABI_VERSION stays where it is) -----------------------------------
 * What the reference's DQN does on the host with ReplayBuffer, add_to_replay and take_one_step (training/dqn.py:21-37,
 * 93-134), on the device.  The struct lives on the HOST; every pointer inside is a device pointer the caller owns.
 *
 * The window.  Every env keeps its last n = multi_step_learning steps (obs, action, float64 reward).  All envs step in
 * lock-step, so the window is ONE ring over t mod n for all of them: slot *head is where the step being added goes, slot
 * (*head - k) mod n holds the step k steps back, and fill[b] (0 .. n) says how many of the slots behind *head env b has
 * filled since its last episode end.  slhip_replay_add, for the step (obs, action, r, done, next_obs) of every env b, in
 * env order:
 *   1. (obs0, act0, R0) = the window's slot *head -- the step n steps back -- as it is, if fill[b] == n;
 *   2. reward of slot (*head - k) mod n += (double)r * gamma_pow[k-1] for k = 1 .. min(fill[b], n-1): a float64 product,
 *      then a float64 add, nothing fused; slot *head = (obs, action, (double)r);
 *   3. if fill[b] was n: push (obs0, act0, R0, obs, done) -- R0 holds n rewards;
 *   4. if done: push (obs_k, act_k, reward_k, next_obs, done) for k = 0 .. min(fill[b] + 1, n) - 1, newest first, and
 *      fill[b] = 0; else fill[b] = min(fill[b] + 1, n).
 * A push writes ring slot *idx mod capacity and increments *idx.  The slots are handed out by an exclusive prefix sum of
 * the envs' push counts (0 .. n + 1) on top of *idx, so the ring's order is the reference's whatever the device's
 * scheduling; capacity >= B * (n + 1) makes the pushes of one call distinct slots. */
#define SL_REPLAY_MAX_N 16        /* largest n */
#define SL_REPLAY_MAX_K 4096      /* largest k of slhip_replay_sample */
#define SL_REPLAY_SHORT 1         /* bit of *status: slhip_replay_sample asked for more rows than the ring holds */
#define SL_REPLAY_BAD_INDEX 2     /* bit of *status: slhip_replay_gather met an index outside [0, capacity) and skipped it */
typedef struct sl_replay {        /* 264 bytes */
    long long capacity;           /* ring slots, >= B * (n + 1) */
    long long obs_bytes;          /* bytes of one env's observation row (any dtype: rows are opaque bytes), >= 1.  Rows are
                                   * moved 16 bytes per lane when obs_bytes and every row pointer are multiples of 16, else
                                   * with the widest of 8 / 4 / 2 / 1 bytes that divides them all */
    int32_t B, n;                 /* envs; window length, 1 .. SL_REPLAY_MAX_N */
    int32_t reward_dtype;         /* SL_REWARD_F32 or SL_REWARD_F64: what slhip_replay_add's `rewards` holds */
    int32_t reserved;
    double gamma_pow[SL_REPLAY_MAX_N - 1];    /* gamma ** k for k = 1 .. n-1, computed by the caller (numpy's
                                   * gamma ** np.arange(1, n) for bit parity with the reference: a device pow need not agree) */
    uint8_t *obs;                 /* ring [capacity, obs_bytes] */
    uint8_t *next_obs;            /* ring [capacity, obs_bytes] */
    int32_t *action;              /* ring [capacity] */
    double *reward;               /* ring [capacity]: the n-step sum, float64 as the reference keeps it */
    uint8_t *done;                /* ring [capacity] 0 / 1 */
    uint8_t *win_obs;             /* window [n, B, obs_bytes] */
    int32_t *win_action;          /* window [n, B] */
    double *win_reward;           /* window [n, B] */
    int32_t *fill;                /* [B], zeroed by the caller */
    int32_t *head;                /* one device word, zeroed by the caller: t mod n */
    long long *idx;               /* one device int64, zeroed by the caller: pushes so far */
    int32_t *status;              /* one device word, zeroed by the caller; the kernels only ever set bits (SL_REPLAY_*) */
    long long *plan_base;         /* workspace [B]: the first ring slot (before the modulo) of each env's pushes */
    int32_t *plan_code;           /* workspace [B]: fill before the step | done << 8 | inactive << 9 */
} sl_replay;

/* add_to_replay for one step of all B envs.  obs, next_obs: [B, obs_bytes]; actions: int32 [B]; rewards: [B] of
 * buf->reward_dtype; done: uint8 [B].  next_obs of a finished env is stored as given (done = 1 masks it in the loss).
 * Two launches on `stream`: a one-workgroup plan (counts, prefix sum, *idx, *head, fill) and one workgroup per env that
 * updates the window and moves the rows. */
int slhip_replay_add(const sl_replay *buf, const void *obs, const int32_t *actions, const void *rewards,
                     const uint8_t *done, const void *next_obs, void *stream);

/* slhip_replay_add for envs with several agents (additive to ABI 13, like slhip_sample_actions_eps_masked below).  The
 * reference's DQN is handed only the agents that are still active, env-major, agent-minor; a trajectory window belongs to
 * (env, num_resets, agent), an agent that is done has its window flushed and takes no further part until its env is
 * reset, which happens once ALL its agents are done (training/base_algo.py:152-244, dqn.py:110-134).  Here buf->B is the
 * number of COLUMNS, envs * n_agents, column e * n_agents + a being agent a of env e (the layout of sl_rollout_multi), and
 * active: uint8 [B] says who took part in this step (NULL: everybody -- the result is then slhip_replay_add's bit for bit).
 *   A column with active == 0 is a no-op for this call: it pushes nothing, its window slots and fill stay as they are,
 *   and NONE of its inputs is read -- obs row, action, reward, done (the env keeps reporting 1 for an agent that has
 *   left), next_obs row.  An active column does exactly what slhip_replay_add does for it, and the ring slots are handed
 *   out by the same exclusive prefix sum of the push counts over the columns in index order: the ring's order is the
 *   reference's.
 * The window stays ONE ring over t mod n for all columns: a column is only ever inactive after a step of its own with
 * done, which set its fill to 0, so the fill slots behind *head that it reads once it is back are its own contiguous
 * steps.  capacity >= B * (n + 1) with B the columns.  Still two launches: the plan records "inactive" in plan_code, and
 * the copy kernel's workgroup of such a column leaves before it loads anything else.  The carried state (who is active,
 * num_resets) is not moved here: slhip_rollout_record_multi is its one implementation. */
int slhip_replay_add_masked(const sl_replay *buf, const void *obs, const int32_t *actions, const void *rewards,
                            const uint8_t *done, const void *next_obs, const uint8_t *active, void *stream);

/* k distinct indices in [0, N), N = min(*idx, capacity) read on the device, by Floyd's algorithm; 1 <= k <=
 * SL_REPLAY_MAX_K.  For i = 0 .. k-1: j = N - k + i; z_i = the splitmix64 finalizer of seed + G * (counter * 0x100000001B3
 * + i + 1) (G as in slhip_sample_actions); t = the high 64 bits of z_i * (j + 1); out_index[i] = t unless t is among
 * out_index[0 .. i), else j.  The set is uniform over the k-subsets up to a bias of (j + 1) / 2^64 per draw; the order has
 * no meaning.  k > N raises SL_REPLAY_SHORT in *status and writes nothing.  out_index: int64 [k]. */
int slhip_replay_sample(const sl_replay *buf, int k, unsigned long long seed, unsigned long long counter,
                        long long *out_index, void *stream);

/* The five tensors of DQN.optimize for ring rows index[0 .. k): obs_out / next_obs_out [k, obs_bytes] as stored, or
 * float32 [k, obs_bytes] widened from uint8 when obs_float32 != 0; action_out int64 [k]; reward_out float32 [k], the
 * float64 sum rounded once; done_out float32 [k].  An index outside [0, capacity) raises SL_REPLAY_BAD_INDEX and its row
 * is left as it was. */
int slhip_replay_gather(const sl_replay *buf, const long long *index, int k, void *obs_out, void *next_obs_out,
                        int obs_float32, long long *action_out, float *reward_out, float *done_out, void *stream);

/* DQN.take_one_step's draw (training/dqn.py:100-104), one thread per env: z as in slhip_sample_actions from (seed,
 * counter, e); u = (z >> 40) * 2^-24; if (double)u < epsilon the action is ((z & 0xFFFFFFFF) * n_actions) >> 32, else
 * the first index of the row's maximum, a NaN counting as the maximum and the first NaN winning (np.argmax).
 * epsilon <= 0 never randomises, epsilon >= 1 always does.  qvals: float32 [B, n_actions]; actions: int32 [B].  A caller
 * that holds envs [lo, lo + B) of a larger batch passes seed + G * lo. */
int slhip_sample_actions_eps(const float *qvals, int B, int n_actions, double epsilon, unsigned long long seed,
                             unsigned long long counter, int32_t *actions, void *stream);

/* slhip_sample_actions_eps with a mask: rows with active[e] == 0 get action 0 and their Q-values are not read (NaN rows
 * included); every other row gets exactly the draw of slhip_sample_actions_eps for row e.  active: uint8 [B] (NULL: all
 * active).  For a multi-agent batch the rows are the columns e * n_agents + a, and a caller that holds envs [lo, hi) of a
 * larger run passes seed + G * lo * n_agents (the rule of slhip_sample_actions_masked). */
int slhip_sample_actions_eps_masked(const float *qvals, const uint8_t *active, int B, int n_actions, double epsilon,
                                    unsigned long long seed, unsigned long long counter, int32_t *actions, void *stream);

/* ---- multi-agent PPO training batches: the masked rollout window (additive to ABI 13: seven new symbols and one new
 * struct, nothing existing changes, so SL_ABI_VERSION stays where it is) ------------------------------------------------
 * The reference's driver loop for envs with several agents (training/base_algo.py:152-244 with ppo.py:74-143): the agents
 * of one env finish at different steps, a finished agent gets no observation row and no action (the env is handed 0 for
 * it), the env resets once ALL its agents are done, and a trajectory is the steps of one (env, reset count, agent).
 * Here the window is [T, B] with B = envs * n_agents COLUMNS, column e * n_agents + a being agent a of env e, plus
 * active [T, B]: 1 where the agent took part in step t.  The rules, per column:
 *   - a trajectory is a run of contiguous active rows; it ends at a row with done != 0 (CLOSED, final_value 0.0) or at the
 *     window's last row (OPEN, final_value = final_values[column]).  Inactive rows only ever sit between a done row and
 *     the next trajectory's first row, or at the head of the window (an agent that was gone when the window began);
 *   - a row starts a trajectory when it is active and t == 0, or the row before it is inactive or has done != 0;
 *   - a column whose last row is inactive or done takes no bootstrap: its final_values entry is not used;
 *   - width, returns and advantages of a trajectory are those of slhip_training_batch, float64 islands included.
 * The carried state between steps -- and between windows -- is active_now [B] (the reference's ~last_done) and
 * num_resets [envs]: after a step, active_now &= ~done; an env with no agent left has been reloaded by the step kernel
 * (auto_reset), so all its agents become active again and its num_resets goes up by one. */
#define SL_ROLLOUT_BAD_INDEX 2    /* bit of *status: slhip_rollout_gather met a row id outside [0, T * B) and skipped it */
#define SL_ROLLOUT_SCAN_CHUNK 4096 /* flags per workgroup of slhip_rollout_compact: its workspace holds one int32 per chunk */
typedef struct sl_rollout_multi { /* 96 bytes */
    sl_rollout w;                 /* the window; w.B = envs * n_agents columns */
    int32_t n_agents;             /* agents per env, 1 .. 8; w.B is a multiple of it */
    int32_t reserved;
    uint8_t *active;              /* [T, w.row_stride] 0 / 1 */
} sl_rollout_multi;

/* slhip_sample_actions with a mask: rows with active[e] == 0 get action 0 whatever their probabilities hold (NaN rows
 * included: they are not read); every other row gets exactly the draw of slhip_sample_actions for row e.  active: uint8
 * [B] (NULL: all active).  For a multi-agent batch the rows are the columns e * n_agents + a, and a caller that holds
 * envs [lo, hi) of a larger run passes seed + G * lo * n_agents. */
int slhip_sample_actions_masked(const float *probs, const uint8_t *active, int B, int n_actions, unsigned long long seed,
                                unsigned long long counter, int32_t *actions, void *stream);

/* Step t of the window, and the carried state moved on, in one launch.  Row t takes what slhip_rollout_record takes for
 * the columns with active_now != 0, and active[t] = active_now; an inactive column records action 0, probability 0,
 * reward 0, value 0 and done 0, and none of its inputs is looked at (no SL_ROLLOUT_BAD_ACTION either).  Then, per env:
 * active_now &= ~done; if no agent is left, active_now = 1 for all of them and num_resets[env] += 1.
 * actions int32, rewards (buf->w.reward_dtype), values float32, done uint8, active_now uint8: [B]; probs float32
 * [B, n_actions]; num_resets int64 [B / n_agents]. */
int slhip_rollout_record_multi(const sl_rollout_multi *buf, int t, const int32_t *actions, const float *probs,
                               int n_actions, const void *rewards, const float *values, const uint8_t *done,
                               uint8_t *active_now, long long *num_resets, void *stream);

/* Returns and advantages of the window by the rules above; arguments as slhip_training_batch.  Outputs at inactive rows
 * are left as they are (traj_start included).  With n_agents == 1 and every row active the outputs equal
 * slhip_training_batch's bit for bit. */
int slhip_training_batch_multi(const sl_rollout_multi *buf, const float *final_values, double gamma, double lmda,
                               float *returns, float *advantages, uint8_t *traj_start, void *stream);

/* The dense row ids t * B + column of the active rows, ascending -- (t, env, agent) order -- and their number: an exclusive
 * prefix sum of the flags over the whole window.  Two launches: every workgroup counts its chunk of SL_ROLLOUT_SCAN_CHUNK
 * flags into workspace[chunk]; then every workgroup sums the counts in front of its chunk, scans the chunk again (from
 * L2) and writes.  A row's place is a function of the flags alone: no atomic and no arrival order takes part.
 * rows_out: int64 [T * B], entries [0, N) are written; count_out: int64 [1] = N; workspace: int32
 * [slhip_rollout_compact_chunks(buf)]. */
int slhip_rollout_compact_chunks(const sl_rollout_multi *buf);
int slhip_rollout_compact(const sl_rollout_multi *buf, long long *rows_out, long long *count_out, int32_t *workspace,
                          void *stream);

/* The reference's flat tensors for rows[0 .. n): row id i = t * B + c reads element t * w.row_stride + c of the window's
 * arrays and t * w.out_stride + c of returns / advantages.  actions_out int64 [n]; action_prob_out, returns_out,
 * advantages_out, values_out float32 [n].  obs (optional, NULL: skipped): [T * B, obs_bytes] dense, rows are opaque bytes,
 * moved to obs_out [n, obs_bytes] 16 bytes per lane when obs_bytes and both pointers are multiples of 16, else with the
 * widest of 8 / 4 / 2 / 1 bytes that divides them all.  A row id outside [0, T * B) raises SL_ROLLOUT_BAD_INDEX in
 * *w.status and its output row is left as it was; nothing is read through it. */
int slhip_rollout_gather(const sl_rollout_multi *buf, const long long *rows, long long n, const float *returns,
                         const float *advantages, const void *obs, long long obs_bytes, void *obs_out,
                         long long *actions_out, float *action_prob_out, float *returns_out, float *advantages_out,
                         float *values_out, void *stream);

/* ---- level schedules: task switching, curricula, exit difficulty (additive to ABI 13: four new symbols and one new
 * struct, nothing existing changes, so SL_ABI_VERSION stays where it is) --------------------------------------------------
 * The reference's trainers draw every reset's level family from a schedule (training/env_factory.py: the coin of
 * SwitchingLevelIterator :155-174 with a scheduled probability, the softmax over recent slopes of performance of
 * CurricularLevelIterator :51-146) and scale every level's min_performance by a LinearSchedule of the training step
 * (MinPerformanceScheduler, :363-373).  Here the pool is a large pre-generated library that stays resident, cut into G
 * groups -- group g is the slot range [start[g], start[g] + len[g]), ranges disjoint, every len >= 1, slots outside every
 * group are never drawn -- and the step kernels stay as they are: these entry points rewrite what they read at launch
 * time, sl_env_batch.pool_next and pool_scalars[l].required_step, between two steps.
 *
 * The draw is PER SLOT AND STEP, not per env: two envs whose episodes end on the same slot in the same step load the same
 * successor (their random streams still differ through sl_env_batch.stream_salt).  The reference's envs share one iterator
 * queue, so neither side promises independent draws per env.
 *
 * The struct lives on the host; every pointer is a device pointer. */
#define SL_SCHEDULE_MAX_GROUPS 8
#define SL_SCHEDULE_MAX_LOOKBACK 1024
#define SL_SCHEDULE_BAD_PROBS 1   /* bit of *status: slhip_schedule_draw met device probabilities with a negative or
                                     non-finite entry, or a sum that is 0 or not finite, and drew uniformly over the groups */
typedef struct sl_level_schedule { /* 168 bytes */
    int32_t G;                    /* groups, 1 .. SL_SCHEDULE_MAX_GROUPS */
    int32_t lookback;             /* records per group ring, 2 .. SL_SCHEDULE_MAX_LOOKBACK (the reference: 100) */
    int32_t L;                    /* slots of the pool (sl_env_batch.L): every group lies inside [0, L) */
    int32_t reserved;
    int32_t start[SL_SCHEDULE_MAX_GROUPS];
    int32_t len[SL_SCHEDULE_MAX_GROUPS];
    /* per pool slot, from the host */
    const double *min_performance;   /* [L] the level's own min_performance (slhip_schedule_required) */
    const int32_t *available;        /* [L] GameWithGoals.initial_available_points of agent 0 (slhip_schedule_required) */
    const int32_t *reward_possible;  /* [L] available + points_on_level_exit (safelife_logger.py:286-294; harvest) */
    /* per env */
    int32_t *cur_slot;            /* [B] the slot the env's running episode was loaded from */
    /* per group (CurricularLevelIterator.perf_records / .best): a fresh schedule has ring[g][0] = 0.0, count = 1, pos = 1
       -- the reference's default record [0.0] -- and everything else 0 */
    double *ring;                 /* [G, lookback] */
    long long *count;             /* [G] records appended so far, the first 0.0 included */
    long long *episodes;          /* [G] episodes harvested */
    int32_t *pos;                 /* [G] where the next record goes = count % lookback */
    double *best;                 /* [G] the largest performance so far (>= 0: best_perf_lvl*) */
    double *mean;                 /* [G] mean of the ring's min(count, lookback) records, summed oldest first and divided
                                     once (recent100_perf_lvl*); written whenever the group takes a record */
    int32_t *status;              /* [1] SL_SCHEDULE_* bits, only ever raised by the library */
} sl_level_schedule;

/* pool_next[s] for every slot s in [0, L), one thread per slot.  With z(i) = splitmix64's finalizer of
 * seed + G64 * (counter * 0x100000001B3 + i + 1) mod 2^64 (G64 = 0x9E3779B97F4A7C15: slhip_sample_actions' construction)
 *   z1 = z(2 s), z2 = z(2 s + 1);
 *   u = (z1 >> 11) * 2^-53, a 53-bit uniform in [0, 1);  cum[g] = the float64 running sum p_0 + ... + p_g, in index order;
 *   t = u * cum[G-1] (one rounding);  g = the first group with cum[g] > t; if rounding leaves none, the last group with
 *   p_g > 0;  pool_next[s] = start[g] + (the high 64 bits of z2 * len[g]).
 * A group with p_g == 0 is never drawn.  The member draw's bias is at most len / 2^64.  Slots outside every group are
 * sources like any other (an env that stands on one moves into a group at its next reload).
 * probs: HOST pointer to G doubles, passed by value into the launch; a negative, NaN or infinite entry or a sum that is 0
 * (or overflows) is SL_E_SHAPE.  probs NULL: the device array device_probs [G] (what slhip_schedule_curriculum writes) is
 * read by the kernel; if it holds a negative or non-finite entry, or sums to 0 or to infinity, the kernel draws with equal
 * probabilities instead and raises SL_SCHEDULE_BAD_PROBS in *status -- nothing is sampled from garbage.
 * Needs of *sched: G, L, start, len, status.  L must be sched->L. */
int slhip_schedule_draw(const sl_level_schedule *sched, const double *probs, const double *device_probs,
                        unsigned long long seed, unsigned long long counter, int32_t *pool_next, int L, void *stream);

/* pool_scalars[l].required_step = max(0, (int32) ceil((min_performance[l] * fraction) * (double) available[l])) for every
 * slot l in [0, L): two float64 products, each rounded on its own -- levels.required_points(np.float64(mp) * fraction,
 * available), i.e. env_wrappers.py:142-145 followed by safelife_game.py:711-714, bit for bit (a NaN gives 0; a value past
 * int32 gives INT32_MAX).  Nothing else of the record is touched: required_reset and ready depend on the level's own
 * min_performance.  An env picks the new value up at its next reload, as the reference's wrapper evaluates its schedule
 * at reset().  fraction must be finite.  Needs of *sched: min_performance, available. */
int slhip_schedule_required(const sl_level_schedule *sched, double fraction, sl_level_scalars *pool_scalars, int L,
                            void *stream);

/* After every step.  For every env e with out[e].done, in ascending e: perf = f64(out[e].episode_reward) /
 * f64(reward_possible[cur_slot[e]]), 0.0 when that is not finite (env_factory.py:95-98), is appended to the ring of the
 * group cur_slot[e] lies in (ring[g][pos] = perf, pos = (pos + 1) % lookback, count += 1, episodes += 1, best = max(best,
 * perf)); an env whose cur_slot lies in no group leaves no record.  A record's place is a function of the done flags alone:
 * no atomic's arrival order takes part.  Then mean[g] is written for every group that took a record, and cur_slot[e] =
 * scalars[e].level_idx for EVERY env -- after an in-kernel reload that is the new level, which is why the schedule remembers
 * the old one.  Whoever reloads envs from outside the step (slhip_env_reset) sets their cur_slot from level_idx itself.
 * `out` takes 16-byte records (not sl_env_batch.out_compact).  One launch. */
int slhip_schedule_harvest(const sl_level_schedule *sched, const sl_step_out *out, const sl_env_scalars *scalars, int B,
                           void *stream);

/* CurricularLevelIterator.get_next_parameters (env_factory.py:111-127) in float64 -> probs_out [G] (device):
 *   tp[g] = 0.2 / lookback while count[g] < lookback; else 10 * m, m the least-squares slope of the ring's records
 *   y_0 (oldest) .. y_{n-1}, n = lookback, against 0 .. n-1 in closed form: xbar = (n - 1) / 2, sxx = n (n^2 - 1) / 12,
 *   sxy = sum_i (i - xbar) * y_i in index order, m = sxy / sxx;
 *   scale = min_g |tp[g]|;  tp = max(tp, 0) / scale, NaN and inf -> 0;  p[g] = exp(tp[g] - max tp) / sum_g exp(...), summed
 *   in index order.
 * Everything but exp() is exactly specified.  Where all records of a ring are equal the closed form gives m = 0 exactly
 * and the reference's polyfit gives rounding noise (which the division by `scale` then blows up): that input is
 * degenerate in the reference; here every group with tp <= 0 gets tp = 0, and if that makes scale 0 every entry becomes
 * NaN or inf -> 0 and the probabilities are equal. */
int slhip_schedule_curriculum(const sl_level_schedule *sched, double *probs_out, void *stream);

/* ---- level schedules for envs with several agents (additive again: two symbols and one wrapping struct; sl_level_schedule
 * stays as it is, 168 bytes, and SL_ABI_VERSION where it is) --------------------------------------------------------------
 * The reference's multi-agent tasks (training/env_factory.py: asym1, curriculum-asym1) run under the same iterators and the
 * same MinPerformanceScheduler.  The draw and the curriculum are those above, called on &m->s.  What differs is per agent:
 * every agent has its own required points (safelife_game.py:696-714 works on arrays over the agents), and the performance a
 * finished episode files is the AVERAGE over the env's agents (env_factory.py:91-101).
 * s.available and s.reward_possible are not read by the two entry points below; the per-agent arrays here are. */
typedef struct sl_level_schedule_multi { /* 208 bytes */
    sl_level_schedule s;
    int32_t n_agents;             /* A, 1 .. SL_MAX_AGENTS */
    int32_t reserved;
    const int32_t *available;        /* [L, A] initial_available_points()[a]: the agent's own table against the level's counts */
    const int32_t *reward_possible;  /* [L, A] available + points_on_level_exit */
    sl_level_agent *pool_agents;     /* [L, A] the env's sl_multi_agent.pool_agents (slhip_schedule_required_multi writes it) */
    const sl_step_out *out;          /* [B, A] the env's sl_multi_agent.out (slhip_schedule_harvest_multi reads it) */
} sl_level_schedule_multi;

/* pool_agents[l][a].required_step = max(0, (int32) ceil((min_performance[l] * fraction) * (double) available[l][a])) for
 * every slot l and agent a, one thread per pair: the two float64 products rounded one after the other, NaN and <= 0 -> 0,
 * >= 2^31 - 1 -> INT32_MAX, exactly as slhip_schedule_required.  Nothing else of a record is touched (required_reset is the
 * level's own min_performance).  The multi-agent step copies required_step into the agent's state when the env reloads, so
 * an env picks the new value up at its next reload.  fraction must be finite.
 * Needs of *m: s.L, s.min_performance, n_agents, available, pool_agents. */
int slhip_schedule_required_multi(const sl_level_schedule_multi *m, double fraction, void *stream);

/* slhip_schedule_harvest for records [B, A].  Env e has finished on this step when ALL of out[e][0 .. A) have done != 0 --
 * the step on which the multi-agent kernel reloads it; an agent that left earlier keeps done = 1 and its episode_reward in
 * `out` on every later step, so an episode whose agents finish on different steps files exactly one record, on the last of
 * them, and an env with only some agents done files nothing.  For every finished env, in ascending e, with slot =
 * cur_slot[e]:
 *   q[a] = f64(out[e][a].episode_reward) / f64(reward_possible[slot][a]);
 *   sum  = np.add.reduce(q): 0.0 + (q[0] + q[1] + ... in index order) for A < 8, and for A = 8 numpy's eight accumulators
 *          0.0 + (((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7)));
 *   perf = sum / f64(A); 0.0 when THAT is NaN or +-inf (the reference tests the average, not each quotient).
 * Everything else -- the ring, count / pos / episodes / best / mean, slots outside every group, cur_slot[e] =
 * scalars[e].level_idx for every env, the placing by the done flags alone -- is slhip_schedule_harvest's.  Records of envs
 * that have not finished are not read beyond their done bytes.  One launch.
 * Needs of *m: s (groups, rings, cur_slot), n_agents, reward_possible, out. */
int slhip_schedule_harvest_multi(const sl_level_schedule_multi *m, const sl_env_scalars *scalars, int B, void *stream);

/* ---- the episode log: rows, combined score, running summaries (additive to ABI 13: four new symbols and one new struct,
 * nothing existing changes, so SL_ABI_VERSION stays where it is) ---------------------------------------------------------
 * The arithmetic of the reference's SafeLifeLogger (safelife_logger.py): log_episode() :262-354 with combined_score()
 * :671-716 per finished episode, the running summaries of log_scalars() :372-381, and summarize_run_file() :719-762 over the
 * rows.  Files, tensorboard, wandb and video stay with the host.  These four entry points serve single-agent batches; the
 * four _multi ones further down serve batches with several agents per env.
 *
 * A finished episode becomes a ROW.  Row i (counted from the log's start) lives at rows[i % capacity]; a row is valid while
 * i >= n_rows - capacity and rows[i % capacity].index == i.  All float64 arithmetic is unfused, every operation rounded on
 * its own. */
typedef struct sl_episode_log_row { /* 96 bytes */
    int64_t index;                /* the row's own global index */
    int64_t training_steps;       /* the reference's cumulative <type>_steps when log_episode() ran for this episode */
    int64_t prev;                 /* global index of the same env's previous row, -1: none */
    int32_t env;
    int32_t level;                /* the pool slot the episode was played on */
    int32_t episode_idx;          /* the env's episode counter during that episode (sl_episode_record.episode_idx) */
    int32_t length;               /* info['episode']['length'] */
    float reward;                 /* info['episode']['reward'] */
    int32_t reward_possible;      /* initial_available_points() + points_on_level_exit of that slot */
    int32_t reward_needed;        /* required_points() of the episode */
    uint8_t success, times_up;
    uint8_t flags;                /* SL_LOG_JOINED: slhip_episode_log_join has filled the four side-effect fields */
    uint8_t reserved;
    double reward_frac;           /* f64(reward) / f64(max(reward_possible, 1)) */
    double side_effects[2];       /* the weighted totals (agent, inaction); NaN until joined */
    double side_effects_frac;     /* side_effects[0] / np.maximum(side_effects[1], 1); NaN until joined */
    double score;                 /* combined_score(); NaN until joined */
} sl_episode_log_row;
#define SL_LOG_JOINED 1
#define SL_LOG_KEYS 5             /* summaries, in the reference's order: side_effects, length, reward, success, score */
#define SL_LOG_COUNTERS 5         /* counters[]: n_rows, steps, episodes, summarised, unmatched */
#define SL_LOG_MAX_HOPS 64        /* rows slhip_episode_log_join follows along `prev` before it gives an entry up */
#define SL_LOG_RUN_SUMMARY 12     /* doubles slhip_episode_log_run_summary writes */

typedef struct sl_episode_log {   /* 104 bytes; every pointer is device memory */
    int64_t capacity;             /* rows of the ring, >= B (one harvest never laps itself) */
    int32_t B, L;                 /* envs; pool slots */
    double polyak;                /* summary_polyak: 0.99 for training, 1.0 for validation and benchmark */
    sl_episode_log_row *rows;     /* [capacity] */
    int64_t *counters;            /* [SL_LOG_COUNTERS] n_rows; steps (<type>_steps); episodes (<type>_episodes); summarised
                                     (rows the summaries have consumed); unmatched (queue entries that found no row) */
    /* per env: the episode the env is PLAYING.  After an in-kernel reload scalars[e] describes the new episode, so the log
     * remembers the old one, as the level schedule does. */
    int32_t *cur_slot;            /* [B] */
    int32_t *cur_required;        /* [B] */
    int32_t *cur_episode;         /* [B] */
    int64_t *last_row;            /* [B] global index of the env's latest row, -1: none */
    const int32_t *reward_possible; /* [L] per pool slot, from the host */
    double *value;                /* [SL_LOG_KEYS] summary_stats */
    int64_t *count;               /* [SL_LOG_KEYS] summary_counts */
    double *weight;               /* [SL_LOG_KEYS] the weight the key's NEXT value meets (the recurrence below) */
} sl_episode_log;

/* One launch after every step.  For every env e with out[e].done, in ascending e, row n_rows + rank(e) is written (rank: the
 * number of done envs below e -- a row's place is a function of the done flags alone, no atomic's arrival order takes
 * part): env = e, level = cur_slot[e], episode_idx = cur_episode[e], length / reward / success / times_up from out[e],
 * training_steps = steps + e + 1 (the reference steps its envs in index order against one shared counter and the wrapper
 * counts before it logs, :572-579), reward_possible = reward_possible[cur_slot[e]] (0 for a slot outside 0 .. L-1),
 * reward_needed = cur_required[e], reward_frac as above, prev = last_row[e], flags = 0, the side-effect fields and score NaN.
 * Then last_row[e] is the new row for those envs and, for EVERY env, cur_slot / cur_required / cur_episode =
 * scalars[e].level_idx / required_points / episode_idx.  steps += B, episodes += n, n_rows += n.  Records of envs that are
 * not done are not read beyond their done byte.  `out` takes 16-byte records (not sl_env_batch.out_compact).  Whoever
 * reloads envs from outside the step sets their cur_* from the scalars itself. */
int slhip_episode_log_harvest(const sl_episode_log *log, const sl_step_out *out, const sl_env_scalars *scalars, int B,
                              void *stream);

/* safelife_env.py:185-192's side_effect_weights: n <= SL_SE_MAX_KEYS pairs (cell, weight).  w(key) = 0.0 + the weights of
 * the pairs whose cell equals key, in index order. */
typedef struct sl_log_weights {
    int32_t n;
    int32_t reserved;
    uint16_t cell[SL_SE_MAX_KEYS];
    double weight[SL_SE_MAX_KEYS];
} sl_log_weights;   /* 248 bytes */

/* After a flush of the finished-episode queue and slhip_emd_batch: queue entry i < min(*count, capacity) carries
 *   total[j] = 0.0 + sum_k w(keys[i,k]) * scores[i,k,j]   over the key slots k in index order, a product rounded before its
 *   add; an empty slot (0xFFFF) contributes nothing and neither does a NaN score; NaN, NaN for an entry whose keys were cut
 *   short (n_cells[i,0] < 0).
 * It finds its row by walking `prev` from last_row[records[i].env] until env and episode_idx match.  The walk ends without
 * a row at -1, at a row that has been overwritten (index < n_rows - capacity, or the stored index differs), after
 * SL_LOG_MAX_HOPS rows, or at once for an env outside 0 .. B-1: the entry then counts into `unmatched`.  Otherwise the row gets
 *   side_effects = total;  side_effects_frac = total[0] / m, m = total[1] if that is NaN, else max(total[1], 1.0)
 *   (np.maximum);  speed = 1.0 - f64(length) / 1000.0;  score = (75.0 * reward_frac + 25.0 * speed) - 200.0 *
 *   side_effects_frac;  flags |= SL_LOG_JOINED.
 * scores double [C,SL_SE_MAX_KEYS,2], keys uint16 [C,SL_SE_MAX_KEYS], n_cells int32 [C,SL_SE_MAX_KEYS] as slhip_emd_batch
 * and slhip_side_effects leave them. */
int slhip_episode_log_join(const sl_episode_log *log, const sl_episode_queue *queue, const double *scores,
                           const uint16_t *keys, const int32_t *n_cells, const sl_log_weights *weights, void *stream);

/* log_scalars() :372-381 over rows [max(summarised, n_rows - capacity), n_rows) in row order, for each of the five keys:
 * v = side_effects_frac, f64(length), reward_frac, success (0.0 / 1.0), score.  A value that is not finite is skipped for
 * that key alone.  Otherwise, with w = weight[key]:
 *   value = (v + w * value) / (1.0 + w);  count += 1;  w = f64(count) when polyak >= 1, else w = polyak * (1.0 + w).
 * w starts at 0.0; the recurrence is the reference's p (1 - p^n) / (1 - p) without a pow, IEEE operations only.
 * Then summarised = n_rows.  One workgroup: lane k walks key k's chain, the others stage the rows through LDS. */
int slhip_episode_log_summaries(const sl_episode_log *log, void *stream);

/* summarize_run_file() :719-762 over rows [max(first_row, n_rows - capacity, 0), n_rows) -> out double
 * [SL_LOG_RUN_SUMMARY] (device):
 *   0 rows n   1 success   2 avg_length   3 side_effects   4 reward   5 score      (means)
 *   6 std side_effects   7 std reward   8 std score   9 mean, 10 std of length over the successful rows   11 their number
 * Per row the side-effect totals go through np.nan_to_num (NaN -> 0, +-inf -> +-DBL_MAX; a row never joined has NaN
 * totals), side_effects_frac and score are recomputed from them as in slhip_episode_log_join.  Every sum is ONE chain in
 * ascending row order starting from 0.0 -- fixed by the row range alone, never by launch geometry or arrival; a mean is
 * sum / f64(n), a standard deviation sqrt((sum of (x - mean) * (x - mean)) / f64(n)) in a second pass (np.std); n = 0 gives
 * NaN.  One workgroup. */
int slhip_episode_log_run_summary(const sl_episode_log *log, long long first_row, double *out, void *stream);

/* ---- the episode log for envs with several agents (additive again: four symbols, one log struct and one row layout beside
 * the single-agent ones, which stay byte for byte; SL_ABI_VERSION stays where it is) -----------------------------------------
 * What SafeLifeLogger does when info['episode'] holds arrays over the agents (safelife_logger.py:289-291, :319-328):
 *   - SafeLifeLogWrapper counts one <type>_steps per env step and logs once, on the step where np.all(done) (:572-579), so
 *     training_steps = steps + e + 1 and steps += B carry over;
 *   - length, reward, success, reward_possible, reward_needed, reward_frac and score are per agent; combined_score() sees one
 *     side_effects['total'] per episode, so the two totals and side_effects_frac are per row;
 *   - log_scalars() gets name-length, name-reward, name-success and name-score per agent, name = game.agent_names[i]; tb_data
 *     is a dict, so of two agents of one level with the same name the LAST one's values stay; tb_data['side_effects'] is a
 *     shape-(1,) array, fails np.isscalar and is never summarised.  (reward_frac_needed stays with the caller, as for the
 *     single-agent log.)
 * A row is a header followed by n_agents agent records: SL_LOG_ROW_MULTI_BYTES(A) bytes, the stride fixed by A when the log
 * is allocated -- 144 bytes for two agents where a stride of SL_MAX_AGENTS would take 384 (the two summary kernels stream
 * whole rows and the ring holds `capacity` of them).  Row i lives at rows + (i % capacity) * SL_LOG_ROW_MULTI_BYTES(A) and is
 * valid under the single-agent rule. */
typedef struct sl_episode_log_agent { /* 40 bytes */
    int32_t length;               /* info['episode']['length'][a] */
    float reward;                 /* info['episode']['reward'][a] */
    int32_t reward_possible;      /* (initial_available_points() + points_on_level_exit)[a] */
    int32_t reward_needed;        /* required_points()[a] of the episode */
    uint8_t success, times_up;
    uint8_t name;                 /* the agent's name id in 0 .. n_names-1; SL_LOG_NO_NAME for a slot outside 0 .. L-1 */
    uint8_t reserved[5];
    double reward_frac;           /* f64(reward) / f64(max(reward_possible, 1)) */
    double score;                 /* (75 reward_frac + 25 (1 - f64(length) / 1000)) - 200 side_effects_frac; NaN until joined */
} sl_episode_log_agent;
typedef struct sl_episode_log_row_multi { /* 64 bytes, then sl_episode_log_agent[n_agents] */
    int64_t index, training_steps, prev;   /* as sl_episode_log_row */
    int32_t env, level, episode_idx;
    uint8_t flags;                /* SL_LOG_JOINED */
    uint8_t n_agents;
    uint8_t reserved[2];
    double side_effects[2];       /* the episode's weighted totals (agent, inaction); NaN until joined */
    double side_effects_frac;     /* one per row; NaN until joined */
} sl_episode_log_row_multi;
#define SL_LOG_ROW_MULTI_BYTES(A) (64 + 40 * (A))
#define SL_LOG_MAX_NAMES 16       /* distinct agent names of a pool */
#define SL_LOG_NO_NAME 0xFF
#define SL_LOG_MULTI_KEYS 4       /* summaries per name, in the reference's order: length, reward, success, score */

typedef struct sl_episode_log_multi { /* 120 bytes; every pointer is device memory */
    int64_t capacity;             /* rows of the ring, >= B */
    int32_t B, L;
    int32_t n_agents;             /* A, 1 .. SL_MAX_AGENTS */
    int32_t n_names;              /* 1 .. SL_LOG_MAX_NAMES */
    double polyak;
    void *rows;                   /* [capacity] rows of SL_LOG_ROW_MULTI_BYTES(n_agents) bytes */
    int64_t *counters;            /* [SL_LOG_COUNTERS], as sl_episode_log */
    int32_t *cur_slot;            /* [B] the episode the env is PLAYING, as sl_episode_log */
    int32_t *cur_required;        /* [B, A] sl_agent_state.required_points of that episode: after an in-kernel reload the agent
                                     state describes the next one, which is why the log remembers */
    int32_t *cur_episode;         /* [B] */
    int64_t *last_row;            /* [B] */
    const int32_t *reward_possible; /* [L, A] per pool slot and agent, from the host (sl_level_schedule_multi's) */
    const uint8_t *name_id;       /* [L, A] per pool slot and agent: index into the host's list of the pool's distinct names */
    double *value;                /* [SL_LOG_MAX_NAMES, SL_LOG_MULTI_KEYS] summary_stats of "<name>-<key>" */
    int64_t *count;               /* [SL_LOG_MAX_NAMES, SL_LOG_MULTI_KEYS] summary_counts */
    double *weight;               /* [SL_LOG_MAX_NAMES, SL_LOG_MULTI_KEYS] */
} sl_episode_log_multi;

/* slhip_episode_log_harvest for records [B, A].  Env e has finished on this step when ALL of out[e][0 .. A) have done != 0
 * (slhip_schedule_harvest_multi's rule: the step on which the multi-agent kernel reloads the env; an agent that left earlier
 * keeps done = 1 and its episode accumulators in `out` on every later step, so an episode files exactly one row, on the step
 * of its last agent).  For every finished env, in ascending e, row n_rows + rank(e) -- rank: the number of finished envs below
 * e, a function of the all-done flags alone -- gets the header of slhip_episode_log_harvest (flags = 0, the totals and
 * side_effects_frac NaN) and per agent a: length / reward / success / times_up from out[e][a], reward_possible =
 * reward_possible[cur_slot[e]][a] and name = name_id[cur_slot[e]][a] (0 and SL_LOG_NO_NAME for a slot outside 0 .. L-1),
 * reward_needed = cur_required[e][a], reward_frac as above, score NaN.  Then last_row[e] is the new row for those envs and,
 * for EVERY env, cur_slot / cur_episode = scalars[e].level_idx / episode_idx and cur_required[e][a] =
 * agents[e][a].required_points.  steps += B, episodes += n, n_rows += n.  Records of envs that have not finished are not read
 * beyond their done bytes.  The env must reload finished envs inside the step (auto_reset): one that stayed all-done would
 * file a row per step where the reference files one.  One launch. */
int slhip_episode_log_harvest_multi(const sl_episode_log_multi *log, const sl_step_out *out, const sl_agent_state *agents,
                                    const sl_env_scalars *scalars, int B, void *stream);

/* slhip_episode_log_join for the multi-agent queue, which files one entry per env episode: the totals, the walk along `prev`
 * (SL_LOG_MAX_HOPS, the same validity checks, the same `unmatched` counter) and side_effects_frac are the single-agent
 * join's; then, per agent, score[a] from reward_frac[a], length[a] and the row's one fraction; flags |= SL_LOG_JOINED. */
int slhip_episode_log_join_multi(const sl_episode_log_multi *log, const sl_episode_queue *queue, const double *scores,
                                 const uint16_t *keys, const int32_t *n_cells, const sl_log_weights *weights, void *stream);

/* log_scalars() over rows [max(summarised, n_rows - capacity), n_rows) in row order.  Key (n, q), n < n_names, q of length,
 * reward, success, score: a row takes part if one of its agents has name n; its value is that of the LAST such agent (v =
 * f64(length), reward_frac, 0.0 / 1.0, score); a value that is not finite is skipped for that key alone (an earlier agent of
 * the name does not stand in).  The recurrence, w and count are slhip_episode_log_summaries'.  Then summarised = n_rows.
 * One workgroup: the 64 lanes of wave 0 walk one chain each out of LDS while the other waves stage the next 64 rows -- per
 * row and agent four values and the name id, so the staging grows with A and not with the number of keys. */
int slhip_episode_log_summaries_multi(const sl_episode_log_multi *log, void *stream);

/* summarize_run_file() over [N, A] arrays: the twelve outputs of slhip_episode_log_run_summary, where success, avg_length,
 * reward, score and the successful length run over the N * A (row, agent) entries -- each sum ONE chain in ascending (row,
 * agent) order starting from 0.0 -- and side_effects over the N rows; out[0] is N, out[11] the number of successful
 * entries.  The totals go through np.nan_to_num and side_effects_frac and every score are recomputed, two passes. */
int slhip_episode_log_run_summary_multi(const sl_episode_log_multi *log, long long first_row, double *out, void *stream);

/* ---- evaluation runs: exactly N episodes, then the envs retire (additive again: five symbols and three structs, nothing
 * existing changes; SL_ABI_VERSION stays where it is) ------------------------------------------------------------------------
 * What the reference's trainers do with run_episodes(envs, num_episodes) (training/base_algo.py:278-318): play N episodes
 * and stop.  No step kernel changes: small kernels on the caller's stream around the fused step read and rewrite what the
 * step reads and writes, as the level schedule and the episode log do.
 *
 * The model.  A run is N TICKETS 0 .. N-1 over the pool's L slots and G envs (G: the env count over all shards; a shard
 * holds envs g = env_offset + e, e in 0 .. B-1):
 *     ticket t  ->  slot t % L,  env t % G,  that env's k-th episode of the run, k = t / G
 * and the other way round env g plays tickets g, g + G, g + 2 G, ... below N.  The deal is static, so it needs no per-env
 * successor: it is what the stride rule does with first_level = g % L and level_stride = G % L under auto_reset.  An env
 * whose first ticket is >= N is never active.  An env that has played its last ticket RETIRES: it keeps stepping (its caller
 * hands it action 0) and the step kernel keeps reloading it, but its output records are zeroed from the next step on, so
 * nothing downstream -- the log's harvest, a rollout, a replay buffer, the caller -- sees these PHANTOM episodes.  The
 * finished-episode queue still receives them (the step kernel files them): slhip_episode_run_tickets tells them apart.  A
 * phantom episode under action 0 ends at the time limit, so a queue of N + B entries holds a whole run.
 * The run's env must not be reset from outside between slhip_episode_run_start and the end of the run: the k of an
 * episode is counted from base_episode. */
typedef struct sl_episode_run_row { /* 32 bytes: one per ticket */
    int32_t slot;                 /* t % L: the pool slot the episode was PLAYED on (scalars hold the reloaded one by then) */
    int32_t env;                  /* t % G: the global index of the env that played it */
    int32_t episode_idx;          /* the env's episode counter during that episode: base_episode + t / G */
    int32_t step;                 /* the `step` argument of the harvest that filed it */
    int32_t length;               /* info['episode']['length'] (several agents: agent 0's, as sl_episode_record) */
    float reward;                 /* info['episode']['reward'] (agent 0's) */
    uint8_t success, times_up;    /* (agent 0's) */
    uint8_t flags;                /* SL_RUN_WRITTEN | SL_RUN_SCORED */
    uint8_t reserved;
    int32_t reserved2;
} sl_episode_run_row;
typedef struct sl_episode_run_agent { /* 16 bytes: one per ticket and agent */
    int32_t length;
    float reward;
    uint8_t success, times_up, reserved[2];
    int32_t reserved2;
} sl_episode_run_agent;
#define SL_RUN_WRITTEN 1          /* a harvest has filed the ticket */
#define SL_RUN_SCORED 2           /* slhip_episode_run_tickets has filled side_effects[t] */
#define SL_RUN_COUNTERS 4         /* counters[]: completed (tickets filed by this shard), in progress (active envs), env steps
                                     taken by active envs, reserved */

typedef struct sl_episode_run {   /* 80 bytes; every pointer is device memory */
    int32_t B, G, env_offset;     /* envs of this shard, of all shards, global index of env 0 */
    int32_t N, L;                 /* tickets, pool slots */
    int32_t n_agents;             /* A, 1 .. SL_MAX_AGENTS */
    uint8_t *active;              /* [B] 1 while the env has a ticket to play */
    int32_t *played;              /* [B] episodes of the run the env has finished */
    int32_t *base_episode;        /* [B] scalars[e].episode_idx when the run started */
    int32_t *counters;            /* [SL_RUN_COUNTERS] */
    sl_episode_run_row *results;  /* [N] by ticket: the content does not depend on finishing order */
    sl_episode_run_agent *agent_results; /* [N, A] */
    double *side_effects;         /* [N, 2] the weighted totals (agent, inaction) of slhip_episode_run_tickets */
} sl_episode_run;

/* After the reset that put env e on slot (env_offset + e) % L: base_episode[e] = scalars[e].episode_idx, played[e] = 0,
 * active[e] = (env_offset + e < N), counters = (0, number of active envs, 0, 0), results, agent_results and side_effects all
 * zero bytes.  One launch. */
int slhip_episode_run_start(const sl_episode_run *run, const sl_env_scalars *scalars, void *stream);

/* One launch behind every step, BEFORE the episode log's harvest.  One thread per env, grid-stride.  With g = env_offset + e:
 *   - active[e] == 0 (retired before this step, or never active): out[e] = 16 zero bytes -- reward 0, done 0, success 0,
 *     times_up 0, episode reward and length 0;
 *   - active[e] != 0: the env took a step (counters[2] += 1).  If out[e].done: t = g + G * played[e]; results[t] = (t % L,
 *     g, base_episode[e] + played[e], step, out[e].episode_length, out[e].episode_reward, out[e].success, out[e].times_up,
 *     SL_RUN_WRITTEN); agent_results[t][0] likewise; played[e] += 1; counters[0] += 1; and if g + G * played[e] >= N the env
 *     retires: active[e] = 0, counters[1] -= 1.  Its record of THIS step stays as the step wrote it.
 * The counters are reduced per wave and take one integer atomicAdd per wave and counter that moved: integer sums are
 * order-free, so the outcome is a function of the records alone.  `out` takes 16-byte records. */
int slhip_episode_run_harvest(const sl_episode_run *run, sl_step_out *out, int step, void *stream);

/* The same for records [B, A]: env e's episode ends on the step where ALL of out[e][0 .. A) have done != 0 (the step on which
 * the multi-agent kernel reloads the env).  The row takes agent 0's length / reward / success / times_up, agent_results[t][a]
 * every agent's; a retired env has all A records zeroed. */
int slhip_episode_run_harvest_multi(const sl_episode_run *run, sl_step_out *out, int step, void *stream);

/* Tickets of the entries of a finished-episode queue: for i < min(*count, capacity), with e = records[i].env -
 * queue->env_base and k = records[i].episode_idx - base_episode[e],
 *     tickets[i] = (env_offset + e) + G * k   if 0 <= e < B, k >= 0 and that is < N,   else -1
 * (-1: an episode from before the run, or a retired env's phantom episode); tickets[i] = -1 for i >= the count.  With
 * `scores` (and keys, n_cells, weights as slhip_episode_log_join takes them) an entry with a ticket also writes
 * side_effects[t] = the entry's weighted totals, by the arithmetic of slhip_episode_log_join bit for bit (NaN, NaN for an
 * entry whose keys were cut short), and sets SL_RUN_SCORED in results[t].flags.  scores == NULL: tickets only. */
int slhip_episode_run_tickets(const sl_episode_run *run, const sl_episode_queue *queue, int32_t *tickets,
                              const double *scores, const uint16_t *keys, const int32_t *n_cells,
                              const sl_log_weights *weights, void *stream);

/* ---- episode histories: the board frames of selected episodes (additive again: two symbols and two structs, nothing existing
 * changes; SL_ABI_VERSION stays where it is) --------------------------------------------------------------------------------
 * What the reference's SafeLifeLogWrapper records (safelife_logger.py:560-592: game.board and game.goals appended after every
 * step) and SafeLifeLogger.log_episode keeps when (num_episodes - 1) % video_interval == 0 (:338-347).  No step kernel
 * changes: a recorder behind every step copies the boards of a small, fixed set of WATCHED envs into frame slots, and the
 * reference's interval rule decides at the episode's end which slots are kept.
 *
 * The model.
 *   watch       n ascending, distinct env indices in 0 .. B-1 (n <= SL_HIST_MAX_WATCH).
 *   slots       K <= SL_HIST_MAX_SLOTS; slot s holds one goals plane goals[s] uint16 [H,W] and T = time_limit board frames
 *               frames[s] uint16 [T,H,W].  slot_state[s]: SL_HIST_SLOT_FREE, _ENV (owned by the watched env i with
 *               owner[i] == s) or _ENTRY (held by the history entries[s]).
 *   owner[i]    the slot watched env i records into, or -1.  An env acquires a slot only where an episode STARTS -- a rewind
 *               (attach, a reset that reloads it) or the capture of the step that ended its previous episode -- never in
 *               mid-episode, so no history is partial at the front.
 *   free order  the envs that need a slot in one call take the free slots in ascending order on both sides: the r-th such
 *               env (ascending env index) takes the r-th free slot (ascending slot index) as slot_state stood when the call
 *               began; an env beyond the last free slot owns none (-1) until a later episode start finds one.
 *   an episode's start (for env e = watch[i]): cur_level[i] = scalars[e].level_idx, cur_episode[i] = scalars[e].episode_idx
 *               (after an in-kernel reload scalars[e] describes the NEXT episode, which is why these are kept), and, if the
 *               env owns a slot s, goals[s] = goals[e] as the reload left it.  A slot keeps ONE goals plane: histories are for
 *               pools whose goals are static (safelife_game.py:753-760).
 *
 * slhip_history_capture, behind every step.  `active` (may be NULL) is a mask uint8 [B]: an env with active[e] == 0 is
 * neither captured nor counted (an evaluation run's retired envs and their phantom episodes).  With done(e) = out[e].done != 0
 * and the env not masked out:
 *   numbering   the episodes that end in this call are numbered counters[0] + rank(e), rank(e) = the number of done envs below
 *               e over ALL B envs: the episode log's row index, the reference's num_episodes - 1.  A function of the done
 *               flags alone.  counters[0] += the number of done envs.
 *   the queue   only entries [counters[4], min(*queue.count, queue.capacity)) are looked at (counters[4], the cursor, then
 *               moves to that end; whoever installs a fresh queue zeroes it).  final(i) = the smallest such j with
 *               records[j].env - env_base == watch[i] and records[j].episode_idx == cur_episode[i], or none.
 *   per watched env i, e = watch[i], not masked out, s = owner[i]:
 *     not done, s >= 0:  frames[s][scalars[e].episode_length - 1] = board[e]
 *     done, number % interval == 0 (KEPT by rule):
 *        s < 0:   counters[2] (missed) += 1
 *        s >= 0:  counters[1] (kept) += 1; entries[s] = (row = number, e, cur_level[i], cur_episode[i], length =
 *                 out[e].episode_length, s, out[e].success, out[e].times_up, flags); slot_state[s] = SL_HIST_SLOT_ENTRY;
 *                 the env owns no slot any more.  With final(i) = j: frames[s][length - 1] = queue.boards[j], the board as the
 *                 agent left it, flags = SL_HIST_LIVE.  Without (the queue overflowed): the history lacks its last frame,
 *                 flags = SL_HIST_LIVE | SL_HIST_NO_FINAL, counters[3] (incomplete) += 1.
 *     done, not kept:    the slot stays with the env; the next episode overwrites it from frame 0.
 *     done (either way): an episode starts, as above; an env without a slot takes one by the free order.
 *   A frame index outside 0 .. T-1 is not written.  The entries of one call, sorted by row, are in ascending env order.
 *
 * Two launches: a bookkeeping pass in ONE workgroup (the done scan of slhip_episode_log_harvest, the new queue entries walked
 * through LDS by the lanes of the watched envs whose episode ended, two more workgroup scans for the free order) leaves one copy order per watched env in orders[i] (8 int32: source 0 none / 1 live board
 * / 2 queue board, queue index, slot, frame, the slot whose goals plane takes goals[e] or -1, 3 reserved); a copy pass over
 * watched envs x {frame, goals plane} carries them out with vector loads and stores of the widest of 16 / 8 / 4 / 2 bytes that
 * divides both addresses (a 25x25 board is 1250 bytes: odd envs are 2-byte aligned), and 2-byte ones for the rest.  No global
 * atomics. */
#define SL_HIST_LIVE 1            /* entries[s].flags: the entry holds slot s */
#define SL_HIST_NO_FINAL 2        /* the final frame (index length - 1) was not in the queue */
#define SL_HIST_SLOT_FREE 0
#define SL_HIST_SLOT_ENV 1
#define SL_HIST_SLOT_ENTRY 2
#define SL_HIST_MAX_WATCH 1024
#define SL_HIST_MAX_SLOTS 1024
#define SL_HIST_COUNTERS 8        /* counters[]: episodes, kept, missed, incomplete, cursor, 3 reserved */
#define SL_HIST_ORDER_WORDS 8
typedef struct sl_history_entry { /* 32 bytes */
    int64_t row;                  /* the episode's number: the episode log's row index */
    int32_t env, level, episode_idx; /* the level slot PLAYED and the env's episode counter during the episode */
    int32_t length;               /* info['episode']['length']: frames 0 .. length - 1 (length - 2 with SL_HIST_NO_FINAL) */
    int32_t slot;
    uint8_t success, times_up;    /* (several agents: success is a bit per agent, times_up their OR -- see _capture_multi) */
    uint8_t flags;                /* SL_HIST_LIVE | SL_HIST_NO_FINAL; 0: released */
    uint8_t reserved;             /* 0 from slhip_history_capture; the agent count A from slhip_history_capture_multi */
} sl_history_entry;

typedef struct sl_episode_history { /* 112 bytes; every pointer is device memory */
    int32_t B, n_watch, n_slots;  /* envs, watched envs n, slots K */
    int32_t T, H, W;              /* frames per slot (the env's time_limit) and the board shape */
    int32_t interval;             /* >= 1 */
    int32_t reserved;
    const int32_t *watch;         /* [n] */
    int32_t *owner;               /* [n] */
    int32_t *cur_level;           /* [n] */
    int32_t *cur_episode;         /* [n] */
    int32_t *slot_state;          /* [K] */
    sl_history_entry *entries;    /* [K]: entries[s] is the history held in slot s */
    long long *counters;          /* [SL_HIST_COUNTERS] */
    uint16_t *goals;              /* [K,H,W] */
    uint16_t *frames;             /* [K,T,H,W] */
    int32_t *orders;              /* [n, SL_HIST_ORDER_WORDS]: workspace between the two launches; 16-byte aligned */
} sl_episode_history;

/* board, goals uint16 [B,H,W]; scalars [B] and out [B] as the step left them; queue: the env's finished-episode queue
 * (capacity 0: none -- every kept history then lacks its final frame). */
int slhip_history_capture(const sl_episode_history *hist, const uint16_t *board, const uint16_t *goals,
                          const sl_env_scalars *scalars, const sl_step_out *out, const sl_episode_queue *queue,
                          const uint8_t *active, void *stream);

/* After the envs with mask[e] != 0 (mask == NULL: all) have been reloaded from outside the step, and once at attach: for
 * every such watched env an episode starts, as above -- it keeps the slot it owns and restarts at frame 0 on its new level, or
 * takes one by the free order.  Counters and entries are not touched.  The same two launches. */
int slhip_history_rewind(const sl_episode_history *hist, const uint16_t *goals, const sl_env_scalars *scalars,
                         const uint8_t *mask, void *stream);

/* ---- episode histories of multi-agent envs (additive: one symbol; SL_ABI_VERSION stays where it is) -------------------------
 * The reference's SafeLifeLogWrapper makes no difference between the env classes: it appends game.board after every step
 * (safelife_logger.py:560-581), logs on np.all(done), and log_episode (:338-347) saves the stack whatever the agent count.
 * Everything of the model above holds unchanged -- watched envs, slots, the free order, one goals plane per slot, the
 * numbering, the queue cursor, the interval rule, `active` -- with `out` holding records [B, A], A = n_agents in
 * 1 .. SL_MAX_AGENTS, and three things defined over the agents:
 *   done        env e ends an episode on the step where ALL of out[e][0 .. A) have done != 0: the rule of
 *               slhip_episode_log_harvest_multi and slhip_schedule_harvest_multi, and the step on which the multi-agent
 *               kernel reloads the env and queues the episode.  The numbering ranks THESE flags over all B envs, masked by
 *               `active`: a kept history's row is the row index of the multi-agent episode log.
 *   frames      the reference appends a frame on every step until np.all(done), so an episode has as many frames as the
 *               env took steps.  A live env writes frame scalars[e].num_steps - 1 (the multi-agent kernels count the env's
 *               steps there and zero it on reload; they do not maintain scalars[e].episode_length, which the single-agent
 *               pass reads).  An ended episode's length = max over a of out[e][a].episode_length: the agent that finished
 *               last was active on every step (safelife_env.py:174-175), so the maximum is the step count, and it equals
 *               the queue record's num_steps.
 *   the entry   sl_history_entry keeps its 32 bytes.  length as above; success is a BIT MASK, bit a = (out[e][a].success
 *               != 0) (at one agent: today's value); times_up = the OR over the agents (the same for all of them);
 *               reserved = A (the single-agent pass keeps writing 0 there).
 * Only the done byte of a record is looked at while the env's episode goes on: the other bytes of an agent that has left
 * are read on the step where the last agent finishes, and by then the step has rewritten none of them.
 * The last frame comes from the finished-episode queue exactly as above (the multi-agent step queues ONE entry per env
 * episode, the board as the agents left it): the first j at or behind the cursor with (records[j].env - env_base,
 * records[j].episode_idx) == (watch[i], cur_episode[i]).  slhip_history_rewind serves both env classes as it is: it reads
 * scalars[e].level_idx, scalars[e].episode_idx and goals[e], which both kinds of kernels keep.
 * The same two launches; the bookkeeping pass is the same body as the single-agent one, instantiated on a reader of A
 * records per env (the done scan takes the nt * A records of a tile as one flat stream of unconditional loads). */
int slhip_history_capture_multi(const sl_episode_history *hist, const uint16_t *board, const uint16_t *goals,
                                const sl_env_scalars *scalars, const sl_step_out *out /* [B, A] */, int n_agents,
                                const sl_episode_queue *queue, const uint8_t *active, void *stream);

/* ---- the PPO update: minibatch deal, fused clipped loss and gradients (additive again: six symbols and one struct, nothing
 * existing changes; SL_ABI_VERSION stays where it is) --------------------------------------------------------------------------
 * What the reference does with a training batch (training/ppo.py:145-182): PPO.calculate_loss and the minibatch loop of
 * PPO.train_batch.  The struct lives on the HOST; every pointer inside is a device pointer the caller owns.
 *
 * Per minibatch row i (r = rows ? rows[i] : i the batch row behind it, a = actions[r]; f32(x) = x rounded to float32; every
 * operation below is a float32 operation in this order, nothing fused, IEEE division, the library's logf):
 *   pd_i     = sign(A_r) * (1 - policy[i][a] / action_prob[r])        sign(0) = 0
 *   policy_i = |A_r| * max(pd_i, -f32(eps_policy))                    a ONE-sided clamp
 *   vc_i     = old_values[r] + clamp(values[i] - old_values[r], -f32(eps_value), +f32(eps_value))
 *   value_i  = max((vc_i - returns[r])^2, (values[i] - returns[r])^2)
 *   ent_i    = sum over k in index order of (-policy[i][k]) * log(policy[i][k] + f32(1e-12))
 * and over the minibatch, in float64 (deterministic sums of the float32 terms: a fixed tree per workgroup of 256 rows, the
 * workgroups in index order):
 *   P = sum(policy_i) / n, V = sum(value_i) / n, E = sum(ent_i) / n
 *   flag = f32(E) <= f32(entropy_clip)                                the entropy bonus has a gradient
 *   term = -f32(entropy_reg) * (flag ? E : f32(entropy_clip))
 *   loss = P + f32(vf_coef) * V + term
 * A row id outside [0, N) raises SL_PPO_BAD_INDEX in *status, an action outside [0, n_actions) SL_PPO_BAD_ACTION; such a row
 * reads nothing through the bad value, adds zero to every sum (n stays the divisor), has entropy 0 and zero gradients. */
#define SL_PPO_BAD_ACTION 1
#define SL_PPO_BAD_INDEX 2
#define SL_PPO_SUMS 8             /* doubles in sums_out */
#define SL_PPO_SUM_POLICY 0       /* P */
#define SL_PPO_SUM_VALUE 1        /* V */
#define SL_PPO_SUM_ENTROPY 2      /* E */
#define SL_PPO_SUM_ENTROPY_TERM 3 /* term */
#define SL_PPO_SUM_LOSS 4         /* loss */
#define SL_PPO_SUM_FLAG 5         /* 1.0 or 0.0 */
#define SL_PPO_SUM_N 6            /* n */
#define SL_PPO_SUM_LOSS_F32 7     /* NOT a double: the slot's first four bytes hold loss rounded to float32, the rest zero */
typedef struct sl_ppo_loss {      /* 136 bytes */
    long long n;                  /* rows of the minibatch: of values, policy and rows; >= 1 */
    long long N;                  /* rows of the batch: of actions .. advantages; >= 1 */
    int32_t n_actions;            /* 2 .. 32 */
    int32_t reserved;
    double eps_policy, eps_value, vf_coef, entropy_reg, entropy_clip;
    const float *values;          /* [n] the model's values for the minibatch */
    const float *policy;          /* [n, n_actions] its probabilities */
    const long long *actions;     /* [N] */
    const float *action_prob;     /* [N] the probability the old policy gave the action taken */
    const float *old_values;      /* [N] */
    const float *returns;         /* [N] */
    const float *advantages;      /* [N] */
    const long long *rows;        /* [n] batch row of every minibatch row, or NULL: row i is batch row i and n == N */
    long long *status;            /* one device word, zeroed by the caller; the kernels only ever set bits (SL_PPO_*) */
} sl_ppo_loss;

/* bytes of `workspace` for a minibatch of n rows (three doubles per workgroup of 256 rows); 8-byte aligned */
size_t slhip_ppo_workspace_bytes(long long n);

/* entropy_out float32 [n]: ent_i;  sums_out double [SL_PPO_SUMS], 8-byte aligned: the SL_PPO_SUM_* above.  Two launches: the
 * row pass and a one-workgroup finish. */
int slhip_ppo_loss_forward(const sl_ppo_loss *loss, float *entropy_out, double *sums_out, void *workspace, void *stream);

/* d_values float32 [n] and d_policy float32 [n, n_actions]: the gradients torch's autograd gives the expression above for
 *   *grad_loss * loss + sum_i grad_entropy[i] * ent_i        (grad_loss: a device float32; grad_entropy: [n] or NULL)
 * computed in float32 the way autograd walks the graph: mean's backward divides by f32(n), a clamp passes the gradient where its
 * input EQUALS a bound, the elementwise maximum gives each side half on a tie, sign(0) = 0, and the entropy term has no gradient
 * when sums[SL_PPO_SUM_FLAG] is 0.  `sums` is what slhip_ppo_loss_forward wrote for the same *loss.  One launch. */
int slhip_ppo_loss_backward(const sl_ppo_loss *loss, const float *grad_loss, const float *grad_entropy, const double *sums,
                            float *d_values, float *d_policy, void *stream);

/* out[i] = row rows[i] of obs for i in [0, n): obs is [N, obs_bytes] opaque bytes, out [n, obs_bytes]; with out_float32 != 0 obs is
 * uint8 and out float32 [n, obs_bytes], widened in the same pass.  Lanes move the widest of 16 / 8 / 4 / 2 / 1 bytes that divides
 * obs_bytes and both pointers (widening: 4 / 2 / 1 bytes in, as many floats out).  A row id outside [0, N) raises SL_PPO_BAD_INDEX
 * in *status and leaves out[i] as it was. */
int slhip_minibatch_obs(const void *obs, long long obs_bytes, long long N, const long long *rows, long long n, void *out,
                        int out_float32, long long *status, void *stream);

/* keys[i] = z(seed, epoch, i) for i in [0, N): splitmix64's finalizer of seed + G * (epoch * 0x100000001B3 + i + 1) mod 2^64 --
 * slhip_sample_actions' construction with the epoch as the counter.  A minibatch deal is the stable argsort of the keys. */
int slhip_minibatch_keys(long long N, unsigned long long seed, unsigned long long epoch, unsigned long long *keys, void *stream);

/* ---- the PPO report: loss / entropy / values / advantages over a WHOLE batch, evaluated chunk by chunk (additive again: three
 * symbols, nothing existing changes; SL_ABI_VERSION stays where it is) ------------------------------------------------------
 * What the reference's PPO.train logs (training/ppo.py:199-205): calculate_loss on the whole batch, its loss, the mean entropy,
 * and the means of batch.values and batch.advantages.  The reference calls the model on the whole batch at once; here the
 * caller calls it on chunks of the batch and hands every chunk's outputs to slhip_ppo_report_rows, then calls
 * slhip_ppo_report_finish once.  The loss clips the entropy bonus at the BATCH's mean entropy, so chunk losses cannot be
 * averaged: the row pass leaves float64 partial sums, one set per 256 batch rows, each at its place in the whole batch, and
 * the finish adds them in index order.  The result is the same, bit for bit, however the batch was cut into chunks, and its
 * first seven doubles are the sums_out slhip_ppo_loss_forward writes for the whole batch in one call (rows == NULL). */
#define SL_PPO_REPORT_PARTIALS 5     /* doubles per 256 rows in the workspace: policy, value, entropy, old_values, advantages */
#define SL_PPO_REPORT_DOUBLES 11     /* doubles in `out`; slots 0 .. 6 are SL_PPO_SUM_POLICY .. SL_PPO_SUM_N */
#define SL_PPO_REPORT_VALUES 7       /* mean of old_values (batch.values) */
#define SL_PPO_REPORT_ADVANTAGES 8   /* mean of advantages */
#define SL_PPO_REPORT_F32 9          /* NOT doubles: slots 9 and 10 hold four float32, the scalars as the reference logs them */
#define SL_PPO_REPORT_F32_LOSS 0
#define SL_PPO_REPORT_F32_ENTROPY 1
#define SL_PPO_REPORT_F32_VALUES 2
#define SL_PPO_REPORT_F32_ADVANTAGES 3

/* bytes of the report's workspace for a batch of N rows (five doubles per 256 rows); 8-byte aligned */
size_t slhip_ppo_report_workspace_bytes(long long N);

/* Rows [first_row, first_row + loss->n) of a batch of loss->N rows: loss->values [n] and loss->policy [n, n_actions] are the
 * model's outputs for THIS CHUNK, the five per-row scalars are read at batch row first_row + i, loss->rows is not looked at.
 * first_row must be a multiple of 256 with first_row + n <= N, and n a multiple of 256 unless the chunk ends the batch:
 * anything else returns SL_E_ARG and writes nothing.  Workgroup b writes SL_PPO_REPORT_PARTIALS doubles at
 * partial[(first_row / 256 + b) * SL_PPO_REPORT_PARTIALS]; the first three are the very numbers slhip_ppo_loss_forward's row pass
 * leaves for the same rows.  A row whose action is outside [0, n_actions) raises SL_PPO_BAD_ACTION in *status and adds zero to
 * all five.  No per-row output, no gradient.  One launch. */
int slhip_ppo_report_rows(const sl_ppo_loss *loss, long long first_row, double *partial, void *stream);

/* After the row pass has covered every row of the batch: `blocks` = ceil(N / 256) sets of partials -> out double
 * [SL_PPO_REPORT_DOUBLES].  The divisor of every mean is loss->N; only N and the five hyper-parameters of *loss are read.  One
 * workgroup. */
int slhip_ppo_report_finish(const sl_ppo_loss *loss, const double *partial, long long blocks, double *out, void *stream);

/* ---- the DQN update: fused TD loss and gradients (additive again: three symbols and one struct, nothing existing changes;
 * SL_ABI_VERSION stays where it is) ------------------------------------------------------------------------------------------
 * What the reference's DQN.optimize does with a sample after the two model calls (training/dqn.py:152-157) and what it reports
 * (:165-170).  The struct lives on the HOST; every pointer inside is a device pointer the caller owns.
 *
 * The three per-row scalars come in one of two forms (`source`):
 *   SL_DQN_FROM_RING    action int32, reward float64, done uint8: the storage of sl_replay's ring, read in place
 *   SL_DQN_FROM_BATCH   action int64, reward float32, done float32: what slhip_replay_gather wrote
 * Per minibatch row i (r = index ? index[i] : i the source row behind it, a = action[r]; f32(x) = x rounded to float32; every
 * operation below is a separate float32 operation in this order, nothing is contracted into an FMA):
 *   rew_i  = f32(reward[r])                        ring form: the float64 n-step sum rounded ONCE, as slhip_replay_gather does
 *   nd_i   = 1 - f32(done[r])
 *   disc_i = f32(discount) * nd_i                  discount: gamma ** multi_step, computed by the caller in double
 *   m_i    = max over k of next_q_values[i][k]     torch.max's value: NaN if any element is NaN
 *   exp_i  = rew_i + disc_i * m_i                  the product rounded, then the sum rounded
 *   td_i   = q_values[i][a] - exp_i
 * and over the minibatch, in float64 (deterministic sums of the float32 terms: a fixed tree per workgroup of 256 rows, the
 * workgroups in index order; a row's elements are added in index order):
 *   loss          = sum(td_i * td_i) / n           each square a float32 product
 *   q_model_mean  = sum of the n * n_actions elements of q_values / (n * n_actions)
 *   q_model_max   = sum over i of (max over k of q_values[i][k]) / n
 *   q_target_mean = sum of the n * n_actions elements of next_q_values / (n * n_actions)
 *   q_target_max  = sum(m_i) / n
 * An index outside [0, N) raises SL_DQN_BAD_INDEX in *status, an action outside [0, n_actions) SL_DQN_BAD_ACTION; such a row
 * reads nothing through the bad value, has td_i = 0, adds zero to the loss sum and to q_target_max (n stays the divisor) and gets
 * zero gradients.  q_model_mean, q_model_max and q_target_mean depend on neither index nor action and count every row. */
#define SL_DQN_BAD_ACTION 1
#define SL_DQN_BAD_INDEX 2
#define SL_DQN_FROM_RING 0
#define SL_DQN_FROM_BATCH 1
#define SL_DQN_SUMS 8               /* doubles in sums_out */
#define SL_DQN_SUM_LOSS 0
#define SL_DQN_SUM_Q_MODEL_MEAN 1
#define SL_DQN_SUM_Q_MODEL_MAX 2
#define SL_DQN_SUM_Q_TARGET_MEAN 3
#define SL_DQN_SUM_Q_TARGET_MAX 4
#define SL_DQN_SUM_N 5              /* n */
#define SL_DQN_SUM_RESERVED 6       /* zero */
#define SL_DQN_SUM_LOSS_F32 7       /* NOT a double: the slot's first four bytes hold loss rounded to float32, the rest zero */
typedef struct sl_dqn_loss {        /* 88 bytes */
    long long n;                    /* rows of the minibatch: of q_values, next_q_values and index; >= 1 */
    long long N;                    /* rows of the source: of action, reward and done; >= 1 */
    int32_t n_actions;              /* 2 .. 32 */
    int32_t source;                 /* SL_DQN_FROM_RING or SL_DQN_FROM_BATCH */
    double discount;                /* gamma ** multi_step */
    const float *q_values;          /* [n, n_actions] the training model's Q-values for the minibatch's observations */
    const float *next_q_values;     /* [n, n_actions] the target model's for its next observations (no gradient) */
    const void *action;             /* [N] int32 (ring) or int64 (batch) */
    const void *reward;             /* [N] float64 (ring) or float32 (batch) */
    const void *done;               /* [N] uint8 (ring) or float32 (batch) */
    const long long *index;         /* [n] source row of every minibatch row, or NULL: row i is source row i and n == N */
    long long *status;              /* one device word, zeroed by the caller; the kernels only ever set bits (SL_DQN_*) */
} sl_dqn_loss;

/* bytes of `workspace` for a minibatch of n rows (five doubles per workgroup of 256 rows); 8-byte aligned */
size_t slhip_dqn_workspace_bytes(long long n);

/* td_out float32 [n]: td_i;  sums_out double [SL_DQN_SUMS], 8-byte aligned: the SL_DQN_SUM_* above.  The row pass and a
 * one-workgroup finish: two launches, or ONE when the minibatch fits the row pass's single workgroup (n <= 256; the reference's
 * batch of 96 rows does) -- the workgroup then finishes its own sums, to the same bits. */
int slhip_dqn_loss_forward(const sl_dqn_loss *loss, float *td_out, double *sums_out, void *workspace, void *stream);

/* d_q float32 [n, n_actions], every element written: the gradient torch's autograd gives the expression above for
 *   *grad_loss * loss + sum_i grad_td[i] * td_i              (grad_loss: a device float32; grad_td: [n] or NULL)
 * with respect to q_values (next_q_values is detached in the reference):
 *   d_q[i][k] = (*grad_loss / f32(n)) * (2 * td_i) (+ grad_td[i]) at k = a, and 0 elsewhere
 * -- mean's backward divides by f32(n), pow's multiplies by 2 * td, gather's scatters.  Reads td (what slhip_dqn_loss_forward
 * wrote for the same *loss), the actions through index, and nothing else.  One launch. */
int slhip_dqn_loss_backward(const sl_dqn_loss *loss, const float *grad_loss, const float *grad_td, const float *td,
                            float *d_q, void *stream);

/* ---- the state digest: a 64-bit checksum of device memory, per segment of a table (additive again: three symbols and one
 * struct, nothing existing changes; SL_ABI_VERSION stays where it is) ---------------------------------------------------------
 * What a checkpoint uses to tell that what it uploaded is what it saved, and what two runs use to compare their whole state,
 * without a host copy.  An INTEGRITY checksum, NOT a cryptographic hash: it is not hard to find two inputs that collide.
 *
 * All arithmetic mod 2^64.  mix(z) is splitmix64's finaliser:
 *   z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 * and G = 0x9E3779B97F4A7C15.  A segment of n bytes is read as ceil(n / 8) little-endian 64-bit words w_i (i from 0), bytes
 * past n counting as zero:
 *   acc    = sum over i of mix(w_i + mix(salt) + (i + 1) * G)
 *   digest = mix(acc + mix((salt ^ n) + G))
 * Known answers: no bytes, salt 0 -> 0x48218226ff3cd4bf; the bytes 0..19, salt 0 -> 0x0c817c4bd668decf; the same with salt 7 ->
 * 0x510af6e63ac50e25.  The sum is an integer sum, so it does not depend on the order of its terms: the split over workgroups is
 * free, and two calls over the same bytes are bit-equal by construction.
 *
 * `segments` and `out` are DEVICE arrays of n_segments entries (8-byte aligned); out[s] is the digest of segment s, and nothing
 * beyond out[n_segments - 1] is written.  A segment's ptr may have ANY byte alignment and its bytes may be 0 (ptr is then not
 * looked at).  The kernels only read the segments, and never a byte outside [ptr, ptr + bytes): words whose aligned 8-byte
 * carriers lie wholly inside the segment are read with aligned loads, 16 bytes per lane; the first and last few are put together
 * byte by byte.
 *
 * `workspace` is a device buffer of slhip_state_digest_workspace_bytes(bytes, n_segments) bytes, 8-byte aligned.  Its HEAD is
 * the chunk prefix table, n_segments + 1 words, which the CALLER fills before the call with what
 * slhip_state_digest_prefix(bytes, n_segments, ...) computes on the host from the same byte counts (it rides along with the
 * upload of the segment table); the rest is the kernels' scratch.  The table deals fixed-size chunks of ALL segments over one
 * capped grid, so a table of many 4-byte counters and one ring of hundreds of MB keeps every workgroup busy.
 * Two launches: the chunk pass and a one-wavefront-per-segment finish.  No atomics, no floating point. */
typedef struct sl_digest_segment {  /* 16 bytes */
    const void *ptr;                /* device memory, any alignment */
    unsigned long long bytes;
} sl_digest_segment;

size_t slhip_state_digest_workspace_bytes(const unsigned long long *bytes /* host */, int n_segments);

/* prefix_out: HOST, n_segments + 1 words -- the head of the workspace (see above) */
int slhip_state_digest_prefix(const unsigned long long *bytes /* host */, int n_segments, unsigned long long *prefix_out);

int slhip_state_digest(const sl_digest_segment *segments /* device */, int n_segments, unsigned long long salt,
                       unsigned long long *out /* device, n_segments */, void *workspace, void *stream);

/* ---- batched pattern generation: N Metropolis chains of the level generator (additive again: two symbols, nothing existing
 * changes; SL_ABI_VERSION stays where it is) ----------------------------------------------------------------------------------
 * The reference's gen_pattern (gen_board.c:316-510) for N independent problems of one (H, W, depth), one wavefront each.
 * Per problem p, all DEVICE memory:
 *   layers     uint16 [N][depth][H][W]  layer 0 is the board; layer n is layer n - 1 after ONE step of the full Life rule at
 *                                       spawn probability 0 (module.c:374-378 -- the caller makes them, with
 *                                       slhip_advance_board, which also consumes the draws a spawner costs)
 *   mask       int32  [N][H][W]         bits SL_GEN_NEW_CELL | SL_GEN_CAN_OSCILLATE | SL_GEN_INCLUDE_VIOLATIONS
 *   seeds      int32  [N][H][W]         non-zero: a seed cell; NULL: the mask stands in (the reference's seeds=None)
 *   params     double [N][12]           rel_max_iter, rel_min_fill, temperature, osc_bonus, cell_penalties[8] -- intercept and
 *                                       slope per cell type EMPTY, WALL, ALIVE, TREE, as module.c:322-325 leaves them
 *   rng        uint64 [N][6]            numpy PCG64: state hi, lo, inc hi, lo, has_uint32, uinteger; advanced IN PLACE.  The
 *                                       32-bit draws of random_int buffer their high half in the last two words and the 64-bit
 *                                       draws of random_float leave it alone, so four words do not carry this function.
 *   out_board  uint16 [N][H][W]         the new layer 0 where status is 0, the input board otherwise
 *   status     int32  [N]               0, SL_GEN_PATTERN_MAX_ITER, or SL_GEN_PATTERN_REFUSED (rel_max_iter * area * depth does
 *                                       not fit an int: the reference's conversion is undefined there; nothing was drawn)
 *   iterations int32  [N]               iterations run
 * Board, status and the six words are bit-equal to the reference's.  All arithmetic is IEEE double without fusion; exp() is
 * the one call whose last bit may differ from a host libm's, which changes a pick only when the uniform draw lands within a
 * few ulps of a cumulative probability.
 * Supported: 3 <= H, W <= 64 and 1 <= depth <= 4; anything else is refused (SL_E_SHAPE below 3x3 with the reference's message,
 * SL_E_ARG for depth < 1, SL_E_UNSUPPORTED above the range).  A chain's state lives in LDS where it fits 64 KiB; for the larger
 * shapes `workspace` is a 16-byte aligned device buffer of slhip_gen_pattern_workspace_bytes bytes (0: none needed, and
 * `workspace` may be NULL).  Nothing outside a problem's own slices is read or written. */
#define SL_GEN_NEW_CELL 1
#define SL_GEN_CAN_OSCILLATE 2
#define SL_GEN_INCLUDE_VIOLATIONS 4
#define SL_GEN_PATTERN_MAX_SIDE 64
#define SL_GEN_PATTERN_MAX_PERIOD 4
#define SL_GEN_PATTERN_PARAMS 12
#define SL_GEN_PATTERN_RNG_WORDS 6
#define SL_GEN_PATTERN_MAX_ITER (-1)
#define SL_GEN_PATTERN_REFUSED (-4)

size_t slhip_gen_pattern_workspace_bytes(int N, int H, int W, int depth);

int slhip_gen_pattern_batch(const uint16_t *layers, const int32_t *mask, const int32_t *seeds, const double *params,
                            unsigned long long *rng, uint16_t *out_board, int32_t *status, int32_t *iterations, int N, int H,
                            int W, int depth, void *workspace, size_t workspace_bytes, void *stream);

/* ---- batched region partition of the level generator (additive again: two symbols, nothing existing changes; SL_ABI_VERSION
 * stays where it is) ---------------------------------------------------------------------------------------------------------------
 * safelife_amd.proc_gen.partition for N independent problems of one (H, W), one wavefront each.  Per problem p, all DEVICE
 * memory:
 *   rng          uint64 [N][6]     numpy PCG64: state hi, lo, inc hi, lo, has_uint32, uinteger; advanced IN PLACE where status
 *                                  is 0.  The draws are numpy's: Generator.integers(0, n) is Lemire's bounded method on
 *                                  next_uint32 (the low half of a 64-bit output first, the high half buffered in the last two
 *                                  words; nothing drawn for n == 1), Generator.random() a fresh 64-bit output.
 *   min_regions  int32  [N]        the problem's bounds as the spec gives them; clamped as the host function clamps them:
 *   max_regions  int32  [N]        lo = max(1, min), hi = max(max, lo)
 *   labels       int16  [N][H][W]  0 = buffer, 1.. = region; written where status is 0
 *   status       int32  [N]        0; SL_PARTITION_REFUSED: H or W outside 3 .. 64, or hi above `regions` -- nothing was drawn;
 *                                  SL_PARTITION_CAPPED: the turn loop passed regions * H * W + 1 turns or a bounded draw 64
 *                                  redraws (neither happens: the caps are there because no loop on a shared device may be
 *                                  unbounded).  Where status is not 0 the problem's labels and words are left untouched.
 * Labels and words are bit-equal to proc_gen.partition on a Generator(PCG64) set to the same words.
 * `regions` (1 .. 8) is how many regions a problem's state has room for: one bitmap and one frontier of H * W cells per region
 * beside the labels.  The state lives in LDS where it fits 64 KiB; above that (64x64 with room for eight) `workspace` is a
 * 16-byte aligned device buffer of slhip_partition_workspace_bytes bytes (0: none needed, and `workspace` may be NULL).
 * Errors of the call itself (SL_E_ARG): N < 0, regions outside 1 .. 8, a null or misaligned pointer, a workspace too small. */
#define SL_PARTITION_MAX_SIDE 64
#define SL_PARTITION_MAX_REGIONS 8
#define SL_PARTITION_RNG_WORDS 6
#define SL_PARTITION_REFUSED (-4)
#define SL_PARTITION_CAPPED (-5)

size_t slhip_partition_workspace_bytes(int N, int H, int W, int max_regions);

int slhip_partition_batch(unsigned long long *rng, const int32_t *min_regions, const int32_t *max_regions, int16_t *labels,
                          int32_t *status, int N, int H, int W, int regions, void *workspace, size_t workspace_bytes,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SAFELIFE_HIP_H */
