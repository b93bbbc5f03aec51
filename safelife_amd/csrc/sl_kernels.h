// sl_kernels.h -- launcher prototypes shared between the kernel translation units and the C-ABI.
#pragma once

#include <hip/hip_runtime.h>

#include "sl_device.h"

namespace sl {

size_t generic_lds_bytes(int HW, int nbuf);

// sl_generic.hip : one workgroup per board, any 3 <= H, W with H*W <= SL_MAX_CELLS
hipError_t launch_advance_generic(const u16 *in, u16 *out, int B, int H, int W, const float *spawn_prob,
                                  int n_steps, sl_pcg64 *rng, const Jump *jump, int32_t *occupancy,
                                  hipStream_t stream, const int32_t *n_each = nullptr, const int32_t *n_valid = nullptr);
// life_occupancy with the counters in LDS (uint16 per cell and colour): boards of up to 4096 cells, n_steps <= 65535;
// the arguments of launch_occupancy_rowlane below, same meaning
bool occupancy_generic_supports(int H, int W, int n_steps);
hipError_t launch_occupancy_generic(const u16 *in, int32_t *counts, size_t counts_stride, int B, const int32_t *n_valid,
                                    int valid_period, const int32_t *pre_steps, int H, int W, const float *spawn_prob,
                                    int n_steps, sl_pcg64 *rng, const Jump *jump, hipStream_t stream);
hipError_t launch_alive_counts(const u16 *board, const u16 *goals, int B, int HW, int64_t *out,
                               hipStream_t stream);
hipError_t launch_execute_actions(u16 *board, int B, int H, int W, int64_t *locs, const int64_t *actions,
                                  int A, int action_stride, int action_batch_stride, hipStream_t stream);
hipError_t launch_env_rollout_generic(const sl_env_batch &env, const int32_t *actions, int T,
                                      float *reward_t, uint8_t *done_t, const Jump *jump,
                                      hipStream_t stream);
hipError_t launch_env_reset_generic(const sl_env_batch &env, const uint8_t *mask, hipStream_t stream);
// SimpleSideEffectPenalty's "inaction" baseline, one CA step on (all envs of `env`)
hipError_t launch_inaction_generic(const sl_env_batch &env, const Jump *jump, hipStream_t stream);
hipError_t launch_env_obs_generic(const sl_env_batch &env, hipStream_t stream);
// multi-agent boards (sl_multi_agent): the fused step / reset, one workgroup per board
// (x != null: with the wrappers, the finished-episode queue and the policy layout -- the _ex entry points)
hipError_t launch_env_step_multi(const sl_env_batch &env, const sl_multi_agent &m, const int32_t *actions, const Jump *jump,
                                 hipStream_t stream, const sl_multi_extras *x = nullptr);
hipError_t launch_env_reset_multi(const sl_env_batch &env, const sl_multi_agent &m, const uint8_t *mask, hipStream_t stream,
                                  const sl_multi_extras *x = nullptr);
// every pool level as the multi-agent reset leaves it -> baseline [L,H,W]
hipError_t launch_multi_baseline(const sl_env_batch &env, const sl_multi_agent &m, uint16_t *baseline, hipStream_t stream);
struct sl_channel_list {
    int32_t c[SL_MAX_CHANNELS];
};
hipError_t launch_obs_to_policy(const u32 *view, int B, int vh, int vw, const sl_channel_list &ch, int C, void *out,
                                int dtype, hipStream_t stream);

// sl_rowlane.hip : row-per-lane SWAR kernels for the shapes listed in SL_ROWLANE_SHAPES
bool rowlane_supports(int H, int W);
// size of sl_env_batch.goal_cache for a batch of B boards (0: no row kernels for the shape); zeroing it lowers every flag
// (spawn: the pool holds spawners -- which plain step kernel the batch runs, and whether that one keeps a cache)
size_t rowlane_goal_cache_bytes(int H, int W, int B, bool spawn, int *boards_per_block = nullptr);
bool rowlane_lean_takes_queue(int H, int W);       // the shape's plain step kernels also serve a finished-episode queue
int rowlane_policy_room(int H, int W);
hipError_t launch_build_score_lut(const int32_t *points_table, int n_tables, int8_t *lut, hipStream_t stream);
hipError_t launch_build_baseline(const sl_env_batch &env, hipStream_t stream);
hipError_t launch_idle(long long ticks, hipStream_t stream);
// n_each (device, optional): one step count per board instead of n_steps; n_valid (device, optional): only
// the first *n_valid boards exist
hipError_t launch_advance_rowlane(const u16 *in, u16 *out, int B, int H, int W, const float *spawn_prob,
                                  int n_steps, const int32_t *n_each, const int32_t *n_valid, sl_pcg64 *rng,
                                  const Jump *jump, hipStream_t stream);
// counts_stride: int32 elements between the outputs of consecutive boards (H*W*8 when dense).  n_valid / valid_period
// (device count, optional): boards come in runs of valid_period (0: one run) of which the first *n_valid exist.
// pre_steps (device, optional): per board, CA steps to run before counting starts.
hipError_t launch_occupancy_rowlane(const u16 *in, int32_t *counts, size_t counts_stride, int B, const int32_t *n_valid,
                                    int valid_period, const int32_t *pre_steps, int H, int W, const float *spawn_prob,
                                    int n_steps, sl_pcg64 *rng, const Jump *jump, hipStream_t stream);

// sl_side_effects.hip : the episode-end pass of side_effect_score for queued episodes
hipError_t launch_se_gather(const sl_env_batch &env, const sl_episode_queue &q, u16 *work_boards, float *spawn_prob,
                            int32_t *num_steps, sl_pcg64 *rng, bool two_runs, hipStream_t stream);
hipError_t launch_se_distributions(const sl_env_batch &env, const sl_episode_queue &q, const int32_t *counts,
                                   double denominator, uint16_t *keys, double *life_dist, uint8_t *type_masks,
                                   hipStream_t stream);
// sl_emd.hip : the earth-mover distances of every (entry, key) of the pass's outputs (workspace rule: see the file)
size_t emd_workspace_bytes(int H, int W, int concurrency);
hipError_t launch_emd(const sl_episode_queue &q, int H, int W, int num_samples, const int32_t *counts,
                      const uint16_t *keys, const uint8_t *type_masks, const double *ground, double penalty,
                      void *workspace, int concurrency, double *scores, int32_t *n_cells, hipStream_t stream);
// sl_render.hip : boards -> RGB frames (variant: 0 the default, 1 cells decoded by every lane, 2 cells staged in LDS)
hipError_t launch_render(const sl_render_args &args, int variant, hipStream_t stream);
// sl_rollout.hip : PPO's window -- the categorical draw (active null: every row), the per-step record, returns / GAE
// advantages (PPO.gen_training_batch; active null: the plain window), and the masked window's compaction and gather
hipError_t launch_sample_actions(const float *probs, const uint8_t *active, int B, int A, unsigned long long seed,
                                 unsigned long long counter, int32_t *actions, hipStream_t stream);
hipError_t launch_rollout_record(const sl_rollout &buf, int t, const int32_t *actions, const float *probs, int n_actions,
                                 const void *rewards, const float *values, const uint8_t *done, hipStream_t stream);
hipError_t launch_rollout_record_multi(const sl_rollout_multi &buf, int t, const int32_t *actions, const float *probs,
                                       int n_actions, const void *rewards, const float *values, const uint8_t *done,
                                       uint8_t *active_now, long long *num_resets, hipStream_t stream);
hipError_t launch_training_batch(const sl_rollout &buf, const uint8_t *active, const float *final_values, double gamma,
                                 double lmda, float *returns, float *advantages, uint8_t *traj_start, hipStream_t stream);
int rollout_compact_chunks(const sl_rollout_multi &buf);
hipError_t launch_rollout_compact(const sl_rollout_multi &buf, long long *rows_out, long long *count_out, int32_t *workspace,
                                  hipStream_t stream);
hipError_t launch_rollout_gather(const sl_rollout_multi &buf, const long long *rows, long long n, const float *returns,
                                 const float *advantages, const void *obs, long long obs_bytes, void *obs_out,
                                 long long *actions_out, float *action_prob_out, float *returns_out, float *advantages_out,
                                 float *values_out, hipStream_t stream);
// sl_replay.hip : DQN's n-step window and replay ring, its sampler and gather, the epsilon-greedy draw (active null: every
// column / row takes part)
hipError_t launch_replay_add(const sl_replay &buf, const void *obs, const int32_t *actions, const void *rewards,
                             const uint8_t *done, const void *next_obs, const uint8_t *active, hipStream_t stream);
hipError_t launch_replay_sample(const sl_replay &buf, int k, unsigned long long seed, unsigned long long counter,
                                long long *out_index, hipStream_t stream);
hipError_t launch_replay_gather(const sl_replay &buf, const long long *index, int k, void *obs_out, void *next_obs_out,
                                int obs_float32, long long *action_out, float *reward_out, float *done_out,
                                hipStream_t stream);
hipError_t launch_sample_actions_eps(const float *qvals, const uint8_t *active, int B, int A, double epsilon,
                                     unsigned long long seed, unsigned long long counter, int32_t *actions,
                                     hipStream_t stream);
// sl_schedule.hip : level schedules -- the successor table's draw (host_p: the G probabilities by value, else dev_p), the
// exit difficulty, the per-group performance rings and the curriculum's probabilities
struct schedule_probs {
    double p[SL_SCHEDULE_MAX_GROUPS];
};
hipError_t launch_schedule_draw(const sl_level_schedule &s, const schedule_probs *host_p, const double *dev_p,
                                unsigned long long seed, unsigned long long counter, int32_t *pool_next, int L,
                                hipStream_t stream);
hipError_t launch_schedule_required(const sl_level_schedule &s, double fraction, sl_level_scalars *pool_scalars, int L,
                                    hipStream_t stream);
hipError_t launch_schedule_harvest(const sl_level_schedule &s, const sl_step_out *out, const sl_env_scalars *scalars, int B,
                                   hipStream_t stream);
hipError_t launch_schedule_curriculum(const sl_level_schedule &s, double *probs_out, hipStream_t stream);
// the same for envs with m.n_agents agents: per-agent required points into m.pool_agents, one record per env whose agents
// are all done from m.out
hipError_t launch_schedule_required_multi(const sl_level_schedule_multi &m, double fraction, hipStream_t stream);
hipError_t launch_schedule_harvest_multi(const sl_level_schedule_multi &m, const sl_env_scalars *scalars, int B,
                                         hipStream_t stream);
// sl_episode_log.hip : the episode log -- a row per finished episode, the side-effect totals and the combined score joined
// in from a flushed queue, the running summaries and the run summary
hipError_t launch_episode_log_harvest(const sl_episode_log &log, const sl_step_out *out, const sl_env_scalars *scalars, int B,
                                      hipStream_t stream);
hipError_t launch_episode_log_join(const sl_episode_log &log, const sl_episode_queue &queue, const double *scores,
                                   const uint16_t *keys, const int32_t *n_cells, const sl_log_weights &weights,
                                   hipStream_t stream);
hipError_t launch_episode_log_summaries(const sl_episode_log &log, hipStream_t stream);
hipError_t launch_episode_log_run_summary(const sl_episode_log &log, long long first_row, double *out, hipStream_t stream);
// the same for envs with several agents: rows of a header and A agent records, a row when ALL agents of an env are done
hipError_t launch_episode_log_harvest_multi(const sl_episode_log_multi &log, const sl_step_out *out,
                                            const sl_agent_state *agents, const sl_env_scalars *scalars, int B,
                                            hipStream_t stream);
hipError_t launch_episode_log_join_multi(const sl_episode_log_multi &log, const sl_episode_queue &queue, const double *scores,
                                         const uint16_t *keys, const int32_t *n_cells, const sl_log_weights &weights,
                                         hipStream_t stream);
hipError_t launch_episode_log_summaries_multi(const sl_episode_log_multi &log, hipStream_t stream);
hipError_t launch_episode_log_run_summary_multi(const sl_episode_log_multi &log, long long first_row, double *out,
                                                hipStream_t stream);
// evaluation runs (sl_episode_run.hip): N tickets dealt statically, retired envs masked, tickets of queue entries
hipError_t launch_episode_run_start(const sl_episode_run &run, const sl_env_scalars *scalars, hipStream_t stream);
hipError_t launch_episode_run_harvest(const sl_episode_run &run, sl_step_out *out, int step, bool multi, hipStream_t stream);
hipError_t launch_episode_run_tickets(const sl_episode_run &run, const sl_episode_queue &queue, int32_t *tickets,
                                      const double *scores, const uint16_t *keys, const int32_t *n_cells,
                                      const sl_log_weights &weights, hipStream_t stream);
// episode histories (sl_history.hip): the board frames of selected episodes of the watched envs; two launches each
hipError_t launch_history_capture(const sl_episode_history &h, const uint16_t *board, const uint16_t *goals,
                                  const sl_env_scalars *scalars, const sl_step_out *out, const sl_episode_queue &queue,
                                  const uint8_t *active, hipStream_t stream);
hipError_t launch_history_capture_multi(const sl_episode_history &h, const uint16_t *board, const uint16_t *goals,
                                        const sl_env_scalars *scalars, const sl_step_out *out, int n_agents,
                                        const sl_episode_queue &queue, const uint8_t *active, hipStream_t stream);
hipError_t launch_history_rewind(const sl_episode_history &h, const uint16_t *goals, const sl_env_scalars *scalars,
                                 const uint8_t *mask, hipStream_t stream);
// the PPO update (sl_ppo.hip): the fused clipped loss and its gradients, a minibatch's observation rows, the deal's keys
size_t ppo_workspace_bytes(long long n);
hipError_t launch_ppo_loss_forward(const sl_ppo_loss &p, float *entropy_out, double *sums_out, void *workspace,
                                   hipStream_t stream);
hipError_t launch_ppo_loss_backward(const sl_ppo_loss &p, const float *grad_loss, const float *grad_entropy,
                                    const double *sums, float *d_values, float *d_policy, hipStream_t stream);
size_t ppo_report_workspace_bytes(long long N);
hipError_t launch_ppo_report_rows(const sl_ppo_loss &p, long long first_row, double *partial, hipStream_t stream);
hipError_t launch_ppo_report_finish(const sl_ppo_loss &p, const double *partial, long long blocks, double *out,
                                    hipStream_t stream);
hipError_t launch_minibatch_obs(const void *obs, long long obs_bytes, long long N, const long long *rows, long long n,
                                void *out, int out_float32, long long *status, hipStream_t stream);
hipError_t launch_minibatch_keys(long long N, unsigned long long seed, unsigned long long epoch, unsigned long long *keys,
                                 hipStream_t stream);
// the DQN update (sl_dqn.hip): the fused TD loss with the report scalars, and its gradient
size_t dqn_workspace_bytes(long long n);
hipError_t launch_dqn_loss_forward(const sl_dqn_loss &p, float *td_out, double *sums_out, void *workspace, hipStream_t stream);
hipError_t launch_dqn_loss_backward(const sl_dqn_loss &p, const float *grad_loss, const float *grad_td, const float *td,
                                    float *d_q, hipStream_t stream);
// the state digest (sl_digest.hip): a 64-bit integrity checksum per segment of a table of device memory segments
size_t digest_workspace_bytes(const unsigned long long *bytes, int n_segments);
void digest_prefix(const unsigned long long *bytes, int n_segments, unsigned long long *prefix_out);
hipError_t launch_state_digest(const sl_digest_segment *segments, int n_segments, unsigned long long salt,
                               unsigned long long *out, void *workspace, hipStream_t stream);
// batched pattern generation (sl_gen_pattern.hip): n Metropolis chains of one (rows, cols, depth), one wavefront each
size_t gen_pattern_workspace_bytes(int n, int rows, int cols, int depth);
hipError_t launch_gen_pattern(const uint16_t *layers, const int32_t *mask, const int32_t *seeds, const double *params,
                              unsigned long long *rng, uint16_t *out_board, int32_t *status, int32_t *iterations, int n,
                              int rows, int cols, int depth, void *workspace, hipStream_t stream);
// batched region partition (sl_partition.hip): n partitions of one (rows, cols) with room for `regions` regions, one wavefront each
size_t partition_workspace_bytes(int n, int rows, int cols, int regions);
hipError_t launch_partition(unsigned long long *rng, const int32_t *min_regions, const int32_t *max_regions, int16_t *labels,
                            int32_t *status, int n, int rows, int cols, int regions, void *workspace, hipStream_t stream);
// envs [e_first, e_first + e_count) of the batch; actions / reward_t / done_t are indexed [t * tstride + e]
// with the env's index in the whole batch
// (sl_aql.hip dispatches the same kernel from queues of the library's own: PreparedStep below)
struct AqlLaunch {
    int queue;              // index of the queue (one per slice)
    bool head;              // first step after work of HIP streams: system-scope acquire
    bool release_free;      // opt-in: no release fence behind this step (valid while workgroup i of the slice's queue keeps
                            // its XCD: the kernel checks itself against the placement found when the queues were opened)
};
// A single-step launch of the fused kernel that is not issued but handed back: kernel handle, geometry and the packed
// argument block with the offsets of the fields that change from step to step -- what the queues dispatch, any number
// of times, with those fields patched in.
struct PreparedStep {
    hipFunction_t f;
    unsigned grid, threads, lds;
    size_t arg_bytes;
    size_t off_actions, off_out, off_base, off_flag, off_trace, off_next;
    alignas(16) unsigned char args[1024];
};
// prepared (optional, T == 1 only): fill it instead of launching
// T == -1: SafeLifeEnv.reset() of the envs with reset_mask[e] != 0 (device uint8 [B] indexed by the env's index in the
// batch; null: all) instead of steps; `actions` is then only a readable dummy
hipError_t launch_env_rollout_rowlane(const sl_env_batch &env, int e_first, int e_count, const int32_t *actions,
                                      int T, int tstride, float *reward_t, uint8_t *done_t, const Jump *jump,
                                      hipStream_t stream, PreparedStep *prepared = nullptr,
                                      const uint8_t *reset_mask = nullptr);

// sl_aql.hip : user-mode queues of the library's own next to HIP's streams
const char *aql_open(int n_queues);                 // null when usable, else why not
const char *aql_probe(hipFunction_t f);             // can HIP's kernel `f` be found in the HSA executables? (null: yes)
hipFunction_t rowlane_probe_function();             // any kernel of the library (sl_rowlane.hip)
// can `f`, with an argument block of `arg_bytes`, be dispatched from the library's queues?  (null: yes; else why not --
// a kernel that spills keeps private memory, which these packets do not set up)
const char *aql_dispatchable(hipFunction_t f, size_t arg_bytes);
// patch (optional): the argument block is `version` of `owner`'s (any non-zero ids the caller keeps unique); where the
// queue's next argument slot already holds exactly that, only the 8-byte words at `offset[0..n)` are written again
struct AqlPatch {
    uint32_t owner, version;
    int n;
    size_t offset[4];
};
hipError_t aql_dispatch(const AqlLaunch &a, hipFunction_t f, unsigned grid, unsigned threads, unsigned lds,
                        const void *args, size_t arg_bytes, const AqlPatch *patch = nullptr);
// write `owner`'s argument block into every idle slot of the queue's argument ring (dispatches then only patch)
void aql_warm(int queue, hipFunction_t f, const void *args, size_t arg_bytes, const AqlPatch &patch);
void aql_begin();                                   // dispatches between begin and commit go out in batches: their
void aql_flush();                                   // argument blocks are flushed once per batch (flush: hand over what
void aql_commit();                                  // has been written so far; commit: flush and leave batch mode)
// marker: a barrier packet with a system-scope release and a completion signal behind everything dispatched so far on
// queues [0, n_queues) that have work since their last marker (force: on every one of them); returns at once.
// *ticket = -1 when there was nothing to mark.  wait: the calling thread spins on the marker's signals (any thread; the
// queues stay usable meanwhile).  fence = marker + wait.
hipError_t aql_marker(int n_queues, bool force, long long *ticket);
hipError_t aql_wait(long long ticket);
hipError_t aql_fence(int n_queues);
hipError_t aql_drain(int n_queues);                // (self-test) every queue idle, no cache action
void aql_timeline_mark(const char *what);           // SL_AQL_TIMELINE=1 (debugging): a host-side mark ...
void aql_timeline_dump();                           // ... and the timeline since the last dump, on stderr
bool aql_poisoned();                                // a wait timed out: work may still be in flight

}  // namespace sl
