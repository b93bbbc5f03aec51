// sl_episode_run.hip -- evaluation runs on the device: exactly N episodes, then the envs retire (what the reference's
// trainers do with run_episodes(envs, num_episodes), training/base_algo.py:278-318).  The model -- ticket t -> slot t % L,
// env t % G, that env's (t / G)-th episode of the run -- is spelled out in include/safelife_hip.h next to the entry points
// and restated in tests/episode_run_ref.py.  No step kernel changes: these kernels run on the caller's stream around the
// fused step.
//
//   k_episode_run_start      after the reset that dealt the first tickets: episode counters noted, active mask, counters, and
//                            the result table zeroed
//   k_episode_run_harvest    behind every step: one thread per env, grid-stride.  A retired env's record(s) are zeroed; an
//                            active env whose episode ended files its ticket and retires when it has none left.  Every env
//                            touches only its own active / played entry and its own tickets' rows, so no thread reads what
//                            another writes; the three counters are reduced per wave (ballot + popcount) and take one
//                            integer atomicAdd per wave and counter that moved -- integer sums are order-free.
//   k_episode_run_tickets    one lane per queue entry: its ticket, or -1 for a phantom episode or one from before the run;
//                            with the EMD scores, the entry's weighted totals into the ticket's row
#include "sl_kernels.h"

#pragma clang fp contract(off)

namespace sl {
namespace {

constexpr int RUN_THREADS = 256;
constexpr int RUN_MAX_BLOCKS = 1024;
constexpr int K = SL_SE_MAX_KEYS;

__global__ __launch_bounds__(RUN_THREADS) void k_episode_run_start(sl_episode_run run, const sl_env_scalars *__restrict__ scalars) {
    const int stride = gridDim.x * RUN_THREADS;
    const int first = blockIdx.x * RUN_THREADS + threadIdx.x;
    for (int e = first; e < run.B; e += stride) {
        run.base_episode[e] = scalars[e].episode_idx;
        run.played[e] = 0;
        run.active[e] = run.env_offset + e < run.N ? 1 : 0;
    }
    const int A = run.n_agents;
    for (int t = first; t < run.N; t += stride) {
        sl_episode_run_row row;
        row.slot = row.env = row.episode_idx = row.step = row.length = 0;
        row.reward = 0.0f;
        row.success = row.times_up = row.flags = row.reserved = 0;
        row.reserved2 = 0;
        run.results[t] = row;
        run.side_effects[2 * (long long)t] = run.side_effects[2 * (long long)t + 1] = 0.0;
        for (int a = 0; a < A; ++a) {
            sl_episode_run_agent ag;
            ag.length = 0, ag.reward = 0.0f, ag.success = ag.times_up = ag.reserved[0] = ag.reserved[1] = 0, ag.reserved2 = 0;
            run.agent_results[(long long)t * A + a] = ag;
        }
    }
    if (first == 0) {
        run.counters[0] = 0;
        run.counters[1] = max(0, min(run.B, run.N - run.env_offset));   // envs with g = env_offset + e < N
        run.counters[2] = 0;
        run.counters[3] = 0;
    }
}

__device__ __forceinline__ sl_step_out zero_record() {
    sl_step_out z;
    z.reward = 0.0f, z.done = z.success = z.times_up = z.reserved = 0, z.episode_reward = 0.0f, z.episode_length = 0;
    return z;
}

__device__ __forceinline__ sl_episode_run_agent agent_of(const sl_step_out &o) {
    sl_episode_run_agent ag;
    ag.length = o.episode_length, ag.reward = o.episode_reward, ag.success = o.success, ag.times_up = o.times_up;
    ag.reserved[0] = ag.reserved[1] = 0, ag.reserved2 = 0;
    return ag;
}

// one integer atomicAdd per wave and counter that moved (every lane of the wave calls this)
__device__ __forceinline__ void wave_count(int32_t *counter, bool mine, int sign) {
    const int n = __popcll(__ballot(mine));
    if (n && (threadIdx.x & 63) == 0) atomicAdd(counter, sign * n);
}

// A: agents per env (the single-agent variant is A = 1 over sl_step_out [B])
template <bool MULTI>
__global__ __launch_bounds__(RUN_THREADS) void k_episode_run_harvest(sl_episode_run run, sl_step_out *__restrict__ out, int step) {
    const int A = MULTI ? run.n_agents : 1;
    const int stride = gridDim.x * RUN_THREADS;
    // (the loop's bounds are uniform over the workgroup: every lane of a wave reaches the ballots)
    for (int base = blockIdx.x * RUN_THREADS; base < run.B; base += stride) {
        const int e = base + threadIdx.x;
        const bool in = e < run.B;
        bool stepped = false, ended = false, retired = false;
        if (in) {
            sl_step_out *rec = out + (long long)e * A;
            if (!run.active[e]) {
                for (int a = 0; a < A; ++a) rec[a] = zero_record();
            } else {
                stepped = true;
                ended = true;
                for (int a = 0; a < A; ++a) ended = ended && rec[a].done != 0;
                if (ended) {
                    const int g = run.env_offset + e, k = run.played[e];
                    const long long t = g + (long long)run.G * k;
                    if (t >= 0 && t < run.N) {      // (an active env's next ticket is below N: kept as a bound all the same)
                        const sl_step_out o = rec[0];
                        sl_episode_run_row row;
                        row.slot = (int32_t)(t % run.L);
                        row.env = g;
                        row.episode_idx = run.base_episode[e] + k;
                        row.step = step;
                        row.length = o.episode_length;
                        row.reward = o.episode_reward;
                        row.success = o.success, row.times_up = o.times_up, row.flags = SL_RUN_WRITTEN, row.reserved = 0;
                        row.reserved2 = 0;
                        run.results[t] = row;
                        for (int a = 0; a < A; ++a) run.agent_results[t * run.n_agents + a] = agent_of(rec[a]);
                    } else {
                        ended = false;
                    }
                    run.played[e] = k + 1;
                    if (g + (long long)run.G * (k + 1) >= run.N) {
                        run.active[e] = 0;
                        retired = true;
                    }
                }
            }
        }
        wave_count(run.counters + 0, ended, 1);
        wave_count(run.counters + 1, retired, -1);
        wave_count(run.counters + 2, stepped, 1);
    }
}

__global__ __launch_bounds__(RUN_THREADS) void k_episode_run_tickets(sl_episode_run run, sl_episode_queue queue,
                                                                     int32_t *__restrict__ tickets,
                                                                     const double *__restrict__ scores,
                                                                     const uint16_t *__restrict__ keys,
                                                                     const int32_t *__restrict__ n_cells, sl_log_weights w) {
    const int i = blockIdx.x * RUN_THREADS + threadIdx.x;
    if (i >= queue.capacity) return;
    const int n = min(max(*queue.count, 0), queue.capacity);
    if (i >= n) {
        tickets[i] = -1;
        return;
    }
    const sl_episode_record rec = queue.records[i];
    const int e = rec.env - queue.env_base;
    long long t = -1;
    if (e >= 0 && e < run.B) {
        const long long k = (long long)rec.episode_idx - run.base_episode[e];
        if (k >= 0) {
            t = (run.env_offset + e) + (long long)run.G * k;
            if (t >= run.N) t = -1;
        }
    }
    tickets[i] = (int32_t)t;
    if (t < 0 || !scores) return;
    // the entry's weighted totals: slhip_episode_log_join's arithmetic (a product rounded before its add, key slots in
    // index order, an empty slot and a NaN score contribute nothing)
    double total[2] = {0.0, 0.0};
    if (n_cells[(long long)i * K] < 0) {
        total[0] = total[1] = __builtin_nan("");
    } else {
        for (int k = 0; k < K; ++k) {
            const uint16_t key = keys[(long long)i * K + k];
            if (key == 0xFFFF) continue;
            double wk = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j < w.n && w.cell[j] == key) wk += w.weight[j];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const double s = scores[((long long)i * K + k) * 2 + j];
                if (s == s) total[j] += wk * s;
            }
        }
    }
    run.side_effects[2 * t] = total[0];
    run.side_effects[2 * t + 1] = total[1];
    run.results[t].flags |= SL_RUN_SCORED;      // (a ticket has one queue entry: no other lane writes this row)
}

inline int run_blocks(int n) { return max(1, min(RUN_MAX_BLOCKS, (n + RUN_THREADS - 1) / RUN_THREADS)); }

}  // namespace

hipError_t launch_episode_run_start(const sl_episode_run &run, const sl_env_scalars *scalars, hipStream_t stream) {
    hipLaunchKernelGGL(k_episode_run_start, dim3(run_blocks(max(run.B, run.N))), dim3(RUN_THREADS), 0, stream, run, scalars);
    return hipGetLastError();
}

hipError_t launch_episode_run_harvest(const sl_episode_run &run, sl_step_out *out, int step, bool multi, hipStream_t stream) {
    if (multi)
        hipLaunchKernelGGL(k_episode_run_harvest<true>, dim3(run_blocks(run.B)), dim3(RUN_THREADS), 0, stream, run, out, step);
    else
        hipLaunchKernelGGL(k_episode_run_harvest<false>, dim3(run_blocks(run.B)), dim3(RUN_THREADS), 0, stream, run, out, step);
    return hipGetLastError();
}

hipError_t launch_episode_run_tickets(const sl_episode_run &run, const sl_episode_queue &queue, int32_t *tickets,
                                      const double *scores, const uint16_t *keys, const int32_t *n_cells,
                                      const sl_log_weights &weights, hipStream_t stream) {
    hipLaunchKernelGGL(k_episode_run_tickets, dim3((queue.capacity + RUN_THREADS - 1) / RUN_THREADS), dim3(RUN_THREADS), 0,
                       stream, run, queue, tickets, scores, keys, n_cells, weights);
    return hipGetLastError();
}

}  // namespace sl
