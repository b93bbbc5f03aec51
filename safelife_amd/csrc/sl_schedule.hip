// sl_schedule.hip -- level schedules on the device: which pool slot an env loads next, what its exit asks for, and the
// per-family performance records a curriculum is steered by (training/env_factory.py: SwitchingLevelIterator :155-174,
// CurricularLevelIterator :51-146, MinPerformanceScheduler's LinearSchedule :363-373).
//
// The step kernels read a successor table at launch time (sl_env_batch.pool_next) and take an env's required points from
// pool_scalars[l].required_step when it reloads.  Nothing in them changes: the kernels here REWRITE those two inputs
// between steps.  The pool is a large pre-generated library cut into G <= 8 groups (level families: contiguous, disjoint
// slot ranges), and per step
//
//   k_schedule_draw        one lane per slot: pool_next[s] = a member of a group, both drawn from splitmix64 words of
//                          (seed, counter, s) -- the exact model is in include/safelife_hip.h and tests/schedule_ref.py
//   k_schedule_required    one lane per slot: required_step = ceil((min_performance * fraction) * available), the two
//                          float64 products rounded one after the other (launched only when the fraction moved)
//   k_schedule_harvest     after the step: every finished episode's performance goes into its group's ring, in ascending
//                          env order, and every env's current slot is noted for the next call
//   k_schedule_curriculum  the softmax over the rings' least-squares slopes (get_next_parameters) -> G probabilities
//
// Envs with A agents (sl_level_schedule_multi) share the draw and the curriculum and have their own two:
//
//   k_schedule_required_multi  one lane per (slot, agent): pool_agents[l][a].required_step from the agent's own available
//                              points
//   k_schedule_harvest_multi   the harvest below with "done" read as ALL A agents of the env done (the step on which the env
//                              reloads) and the performance the average of the A agents' quotients, summed as np.average
//                              sums them (env_factory.py:91-101)
//
// Nothing is fused (the library is built with -ffp-contract=off; the pragma says it again), so everything but exp() is the
// arithmetic the host model spells out, bit for bit.
//
// The harvest is one launch.  Workgroup 0 owns the rings: per tile of 16384 envs it stages the done flags in LDS (coalesced,
// independent loads), lane t takes the 64 consecutive envs [64 t, 64 t + 64) of the tile as a bit mask, counts its finished
// episodes per group, one workgroup scan per group turns the counts into places -- a record's place is a function of the
// done flags alone -- and the lane walks its finished envs again and writes.  It also moves cur_slot of the envs that
// finished.  Workgroups 1 .. move cur_slot of the envs that did NOT finish, 256 each: the two sets are told apart by
// out[e].done, which nobody writes, so no workgroup reads what another one writes.  Finished episodes are few (about 8
// of 8192 per step), so workgroup 0's time is its staging loads and 2 * G barriers.  (A first version gave every lane
// ceil(B / 256) consecutive envs to read straight from global memory: 32 dependent round trips per lane at 8192 envs,
// 21 us per call.)  The multi-agent harvest is the same code: the staged byte is the AND of the env's A done flags (A
// independent loads per lane, 16 A bytes per env), and workgroups 1 .. decide "did not finish" by the same AND of `out`.
#include "sl_kernels.h"

#pragma clang fp contract(off)

namespace sl {
namespace {

constexpr int SCHED_THREADS = 256;
constexpr int MAXG = SL_SCHEDULE_MAX_GROUPS;
constexpr int HARVEST_PER_LANE = 64;                            // envs a lane of the harvest's workgroup 0 places per tile
constexpr int HARVEST_TILE = SCHED_THREADS * HARVEST_PER_LANE;

// the group slot s belongs to, -1: none
__device__ __forceinline__ int group_of(const sl_level_schedule &s, int slot) {
    int g = -1;
#pragma unroll
    for (int j = 0; j < MAXG; ++j)
        if (j < s.G && slot >= s.start[j] && slot - s.start[j] < s.len[j]) g = j;
    return g;
}

__global__ __launch_bounds__(SCHED_THREADS) void k_schedule_draw(sl_level_schedule s, schedule_probs host_p,
                                                                 const double *__restrict__ dev_p, unsigned long long seed,
                                                                 unsigned long long counter, int32_t *__restrict__ pool_next,
                                                                 int L) {
    const int slot = blockIdx.x * SCHED_THREADS + threadIdx.x;
    if (slot >= L) return;
    double p[MAXG];
    if (dev_p) {            // the curriculum's output: nothing is sampled from garbage
        bool bad = false;
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < MAXG; ++j) {
            p[j] = j < s.G ? dev_p[j] : 0.0;
            bad |= !(p[j] >= 0.0) || p[j] == __builtin_inf();
            sum += p[j];
        }
        if (bad || !(sum > 0.0) || sum == __builtin_inf()) {
#pragma unroll
            for (int j = 0; j < MAXG; ++j) p[j] = j < s.G ? 1.0 : 0.0;
            if (slot == 0) atomicOr(s.status, (int32_t)SL_SCHEDULE_BAD_PROBS);
        }
    } else {
#pragma unroll
        for (int j = 0; j < MAXG; ++j) p[j] = j < s.G ? host_p.p[j] : 0.0;
    }
    double total = 0.0;
#pragma unroll
    for (int j = 0; j < MAXG; ++j) total += p[j];       // (entries past G are 0.0: the sum is cum[G-1])
    const u64 z1 = draw_hash(seed, counter, 2ull * (u64)slot);
    const u64 z2 = draw_hash(seed, counter, 2ull * (u64)slot + 1ull);
    const double t = ((double)(z1 >> 11) * (1.0 / 9007199254740992.0)) * total;
    int g = -1, last = 0;
    double cum = 0.0;
#pragma unroll
    for (int j = 0; j < MAXG; ++j) {
        cum += p[j];
        if (p[j] > 0.0) last = j;
        if (g < 0 && cum > t) g = j;
    }
    if (g < 0) g = last;
    int start = 0, len = 1;
#pragma unroll
    for (int j = 0; j < MAXG; ++j)
        if (j == g) start = s.start[j], len = s.len[j];
    pool_next[slot] = start + (int)__umul64hi(z2, (u64)len);
}

__global__ __launch_bounds__(SCHED_THREADS) void k_schedule_required(const double *__restrict__ min_performance,
                                                                     const int32_t *__restrict__ available, double fraction,
                                                                     sl_level_scalars *__restrict__ pool_scalars, int L) {
    const int l = blockIdx.x * SCHED_THREADS + threadIdx.x;
    if (l >= L) return;
    const double c = ceil(__dmul_rn(__dmul_rn(min_performance[l], fraction), (double)available[l]));
    int32_t r = 0;                                      // NaN and everything <= 0
    if (c >= 2147483647.0)
        r = 2147483647;
    else if (c > 0.0)
        r = (int32_t)c;
    pool_scalars[l].required_step = r;
}

__global__ __launch_bounds__(SCHED_THREADS) void k_schedule_required_multi(const double *__restrict__ min_performance,
                                                                           const int32_t *__restrict__ available,
                                                                           double fraction,
                                                                           sl_level_agent *__restrict__ pool_agents, int A,
                                                                           int n) {
    const int i = blockIdx.x * SCHED_THREADS + threadIdx.x;     // slot i / A, agent i % A
    if (i >= n) return;
    const double c = ceil(__dmul_rn(__dmul_rn(min_performance[i / A], fraction), (double)available[i]));
    int32_t r = 0;                                      // NaN and everything <= 0
    if (c >= 2147483647.0)
        r = 2147483647;
    else if (c > 0.0)
        r = (int32_t)c;
    pool_agents[i].required_step = r;
}

// the ring's records, oldest first, into LDS: n = min(count, lookback) of them
__device__ __forceinline__ int ring_to_lds(const sl_level_schedule &s, int g, long long count, int pos, double *lds) {
    const int n = count < s.lookback ? (int)max(count, 0ll) : s.lookback;
    const int oldest = count < s.lookback ? 0 : pos_mod(pos, s.lookback);  // (a caller's pos is not trusted with an index)
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        int k = oldest + i;
        if (k >= s.lookback) k -= s.lookback;
        lds[i] = s.ring[(long long)g * s.lookback + k];
    }
    return n;
}

// sum of lds[0 .. m) -- of w(i) * lds[i] -- in index order: the loads (and products) of eight elements go ahead of their
// adds, which stay one dependent chain (one thread walks up to 1024 elements: LDS latency paid per batch, not per element)
template <typename W>
__device__ __forceinline__ double sum_in_order(const double *lds, int m, W w) {
    double sum = 0.0;
    int i = 0;
    for (; i + 8 <= m; i += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = w(i + j) * lds[i + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += v[j];
    }
    for (; i < m; ++i) sum += w(i) * lds[i];
    return sum;
}

// np.average(reward / reward_possible) over the env's A agents (env_factory.py:95): float64 quotients, np.add.reduce -- the
// identity 0.0 plus the sum in index order for fewer than 8 elements, plus numpy's eight-accumulator tree for exactly 8 --
// divided by A once
__device__ __forceinline__ double performance_multi(const sl_step_out *__restrict__ rec, const int32_t *__restrict__ possible,
                                                    int A) {
    double q[SL_MAX_AGENTS];
#pragma unroll
    for (int a = 0; a < SL_MAX_AGENTS; ++a) q[a] = a < A ? (double)rec[a].episode_reward / (double)possible[a] : 0.0;
    double sum;
    if (A == SL_MAX_AGENTS) {
        sum = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    } else {
        sum = q[0];
#pragma unroll
        for (int a = 1; a < SL_MAX_AGENTS - 1; ++a)
            if (a < A) sum += q[a];
    }
    return (0.0 + sum) / (double)A;                     // (0.0 + -0.0 is +0.0, as numpy's is)
}

// MULTI: out is [B, A] and reward_possible [L, A]; else A is 1
template <bool MULTI>
__device__ __forceinline__ void harvest(const sl_level_schedule &s, const int32_t *__restrict__ reward_possible,
                                        const sl_step_out *__restrict__ out, const sl_env_scalars *__restrict__ scalars,
                                        int B, int A) {
    if (blockIdx.x > 0) {       // the envs that go on
        const int e = (blockIdx.x - 1) * SCHED_THREADS + threadIdx.x;
        if (e < B && !env_done<MULTI>(out, e, A)) s.cur_slot[e] = scalars[e].level_idx;
        return;
    }
    __shared__ int wave_sum[SCHED_THREADS / 64];
    __shared__ double lds[SL_SCHEDULE_MAX_LOOKBACK];
    __shared__ uint32_t flags[HARVEST_TILE / 4];        // one byte per env of the tile: 0 / 1
    uint8_t *flag = (uint8_t *)flags;
    int total[MAXG], pos0[MAXG];                        // records placed so far (uniform); the rings' positions at entry
#pragma unroll
    for (int j = 0; j < MAXG; ++j) total[j] = 0, pos0[j] = j < s.G ? pos_mod(s.pos[j], s.lookback) : 0;
    // Tiles of 64 envs per lane.  The done flags come in coalesced (lane t reads env tile + i * 256 + t: independent
    // loads, eight in flight) and go through LDS, from where lane t takes the 64 CONSECUTIVE envs it places.
    for (int tile = 0; tile < B; tile += HARVEST_TILE) {
        const int nt = min(HARVEST_TILE, B - tile);
        __syncthreads();                                // (the previous tile's flags have been read)
#pragma unroll 8
        for (int i = threadIdx.x; i < nt; i += SCHED_THREADS) flag[i] = env_done<MULTI>(out, tile + i, A) ? 1 : 0;
        for (int i = nt + threadIdx.x; i < ((nt + 63) & ~63); i += SCHED_THREADS) flag[i] = 0;
        __syncthreads();
        const int lo = threadIdx.x * HARVEST_PER_LANE;
        unsigned long long mask = 0;                    // bit i: env tile + lo + i is done
        if (lo < nt) { SL_FLAG_BYTES_TO_MASK(mask, flags, lo, HARVEST_PER_LANE); }
        int cnt[MAXG], n_tile[MAXG];
#pragma unroll
        for (int j = 0; j < MAXG; ++j) cnt[j] = 0;
        for (unsigned long long m = mask; m; m &= m - 1) {
            const int g = group_of(s, s.cur_slot[tile + lo + __ffsll((long long)m) - 1]);
#pragma unroll
            for (int j = 0; j < MAXG; ++j) cnt[j] += g == j;
        }
#pragma unroll
        for (int j = 0; j < MAXG; ++j) {
            n_tile[j] = 0;
            if (j < s.G) cnt[j] = block_exclusive_scan<SCHED_THREADS>(cnt[j], wave_sum, n_tile[j]);   // -> my first place
        }
        for (unsigned long long m = mask; m; m &= m - 1) {
            const int e = tile + lo + __ffsll((long long)m) - 1;
            const int slot = s.cur_slot[e];
            const int g = group_of(s, slot);
            s.cur_slot[e] = scalars[e].level_idx;
            if (g < 0) continue;                        // a slot outside every group: no record
            double perf;
            if (MULTI)
                perf = performance_multi(out + (long long)e * A, reward_possible + (long long)slot * A, A);
            else
                perf = (double)out[e].episode_reward / (double)reward_possible[slot];
            if (!(perf - perf == 0.0)) perf = 0.0;      // NaN, +-inf
            int r = 0, n = 0, at = 0;
#pragma unroll
            for (int j = 0; j < MAXG; ++j)
                if (j == g) r = cnt[j]++, n = n_tile[j], at = pos0[j] + (total[j] + r) % s.lookback;
            // of more than `lookback` records of a tile the last ones stay; a later tile's records go over an earlier
            // tile's in program order (the barriers above)
            if (r >= n - s.lookback) s.ring[(long long)g * s.lookback + at % s.lookback] = perf;
            if (perf > 0.0) atomicMax((long long *)&s.best[g], __double_as_longlong(perf));   // best >= 0: ordered as int64
        }
#pragma unroll
        for (int j = 0; j < MAXG; ++j) total[j] += n_tile[j];
    }
    __syncthreads();
    // counters, and the ring's mean (summed oldest first)
    for (int g = 0; g < s.G; ++g) {
        int n = 0;
#pragma unroll
        for (int j = 0; j < MAXG; ++j)
            if (j == g) n = total[j];
        if (n == 0) continue;                           // (uniform: every lane holds the same totals)
        const long long count = s.count[g] + n;
        int pos = 0;
#pragma unroll
        for (int j = 0; j < MAXG; ++j)
            if (j == g) pos = (int)((pos0[j] + (long long)n) % s.lookback);
        __syncthreads();                                // (everybody has read count[g]; lds is free again)
        const int m = ring_to_lds(s, g, count, pos, lds);
        __syncthreads();
        if (threadIdx.x == 0) {
            s.mean[g] = sum_in_order(lds, m, [](int) { return 1.0; }) / (double)m;
            s.count[g] = count;
            s.episodes[g] += n;
            s.pos[g] = pos;
        }
    }
}

__global__ __launch_bounds__(SCHED_THREADS) void k_schedule_harvest(sl_level_schedule s, const sl_step_out *__restrict__ out,
                                                                    const sl_env_scalars *__restrict__ scalars, int B) {
    harvest<false>(s, s.reward_possible, out, scalars, B, 1);
}

__global__ __launch_bounds__(SCHED_THREADS) void k_schedule_harvest_multi(sl_level_schedule s,
                                                                          const int32_t *__restrict__ reward_possible,
                                                                          const sl_step_out *__restrict__ out,
                                                                          const sl_env_scalars *__restrict__ scalars, int B,
                                                                          int A) {
    harvest<true>(s, reward_possible, out, scalars, B, A);
}

// get_next_parameters (env_factory.py:111-127) in float64, one workgroup:
//   tp[g] = 0.2 / lookback while the group holds fewer than `lookback` records, else 10 * m with m the least-squares slope
//   of the ring's records y_0 (oldest) .. y_{n-1} against 0 .. n-1 in closed form: xbar = (n - 1) / 2, sxx = n (n^2 - 1) / 12,
//   sxy = sum_i (i - xbar) * y_i (in index order), m = sxy / sxx;
//   scale = min |tp|; tp = tp < 0 ? 0 : tp; tp /= scale; NaN / inf -> 0; p = exp(tp - max tp) / their sum (index order).
__global__ __launch_bounds__(SCHED_THREADS) void k_schedule_curriculum(sl_level_schedule s, double *__restrict__ probs_out) {
    __shared__ double lds[SL_SCHEDULE_MAX_LOOKBACK];
    __shared__ double tp[MAXG];
    const double n = (double)s.lookback;
    for (int g = 0; g < s.G; ++g) {
        const long long count = s.count[g];
        if (count < s.lookback) {
            if (threadIdx.x == 0) tp[g] = 0.2 / n;
            continue;
        }
        __syncthreads();
        ring_to_lds(s, g, count, s.pos[g], lds);
        __syncthreads();
        if (threadIdx.x == 0) {
            const double xbar = (n - 1.0) / 2.0, sxx = n * (n * n - 1.0) / 12.0;
            const double sxy = sum_in_order(lds, s.lookback, [xbar](int i) { return (double)i - xbar; });
            tp[g] = 10.0 * (sxy / sxx);
        }
    }
    if (threadIdx.x != 0) return;
    double scale = fabs(tp[0]);
    for (int g = 1; g < s.G; ++g) {
        const double a = fabs(tp[g]);
        if (a < scale || a != a) scale = a;             // (np.min: a NaN wins)
    }
    double mx = 0.0;
    for (int g = 0; g < s.G; ++g) {
        double v = tp[g] < 0.0 ? 0.0 : tp[g];
        v = v / scale;
        if (!(v - v == 0.0)) v = 0.0;
        tp[g] = v;
        if (g == 0 || v > mx) mx = v;
    }
    double sum = 0.0;
    for (int g = 0; g < s.G; ++g) {
        tp[g] = exp(tp[g] - mx);
        sum += tp[g];
    }
    for (int g = 0; g < s.G; ++g) probs_out[g] = tp[g] / sum;
}

}  // namespace

hipError_t launch_schedule_draw(const sl_level_schedule &s, const schedule_probs *host_p, const double *dev_p,
                                unsigned long long seed, unsigned long long counter, int32_t *pool_next, int L,
                                hipStream_t stream) {
    schedule_probs hp = {};
    if (host_p) hp = *host_p;
    hipLaunchKernelGGL(k_schedule_draw, dim3((L + SCHED_THREADS - 1) / SCHED_THREADS), dim3(SCHED_THREADS), 0, stream, s, hp,
                       host_p ? nullptr : dev_p, seed, counter, pool_next, L);
    return hipGetLastError();
}

hipError_t launch_schedule_required(const sl_level_schedule &s, double fraction, sl_level_scalars *pool_scalars, int L,
                                    hipStream_t stream) {
    hipLaunchKernelGGL(k_schedule_required, dim3((L + SCHED_THREADS - 1) / SCHED_THREADS), dim3(SCHED_THREADS), 0, stream,
                       s.min_performance, s.available, fraction, pool_scalars, L);
    return hipGetLastError();
}

hipError_t launch_schedule_harvest(const sl_level_schedule &s, const sl_step_out *out, const sl_env_scalars *scalars, int B,
                                   hipStream_t stream) {
    hipLaunchKernelGGL(k_schedule_harvest, dim3(1 + (B + SCHED_THREADS - 1) / SCHED_THREADS), dim3(SCHED_THREADS), 0, stream,
                       s, out, scalars, B);
    return hipGetLastError();
}

hipError_t launch_schedule_required_multi(const sl_level_schedule_multi &m, double fraction, hipStream_t stream) {
    const int n = m.s.L * m.n_agents;
    hipLaunchKernelGGL(k_schedule_required_multi, dim3((n + SCHED_THREADS - 1) / SCHED_THREADS), dim3(SCHED_THREADS), 0, stream,
                       m.s.min_performance, m.available, fraction, m.pool_agents, m.n_agents, n);
    return hipGetLastError();
}

hipError_t launch_schedule_harvest_multi(const sl_level_schedule_multi &m, const sl_env_scalars *scalars, int B,
                                         hipStream_t stream) {
    hipLaunchKernelGGL(k_schedule_harvest_multi, dim3(1 + (B + SCHED_THREADS - 1) / SCHED_THREADS), dim3(SCHED_THREADS), 0,
                       stream, m.s, m.reward_possible, m.out, scalars, B, m.n_agents);
    return hipGetLastError();
}

hipError_t launch_schedule_curriculum(const sl_level_schedule &s, double *probs_out, hipStream_t stream) {
    hipLaunchKernelGGL(k_schedule_curriculum, dim3(1), dim3(SCHED_THREADS), 0, stream, s, probs_out);
    return hipGetLastError();
}

}  // namespace sl
