// sl_episode_log.hip -- the episode log on the device: the arithmetic of the reference's SafeLifeLogger
// (safelife_logger.py: log_episode :262-354 with combined_score :671-716, the running summaries of log_scalars :372-381,
// summarize_run_file :719-762).  The exact model of every kernel is in include/safelife_hip.h next to its entry point and
// restated in tests/episode_log_ref.py.
//
//   k_episode_log_harvest      after the step: a row per finished episode, in ascending env order, and every env's current
//                              slot / required points / episode counter noted for the next call
//   k_episode_log_join         after a flush of the finished-episode queue and the EMD batch: one lane per queue entry sums
//                              the weighted totals, finds the entry's row along the env's `prev` chain and fills in the
//                              side-effect fraction and the combined score
//   k_episode_log_summaries    the five running summaries over the rows not yet consumed, in row order
//   k_episode_log_run_summary  means and population standard deviations over a row range, two passes
//
// Nothing is fused (the library is built with -ffp-contract=off; the pragma says it again): every float64 operation is
// rounded on its own, which is what lets the host model agree bit for bit.
//
// The harvest has the structure of k_schedule_harvest (sl_schedule.hip): workgroup 0 stages the done flags of a tile of
// 16384 envs in LDS, lane t takes 64 consecutive envs as a bit mask, ONE workgroup scan turns the lanes' counts into places
// and the lane walks its finished envs again and writes their rows; workgroups 1 .. move cur_* of the envs that did not
// finish.  The two sets are told apart by out[e].done, which nobody writes, so no workgroup reads what another one writes.
//
// The two summary kernels are dependent chains (value = (v + w * value) / (1 + w) per row; one running sum per quantity).
// One lane per chain walks it out of LDS, eight values loaded ahead of their dependent operations as sum_in_order does;
// all 256 lanes stage the rows -- a 96-byte row per lane, consecutive lanes consecutive rows -- and fetch the next batch's
// rows into registers before the chain of the current batch starts, so global latency hides behind the chain.
#include "sl_kernels.h"

#pragma clang fp contract(off)

namespace sl {
namespace {

constexpr int LOG_THREADS = 256;
constexpr int HARVEST_PER_LANE = 64;                            // envs a lane of the harvest's workgroup 0 places per tile
constexpr int HARVEST_TILE = LOG_THREADS * HARVEST_PER_LANE;
constexpr int K = SL_SE_MAX_KEYS;

__device__ __forceinline__ double log_nan() { return __builtin_nan(""); }
__device__ __forceinline__ bool is_finite_f64(double v) { return v - v == 0.0; }

__device__ __forceinline__ void note_current(const sl_episode_log &log, const sl_env_scalars *__restrict__ scalars, int e) {
    log.cur_slot[e] = scalars[e].level_idx;
    log.cur_required[e] = scalars[e].required_points;
    log.cur_episode[e] = scalars[e].episode_idx;
}

// np.maximum(x, 1): a NaN stays
__device__ __forceinline__ double at_least_one(double x) { return x != x ? x : (x > 1.0 ? x : 1.0); }

// combined_score() from the two totals: the fraction and the score
__device__ __forceinline__ void combined(double agent, double inaction, double reward_frac, int length, double &frac,
                                         double &score) {
    frac = agent / at_least_one(inaction);
    const double speed = 1.0 - (double)length / 1000.0;
    score = (75.0 * reward_frac + 25.0 * speed) - 200.0 * frac;
}

__global__ __launch_bounds__(LOG_THREADS) void k_episode_log_harvest(sl_episode_log log, const sl_step_out *__restrict__ out,
                                                                     const sl_env_scalars *__restrict__ scalars, int B) {
    if (blockIdx.x > 0) {       // the envs that go on
        const int e = (blockIdx.x - 1) * LOG_THREADS + threadIdx.x;
        if (e < B && out[e].done == 0) note_current(log, scalars, e);
        return;
    }
    __shared__ int wave_sum[LOG_THREADS / 64];
    __shared__ uint32_t flags[HARVEST_TILE / 4];        // one byte per env of the tile: 0 / 1
    uint8_t *flag = (uint8_t *)flags;
    const long long n_rows = log.counters[0], steps = log.counters[1];   // (written below, behind the last barrier)
    int total = 0;                                      // rows placed so far (uniform)
    for (int tile = 0; tile < B; tile += HARVEST_TILE) {
        const int nt = min(HARVEST_TILE, B - tile);
        __syncthreads();                                // (the previous tile's flags have been read)
#pragma unroll 8
        for (int i = threadIdx.x; i < nt; i += LOG_THREADS) flag[i] = out[tile + i].done != 0 ? 1 : 0;
        for (int i = nt + threadIdx.x; i < ((nt + 63) & ~63); i += LOG_THREADS) flag[i] = 0;
        __syncthreads();
        const int lo = threadIdx.x * HARVEST_PER_LANE;
        unsigned long long mask = 0;                    // bit i: env tile + lo + i is done
        if (lo < nt) {
#pragma unroll
            for (int k = 0; k < HARVEST_PER_LANE / 4; ++k)      // bytes b0 b1 b2 b3 of a word -> bits 24..27 of the product
                mask |= (unsigned long long)((flags[lo / 4 + k] * 0x01020408u >> 24) & 0xFu) << (4 * k);
        }
        int n_tile = 0;
        int place = block_exclusive_scan<LOG_THREADS>(__popcll(mask), wave_sum, n_tile);      // -> my first place
        for (unsigned long long m = mask; m; m &= m - 1, ++place) {
            const int e = tile + lo + __ffsll((long long)m) - 1;
            const long long idx = n_rows + total + place;
            const sl_step_out o = out[e];
            const int slot = log.cur_slot[e];
            sl_episode_log_row row;
            row.index = idx;
            row.training_steps = steps + e + 1;
            row.prev = log.last_row[e];
            row.env = e;
            row.level = slot;
            row.episode_idx = log.cur_episode[e];
            row.length = o.episode_length;
            row.reward = o.episode_reward;
            row.reward_possible = slot >= 0 && slot < log.L ? log.reward_possible[slot] : 0;
            row.reward_needed = log.cur_required[e];
            row.success = o.success, row.times_up = o.times_up, row.flags = 0, row.reserved = 0;
            row.reward_frac = (double)o.episode_reward / (double)max(row.reward_possible, 1);
            row.side_effects[0] = row.side_effects[1] = row.side_effects_frac = row.score = log_nan();
            log.rows[idx % log.capacity] = row;         // (capacity >= B: the rows of one call never meet)
            log.last_row[e] = idx;
            note_current(log, scalars, e);
        }
        total += n_tile;
    }
    __syncthreads();                                    // (everybody has read the counters)
    if (threadIdx.x == 0) {
        log.counters[0] = n_rows + total;
        log.counters[1] = steps + B;
        log.counters[2] += total;
    }
}

__global__ __launch_bounds__(LOG_THREADS) void k_episode_log_join(sl_episode_log log, sl_episode_queue queue,
                                                                  const double *__restrict__ scores,
                                                                  const uint16_t *__restrict__ keys,
                                                                  const int32_t *__restrict__ n_cells, sl_log_weights w) {
    const int i = blockIdx.x * LOG_THREADS + threadIdx.x;
    const int n = min(max(*queue.count, 0), queue.capacity);
    if (i >= n) return;
    const sl_episode_record rec = queue.records[i];
    double total[2] = {0.0, 0.0};
    if (n_cells[(long long)i * K] < 0) {
        total[0] = total[1] = log_nan();
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
    // the entry's row: along the env's chain, newest first.  Every bound is a launch constant or a kernel argument.
    const long long n_rows = log.counters[0];
    long long r = rec.env >= 0 && rec.env < log.B ? log.last_row[rec.env] : -1;
    sl_episode_log_row *row = nullptr;
    for (int hop = 0; hop < SL_LOG_MAX_HOPS; ++hop) {
        if (r < 0 || r >= n_rows || r < n_rows - log.capacity) break;
        sl_episode_log_row *at = log.rows + r % log.capacity;
        if (at->index != r) break;
        if (at->env == rec.env && at->episode_idx == rec.episode_idx) {
            row = at;
            break;
        }
        r = at->prev;
    }
    if (!row) {
        atomicAdd((unsigned long long *)&log.counters[4], 1ull);
        return;
    }
    double frac, score;
    combined(total[0], total[1], row->reward_frac, row->length, frac, score);
    row->side_effects[0] = total[0];
    row->side_effects[1] = total[1];
    row->side_effects_frac = frac;
    row->score = score;
    row->flags |= SL_LOG_JOINED;
}

// Rows [first, last) in row order: load(row, v) turns a row into NK values, and lane k < NK calls step(v_k) for every row.
// `stage` holds NK * LOG_THREADS doubles.  Every lane of the workgroup calls it (barriers inside); first and last are
// uniform.
template <int NK, typename Load, typename Step>
__device__ __forceinline__ void walk_rows(const sl_episode_log &log, long long first, long long last, double *stage, Load load,
                                          Step step) {
    double next[NK];
    auto fetch = [&](long long base) {
        if (base + threadIdx.x < last) load(log.rows[(base + threadIdx.x) % log.capacity], next);
    };
    fetch(first);
    for (long long base = first; base < last; base += LOG_THREADS) {
        const int n = (int)min((long long)LOG_THREADS, last - base);
        __syncthreads();                                // (the previous batch's chain has read its values)
        if ((int)threadIdx.x < n) {
#pragma unroll
            for (int k = 0; k < NK; ++k) stage[k * LOG_THREADS + threadIdx.x] = next[k];
        }
        __syncthreads();
        fetch(base + LOG_THREADS);                      // (in flight while the chains below run)
        if (threadIdx.x < NK) {
            const double *s = stage + threadIdx.x * LOG_THREADS;
            int i = 0;
            for (; i + 8 <= n; i += 8) {
                double v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = s[i + j];
#pragma unroll
                for (int j = 0; j < 8; ++j) step(v[j]);
            }
            for (; i < n; ++i) step(s[i]);
        }
    }
}

__global__ __launch_bounds__(LOG_THREADS) void k_episode_log_summaries(sl_episode_log log) {
    __shared__ double stage[SL_LOG_KEYS * LOG_THREADS];
    const long long n_rows = log.counters[0];           // (summarised is written below, behind the walk's barriers)
    const long long first = max(max(log.counters[3], n_rows - log.capacity), 0ll);
    const int k = threadIdx.x < SL_LOG_KEYS ? threadIdx.x : 0;
    double value = log.value[k], w = log.weight[k];
    long long count = log.count[k];
    const double polyak = log.polyak;
    walk_rows<SL_LOG_KEYS>(
        log, first, n_rows, stage,
        [](const sl_episode_log_row &row, double *v) {
            v[0] = row.side_effects_frac;
            v[1] = (double)row.length;
            v[2] = row.reward_frac;
            v[3] = row.success ? 1.0 : 0.0;
            v[4] = row.score;
        },
        [&](double v) {
            if (!is_finite_f64(v)) return;
            value = (v + w * value) / (1.0 + w);
            count += 1;
            w = polyak < 1.0 ? polyak * (1.0 + w) : (double)count;
        });
    if (threadIdx.x < SL_LOG_KEYS) {
        log.value[k] = value;
        log.weight[k] = w;
        log.count[k] = count;
    }
    __syncthreads();
    if (threadIdx.x == 0) log.counters[3] = n_rows;
}

__device__ __forceinline__ double nan_to_num(double x) {
    if (x != x) return 0.0;
    if (x == __builtin_inf()) return 1.7976931348623157e308;
    if (x == -__builtin_inf()) return -1.7976931348623157e308;
    return x;
}

__global__ __launch_bounds__(LOG_THREADS) void k_episode_log_run_summary(sl_episode_log log, long long first_row,
                                                                         double *__restrict__ out) {
    constexpr int NK = 6;       // success, length, side_effects_frac, reward_frac, score, length of a successful row
    __shared__ double stage[NK * LOG_THREADS];
    const long long n_rows = log.counters[0];
    const long long first = min(max(max(first_row, n_rows - log.capacity), 0ll), n_rows);
    auto load = [](const sl_episode_log_row &row, double *v) {
        double frac, score;
        combined(nan_to_num(row.side_effects[0]), nan_to_num(row.side_effects[1]), row.reward_frac, row.length, frac, score);
        v[0] = row.success ? 1.0 : 0.0;
        v[1] = (double)row.length;
        v[2] = frac;
        v[3] = row.reward_frac;
        v[4] = score;
        v[5] = row.success ? (double)row.length : log_nan();       // (NaN: not a successful row)
    };
    const bool picky = threadIdx.x == NK - 1;           // the lane that skips the rows without success
    double sum = 0.0, sq = 0.0;
    long long n = 0;
    walk_rows<NK>(log, first, n_rows, stage, load, [&](double v) {
        if (picky && v != v) return;
        sum += v;
        n += 1;
    });
    const double mean = sum / (double)n;
    walk_rows<NK>(log, first, n_rows, stage, load, [&](double v) {
        if (picky && v != v) return;
        const double d = v - mean;
        sq += d * d;
    });
    const double sd = sqrt(sq / (double)n);
    switch (threadIdx.x) {
    case 0: out[0] = (double)n, out[1] = mean; break;
    case 1: out[2] = mean; break;
    case 2: out[3] = mean, out[6] = sd; break;
    case 3: out[4] = mean, out[7] = sd; break;
    case 4: out[5] = mean, out[8] = sd; break;
    case 5: out[9] = mean, out[10] = sd, out[11] = (double)n; break;
    default: break;
    }
}

}  // namespace

hipError_t launch_episode_log_harvest(const sl_episode_log &log, const sl_step_out *out, const sl_env_scalars *scalars, int B,
                                      hipStream_t stream) {
    hipLaunchKernelGGL(k_episode_log_harvest, dim3(1 + (B + LOG_THREADS - 1) / LOG_THREADS), dim3(LOG_THREADS), 0, stream, log,
                       out, scalars, B);
    return hipGetLastError();
}

hipError_t launch_episode_log_join(const sl_episode_log &log, const sl_episode_queue &queue, const double *scores,
                                   const uint16_t *keys, const int32_t *n_cells, const sl_log_weights &weights,
                                   hipStream_t stream) {
    hipLaunchKernelGGL(k_episode_log_join, dim3((queue.capacity + LOG_THREADS - 1) / LOG_THREADS), dim3(LOG_THREADS), 0,
                       stream, log, queue, scores, keys, n_cells, weights);
    return hipGetLastError();
}

hipError_t launch_episode_log_summaries(const sl_episode_log &log, hipStream_t stream) {
    hipLaunchKernelGGL(k_episode_log_summaries, dim3(1), dim3(LOG_THREADS), 0, stream, log);
    return hipGetLastError();
}

hipError_t launch_episode_log_run_summary(const sl_episode_log &log, long long first_row, double *out, hipStream_t stream) {
    hipLaunchKernelGGL(k_episode_log_run_summary, dim3(1), dim3(LOG_THREADS), 0, stream, log, first_row, out);
    return hipGetLastError();
}

}  // namespace sl
