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
//   k_episode_log_*_multi      the same four for envs with several agents: a row when ALL agents of an env are done, per-agent
//                              fields behind a common header, summaries per agent name (second half of this file)
//
// The single- and the multi-agent harvest are ONE body, harvest(): a kernel hands it a small policy struct that says what
// differs (how a tile's done flags are staged, how a row is written, what is noted of an env's current episode) and
// everything is inlined, as in k_schedule_harvest / _multi.  The two joins share the queue entry's totals (entry_totals), the
// walk along `prev` (find_row, which is told how a row index becomes a pointer) and the score (joined_score).  The four
// summary kernels stage different things and stay apart.
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

// np.maximum(x, 1): a NaN stays
__device__ __forceinline__ double at_least_one(double x) { return x != x ? x : (x > 1.0 ? x : 1.0); }

// combined_score()'s score from an episode's reward fraction and length and its side-effect fraction
__device__ __forceinline__ double agent_score(double reward_frac, int length, double frac) {
    const double speed = 1.0 - (double)length / 1000.0;
    return (75.0 * reward_frac + 25.0 * speed) - 200.0 * frac;
}

// combined_score() from the two totals: the fraction and the score
__device__ __forceinline__ void combined(double agent, double inaction, double reward_frac, int length, double &frac,
                                         double &score) {
    frac = agent / at_least_one(inaction);
    score = agent_score(reward_frac, length, frac);
}

// ---- the harvest under both kernels ------------------------------------------------------------------------------------------
//
// A policy P holds the kernel's arguments (log, out, A; MULTI says how env_done reads `out`) and says what differs:
//   stage(flag, tile, nt)      called by every lane of workgroup 0 between two barriers: flag[i] = has env tile + i finished
//                              for i < nt, 0 from nt up to the next multiple of 64
//   write_row(e, idx, steps)   row idx, that of env e's finished episode (its prev is last_row[e], which the body moves after)
//   note_current(e)            cur_* of env e from what the step left
template <typename P>
__device__ __forceinline__ void harvest(const P &p, int B) {
    const auto &log = p.log;
    if (blockIdx.x > 0) {       // the envs that go on
        const int e = (blockIdx.x - 1) * LOG_THREADS + threadIdx.x;
        if (e < B && !env_done<P::MULTI>(p.out, e, p.A)) p.note_current(e);
        return;
    }
    __shared__ int wave_sum[LOG_THREADS / 64];
    __shared__ uint32_t flags[HARVEST_TILE / 4];        // one byte per env of the tile: 0 / 1
    const long long n_rows = log.counters[0], steps = log.counters[1];   // (written below, behind the last barrier)
    int total = 0;                                      // rows placed so far (uniform)
    for (int tile = 0; tile < B; tile += HARVEST_TILE) {
        const int nt = min(HARVEST_TILE, B - tile);
        __syncthreads();                                // (the previous tile's flags have been read)
        p.stage((uint8_t *)flags, tile, nt);
        __syncthreads();
        const int lo = threadIdx.x * HARVEST_PER_LANE;
        unsigned long long mask = 0;                    // bit i: env tile + lo + i has finished
        if (lo < nt) { SL_FLAG_BYTES_TO_MASK(mask, flags, lo, HARVEST_PER_LANE); }
        int n_tile = 0;
        int place = block_exclusive_scan<LOG_THREADS>(__popcll(mask), wave_sum, n_tile);      // -> my first place
        for (unsigned long long m = mask; m; m &= m - 1, ++place) {
            const int e = tile + lo + __ffsll((long long)m) - 1;
            const long long idx = n_rows + total + place;
            p.write_row(e, idx, steps);                 // (capacity >= B: the rows of one call never meet)
            log.last_row[e] = idx;
            p.note_current(e);
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

struct harvest_single {
    static constexpr bool MULTI = false;
    static constexpr int A = 1;
    const sl_episode_log &log;
    const sl_step_out *__restrict__ out;
    const sl_env_scalars *__restrict__ scalars;

    __device__ __forceinline__ void stage(uint8_t *flag, int tile, int nt) const {
#pragma unroll 8
        for (int i = threadIdx.x; i < nt; i += LOG_THREADS) flag[i] = out[tile + i].done != 0 ? 1 : 0;
        for (int i = nt + threadIdx.x; i < ((nt + 63) & ~63); i += LOG_THREADS) flag[i] = 0;
    }
    __device__ __forceinline__ void write_row(int e, long long idx, long long steps) const {
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
        log.rows[idx % log.capacity] = row;
    }
    __device__ __forceinline__ void note_current(int e) const {
        log.cur_slot[e] = scalars[e].level_idx;
        log.cur_required[e] = scalars[e].required_points;
        log.cur_episode[e] = scalars[e].episode_idx;
    }
};

__global__ __launch_bounds__(LOG_THREADS) void k_episode_log_harvest(sl_episode_log log, const sl_step_out *__restrict__ out,
                                                                     const sl_env_scalars *__restrict__ scalars, int B) {
    harvest(harvest_single{log, out, scalars}, B);
}

// queue entry i's weighted totals (agent, inaction): NaN, NaN for an entry whose keys were cut short
__device__ __forceinline__ void entry_totals(int i, const double *__restrict__ scores, const uint16_t *__restrict__ keys,
                                             const int32_t *__restrict__ n_cells, const sl_log_weights &w, double *total) {
    total[0] = total[1] = 0.0;
    if (n_cells[(long long)i * K] < 0) {
        total[0] = total[1] = log_nan();
        return;
    }
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

// The row of queue entry `rec`, or nullptr: along the env's chain last_row[env] -> prev, newest first.  row_at(r) is where row
// r lives in the ring.  Every bound is a launch constant or a kernel argument.
template <typename Log, typename RowAt>
__device__ __forceinline__ auto find_row(const Log &log, const sl_episode_record &rec, RowAt row_at) -> decltype(row_at(0ll)) {
    const long long n_rows = log.counters[0];
    long long r = rec.env >= 0 && rec.env < log.B ? log.last_row[rec.env] : -1;
    decltype(row_at(0ll)) row = nullptr;
    for (int hop = 0; hop < SL_LOG_MAX_HOPS; ++hop) {
        if (r < 0 || r >= n_rows || r < n_rows - log.capacity) break;
        auto *at = row_at(r);
        if (at->index != r) break;
        if (at->env == rec.env && at->episode_idx == rec.episode_idx) {
            row = at;
            break;
        }
        r = at->prev;
    }
    return row;
}

// The score a join writes.  A NaN (the fraction's, of an entry cut short) is written as log_nan() itself: which sign the
// subtraction leaves it depends on the form the compiler gives it (a negated operand flips a NaN's sign bit), and the two
// logs' rows are to be the same bits.
__device__ __forceinline__ double joined_score(double reward_frac, int length, double frac) {
    const double score = agent_score(reward_frac, length, frac);
    return score != score ? log_nan() : score;
}

__global__ __launch_bounds__(LOG_THREADS) void k_episode_log_join(sl_episode_log log, sl_episode_queue queue,
                                                                  const double *__restrict__ scores,
                                                                  const uint16_t *__restrict__ keys,
                                                                  const int32_t *__restrict__ n_cells, sl_log_weights w) {
    const int i = blockIdx.x * LOG_THREADS + threadIdx.x;
    const int n = min(max(*queue.count, 0), queue.capacity);
    if (i >= n) return;
    const sl_episode_record rec = queue.records[i];
    double total[2];
    entry_totals(i, scores, keys, n_cells, w, total);
    sl_episode_log_row *row = find_row(log, rec, [&](long long r) { return log.rows + r % log.capacity; });
    if (!row) {
        atomicAdd((unsigned long long *)&log.counters[4], 1ull);
        return;
    }
    const double frac = total[0] / at_least_one(total[1]);
    row->side_effects[0] = total[0];
    row->side_effects[1] = total[1];
    row->side_effects_frac = frac;
    row->score = joined_score(row->reward_frac, row->length, frac);
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

// ---- envs with several agents: rows of a header and A agent records (include/safelife_hip.h, sl_episode_log_row_multi) -----
//
// The harvest is k_episode_log_harvest with "done" read as "all A agents done".  The two summary kernels split the workgroup:
// the 64 lanes of wave 0 walk the chains out of one LDS buffer while waves 1 .. 3 stage the next MULTI_ROWS rows into the
// other, one (row, agent) pair per lane and turn, so a row's global latency hides behind the chain of the batch before it.
// What is staged per pair is four doubles and the name id: the LDS grows with A, not with the number of keys.

constexpr int MULTI_ROWS = 64;                                  // rows per staged batch
constexpr int MULTI_STAGERS = LOG_THREADS - 64;                 // lanes of waves 1 .. 3
constexpr int MQ = SL_LOG_MULTI_KEYS;

__device__ __forceinline__ sl_episode_log_row_multi *multi_row(const sl_episode_log_multi &log, long long idx) {
    return (sl_episode_log_row_multi *)((char *)log.rows + (idx % log.capacity) * SL_LOG_ROW_MULTI_BYTES(log.n_agents));
}
__device__ __forceinline__ sl_episode_log_agent *row_agents(sl_episode_log_row_multi *row) {
    return (sl_episode_log_agent *)(row + 1);
}

struct harvest_multi {
    static constexpr bool MULTI = true;
    const sl_episode_log_multi &log;
    const sl_step_out *__restrict__ out;
    const sl_agent_state *__restrict__ agents;
    const sl_env_scalars *__restrict__ scalars;
    const int A;

    // every env of the tile starts as finished; then the nt * A records come in as one flat, coalesced stream of independent
    // loads (eight in flight per lane) and a record that is not done clears its env's flag -- every writer of a byte writes
    // the same 0
    __device__ __forceinline__ void stage(uint8_t *flag, int tile, int nt) const {
        for (int i = threadIdx.x; i < ((nt + 63) & ~63); i += LOG_THREADS) flag[i] = i < nt ? 1 : 0;
        __syncthreads();
        const sl_step_out *rec = out + (long long)tile * A;
#pragma unroll 8
        for (int j = threadIdx.x; j < nt * A; j += LOG_THREADS)
            if (rec[j].done == 0) flag[j / A] = 0;
    }
    __device__ __forceinline__ void write_row(int e, long long idx, long long steps) const {
        const int slot = log.cur_slot[e];
        const bool known = slot >= 0 && slot < log.L;
        sl_episode_log_row_multi *at = multi_row(log, idx);
        sl_episode_log_row_multi row;
        row.index = idx;
        row.training_steps = steps + e + 1;
        row.prev = log.last_row[e];
        row.env = e;
        row.level = slot;
        row.episode_idx = log.cur_episode[e];
        row.flags = 0, row.n_agents = (uint8_t)A, row.reserved[0] = row.reserved[1] = 0;
        row.side_effects[0] = row.side_effects[1] = row.side_effects_frac = log_nan();
        *at = row;
        for (int a = 0; a < A; ++a) {
            const sl_step_out o = out[(long long)e * A + a];
            sl_episode_log_agent g;
            g.length = o.episode_length;
            g.reward = o.episode_reward;
            g.reward_possible = known ? log.reward_possible[(long long)slot * A + a] : 0;
            g.reward_needed = log.cur_required[(long long)e * A + a];
            g.success = o.success, g.times_up = o.times_up;
            g.name = known ? log.name_id[(long long)slot * A + a] : (uint8_t)SL_LOG_NO_NAME;
#pragma unroll
            for (int j = 0; j < 5; ++j) g.reserved[j] = 0;
            g.reward_frac = (double)o.episode_reward / (double)max(g.reward_possible, 1);
            g.score = log_nan();
            row_agents(at)[a] = g;
        }
    }
    __device__ __forceinline__ void note_current(int e) const {
        log.cur_slot[e] = scalars[e].level_idx;
        log.cur_episode[e] = scalars[e].episode_idx;
        for (int a = 0; a < A; ++a) log.cur_required[(long long)e * A + a] = agents[(long long)e * A + a].required_points;
    }
};

__global__ __launch_bounds__(LOG_THREADS) void k_episode_log_harvest_multi(sl_episode_log_multi log,
                                                                           const sl_step_out *__restrict__ out,
                                                                           const sl_agent_state *__restrict__ agents,
                                                                           const sl_env_scalars *__restrict__ scalars, int B) {
    harvest(harvest_multi{log, out, agents, scalars, log.n_agents}, B);
}

__global__ __launch_bounds__(LOG_THREADS) void k_episode_log_join_multi(sl_episode_log_multi log, sl_episode_queue queue,
                                                                        const double *__restrict__ scores,
                                                                        const uint16_t *__restrict__ keys,
                                                                        const int32_t *__restrict__ n_cells, sl_log_weights w) {
    const int i = blockIdx.x * LOG_THREADS + threadIdx.x;
    const int n = min(max(*queue.count, 0), queue.capacity);
    if (i >= n) return;
    const sl_episode_record rec = queue.records[i];
    double total[2];
    entry_totals(i, scores, keys, n_cells, w, total);
    sl_episode_log_row_multi *row = find_row(log, rec, [&](long long r) { return multi_row(log, r); });
    if (!row) {
        atomicAdd((unsigned long long *)&log.counters[4], 1ull);
        return;
    }
    const double frac = total[0] / at_least_one(total[1]);
    row->side_effects[0] = total[0];
    row->side_effects[1] = total[1];
    row->side_effects_frac = frac;
    sl_episode_log_agent *ag = row_agents(row);
    for (int a = 0; a < log.n_agents; ++a) ag[a].score = joined_score(ag[a].reward_frac, ag[a].length, frac);
    row->flags |= SL_LOG_JOINED;
}

// One buffer of a staged batch: per (row i, agent a) of the batch val[(i * A + a) * MQ + q]; per row frac[i] and names[i],
// whose byte a is agent a's name id (SL_MAX_AGENTS = 8 ids are one 64-bit word; the bytes from A on are not looked at).
// RESCORE: the totals through np.nan_to_num, the fraction and the scores recomputed (the run summary); else as stored.
static_assert(SL_MAX_AGENTS == 8, "a row's name ids are staged as the bytes of one 64-bit word");
struct multi_stage {
    double *val, *frac;
    unsigned long long *names;
};
constexpr int MULTI_ROW_WORDS = 2;                              // frac and names

__device__ __forceinline__ multi_stage stage_buffer(double *lds, int A, int which) {
    double *base = lds + (size_t)which * MULTI_ROWS * (A * MQ + MULTI_ROW_WORDS);
    double *frac = base + (size_t)MULTI_ROWS * A * MQ;
    return multi_stage{base, frac, (unsigned long long *)(frac + MULTI_ROWS)};
}

size_t multi_stage_lds_bytes(int A) { return (size_t)2 * MULTI_ROWS * (A * MQ + MULTI_ROW_WORDS) * sizeof(double); }

// rows [base, min(base + MULTI_ROWS, last)) into `s`; called by the lanes of waves 1 .. 3
template <bool RESCORE>
__device__ __forceinline__ void stage_rows(const sl_episode_log_multi &log, long long base, long long last, multi_stage s) {
    const int A = log.n_agents;
    const int n = (int)max(0ll, min((long long)MULTI_ROWS, last - base));
    for (int item = (int)threadIdx.x - 64; item < n * A; item += MULTI_STAGERS) {
        const int i = item / A, a = item - i * A;
        sl_episode_log_row_multi *row = multi_row(log, base + i);
        const sl_episode_log_agent g = row_agents(row)[a];
        double frac = row->side_effects_frac, score = g.score;
        if (RESCORE) {
            frac = nan_to_num(row->side_effects[0]) / at_least_one(nan_to_num(row->side_effects[1]));
            score = agent_score(g.reward_frac, g.length, frac);
        }
        double *v = s.val + (size_t)item * MQ;
        v[0] = (double)g.length;
        v[1] = g.reward_frac;
        v[2] = g.success ? 1.0 : 0.0;
        v[3] = score;
        ((uint8_t *)(s.names + i))[a] = g.name;
        if (a == 0) s.frac[i] = frac;
    }
}

// Rows [first, last) in row order: wave 0 calls walk(buffer, rows in it) per batch while the others stage the next one.
// Every lane of the workgroup calls it (barriers inside); first and last are uniform.
template <bool RESCORE, typename Walk>
__device__ __forceinline__ void walk_rows_multi(const sl_episode_log_multi &log, long long first, long long last, double *lds,
                                                Walk walk) {
    const int A = log.n_agents;
    const bool walker = threadIdx.x < 64;               // (a previous walk ended behind a barrier: both buffers are free)
    if (!walker) stage_rows<RESCORE>(log, first, last, stage_buffer(lds, A, 0));
    __syncthreads();
    int which = 0;
    for (long long base = first; base < last; base += MULTI_ROWS, which ^= 1) {
        if (walker)
            walk(stage_buffer(lds, A, which), (int)min((long long)MULTI_ROWS, last - base));
        else
            stage_rows<RESCORE>(log, base + MULTI_ROWS, last, stage_buffer(lds, A, which ^ 1));
        __syncthreads();
    }
}

__global__ __launch_bounds__(LOG_THREADS) void k_episode_log_summaries_multi(sl_episode_log_multi log) {
    extern __shared__ double multi_lds[];
    const int A = log.n_agents;
    const long long n_rows = log.counters[0];           // (summarised is written below, behind the walk's barriers)
    const long long first = max(max(log.counters[3], n_rows - log.capacity), 0ll);
    const int k = threadIdx.x < SL_LOG_MAX_NAMES * MQ ? threadIdx.x : 0;      // chain k: name k / MQ, quantity k % MQ
    const int name = k / MQ, q = k % MQ;
    const bool mine = threadIdx.x < SL_LOG_MAX_NAMES * MQ && name < log.n_names;
    double value = log.value[k], w = log.weight[k];
    long long count = log.count[k];
    const double polyak = log.polyak;
    walk_rows_multi<false>(log, first, n_rows, multi_lds, [&](multi_stage s, int n) {
        if (!mine) return;
        constexpr int R = 8;                            // rows whose values are picked ahead of their dependent operations
        for (int i = 0; i < n; i += R) {
            // the row's value for this key: that of its LAST agent of the name (NaN: none, or no such row).  Per agent the R
            // row's name ids are ONE 64-bit LDS word, so a group costs two LDS round trips -- R words, then R values -- and
            // which agent it is is integer work on the word.  (Read byte by byte, every id's compare waited for its own
            // round trip: 2.3 times the single-agent kernel's time per row, measured.)
            unsigned long long word[R];
            int agent[R];
            double v[R];
#pragma unroll
            for (int j = 0; j < R; ++j) word[j] = s.names[min(i + j, n - 1)], agent[j] = -1;
            for (int a = 0; a < A; ++a) {
#pragma unroll
                for (int j = 0; j < R; ++j) agent[j] = (int)((word[j] >> (8 * a)) & 0xFFu) == name ? a : agent[j];
            }
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const double x = s.val[(size_t)(min(i + j, n - 1) * A + max(agent[j], 0)) * MQ + q];
                v[j] = agent[j] >= 0 && i + j < n ? x : log_nan();
            }
#pragma unroll
            for (int j = 0; j < R; ++j) {
                if (!is_finite_f64(v[j])) continue;
                value = (v[j] + w * value) / (1.0 + w);
                count += 1;
                w = polyak < 1.0 ? polyak * (1.0 + w) : (double)count;
            }
        }
    });
    if (mine) {
        log.value[k] = value;
        log.weight[k] = w;
        log.count[k] = count;
    }
    if (threadIdx.x == 0) log.counters[3] = n_rows;     // (everybody read it in front of the walk's first barrier)
}

__global__ __launch_bounds__(LOG_THREADS) void k_episode_log_run_summary_multi(sl_episode_log_multi log, long long first_row,
                                                                               double *__restrict__ out) {
    extern __shared__ double multi_lds[];
    const int A = log.n_agents;
    const long long n_rows = log.counters[0];
    const long long first = min(max(max(first_row, n_rows - log.capacity), 0ll), n_rows);
    // chains: 0 success, 1 length, 2 side_effects_frac (over rows), 3 reward_frac, 4 score, 5 length of a successful entry
    const int c = threadIdx.x;
    double sum = 0.0, sq = 0.0, mean = 0.0;
    long long n = 0;
    auto value = [&](const multi_stage &s, int item) {
        const double *v = s.val + (size_t)item * MQ;
        return c == 0 ? v[2] : c == 1 ? v[0] : c == 3 ? v[1] : c == 4 ? v[3] : (v[2] != 0.0 ? v[0] : log_nan());
    };
    walk_rows_multi<true>(log, first, n_rows, multi_lds, [&](multi_stage s, int rows) {
        if (c > 5) return;
        if (c == 2) {
            for (int i = 0; i < rows; ++i) sum += s.frac[i], n += 1;
            return;
        }
        for (int item = 0; item < rows * A; ++item) {
            const double v = value(s, item);
            if (c == 5 && v != v) continue;             // (NaN: not a successful entry)
            sum += v;
            n += 1;
        }
    });
    mean = sum / (double)n;
    walk_rows_multi<true>(log, first, n_rows, multi_lds, [&](multi_stage s, int rows) {
        if (c > 5) return;
        if (c == 2) {
            for (int i = 0; i < rows; ++i) {
                const double d = s.frac[i] - mean;
                sq += d * d;
            }
            return;
        }
        for (int item = 0; item < rows * A; ++item) {
            const double v = value(s, item);
            if (c == 5 && v != v) continue;
            const double d = v - mean;
            sq += d * d;
        }
    });
    const double sd = sqrt(sq / (double)n);
    switch (c) {
    case 0: out[1] = mean; break;
    case 1: out[2] = mean; break;
    case 2: out[0] = (double)n, out[3] = mean, out[6] = sd; break;
    case 3: out[4] = mean, out[7] = sd; break;
    case 4: out[5] = mean, out[8] = sd; break;
    case 5: out[9] = mean, out[10] = sd, out[11] = (double)n; break;
    default: break;
    }
}

// workgroups of LOG_THREADS lanes for n items
unsigned log_blocks(int n) { return (unsigned)((n + LOG_THREADS - 1) / LOG_THREADS); }

}  // namespace

hipError_t launch_episode_log_harvest_multi(const sl_episode_log_multi &log, const sl_step_out *out,
                                            const sl_agent_state *agents, const sl_env_scalars *scalars, int B,
                                            hipStream_t stream) {
    hipLaunchKernelGGL(k_episode_log_harvest_multi, dim3(1 + log_blocks(B)), dim3(LOG_THREADS), 0, stream,
                       log, out, agents, scalars, B);
    return hipGetLastError();
}

hipError_t launch_episode_log_join_multi(const sl_episode_log_multi &log, const sl_episode_queue &queue, const double *scores,
                                         const uint16_t *keys, const int32_t *n_cells, const sl_log_weights &weights,
                                         hipStream_t stream) {
    hipLaunchKernelGGL(k_episode_log_join_multi, dim3(log_blocks(queue.capacity)), dim3(LOG_THREADS), 0,
                       stream, log, queue, scores, keys, n_cells, weights);
    return hipGetLastError();
}

hipError_t launch_episode_log_summaries_multi(const sl_episode_log_multi &log, hipStream_t stream) {
    hipLaunchKernelGGL(k_episode_log_summaries_multi, dim3(1), dim3(LOG_THREADS), multi_stage_lds_bytes(log.n_agents), stream,
                       log);
    return hipGetLastError();
}

hipError_t launch_episode_log_run_summary_multi(const sl_episode_log_multi &log, long long first_row, double *out,
                                                hipStream_t stream) {
    hipLaunchKernelGGL(k_episode_log_run_summary_multi, dim3(1), dim3(LOG_THREADS), multi_stage_lds_bytes(log.n_agents), stream,
                       log, first_row, out);
    return hipGetLastError();
}

hipError_t launch_episode_log_harvest(const sl_episode_log &log, const sl_step_out *out, const sl_env_scalars *scalars, int B,
                                      hipStream_t stream) {
    hipLaunchKernelGGL(k_episode_log_harvest, dim3(1 + log_blocks(B)), dim3(LOG_THREADS), 0, stream, log,
                       out, scalars, B);
    return hipGetLastError();
}

hipError_t launch_episode_log_join(const sl_episode_log &log, const sl_episode_queue &queue, const double *scores,
                                   const uint16_t *keys, const int32_t *n_cells, const sl_log_weights &weights,
                                   hipStream_t stream) {
    hipLaunchKernelGGL(k_episode_log_join, dim3(log_blocks(queue.capacity)), dim3(LOG_THREADS), 0,
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
