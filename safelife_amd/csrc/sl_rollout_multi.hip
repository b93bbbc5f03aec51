// sl_rollout_multi.hip -- PPO training batches for envs with several agents: the masked window of the reference's driver
// loop (training/base_algo.py:152-244 with training/ppo.py:74-143), on the device.  include/safelife_hip.h states the
// contract (sl_rollout_multi); sl_rollout.hip explains the arithmetic of a trajectory, which is unchanged here.
//
// The window is [T, B] with B = envs * n_agents columns and one more array, active [T, B].  A trajectory is a run of
// contiguous active rows of a column, closed by `done` or left open at the window's end; inactive rows sit only behind a
// done row or at the window's head.
//
//   k_sample_actions_masked   the draw of k_sample_actions (sl_generic.hip) for active rows, 0 for the others
//   k_rollout_record_multi    one lane per ENV: its n_agents columns of row t, then the carried state -- active &= ~done,
//                             or everybody back and num_resets + 1 when nobody is left (the step kernel has reloaded the env)
//   k_training_batch_multi    k_training_batch with the mask: one lane per column, one backward walk; an inactive row is
//                             stepped over (nothing written), an active row whose predecessor is inactive starts a trajectory
//   k_compact_count / _write  the dense ids of the active rows in (t, env, agent) order: a two-level exclusive scan.  Every
//                             workgroup owns SL_ROLLOUT_SCAN_CHUNK flags, 16 per lane (one 16-byte load when the window is
//                             dense); the first launch leaves one count per chunk, the second sums the counts in front of
//                             its chunk, scans the chunk again (327 KB at 8192 x 2 x 20: it comes from L2) and writes.  No
//                             workgroup waits for another, and no atomic's arrival order decides a row's place.
//   k_gather_scalars / _obs   the flat tensors for the ids: one lane per row for the five scalars, one wavefront per row
//                             for the observation bytes, 16 bytes per lane when size and pointers allow
#include "sl_kernels.h"

#pragma clang fp contract(off)

namespace sl {
namespace {

constexpr int MULTI_THREADS = 64;
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_PER_LANE = SL_ROLLOUT_SCAN_CHUNK / SCAN_THREADS;
static_assert(SCAN_PER_LANE == 16, "one 16-byte load of flags per lane");
constexpr int GATHER_THREADS = 256;

__global__ __launch_bounds__(256) void k_sample_actions_masked(const float *__restrict__ probs,
                                                               const uint8_t *__restrict__ active, int B, int A,
                                                               unsigned long long seed, unsigned long long counter,
                                                               int32_t *__restrict__ actions) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B) return;
    if (active && !active[e]) {
        actions[e] = 0;
        return;
    }
    // k_sample_actions, statement for statement
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (counter * 0x100000001B3ull + (unsigned long long)e + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const float u = (float)(unsigned)(z >> 40) * (1.0f / 16777216.0f);
    const float *p = probs + (size_t)e * A;
    float cum = 0.0f;
    int a = A - 1;
    for (int k = 0; k < A; ++k) {
        const float pk = p[k];
        cum += pk;
        if (pk > 0.0f) a = k;
        if (u < cum) {
            a = k;
            break;
        }
    }
    actions[e] = a;
}

template <typename R>
__global__ __launch_bounds__(MULTI_THREADS) void k_rollout_record_multi(sl_rollout_multi m, int t, const int32_t *actions,
                                                                        const float *probs, int NA, const R *rewards,
                                                                        const float *values, const uint8_t *done,
                                                                        uint8_t *active_now, long long *num_resets) {
    const sl_rollout &buf = m.w;
    const int A = m.n_agents;
    const int e = blockIdx.x * MULTI_THREADS + threadIdx.x;
    if (e >= buf.B / A) return;
    unsigned left = 0;                          // bit a: agent a goes on after this step
    for (int k = 0; k < A; ++k) {
        const int c = e * A + k;
        const long long o = (long long)t * buf.row_stride + c;
        const bool act = active_now[c] != 0;
        int32_t a = 0;
        float p = 0.f, v = 0.f;
        R r = 0;
        bool d = false;
        if (act) {
            a = actions[c];
            if (a >= 0 && a < NA)
                p = probs[(long long)c * NA + a];
            else
                atomicOr(buf.status, (int32_t)SL_ROLLOUT_BAD_ACTION);
            r = rewards[c];
            v = values[c];
            d = done[c] != 0;
            if (!d) left |= 1u << k;
        }
        buf.actions[o] = a;
        buf.action_prob[o] = p;
        ((R *)buf.rewards)[o] = r;
        buf.values[o] = v;
        buf.done[o] = d ? 1 : 0;
        m.active[o] = act ? 1 : 0;
    }
    for (int k = 0; k < A; ++k) active_now[e * A + k] = (!left || ((left >> k) & 1u)) ? 1 : 0;
    if (!left) num_resets[e] += 1;
}

template <typename R>
__global__ __launch_bounds__(MULTI_THREADS) void k_training_batch_multi(sl_rollout_multi m, const float *final_values,
                                                                        double gamma, double lmda, float *returns,
                                                                        float *advantages, uint8_t *traj_start) {
    const sl_rollout &buf = m.w;
    const int b = blockIdx.x * MULTI_THREADS + threadIdx.x;
    if (b >= buf.B) return;
    constexpr bool R64 = sizeof(R) == 8;
    const long long rs = buf.row_stride, os = buf.out_stride;
    const R *rew = (const R *)buf.rewards + b;
    const float *val = buf.values + b;
    const uint8_t *dn = buf.done + b;
    const uint8_t *ac = m.active + b;
    const int T = buf.T;
    const float gf = (float)gamma, lf = (float)lmda;
    const R gr = (R)gamma;
    const float fv = final_values[b];

    R r = rew[(T - 1) * rs];
    float v = val[(T - 1) * rs];
    bool d = dn[(T - 1) * rs] != 0;
    bool act = ac[(T - 1) * rs] != 0;
    float v_next = 0.f;
    bool wide = false;
    double adv_d = 0.0;
    float adv_f = 0.f;
    R ret = 0;
    for (int t = T - 1; t >= 0; --t) {
        // row t - 1, ahead of the arithmetic; in front of the window "the step before" counts as done
        R r_prev = 0;
        float v_prev = 0.f;
        bool d_prev = true, act_prev = false;
        if (t > 0) {
            r_prev = rew[(t - 1) * rs];
            v_prev = val[(t - 1) * rs];
            d_prev = dn[(t - 1) * rs] != 0;
            act_prev = ac[(t - 1) * rs] != 0;
        }
        if (act) {
            const bool first = d_prev || !act_prev;     // nothing of this trajectory lies in front of row t
            if (t == T - 1 || d) {                      // the last step of a trajectory
                wide = d || first;
                if (d) {                                // closed: final_value is 0.0
                    ret = r + (R)0;
                    adv_d = ((double)r + gamma * 0.0) - (double)v;
                } else {
                    const float boot = gf * fv;
                    ret = r + (R)boot;
                    if (wide)
                        adv_d = ((double)r + gamma * (double)fv) - (double)v;
                    else if (R64)
                        adv_d = ((double)r + (double)boot) - (double)v;
                    else
                        adv_f = ((float)r + boot) - v;
                }
            } else {
                ret = r + gr * ret;
                if (wide) {
                    const double a = ((double)r + gamma * (double)v_next) - (double)v;
                    adv_d = a + lmda * adv_d;
                } else if (R64) {
                    const float gv = gf * v_next;
                    const double a = ((double)r + (double)gv) - (double)v;
                    adv_d = a + lmda * adv_d;
                } else {
                    const float a = ((float)r + gf * v_next) - v;
                    adv_f = a + lf * adv_f;
                }
            }
            returns[t * os + b] = (float)ret;
            advantages[t * os + b] = (wide || R64) ? (float)adv_d : adv_f;
            if (traj_start) traj_start[t * os + b] = first ? 1 : 0;
            v_next = v;
        }
        r = r_prev, v = v_prev, d = d_prev, act = act_prev;
    }
}

// The 16 flags of dense ids [base, base + 16) as 16 bytes of 0 / 1 (ids past `total` read as 0); -> how many are set.
__device__ __forceinline__ int load_flags16(const sl_rollout_multi &m, long long base, long long total, bool dense16,
                                            uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    if (base >= total) return 0;
    if (dense16 && base + 16 <= total) {
        const uint4 q = *(const uint4 *)(m.active + base);
        const uint32_t raw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)     // byte != 0 -> 1
            w[j] = ((raw[j] | ((raw[j] & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u;
    } else {
        const long long B = m.w.B, rs = m.w.row_stride;
        long long t = base / B, c = base - t * B;
        for (int k = 0; k < 16 && base + k < total; ++k) {
            if (m.active[t * rs + c]) w[k >> 2] |= 1u << (8 * (k & 3));
            if (++c == B) c = 0, ++t;
        }
    }
    return __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
}

// exclusive prefix of x over the workgroup's lanes, and the workgroup's total
__device__ __forceinline__ int block_scan(int x, int *wave_sum, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = x;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
    for (int k = 0; k < SCAN_THREADS / 64; ++k) {
        const int s = wave_sum[k];
        before += k < wave ? s : 0;
        total += s;
    }
    __syncthreads();
    return before + incl - x;
}

__global__ __launch_bounds__(SCAN_THREADS) void k_compact_count(sl_rollout_multi m, long long total, bool dense16,
                                                                int32_t *__restrict__ chunk_count) {
    __shared__ int wave_sum[SCAN_THREADS / 64];
    uint32_t w[4];
    const long long base = (long long)blockIdx.x * SL_ROLLOUT_SCAN_CHUNK + threadIdx.x * SCAN_PER_LANE;
    int sum;
    block_scan(load_flags16(m, base, total, dense16, w), wave_sum, sum);
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = sum;
}

__global__ __launch_bounds__(SCAN_THREADS) void k_compact_write(sl_rollout_multi m, long long total, bool dense16,
                                                                const int32_t *__restrict__ chunk_count,
                                                                long long *__restrict__ rows_out,
                                                                long long *__restrict__ count_out) {
    __shared__ int wave_sum[SCAN_THREADS / 64];
    __shared__ long long part[SCAN_THREADS / 64];
    // rows in front of this chunk
    long long mine = 0;
    for (int k = threadIdx.x; k < (int)blockIdx.x; k += SCAN_THREADS) mine += chunk_count[k];
    for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    long long front = 0;
    for (int k = 0; k < SCAN_THREADS / 64; ++k) front += part[k];

    uint32_t w[4];
    const long long base = (long long)blockIdx.x * SL_ROLLOUT_SCAN_CHUNK + threadIdx.x * SCAN_PER_LANE;
    const int cnt = load_flags16(m, base, total, dense16, w);
    int sum;
    long long at = front + block_scan(cnt, wave_sum, sum);
    if (cnt) {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if ((w[k >> 2] >> (8 * (k & 3))) & 1u) rows_out[at++] = base + k;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *count_out = front + sum;
}

__global__ __launch_bounds__(GATHER_THREADS) void k_gather_scalars(sl_rollout buf, const long long *__restrict__ rows,
                                                                   long long n, const float *__restrict__ returns,
                                                                   const float *__restrict__ advantages,
                                                                   long long *__restrict__ actions_out,
                                                                   float *__restrict__ prob_out, float *__restrict__ ret_out,
                                                                   float *__restrict__ adv_out, float *__restrict__ val_out) {
    const long long i = (long long)blockIdx.x * GATHER_THREADS + threadIdx.x;
    if (i >= n) return;
    const long long r = rows[i];
    if (r < 0 || r >= (long long)buf.T * buf.B) {
        atomicOr(buf.status, (int32_t)SL_ROLLOUT_BAD_INDEX);
        return;
    }
    const long long t = r / buf.B, c = r - t * buf.B;
    const long long s = t * buf.row_stride + c, so = t * buf.out_stride + c;
    actions_out[i] = (long long)buf.actions[s];
    prob_out[i] = buf.action_prob[s];
    ret_out[i] = returns[so];
    adv_out[i] = advantages[so];
    val_out[i] = buf.values[s];
}

// one wavefront per row: lanes stride over the row's elements of type V
template <typename V>
__global__ __launch_bounds__(GATHER_THREADS) void k_gather_obs(const long long *__restrict__ rows, long long n,
                                                               long long total, const V *__restrict__ obs, long long nv,
                                                               V *__restrict__ out) {
    const long long i = (long long)blockIdx.x * (GATHER_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    const long long r = rows[i];
    if (r < 0 || r >= total) return;            // (k_gather_scalars raises the status bit)
    const V *src = obs + r * nv;
    V *dst = out + i * nv;
    for (long long c = threadIdx.x & 63; c < nv; c += 64) dst[c] = src[c];
}

// the widest of 16 / 8 / 4 / 2 / 1 bytes that divides the row size and every pointer
int row_align(long long bytes, const void *a, const void *b) {
    const unsigned long long bits = (unsigned long long)bytes | 16ull | (unsigned long long)(uintptr_t)a |
                                    (unsigned long long)(uintptr_t)b;
    return (int)(bits & (~bits + 1ull));
}

}  // namespace

hipError_t launch_sample_actions_masked(const float *probs, const uint8_t *active, int B, int A, unsigned long long seed,
                                        unsigned long long counter, int32_t *actions, hipStream_t stream) {
    hipLaunchKernelGGL(k_sample_actions_masked, dim3((B + 255) / 256), dim3(256), 0, stream, probs, active, B, A, seed,
                       counter, actions);
    return hipGetLastError();
}

hipError_t launch_rollout_record_multi(const sl_rollout_multi &buf, int t, const int32_t *actions, const float *probs,
                                       int n_actions, const void *rewards, const float *values, const uint8_t *done,
                                       uint8_t *active_now, long long *num_resets, hipStream_t stream) {
    const int envs = buf.w.B / buf.n_agents;
    const dim3 grid((unsigned)((envs + MULTI_THREADS - 1) / MULTI_THREADS));
    if (buf.w.reward_dtype == SL_REWARD_F64)
        hipLaunchKernelGGL(k_rollout_record_multi<double>, grid, dim3(MULTI_THREADS), 0, stream, buf, t, actions, probs,
                           n_actions, (const double *)rewards, values, done, active_now, num_resets);
    else
        hipLaunchKernelGGL(k_rollout_record_multi<float>, grid, dim3(MULTI_THREADS), 0, stream, buf, t, actions, probs,
                           n_actions, (const float *)rewards, values, done, active_now, num_resets);
    return hipGetLastError();
}

hipError_t launch_training_batch_multi(const sl_rollout_multi &buf, const float *final_values, double gamma, double lmda,
                                       float *returns, float *advantages, uint8_t *traj_start, hipStream_t stream) {
    const dim3 grid((unsigned)((buf.w.B + MULTI_THREADS - 1) / MULTI_THREADS));
    if (buf.w.reward_dtype == SL_REWARD_F64)
        hipLaunchKernelGGL(k_training_batch_multi<double>, grid, dim3(MULTI_THREADS), 0, stream, buf, final_values, gamma,
                           lmda, returns, advantages, traj_start);
    else
        hipLaunchKernelGGL(k_training_batch_multi<float>, grid, dim3(MULTI_THREADS), 0, stream, buf, final_values, gamma,
                           lmda, returns, advantages, traj_start);
    return hipGetLastError();
}

int rollout_compact_chunks(const sl_rollout_multi &buf) {
    const long long total = (long long)buf.w.T * buf.w.B;
    return (int)((total + SL_ROLLOUT_SCAN_CHUNK - 1) / SL_ROLLOUT_SCAN_CHUNK);
}

hipError_t launch_rollout_compact(const sl_rollout_multi &buf, long long *rows_out, long long *count_out, int32_t *workspace,
                                  hipStream_t stream) {
    const long long total = (long long)buf.w.T * buf.w.B;
    const dim3 grid((unsigned)rollout_compact_chunks(buf));
    const bool dense16 = buf.w.row_stride == buf.w.B && ((uintptr_t)buf.active & 15) == 0;
    hipLaunchKernelGGL(k_compact_count, grid, dim3(SCAN_THREADS), 0, stream, buf, total, dense16, workspace);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_compact_write, grid, dim3(SCAN_THREADS), 0, stream, buf, total, dense16, workspace, rows_out,
                       count_out);
    return hipGetLastError();
}

hipError_t launch_rollout_gather(const sl_rollout_multi &buf, const long long *rows, long long n, const float *returns,
                                 const float *advantages, const void *obs, long long obs_bytes, void *obs_out,
                                 long long *actions_out, float *action_prob_out, float *returns_out, float *advantages_out,
                                 float *values_out, hipStream_t stream) {
    hipLaunchKernelGGL(k_gather_scalars, dim3((unsigned)((n + GATHER_THREADS - 1) / GATHER_THREADS)), dim3(GATHER_THREADS), 0,
                       stream, buf.w, rows, n, returns, advantages, actions_out, action_prob_out, returns_out, advantages_out,
                       values_out);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || !obs) return err;
    const long long total = (long long)buf.w.T * buf.w.B;
    const int rows_per_block = GATHER_THREADS / 64;
    const dim3 grid((unsigned)((n + rows_per_block - 1) / rows_per_block)), block(GATHER_THREADS);
    switch (row_align(obs_bytes, obs, obs_out)) {
#define SL_GATHER_OBS(V) \
    hipLaunchKernelGGL(k_gather_obs<V>, grid, block, 0, stream, rows, n, total, (const V *)obs, \
                       obs_bytes / (long long)sizeof(V), (V *)obs_out)
    case 16: SL_GATHER_OBS(uint4); break;
    case 8: SL_GATHER_OBS(uint2); break;
    case 4: SL_GATHER_OBS(uint32_t); break;
    case 2: SL_GATHER_OBS(uint16_t); break;
    default: SL_GATHER_OBS(uint8_t); break;
#undef SL_GATHER_OBS
    }
    return hipGetLastError();
}

}  // namespace sl
