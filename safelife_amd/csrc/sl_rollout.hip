// sl_rollout.hip -- PPO training batches on the device: the rollout buffer's per-step record and the returns / GAE
// advantages of the reference's PPO.gen_training_batch (training/ppo.py:74-143), bit exact with what numpy computes there.
//
// The reference strings the steps of a window of T steps into per-agent trajectories -- the steps of one env between
// resets -- and computes, per trajectory (numpy 2 promotion rules; g, l = the Python floats gamma, lmda):
//     val1       = np.append(values[1:], final_value)          final_value: the Python float 0.0 if the trajectory's last
//                                                              step has `done` (CLOSED), else float32 V(next_obs) (OPEN)
//     advantages = rewards + g * val1 - val0;   advantages[i] += l * advantages[i+1]   (backwards)
//     returns    = rewards;  returns[-1] += g * final_value;  returns[i] += g * returns[i+1]
// np.append promotes val1 to float64 when the trajectory is closed (a Python float joins a float32 array) or has one step
// (np.append([], x) is float64 whatever x is); otherwise val1 stays float32.  So a trajectory is
//     WIDE    closed, or of length 1: adv[i] = (f64(r[i]) + g * f64(v[i+1])) - f64(v[i]), adv[i] += l * adv[i+1], in float64
//     NARROW  open with two steps or more: g * v[i+1] is a float32 product with f32(g); with float32 rewards the rest is
//             float32 as well ((r + f32(g) v') - v, then + f32(l) adv'), with float64 rewards the product is widened and
//             the rest is float64
// and the returns are always in the rewards' dtype: ret[last] = r + f32(g) * final_value (a float32 product, widened for
// float64 rewards; a closed trajectory adds 0.0), ret[i] = r[i] + g_r * ret[i+1], g_r = g in the rewards' dtype.
// Everything is rounded to float32 once, at the end.  Nothing is fused: the library is built with -ffp-contract=off and
// the pragma below says it again.
//
// k_training_batch: one lane per env column of the time-major [T,B] arrays (a wavefront reads 64 consecutive elements of a
// row: coalesced), one backward walk t = T-1 .. 0.  The walk meets a trajectory's END first, which is where its width is
// known: closed -> wide; open (only the window's last step can be) -> wide iff the step before it has `done` or there is
// none (its length is 1).  The chain of T dependent steps per lane is what the kernel costs (latency, not bandwidth:
// 3 MB at 8192 x 20), so blocks are one wavefront -- 8192 envs are 128 workgroups, spread over the chip -- the next row's
// loads are issued before the current row's arithmetic, and nothing goes through LDS.
//
// The window of envs with several agents (sl_rollout_multi: the reference's driver loop, training/base_algo.py:152-244) is
// [T, B] with B = envs * n_agents columns and one more array, active [T, B].  A trajectory is then a run of contiguous
// active rows of a column, closed by `done` or left open at the window's end; inactive rows sit only behind a done row or
// at the window's head.  The arithmetic of a trajectory is the one above: k_training_batch<R, MASKED> is one walk for both
// windows -- an inactive row is stepped over (nothing written), an active row whose predecessor is inactive starts a
// trajectory; without the mask every row is active and `active` is never read.  Around it:
//
//   k_sample_actions          the categorical draw, one lane per row: 0 for rows the mask leaves out (null mask: none)
//   k_rollout_record          one lane per column: row t of the window
//   k_rollout_record_multi    one lane per ENV: its n_agents columns of row t, then the carried state -- active &= ~done,
//                             or everybody back and num_resets + 1 when nobody is left (the step kernel has reloaded the env)
//   k_compact_count / _write  the dense ids of the active rows in (t, env, agent) order: a two-level exclusive scan.  Every
//                             workgroup owns SL_ROLLOUT_SCAN_CHUNK flags, 16 per lane (one 16-byte load when the window is
//                             dense); the first launch leaves one count per chunk, the second sums the counts in front of
//                             its chunk, scans the chunk again (327 KB at 8192 x 2 x 20: it comes from L2) and writes.  No
//                             workgroup waits for another, and no atomic's arrival order decides a row's place.
//   k_gather_scalars / _obs   the flat tensors for the ids: one lane per row for the five scalars, one wavefront per row
//                             for the observation bytes, 16 bytes per lane when size and pointers allow
#include "sl_kernels.h"
#include "sl_rows.h"

#pragma clang fp contract(off)

namespace sl {
namespace {

constexpr int ROLLOUT_THREADS = 64;
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_PER_LANE = SL_ROLLOUT_SCAN_CHUNK / SCAN_THREADS;
static_assert(SCAN_PER_LANE == 16, "one 16-byte load of flags per lane");
constexpr int GATHER_THREADS = 256;

// One categorical draw per row from the policy's probabilities (training/ppo.py:66-69 draws on the host with numpy):
// u = a 24-bit uniform from splitmix64(seed, counter, row); cum_k = the fp32 running sum p_0 + ... + p_k over ALL A
// entries, in index order.  The action is the first k with u < cum_k; if there is none (the fp32 sum of a row can stay
// below 1 while u reaches 1 - 2^-24), the largest k with p_k > 0, which takes what rounding leaves; A-1 only when no
// entry is positive.  So an action of probability zero is never drawn while any entry is positive, and the result is
// in [0, A) whatever the row holds (NaN, inf, negative entries).  z = seed + G * (counter * K + e + 1): a caller that
// holds rows [lo, hi) of a larger batch passes seed + G * lo (mod 2^64) and gets the draws of rows lo + e of the whole.
// One thread per row; the result goes straight into the int32 buffer the step reads.  A row with active[e] == 0 gets
// action 0 and its probabilities are not read (active null: every row is drawn).
__global__ __launch_bounds__(256) void k_sample_actions(const float *__restrict__ probs, const uint8_t *__restrict__ active,
                                                        int B, int A, unsigned long long seed, unsigned long long counter,
                                                        int32_t *__restrict__ actions) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B) return;
    if (active && !active[e]) {
        actions[e] = 0;
        return;
    }
    const float u = draw_uniform24(draw_hash(seed, counter, (unsigned long long)e));
    const float *p = probs + (size_t)e * A;
    float cum = 0.0f;
    int a = A - 1;                  // the largest k with p_k > 0 seen so far (A-1 while there is none)
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

// Column c of row t from the step's arrays (indexed by column): the action with its own probability -- 0, and the status
// bit, when it lies outside [0, NA) -- reward, value and done; zeros when the column sits this step out (!act).  A masked
// window also notes who took part.  -> the column goes on after this step: it took part and is not done
template <typename R, bool MASKED>
__device__ __forceinline__ bool record_column(const sl_rollout &buf, uint8_t *active, int t, int c, bool act,
                                              const int32_t *actions, const float *probs, int NA, const R *rewards,
                                              const float *values, const uint8_t *done) {
    const long long o = (long long)t * buf.row_stride + c;
    int32_t a = 0;
    float p = 0.f, v = 0.f;
    R r = 0;
    bool d = false, goes_on = false;
    if (act) {
        a = actions[c];
        if (a >= 0 && a < NA)
            p = probs[(long long)c * NA + a];
        else
            atomicOr(buf.status, (int32_t)SL_ROLLOUT_BAD_ACTION);
        r = rewards[c];
        v = values[c];
        d = done[c] != 0;
        goes_on = !d;
    }
    buf.actions[o] = a;
    buf.action_prob[o] = p;
    ((R *)buf.rewards)[o] = r;
    buf.values[o] = v;
    buf.done[o] = d ? 1 : 0;
    if (MASKED) active[o] = act ? 1 : 0;
    return goes_on;
}

template <typename R>
__global__ __launch_bounds__(ROLLOUT_THREADS) void k_rollout_record(sl_rollout buf, int t, const int32_t *actions,
                                                                    const float *probs, int A, const R *rewards,
                                                                    const float *values, const uint8_t *done) {
    const int b = blockIdx.x * ROLLOUT_THREADS + threadIdx.x;
    if (b >= buf.B) return;
    record_column<R, false>(buf, nullptr, t, b, true, actions, probs, A, rewards, values, done);
}

template <typename R>
__global__ __launch_bounds__(ROLLOUT_THREADS) void k_rollout_record_multi(sl_rollout_multi m, int t, const int32_t *actions,
                                                                          const float *probs, int NA, const R *rewards,
                                                                          const float *values, const uint8_t *done,
                                                                          uint8_t *active_now, long long *num_resets) {
    const int A = m.n_agents;
    const int e = blockIdx.x * ROLLOUT_THREADS + threadIdx.x;
    if (e >= m.w.B / A) return;
    unsigned left = 0;                          // bit a: agent a goes on after this step
    for (int k = 0; k < A; ++k) {
        const int c = e * A + k;
        if (record_column<R, true>(m.w, m.active, t, c, active_now[c] != 0, actions, probs, NA, rewards, values, done))
            left |= 1u << k;
    }
    for (int k = 0; k < A; ++k) active_now[e * A + k] = (!left || ((left >> k) & 1u)) ? 1 : 0;
    if (!left) num_resets[e] += 1;
}

template <typename R, bool MASKED>
__global__ __launch_bounds__(ROLLOUT_THREADS) void k_training_batch(sl_rollout buf, const uint8_t *active,
                                                                    const float *final_values, double gamma, double lmda,
                                                                    float *returns, float *advantages,
                                                                    uint8_t *traj_start) {
    const int b = blockIdx.x * ROLLOUT_THREADS + threadIdx.x;
    if (b >= buf.B) return;
    constexpr bool R64 = sizeof(R) == 8;
    const long long rs = buf.row_stride, os = buf.out_stride;
    const R *rew = (const R *)buf.rewards + b;
    const float *val = buf.values + b;
    const uint8_t *dn = buf.done + b;
    const uint8_t *ac = MASKED ? active + b : nullptr;
    const int T = buf.T;
    const float gf = (float)gamma, lf = (float)lmda;
    const R gr = (R)gamma;
    const float fv = final_values[b];

    R r = rew[(T - 1) * rs];
    float v = val[(T - 1) * rs];
    bool d = dn[(T - 1) * rs] != 0;
    bool act = true;                            // without the mask every row takes part
    if (MASKED) act = ac[(T - 1) * rs] != 0;
    float v_next = 0.f;
    bool wide = false;
    double adv_d = 0.0;         // the running advantage of a wide trajectory, and of a narrow one with float64 rewards
    float adv_f = 0.f;          // ... of a narrow one with float32 rewards
    R ret = 0;
    for (int t = T - 1; t >= 0; --t) {
        // row t - 1, ahead of the arithmetic; in front of the window "the step before" counts as done
        R r_prev = 0;
        float v_prev = 0.f;
        bool d_prev = true, act_prev = !MASKED;
        if (t > 0) {
            r_prev = rew[(t - 1) * rs];
            v_prev = val[(t - 1) * rs];
            d_prev = dn[(t - 1) * rs] != 0;
            if (MASKED) act_prev = ac[(t - 1) * rs] != 0;
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

__global__ __launch_bounds__(SCAN_THREADS) void k_compact_count(sl_rollout_multi m, long long total, bool dense16,
                                                                int32_t *__restrict__ chunk_count) {
    __shared__ int wave_sum[SCAN_THREADS / 64];
    uint32_t w[4];
    const long long base = (long long)blockIdx.x * SL_ROLLOUT_SCAN_CHUNK + threadIdx.x * SCAN_PER_LANE;
    int sum;
    block_exclusive_scan<SCAN_THREADS>(load_flags16(m, base, total, dense16, w), wave_sum, sum);
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
    long long at = front + block_exclusive_scan<SCAN_THREADS>(cnt, wave_sum, sum);
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

}  // namespace

hipError_t launch_sample_actions(const float *probs, const uint8_t *active, int B, int A, unsigned long long seed,
                                 unsigned long long counter, int32_t *actions, hipStream_t stream) {
    hipLaunchKernelGGL(k_sample_actions, dim3((B + 255) / 256), dim3(256), 0, stream, probs, active, B, A, seed, counter,
                       actions);
    return hipGetLastError();
}

hipError_t launch_rollout_record(const sl_rollout &buf, int t, const int32_t *actions, const float *probs, int n_actions,
                                 const void *rewards, const float *values, const uint8_t *done, hipStream_t stream) {
    const dim3 grid((unsigned)((buf.B + ROLLOUT_THREADS - 1) / ROLLOUT_THREADS));
    if (buf.reward_dtype == SL_REWARD_F64)
        hipLaunchKernelGGL(k_rollout_record<double>, grid, dim3(ROLLOUT_THREADS), 0, stream, buf, t, actions, probs,
                           n_actions, (const double *)rewards, values, done);
    else
        hipLaunchKernelGGL(k_rollout_record<float>, grid, dim3(ROLLOUT_THREADS), 0, stream, buf, t, actions, probs,
                           n_actions, (const float *)rewards, values, done);
    return hipGetLastError();
}

hipError_t launch_rollout_record_multi(const sl_rollout_multi &buf, int t, const int32_t *actions, const float *probs,
                                       int n_actions, const void *rewards, const float *values, const uint8_t *done,
                                       uint8_t *active_now, long long *num_resets, hipStream_t stream) {
    const int envs = buf.w.B / buf.n_agents;
    const dim3 grid((unsigned)((envs + ROLLOUT_THREADS - 1) / ROLLOUT_THREADS));
    if (buf.w.reward_dtype == SL_REWARD_F64)
        hipLaunchKernelGGL(k_rollout_record_multi<double>, grid, dim3(ROLLOUT_THREADS), 0, stream, buf, t, actions, probs,
                           n_actions, (const double *)rewards, values, done, active_now, num_resets);
    else
        hipLaunchKernelGGL(k_rollout_record_multi<float>, grid, dim3(ROLLOUT_THREADS), 0, stream, buf, t, actions, probs,
                           n_actions, (const float *)rewards, values, done, active_now, num_resets);
    return hipGetLastError();
}

template <bool MASKED>
static void training_batch(const sl_rollout &buf, const uint8_t *active, const float *final_values, double gamma,
                           double lmda, float *returns, float *advantages, uint8_t *traj_start, hipStream_t stream) {
    const dim3 grid((unsigned)((buf.B + ROLLOUT_THREADS - 1) / ROLLOUT_THREADS));
    if (buf.reward_dtype == SL_REWARD_F64)
        hipLaunchKernelGGL((k_training_batch<double, MASKED>), grid, dim3(ROLLOUT_THREADS), 0, stream, buf, active,
                           final_values, gamma, lmda, returns, advantages, traj_start);
    else
        hipLaunchKernelGGL((k_training_batch<float, MASKED>), grid, dim3(ROLLOUT_THREADS), 0, stream, buf, active,
                           final_values, gamma, lmda, returns, advantages, traj_start);
}

hipError_t launch_training_batch(const sl_rollout &buf, const uint8_t *active, const float *final_values, double gamma,
                                 double lmda, float *returns, float *advantages, uint8_t *traj_start, hipStream_t stream) {
    if (active)
        training_batch<true>(buf, active, final_values, gamma, lmda, returns, advantages, traj_start, stream);
    else
        training_batch<false>(buf, active, final_values, gamma, lmda, returns, advantages, traj_start, stream);
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
    with_row_type(row_align(obs_bytes, {obs, obs_out}), [&](auto v) {
        typedef decltype(v) V;
        hipLaunchKernelGGL(k_gather_obs<V>, grid, block, 0, stream, rows, n, total, (const V *)obs,
                           obs_bytes / (long long)sizeof(V), (V *)obs_out);
    });
    return hipGetLastError();
}

}  // namespace sl
