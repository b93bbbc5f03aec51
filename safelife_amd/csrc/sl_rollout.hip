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
#include "sl_kernels.h"

#pragma clang fp contract(off)

namespace sl {
namespace {

constexpr int ROLLOUT_THREADS = 64;

template <typename R>
__global__ __launch_bounds__(ROLLOUT_THREADS) void k_rollout_record(sl_rollout buf, int t, const int32_t *actions,
                                                                    const float *probs, int A, const R *rewards,
                                                                    const float *values, const uint8_t *done) {
    const int b = blockIdx.x * ROLLOUT_THREADS + threadIdx.x;
    if (b >= buf.B) return;
    const long long o = (long long)t * buf.row_stride + b;
    const int a = actions[b];
    float p = 0.f;
    if (a >= 0 && a < A)
        p = probs[(long long)b * A + a];
    else
        atomicOr(buf.status, (int32_t)SL_ROLLOUT_BAD_ACTION);
    buf.actions[o] = a;
    buf.action_prob[o] = p;
    ((R *)buf.rewards)[o] = rewards[b];
    buf.values[o] = values[b];
    buf.done[o] = done[b] ? 1 : 0;
}

template <typename R>
__global__ __launch_bounds__(ROLLOUT_THREADS) void k_training_batch(sl_rollout buf, const float *final_values, double gamma,
                                                                    double lmda, float *returns, float *advantages,
                                                                    uint8_t *traj_start) {
    const int b = blockIdx.x * ROLLOUT_THREADS + threadIdx.x;
    if (b >= buf.B) return;
    constexpr bool R64 = sizeof(R) == 8;
    const long long rs = buf.row_stride, os = buf.out_stride;
    const R *rew = (const R *)buf.rewards + b;
    const float *val = buf.values + b;
    const uint8_t *dn = buf.done + b;
    const int T = buf.T;
    const float gf = (float)gamma, lf = (float)lmda;
    const R gr = (R)gamma;
    const float fv = final_values[b];

    R r = rew[(T - 1) * rs];
    float v = val[(T - 1) * rs];
    bool d = dn[(T - 1) * rs] != 0;
    float v_next = 0.f;
    bool wide = false;
    double adv_d = 0.0;         // the running advantage of a wide trajectory, and of a narrow one with float64 rewards
    float adv_f = 0.f;          // ... of a narrow one with float32 rewards
    R ret = 0;
    for (int t = T - 1; t >= 0; --t) {
        // row t - 1, ahead of the arithmetic; in front of the window "the step before" counts as done
        R r_prev = 0;
        float v_prev = 0.f;
        bool d_prev = true;
        if (t > 0) {
            r_prev = rew[(t - 1) * rs];
            v_prev = val[(t - 1) * rs];
            d_prev = dn[(t - 1) * rs] != 0;
        }
        if (t == T - 1 || d) {                  // the last step of a trajectory
            wide = d || d_prev;
            if (d) {                            // closed: final_value is 0.0
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
        if (traj_start) traj_start[t * os + b] = d_prev ? 1 : 0;
        v_next = v;
        r = r_prev, v = v_prev, d = d_prev;
    }
}

}  // namespace

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

hipError_t launch_training_batch(const sl_rollout &buf, const float *final_values, double gamma, double lmda,
                                 float *returns, float *advantages, uint8_t *traj_start, hipStream_t stream) {
    const dim3 grid((unsigned)((buf.B + ROLLOUT_THREADS - 1) / ROLLOUT_THREADS));
    if (buf.reward_dtype == SL_REWARD_F64)
        hipLaunchKernelGGL(k_training_batch<double>, grid, dim3(ROLLOUT_THREADS), 0, stream, buf, final_values, gamma, lmda,
                           returns, advantages, traj_start);
    else
        hipLaunchKernelGGL(k_training_batch<float>, grid, dim3(ROLLOUT_THREADS), 0, stream, buf, final_values, gamma, lmda,
                           returns, advantages, traj_start);
    return hipGetLastError();
}

}  // namespace sl
