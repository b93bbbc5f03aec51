// sl_replay.hip -- DQN's replay machinery on the device: the n-step window and the ring of the reference's
// DQN.add_to_replay / ReplayBuffer (training/dqn.py:21-37, 110-134), a sampler of distinct rows, the gather that builds the
// tensors of DQN.optimize, and take_one_step's epsilon-greedy draw.  include/safelife_hip.h states the contract.
//
// slhip_replay_add is two launches.  k_replay_plan, ONE workgroup: per env the number of pushes of this step (0 .. n+1)
// from fill[b] and done[b], an exclusive prefix sum over the envs (wave scan, wave totals through LDS, a carry from chunk
// to chunk of 1024 envs) on top of *idx -- every push's ring slot is then a function of the data alone, no atomic's
// arrival order takes part -- and fill / *idx / *head moved on.  It touches 5 bytes per env; what it costs is its launch
// and a few barriers.  k_replay_copy, one workgroup per env, is the bandwidth part: the step's obs row goes into the
// window, the row it displaces (the step n steps back) and obs go into the ring if the window was full, and the window's
// rows with next_obs go into the ring if the episode ended -- about six rows moved per env-step in steady state, 16
// bytes per lane when the rows allow it.  The first n lanes also carry the scalars: lane k owns the window slot k steps
// back, adds r * gamma^k to its float64 reward (product, then sum: contraction is off), and writes action / reward /
// done of the pushes that come from its slot.
//
// slhip_replay_add_masked is the same two launches with one more input, active [B] (null: everybody), for envs with
// several agents: B is then envs * n_agents columns, and an agent that has left its level sits out until the env reloads.
// The plan reads active[b] FIRST: an inactive column counts no push, keeps its fill, and gets PLAN_INACTIVE as its plan
// code -- its done flag is not looked at (the env keeps reporting 1 for an agent that is gone).  The copy kernel's
// workgroup of such a column reads its plan code and leaves: no row, action, reward or window slot of it is touched.
//
// The window is a ring over t mod n shared by all envs, so slot *head (where this step goes) is also the slot of the
// step n steps back: every lane reads its piece of the old row before it writes the new one to the same address.
#include "sl_kernels.h"
#include "sl_rows.h"

#pragma clang fp contract(off)

namespace sl {
namespace {

constexpr int PLAN_THREADS = 1024;
constexpr int ROW_THREADS = 256;
constexpr int PLAN_DONE = 1 << 8;           // plan_code: fill before the step | PLAN_DONE | PLAN_INACTIVE
constexpr int PLAN_INACTIVE = 1 << 9;

__global__ __launch_bounds__(PLAN_THREADS) void k_replay_plan(sl_replay buf, const uint8_t *__restrict__ done,
                                                              const uint8_t *__restrict__ active) {
    __shared__ int wave_sum[PLAN_THREADS / 64];
    const int tid = threadIdx.x;
    const int B = buf.B, n = buf.n;
    const long long cap = buf.capacity;
    const long long idx0 = *buf.idx;
    const int head_word = *buf.head;
    const int head = head_word >= 0 && head_word < n ? head_word : 0;
    const long long start = (idx0 >= 0 ? idx0 : 0) % cap;
    long long carry = 0;                        // pushes of the envs in front of this chunk
    for (int b0 = 0; b0 < B; b0 += PLAN_THREADS) {
        const int b = b0 + tid;
        int cnt = 0;
        if (b < B) {
            if (active && active[b] == 0) {
                buf.plan_code[b] = PLAN_INACTIVE;       // pushes nothing; fill[b] stays, done[b] is not read
            } else {
                const int f = min(max(buf.fill[b], 0), n);
                const bool d = done[b] != 0;
                const int fn = min(f + 1, n);
                cnt = (f == n ? 1 : 0) + (d ? fn : 0);
                buf.fill[b] = d ? 0 : fn;
                buf.plan_code[b] = f | (d ? PLAN_DONE : 0);
            }
        }
        int total;
        const int before = block_exclusive_scan<PLAN_THREADS>(cnt, wave_sum, total);
        if (b < B) {
            long long s = start + carry + before;       // < 2 * cap: one step pushes at most B * (n+1) <= cap
            if (s >= cap) s -= cap;
            buf.plan_base[b] = s;
        }
        carry += total;
    }
    if (tid == 0) {
        *buf.idx = idx0 + carry;
        *buf.head = head + 1 < n ? head + 1 : 0;
    }
}

template <typename V>
__global__ __launch_bounds__(ROW_THREADS) void k_replay_copy(sl_replay buf, const V *__restrict__ obs,
                                                             const int32_t *__restrict__ actions, const void *rewards,
                                                             const V *__restrict__ next_obs) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int B = buf.B, n = buf.n;
    const long long cap = buf.capacity;
    const int code = buf.plan_code[b];
    if (code & PLAN_INACTIVE) return;                   // before anything of the column is loaded
    const int fill_old = code & 0xff;
    const bool done = (code & PLAN_DONE) != 0;
    const int head = *buf.head;                         // the plan has moved it on
    const int cur = head > 0 ? head - 1 : n - 1;        // the slot of this step
    const bool push = fill_old == n;                    // the window was full: the step n steps back leaves it
    const int fill_new = min(fill_old + 1, n);
    const int m = done ? fill_new : 0;                  // rows flushed
    const long long s_push = buf.plan_base[b];
    long long s_flush = s_push + (push ? 1 : 0);
    if (s_flush >= cap) s_flush -= cap;

    if (tid < n) {
        const int k = tid;                              // this lane's slot holds the step k steps back
        const double r = buf.reward_dtype == SL_REWARD_F64 ? ((const double *)rewards)[b]
                                                           : (double)((const float *)rewards)[b];
        const int slot = cur - k < 0 ? cur - k + n : cur - k;
        const long long w = (long long)slot * B + b;
        long long s = s_flush + k;
        if (s >= cap) s -= cap;
        if (k == 0) {
            if (push) {
                buf.action[s_push] = buf.win_action[w];
                buf.reward[s_push] = buf.win_reward[w];
                buf.done[s_push] = done ? 1 : 0;
            }
            const int32_t a = actions[b];
            buf.win_action[w] = a;
            buf.win_reward[w] = r;
            if (done) {
                buf.action[s] = a;
                buf.reward[s] = r;
                buf.done[s] = 1;
            }
        } else if (k < fill_new) {
            double g = 0.0;
#pragma unroll
            for (int j = 0; j < SL_REPLAY_MAX_N - 1; ++j)
                if (j == k - 1) g = buf.gamma_pow[j];
            const double prod = r * g;
            const double v = buf.win_reward[w] + prod;
            buf.win_reward[w] = v;
            if (done) {
                buf.action[s] = buf.win_action[w];
                buf.reward[s] = v;
                buf.done[s] = 1;
            }
        }
    }

    const long long nv = buf.obs_bytes / (long long)sizeof(V);
    const V *o = obs + (long long)b * nv;
    const V *nx = next_obs + (long long)b * nv;
    V *win = (V *)buf.win_obs;
    V *wcur = win + ((long long)cur * B + b) * nv;
    V *ring_o = (V *)buf.obs, *ring_n = (V *)buf.next_obs;
    for (long long c = tid; c < nv; c += ROW_THREADS) {
        const V ov = o[c];
        if (push) {
            ring_o[s_push * nv + c] = wcur[c];
            ring_n[s_push * nv + c] = ov;
        }
        wcur[c] = ov;
        if (m) {
            const V nxv = nx[c];
            int slot = cur;
            long long s = s_flush;
            ring_o[s * nv + c] = ov;
            ring_n[s * nv + c] = nxv;
            for (int k = 1; k < m; ++k) {
                slot = slot > 0 ? slot - 1 : n - 1;
                s = s + 1 < cap ? s + 1 : 0;
                ring_o[s * nv + c] = win[((long long)slot * B + b) * nv + c];
                ring_n[s * nv + c] = nxv;
            }
        }
    }
}

// Floyd's algorithm, k draws t_i in [0, j_i], j_i = N - k + i: out_i = t_i unless t_i is already out, else j_i.  Every
// out_m is t_m or j_m, so "t_i is already out" is: t_i equals an earlier t_m (whether or not that one was kept, t_m is out
// by then), or t_i equals an earlier j_m whose draw collided.  The first test is done for all i side by side; the second
// is a chain that points strictly backwards, resolved by one lane in one pass over flags in LDS.
__global__ __launch_bounds__(PLAN_THREADS) void k_replay_sample(sl_replay buf, int k, unsigned long long seed,
                                                                unsigned long long counter, long long *__restrict__ out) {
    __shared__ unsigned long long ts[SL_REPLAY_MAX_K];
    __shared__ uint8_t collided[SL_REPLAY_MAX_K];
    const int tid = threadIdx.x;
    const long long idx = *buf.idx;
    const long long N = idx < buf.capacity ? idx : buf.capacity;
    if ((long long)k > N) {
        if (tid == 0) atomicOr(buf.status, (int32_t)SL_REPLAY_SHORT);
        return;
    }
    const unsigned long long base = (unsigned long long)(N - k);
    for (int i = tid; i < k; i += PLAN_THREADS)
        ts[i] = __umul64hi(draw_hash(seed, counter, (unsigned long long)i), base + (unsigned long long)i + 1ull);
    __syncthreads();
    for (int i = tid; i < k; i += PLAN_THREADS) {
        const unsigned long long t = ts[i];
        bool dup = false;
        for (int mm = 0; mm < i; ++mm) dup |= ts[mm] == t;
        collided[i] = dup ? 1 : 0;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 0; i < k; ++i) {
            const unsigned long long t = ts[i];
            if (!collided[i] && t >= base) {
                const unsigned long long mm = t - base;
                if (mm < (unsigned long long)i && collided[mm]) collided[i] = 1;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < k; i += PLAN_THREADS)
        out[i] = (long long)(collided[i] ? base + (unsigned long long)i : ts[i]);
}

__device__ __forceinline__ bool gather_row(const sl_replay &buf, const long long *index, long long *action_out,
                                           float *reward_out, float *done_out, long long &s) {
    const int i = blockIdx.x;
    s = index[i];
    if (s < 0 || s >= buf.capacity) {
        if (threadIdx.x == 0) atomicOr(buf.status, (int32_t)SL_REPLAY_BAD_INDEX);
        return false;
    }
    if (threadIdx.x == 0) {
        action_out[i] = (long long)buf.action[s];
        reward_out[i] = (float)buf.reward[s];
        done_out[i] = buf.done[s] ? 1.0f : 0.0f;
    }
    return true;
}

template <typename V>
__global__ __launch_bounds__(ROW_THREADS) void k_replay_gather(sl_replay buf, const long long *__restrict__ index,
                                                               V *__restrict__ obs_out, V *__restrict__ next_out,
                                                               long long *action_out, float *reward_out, float *done_out) {
    long long s;
    if (!gather_row(buf, index, action_out, reward_out, done_out, s)) return;
    const long long nv = buf.obs_bytes / (long long)sizeof(V);
    const V *o = (const V *)buf.obs + s * nv, *nx = (const V *)buf.next_obs + s * nv;
    V *oo = obs_out + (long long)blockIdx.x * nv, *no = next_out + (long long)blockIdx.x * nv;
    for (long long c = threadIdx.x; c < nv; c += ROW_THREADS) {
        oo[c] = o[c];
        no[c] = nx[c];
    }
}

template <int U> struct Widen;
template <> struct Widen<1> {
    typedef uint8_t In;
    typedef float Out;
    static __device__ __forceinline__ Out of(In v) { return (float)v; }
};
template <> struct Widen<2> {
    typedef uint16_t In;
    typedef float2 Out;
    static __device__ __forceinline__ Out of(In v) { return make_float2((float)(v & 0xff), (float)(v >> 8)); }
};
template <> struct Widen<4> {
    typedef uint32_t In;
    typedef float4 Out;
    static __device__ __forceinline__ Out of(In v) {
        return make_float4((float)(v & 0xff), (float)((v >> 8) & 0xff), (float)((v >> 16) & 0xff), (float)(v >> 24));
    }
};

// uint8 rows widened to float32 on the way out: U bytes loaded, U floats stored per lane (4 bytes -> one 16-byte store)
template <int U>
__global__ __launch_bounds__(ROW_THREADS) void k_replay_gather_f32(sl_replay buf, const long long *__restrict__ index,
                                                                   float *__restrict__ obs_out, float *__restrict__ next_out,
                                                                   long long *action_out, float *reward_out,
                                                                   float *done_out) {
    typedef typename Widen<U>::In In;
    typedef typename Widen<U>::Out Out;
    long long s;
    if (!gather_row(buf, index, action_out, reward_out, done_out, s)) return;
    const long long nv = buf.obs_bytes / U;
    const In *o = (const In *)buf.obs + s * nv, *nx = (const In *)buf.next_obs + s * nv;
    Out *oo = (Out *)obs_out + (long long)blockIdx.x * nv, *no = (Out *)next_out + (long long)blockIdx.x * nv;
    for (long long c = threadIdx.x; c < nv; c += ROW_THREADS) {
        oo[c] = Widen<U>::of(o[c]);
        no[c] = Widen<U>::of(nx[c]);
    }
}

__global__ __launch_bounds__(256) void k_sample_actions_eps(const float *__restrict__ qvals,
                                                            const uint8_t *__restrict__ active, int B, int A,
                                                            double epsilon, unsigned long long seed,
                                                            unsigned long long counter, int32_t *__restrict__ actions) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B) return;
    if (active && active[e] == 0) {                     // an agent that is gone: action 0, its Q-values are not read
        actions[e] = 0;
        return;
    }
    const unsigned long long z = draw_hash(seed, counter, (unsigned long long)e);
    const float u = draw_uniform24(z);
    int a;
    if ((double)u < epsilon) {
        a = (int)(((z & 0xFFFFFFFFull) * (unsigned long long)A) >> 32);
    } else {
        // np.argmax: the first maximum; a NaN counts as the maximum and the first NaN wins
        const float *q = qvals + (size_t)e * A;
        float best = q[0];
        a = 0;
        for (int k = 1; k < A && best == best; ++k) {
            const float v = q[k];
            if (v > best || v != v) {
                best = v;
                a = k;
            }
        }
    }
    actions[e] = a;
}

}  // namespace

hipError_t launch_replay_add(const sl_replay &buf, const void *obs, const int32_t *actions, const void *rewards,
                             const uint8_t *done, const void *next_obs, const uint8_t *active, hipStream_t stream) {
    hipLaunchKernelGGL(k_replay_plan, dim3(1), dim3(PLAN_THREADS), 0, stream, buf, done, active);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const dim3 grid((unsigned)buf.B), block(ROW_THREADS);
    with_row_type(row_align(buf.obs_bytes, {obs, next_obs, buf.obs, buf.next_obs, buf.win_obs}), [&](auto v) {
        typedef decltype(v) V;
        hipLaunchKernelGGL(k_replay_copy<V>, grid, block, 0, stream, buf, (const V *)obs, actions, rewards,
                           (const V *)next_obs);
    });
    return hipGetLastError();
}

hipError_t launch_replay_sample(const sl_replay &buf, int k, unsigned long long seed, unsigned long long counter,
                                long long *out_index, hipStream_t stream) {
    hipLaunchKernelGGL(k_replay_sample, dim3(1), dim3(PLAN_THREADS), 0, stream, buf, k, seed, counter, out_index);
    return hipGetLastError();
}

hipError_t launch_replay_gather(const sl_replay &buf, const long long *index, int k, void *obs_out, void *next_obs_out,
                                int obs_float32, long long *action_out, float *reward_out, float *done_out,
                                hipStream_t stream) {
    const dim3 grid((unsigned)k), block(ROW_THREADS);
    if (obs_float32) {
        // the float rows start at multiples of 4 * obs_bytes: U bytes in, U floats out, both aligned when U divides the
        // row size and the outputs are 16-byte aligned
        int a = row_align(buf.obs_bytes, {buf.obs, buf.next_obs});
        if (row_align(16, {obs_out, next_obs_out}) < 16) a = 1;
        const auto widen = [&](auto u) {
            hipLaunchKernelGGL(k_replay_gather_f32<(int)sizeof(u)>, grid, block, 0, stream, buf, index, (float *)obs_out,
                               (float *)next_obs_out, action_out, reward_out, done_out);
        };
        if (a >= 4) widen(uint32_t());
        else if (a == 2) widen(uint16_t());
        else widen(uint8_t());
        return hipGetLastError();
    }
    with_row_type(row_align(buf.obs_bytes, {buf.obs, buf.next_obs, obs_out, next_obs_out}), [&](auto v) {
        typedef decltype(v) V;
        hipLaunchKernelGGL(k_replay_gather<V>, grid, block, 0, stream, buf, index, (V *)obs_out, (V *)next_obs_out,
                           action_out, reward_out, done_out);
    });
    return hipGetLastError();
}

hipError_t launch_sample_actions_eps(const float *qvals, const uint8_t *active, int B, int A, double epsilon,
                                     unsigned long long seed, unsigned long long counter, int32_t *actions,
                                     hipStream_t stream) {
    hipLaunchKernelGGL(k_sample_actions_eps, dim3((B + 255) / 256), dim3(256), 0, stream, qvals, active, B, A, epsilon, seed,
                       counter, actions);
    return hipGetLastError();
}

}  // namespace sl
