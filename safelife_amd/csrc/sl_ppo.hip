// sl_ppo.hip -- the PPO minibatch update of the reference (training/ppo.py:145-182) on the device: the clipped loss of
// PPO.calculate_loss with its gradients, the observation rows of a minibatch, and the keys its row order is dealt from.
//
// The reference's expression, per row i of a minibatch of n rows (float32 tensors; eps_p, eps_v, vf, reg, clip are Python
// floats that meet them, so they act as their float32 roundings):
//     pd_i   = sign(A_i) * (1 - pi_i[a_i] / pi_old_i)            policy_i = |A_i| * max(pd_i, -eps_p)
//     vc_i   = v_old_i + clamp(v_i - v_old_i, -eps_v, +eps_v)    value_i  = max((vc_i - R_i)^2, (v_i - R_i)^2)
//     ent_i  = sum_k -pi_i[k] * log(pi_i[k] + 1e-12)
//     loss   = mean(policy) + vf * mean(value) - reg * min(mean(ent), clip)
// Every per-row operation is the reference's float32 operation in the reference's order: nothing is contracted into an
// FMA (the library is built with -ffp-contract=off and the pragma below says it again), `/` is IEEE division and logf is
// the device library's, not a fast approximation.  The three means are float64 sums of those float32 terms.
//
//   k_ppo_rows      one lane per row, PPO_THREADS rows per workgroup.  The [rows, A] tile of the policy is contiguous in
//                   memory: the lanes load it with consecutive 4-byte loads into LDS and then each walks its own row there
//                   (a row of 9 floats is 36 bytes; lanes reading their own rows from memory would touch 64 lines per load).
//                   LDS rows are A | 1 words apart, so the 32 lanes of a half wave sit on 32 banks.  The five per-row
//                   scalars come through rows[i]; a row id outside [0, N) or an action outside [0, A) raises its status
//                   bit, reads nothing through the bad value and contributes zero.  The workgroup's three sums go to the
//                   workspace: a butterfly over the wavefront, then the waves in order -- a fixed tree, no atomics.
//   k_ppo_finish    one workgroup: the partials through LDS, added in index order by one lane per quantity; the means,
//                   the entropy term, the total, the flag "the entropy bonus has a gradient" and n.
//   k_ppo_report_rows / k_ppo_report_finish   the report of PPO.train (training/ppo.py:199-205) over a batch too large for
//                   one model call: k_ppo_rows' per-row body and tree on one chunk of the batch at a time, five partials
//                   per workgroup (the three terms, old_values, advantages) at the workgroup's place in the whole batch,
//                   then one workgroup for the means -- the same bits however the batch was cut.  No gradient.
//   k_ppo_backward  one pass, the same tile: the gradients torch's autograd gives the expression above (a clamp passes
//                   the gradient at equality, a maximum halves it on a tie, sign(0) = 0, the bonus stops above the clip),
//                   recomputed from the inputs and the flag, written into the tile and stored from there with
//                   consecutive 4-byte stores.
//   k_minibatch_obs one wavefront per row, lanes stride over the row's elements (k_gather_obs of sl_rollout.hip with a
//                   status word and a bound of its own); k_minibatch_obs_f32 widens uint8 to float32 on the way.
//   k_minibatch_keys  key i = the splitmix64 mix of (seed, epoch, i): draw_hash, the one generator of the library.
#include "sl_kernels.h"
#include "sl_rows.h"

#pragma clang fp contract(off)

namespace sl {
namespace {

constexpr int PPO_THREADS = 256;
constexpr int PPO_WAVES = PPO_THREADS / 64;
constexpr int FINISH_CHUNK = 256;       // partial triples staged per round of k_ppo_finish
constexpr int OBS_THREADS = 256;

__device__ __forceinline__ int tile_stride(int A) { return A | 1; }

// the workgroup's rows of the [n, A] array -> LDS, consecutive lanes on consecutive words of memory
__device__ __forceinline__ void tile_load(const float *__restrict__ src, long long row0, int nrows, int A, float *tile) {
    const int S = tile_stride(A), total = nrows * A;
    const float *base = src + row0 * A;
    for (int j = threadIdx.x; j < total; j += PPO_THREADS) {
        const int r = j / A;
        tile[r * S + (j - r * A)] = base[j];
    }
}

__device__ __forceinline__ void tile_store(float *__restrict__ dst, long long row0, int nrows, int A, const float *tile) {
    const int S = tile_stride(A), total = nrows * A;
    float *base = dst + row0 * A;
    for (int j = threadIdx.x; j < total; j += PPO_THREADS) {
        const int r = j / A;
        base[j] = tile[r * S + (j - r * A)];
    }
}

// the batch row behind minibatch row i and its action; false (and the status bit) when either is out of range
__device__ __forceinline__ bool ppo_row(const sl_ppo_loss &p, long long i, long long &r, int &a) {
    r = p.rows ? p.rows[i] : i;
    if (r < 0 || r >= p.N) {
        atomicOr((unsigned long long *)p.status, (unsigned long long)SL_PPO_BAD_INDEX);
        return false;
    }
    const long long act = p.actions[r];
    if (act < 0 || act >= p.n_actions) {
        atomicOr((unsigned long long *)p.status, (unsigned long long)SL_PPO_BAD_ACTION);
        return false;
    }
    a = (int)act;
    return true;
}

__device__ __forceinline__ float sign_of(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

__device__ __forceinline__ double wave_sum(double x) {
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// The three float32 terms of minibatch row i (batch row r, action a, its policy row `pi` in LDS): the one per-row body of
// the loss pass and the report pass, so both give the same bits for the same row.
__device__ __forceinline__ void ppo_row_terms(const sl_ppo_loss &p, long long i, long long r, int a, const float *pi,
                                              float &pol, float &val, float &ent) {
    const int A = p.n_actions;
    for (int k = 0; k < A; ++k) {
        const float pk = pi[k];
        const float t = (-pk) * logf(pk + 1e-12f);
        ent = k ? ent + t : t;
    }
    const float adv = p.advantages[r], old_p = p.action_prob[r], old_v = p.old_values[r], ret = p.returns[r];
    const float v = p.values[i];
    const float lo = -(float)p.eps_policy, ev = (float)p.eps_value;
    const float pd = sign_of(adv) * (1.0f - pi[a] / old_p);
    pol = fabsf(adv) * (pd < lo ? lo : pd);
    const float dv = v - old_v;
    const float vc = old_v + (dv < -ev ? -ev : (dv > ev ? ev : dv));
    const float ea = vc - ret, eb = v - ret;
    const float sa = ea * ea, sb = eb * eb;
    val = (sa > sb || sa != sa) ? sa : sb;
}

// the workgroup's sum of Q quantities: a butterfly over the wavefront, then the waves in order; lane q < Q returns quantity q
template <int Q>
__device__ __forceinline__ double block_sums(const double (&x)[Q], double *wave_part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = 0; q < Q; ++q) {
        const double s = wave_sum(x[q]);
        if (lane == 0) wave_part[wave * Q + q] = s;
    }
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x < Q) {
        s = wave_part[threadIdx.x];
        for (int w = 1; w < PPO_WAVES; ++w) s += wave_part[w * Q + threadIdx.x];
    }
    return s;
}

__global__ __launch_bounds__(PPO_THREADS) void k_ppo_rows(sl_ppo_loss p, float *__restrict__ entropy_out,
                                                          double *__restrict__ partial) {
    extern __shared__ double lds[];
    double *wave_part = lds;                                // [PPO_WAVES][3]
    float *tile = (float *)(lds + PPO_WAVES * 3);
    const int A = p.n_actions, S = tile_stride(A);
    const long long row0 = (long long)blockIdx.x * PPO_THREADS;
    const int nrows = (int)(p.n - row0 < PPO_THREADS ? p.n - row0 : PPO_THREADS);
    tile_load(p.policy, row0, nrows, A, tile);
    __syncthreads();

    float pol = 0.f, val = 0.f, ent = 0.f;
    const long long i = row0 + threadIdx.x;
    if ((int)threadIdx.x < nrows) {
        long long r;
        int a;
        if (ppo_row(p, i, r, a)) ppo_row_terms(p, i, r, a, tile + threadIdx.x * S, pol, val, ent);
        entropy_out[i] = ent;
    }
    const double x[3] = {(double)pol, (double)val, (double)ent};
    const double s = block_sums<3>(x, wave_part);
    if (threadIdx.x < 3) partial[(long long)blockIdx.x * 3 + threadIdx.x] = s;
}

// The report pass: rows [first_row, first_row + p.n) of a batch of p.N rows, p.values and p.policy being the model's outputs
// for this chunk alone.  The same tile, the same per-row body and the same tree as k_ppo_rows, so a workgroup's first three
// partials are the ones k_ppo_rows writes for the same 256 rows; two more carry the float64 sums of old_values and
// advantages.  The workgroup's slot is its place in the WHOLE batch: however the batch is cut into chunks of a multiple of
// 256 rows, the workspace ends up holding the same numbers.
__global__ __launch_bounds__(PPO_THREADS) void k_ppo_report_rows(sl_ppo_loss p, long long first_row,
                                                                 double *__restrict__ partial) {
    extern __shared__ double lds[];
    double *wave_part = lds;                                // [PPO_WAVES][SL_PPO_REPORT_PARTIALS]
    float *tile = (float *)(lds + PPO_WAVES * SL_PPO_REPORT_PARTIALS);
    const int A = p.n_actions, S = tile_stride(A);
    const long long row0 = (long long)blockIdx.x * PPO_THREADS;
    const int nrows = (int)(p.n - row0 < PPO_THREADS ? p.n - row0 : PPO_THREADS);
    tile_load(p.policy, row0, nrows, A, tile);
    __syncthreads();

    float pol = 0.f, val = 0.f, ent = 0.f, old_v = 0.f, adv = 0.f;
    if ((int)threadIdx.x < nrows) {
        const long long i = row0 + threadIdx.x, r = first_row + i;      // (the launcher checked first_row + p.n <= p.N)
        const long long act = p.actions[r];
        if (act < 0 || act >= A) {
            atomicOr((unsigned long long *)p.status, (unsigned long long)SL_PPO_BAD_ACTION);
        } else {
            ppo_row_terms(p, i, r, (int)act, tile + threadIdx.x * S, pol, val, ent);
            old_v = p.old_values[r];
            adv = p.advantages[r];
        }
    }
    const double x[SL_PPO_REPORT_PARTIALS] = {(double)pol, (double)val, (double)ent, (double)old_v, (double)adv};
    const double s = block_sums<SL_PPO_REPORT_PARTIALS>(x, wave_part);
    if (threadIdx.x < SL_PPO_REPORT_PARTIALS)
        partial[(first_row / PPO_THREADS + blockIdx.x) * SL_PPO_REPORT_PARTIALS + threadIdx.x] = s;
}

// Q partials per workgroup, added in index order by lane q < Q -> total[q]; the workgroup is FINISH_CHUNK lanes
template <int Q>
__device__ __forceinline__ void sum_partials(const double *__restrict__ partial, long long blocks, double *stage,
                                             double *total) {
    double s = 0.0;
    for (long long b0 = 0; b0 < blocks; b0 += FINISH_CHUNK) {
        const int nb = (int)(blocks - b0 < FINISH_CHUNK ? blocks - b0 : FINISH_CHUNK);
        for (int j = threadIdx.x; j < nb * Q; j += FINISH_CHUNK) stage[j] = partial[b0 * Q + j];
        __syncthreads();
        if (threadIdx.x < Q)
            for (int b = 0; b < nb; ++b) s += stage[b * Q + threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x < Q) total[threadIdx.x] = s;
    __syncthreads();
}

// the means over n rows, the entropy term, the total, the flag and n -> the first seven doubles of `out`; returns the total
__device__ __forceinline__ double ppo_totals(const sl_ppo_loss &p, double n, const double *total, double *__restrict__ out) {
    const double pm = total[0] / n, vm = total[1] / n, em = total[2] / n;
    const double clip = (double)(float)p.entropy_clip;
    const bool open = (float)em <= (float)p.entropy_clip;       // the comparison the reference makes in float32
    const double term = -(double)(float)p.entropy_reg * (open ? em : clip);
    const double loss = pm + (double)(float)p.vf_coef * vm + term;
    out[SL_PPO_SUM_POLICY] = pm;
    out[SL_PPO_SUM_VALUE] = vm;
    out[SL_PPO_SUM_ENTROPY] = em;
    out[SL_PPO_SUM_ENTROPY_TERM] = term;
    out[SL_PPO_SUM_LOSS] = loss;
    out[SL_PPO_SUM_FLAG] = open ? 1.0 : 0.0;
    out[SL_PPO_SUM_N] = n;
    return loss;
}

__global__ __launch_bounds__(FINISH_CHUNK) void k_ppo_finish(sl_ppo_loss p, const double *__restrict__ partial,
                                                            long long blocks, double *__restrict__ sums_out) {
    __shared__ double stage[FINISH_CHUNK * 3];
    __shared__ double total[3];
    sum_partials<3>(partial, blocks, stage, total);
    if (threadIdx.x == 0) {
        const double loss = ppo_totals(p, (double)p.n, total, sums_out);
        float *f = (float *)(sums_out + SL_PPO_SUM_LOSS_F32);     // the total as float32 in the slot's first four bytes
        f[0] = (float)loss;
        f[1] = 0.f;
    }
}

// the report's finish: the divisor is the BATCH's row count
__global__ __launch_bounds__(FINISH_CHUNK) void k_ppo_report_finish(sl_ppo_loss p, const double *__restrict__ partial,
                                                                   long long blocks, double *__restrict__ out) {
    __shared__ double stage[FINISH_CHUNK * SL_PPO_REPORT_PARTIALS];
    __shared__ double total[SL_PPO_REPORT_PARTIALS];
    sum_partials<SL_PPO_REPORT_PARTIALS>(partial, blocks, stage, total);
    if (threadIdx.x == 0) {
        const double n = (double)p.N;
        const double loss = ppo_totals(p, n, total, out);
        const double values = total[3] / n, advantages = total[4] / n;
        out[SL_PPO_REPORT_VALUES] = values;
        out[SL_PPO_REPORT_ADVANTAGES] = advantages;
        float *f = (float *)(out + SL_PPO_REPORT_F32);            // what the reference logs, in the precision it logs it
        f[SL_PPO_REPORT_F32_LOSS] = (float)loss;
        f[SL_PPO_REPORT_F32_ENTROPY] = (float)(total[2] / n);
        f[SL_PPO_REPORT_F32_VALUES] = (float)values;
        f[SL_PPO_REPORT_F32_ADVANTAGES] = (float)advantages;
    }
}

__global__ __launch_bounds__(PPO_THREADS) void k_ppo_backward(sl_ppo_loss p, const float *__restrict__ grad_loss,
                                                              const float *__restrict__ grad_entropy,
                                                              const double *__restrict__ sums, float *__restrict__ d_values,
                                                              float *__restrict__ d_policy) {
    extern __shared__ double lds[];
    float *tile = (float *)lds;
    const int A = p.n_actions, S = tile_stride(A);
    const long long row0 = (long long)blockIdx.x * PPO_THREADS;
    const int nrows = (int)(p.n - row0 < PPO_THREADS ? p.n - row0 : PPO_THREADS);
    tile_load(p.policy, row0, nrows, A, tile);
    __syncthreads();

    const long long i = row0 + threadIdx.x;
    if ((int)threadIdx.x < nrows) {
        float *pi = tile + threadIdx.x * S;
        long long r;
        int a;
        float dval = 0.f;
        if (ppo_row(p, i, r, a)) {
            // what reaches the three means: mean's backward divides by n, the in-place `*= -reg` and `* vf` multiply first
            const float g = *grad_loss, nf = (float)p.n;
            const float gp = g / nf;
            const float gv = (g * (float)p.vf_coef) / nf;
            float ge = sums[SL_PPO_SUM_FLAG] != 0.0 ? (g * -(float)p.entropy_reg) / nf : 0.f;
            if (grad_entropy) ge += grad_entropy[i];
            const float adv = p.advantages[r], old_p = p.action_prob[r], old_v = p.old_values[r], ret = p.returns[r];
            const float v = p.values[i];
            const float lo = -(float)p.eps_policy, ev = (float)p.eps_value;
            // policy: |A| * clamp(s * (1 - pi_a / old), min = lo)
            const float sg = sign_of(adv);
            const float pa = pi[a];
            const float pd = sg * (1.0f - pa / old_p);
            float t = gp * fabsf(adv);
            if (pd < lo) t = 0.f;
            const float dpa = (-(t * sg)) / old_p;
            // value: max(sa, sb), sa = (old + clamp(v - old) - R)^2, sb = (v - R)^2
            const float dv = v - old_v;
            const bool inside = dv >= -ev && dv <= ev;
            const float vc = old_v + (dv < -ev ? -ev : (dv > ev ? ev : dv));
            const float ea = vc - ret, eb = v - ret;
            const float sa = ea * ea, sb = eb * eb;
            const float ga = sa > sb ? gv : (sa == sb ? gv * 0.5f : 0.f);
            const float gb = sb > sa ? gv : (sa == sb ? gv * 0.5f : 0.f);
            const float da = inside ? ga * (2.0f * ea) : 0.f;
            dval = da + gb * (2.0f * eb);
            // entropy: sum_k (-p_k) * log(p_k + 1e-12)
            for (int k = 0; k < A; ++k) {
                const float pk = pi[k];
                const float x = pk + 1e-12f;
                const float L = logf(x);
                pi[k] = (-(ge * L)) + (ge * (-pk)) / x;
            }
            pi[a] += dpa;
        } else {
            for (int k = 0; k < A; ++k) pi[k] = 0.f;
        }
        d_values[i] = dval;
    }
    __syncthreads();
    tile_store(d_policy, row0, nrows, A, tile);
}

// one wavefront per minibatch row: lanes stride over the row's elements of type V
template <typename V>
__global__ __launch_bounds__(OBS_THREADS) void k_minibatch_obs(const long long *__restrict__ rows, long long n, long long N,
                                                               const V *__restrict__ obs, long long nv, V *__restrict__ out,
                                                               long long *status) {
    const long long i = (long long)blockIdx.x * (OBS_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    const long long r = rows[i];
    if (r < 0 || r >= N) {
        if ((threadIdx.x & 63) == 0) atomicOr((unsigned long long *)status, (unsigned long long)SL_PPO_BAD_INDEX);
        return;
    }
    const V *src = obs + r * nv;
    V *dst = out + i * nv;
    for (long long c = threadIdx.x & 63; c < nv; c += 64) dst[c] = src[c];
}

// U bytes in one load -> U floats in one store (the rule of sl_replay.hip's gather, which keeps its own copy: that file
// is not touched by this one)
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

// uint8 rows widened to float32 on the way: U bytes loaded, U floats stored per lane
template <int U>
__global__ __launch_bounds__(OBS_THREADS) void k_minibatch_obs_f32(const long long *__restrict__ rows, long long n, long long N,
                                                                   const uint8_t *__restrict__ obs, long long obs_bytes,
                                                                   float *__restrict__ out, long long *status) {
    typedef typename Widen<U>::In In;
    typedef typename Widen<U>::Out Out;
    const long long i = (long long)blockIdx.x * (OBS_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    const long long r = rows[i];
    if (r < 0 || r >= N) {
        if ((threadIdx.x & 63) == 0) atomicOr((unsigned long long *)status, (unsigned long long)SL_PPO_BAD_INDEX);
        return;
    }
    const long long nv = obs_bytes / U;
    const In *src = (const In *)(obs + r * obs_bytes);
    Out *dst = (Out *)(out + i * obs_bytes);
    for (long long c = threadIdx.x & 63; c < nv; c += 64) dst[c] = Widen<U>::of(src[c]);
}

__global__ __launch_bounds__(256) void k_minibatch_keys(long long N, unsigned long long seed, unsigned long long epoch,
                                                        unsigned long long *__restrict__ keys) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < N) keys[i] = draw_hash(seed, epoch, (unsigned long long)i);
}

inline unsigned ppo_blocks(long long n) { return (unsigned)((n + PPO_THREADS - 1) / PPO_THREADS); }
inline size_t tile_bytes(int A) { return (size_t)PPO_THREADS * (A | 1) * sizeof(float); }

}  // namespace

size_t ppo_workspace_bytes(long long n) { return (size_t)ppo_blocks(n) * 3 * sizeof(double); }

hipError_t launch_ppo_loss_forward(const sl_ppo_loss &p, float *entropy_out, double *sums_out, void *workspace,
                                   hipStream_t stream) {
    const unsigned blocks = ppo_blocks(p.n);
    const size_t lds = PPO_WAVES * 3 * sizeof(double) + tile_bytes(p.n_actions);
    hipLaunchKernelGGL(k_ppo_rows, dim3(blocks), dim3(PPO_THREADS), lds, stream, p, entropy_out, (double *)workspace);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_ppo_finish, dim3(1), dim3(FINISH_CHUNK), 0, stream, p, (const double *)workspace, (long long)blocks,
                       sums_out);
    return hipGetLastError();
}

size_t ppo_report_workspace_bytes(long long N) { return (size_t)ppo_blocks(N) * SL_PPO_REPORT_PARTIALS * sizeof(double); }

hipError_t launch_ppo_report_rows(const sl_ppo_loss &p, long long first_row, double *partial, hipStream_t stream) {
    const size_t lds = PPO_WAVES * SL_PPO_REPORT_PARTIALS * sizeof(double) + tile_bytes(p.n_actions);
    hipLaunchKernelGGL(k_ppo_report_rows, dim3(ppo_blocks(p.n)), dim3(PPO_THREADS), lds, stream, p, first_row, partial);
    return hipGetLastError();
}

hipError_t launch_ppo_report_finish(const sl_ppo_loss &p, const double *partial, long long blocks, double *out,
                                    hipStream_t stream) {
    hipLaunchKernelGGL(k_ppo_report_finish, dim3(1), dim3(FINISH_CHUNK), 0, stream, p, partial, blocks, out);
    return hipGetLastError();
}

hipError_t launch_ppo_loss_backward(const sl_ppo_loss &p, const float *grad_loss, const float *grad_entropy,
                                    const double *sums, float *d_values, float *d_policy, hipStream_t stream) {
    hipLaunchKernelGGL(k_ppo_backward, dim3(ppo_blocks(p.n)), dim3(PPO_THREADS), tile_bytes(p.n_actions), stream, p, grad_loss,
                       grad_entropy, sums, d_values, d_policy);
    return hipGetLastError();
}

hipError_t launch_minibatch_obs(const void *obs, long long obs_bytes, long long N, const long long *rows, long long n,
                                void *out, int out_float32, long long *status, hipStream_t stream) {
    const int rows_per_block = OBS_THREADS / 64;
    const dim3 grid((unsigned)((n + rows_per_block - 1) / rows_per_block)), block(OBS_THREADS);
    if (out_float32) {
        // the float rows start at multiples of 4 * obs_bytes: U bytes in, U floats out, both aligned when U divides the
        // row size and the output is 16-byte aligned
        int a = row_align(obs_bytes, {obs});
        if (row_align(16, {out}) < 16) a = 1;
        const auto widen = [&](auto u) {
            hipLaunchKernelGGL(k_minibatch_obs_f32<(int)sizeof(u)>, grid, block, 0, stream, rows, n, N, (const uint8_t *)obs,
                               obs_bytes, (float *)out, status);
        };
        if (a >= 4) widen(uint32_t());
        else if (a == 2) widen(uint16_t());
        else widen(uint8_t());
        return hipGetLastError();
    }
    with_row_type(row_align(obs_bytes, {obs, out}), [&](auto v) {
        typedef decltype(v) V;
        hipLaunchKernelGGL(k_minibatch_obs<V>, grid, block, 0, stream, rows, n, N, (const V *)obs,
                           obs_bytes / (long long)sizeof(V), (V *)out, status);
    });
    return hipGetLastError();
}

hipError_t launch_minibatch_keys(long long N, unsigned long long seed, unsigned long long epoch, unsigned long long *keys,
                                 hipStream_t stream) {
    hipLaunchKernelGGL(k_minibatch_keys, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, N, seed, epoch, keys);
    return hipGetLastError();
}

}  // namespace sl
