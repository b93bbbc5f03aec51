// sl_dqn.hip -- the DQN update of the reference (training/dqn.py:136-175) on the device: the TD loss of DQN.optimize after its
// two model calls, the four scalars it reports, and the gradient of the loss.
//
// The reference's expression, per row i of a minibatch of n rows (float32 tensors; gamma ** multi_step is a Python float that
// meets them, so it acts as its float32 rounding):
//     q_i    = q_values[i][a_i]                                    m_i   = max_k next_q_values[i][k]
//     exp_i  = reward_i + (gamma ** multi_step * (1 - done_i)) * m_i
//     td_i   = q_i - exp_i                                         loss  = mean(td ** 2)
// Every per-row operation is the reference's float32 operation in the reference's order: nothing is contracted into an FMA
// (the library is built with -ffp-contract=off, the pragma below says it again and the arithmetic is written with the
// round-to-nearest intrinsics).  The five means are float64 sums of float32 terms.
//
//   k_dqn_rows      one lane per row, DQN_THREADS rows per workgroup.  The [rows, A] tile of q_values, then that of
//                   next_q_values, goes through ONE LDS tile (two tiles of 32 actions would not fit 64 KB): consecutive
//                   lanes load consecutive words of memory, then each lane walks its own row there; LDS rows are A | 1
//                   words apart.  The three per-row scalars come through index[i], in the ring's storage types or in a
//                   gathered batch's; an index outside [0, N) or an action outside [0, A) raises its status bit, reads
//                   nothing through the bad value and contributes zero.  The workgroup's five sums: a butterfly over the
//                   wavefront, then the waves in order -- a fixed tree, no atomics.  A grid of one workgroup finishes its own
//                   sums (the same additions k_dqn_finish would make: 0 + the one partial), otherwise they go to the
//                   workspace.
//   k_dqn_finish    one workgroup: the partials through LDS, added in index order by one lane per quantity; the means.
//   k_dqn_backward  one lane per ELEMENT of d_q, consecutive 4-byte stores: (g / n) * (2 * td_i) (+ grad_td[i]) in the
//                   column of the action taken, zero elsewhere.
#include "sl_kernels.h"

#pragma clang fp contract(off)

namespace sl {
namespace {

constexpr int DQN_THREADS = 256;
constexpr int DQN_WAVES = DQN_THREADS / 64;
constexpr int DQN_PARTS = 5;            // td^2, q elements, q row maxima, next_q elements, m
constexpr int FINISH_CHUNK = 256;       // partial quintuples staged per round of k_dqn_finish

__host__ __device__ __forceinline__ int tile_stride(int A) { return A | 1; }

// the workgroup's rows of the [n, A] array -> LDS, consecutive lanes on consecutive words of memory
__device__ __forceinline__ void tile_load(const float *__restrict__ src, long long row0, int nrows, int A, float *tile) {
    const int S = tile_stride(A), total = nrows * A;
    const float *base = src + row0 * A;
    for (int j = threadIdx.x; j < total; j += DQN_THREADS) {
        const int r = j / A;
        tile[r * S + (j - r * A)] = base[j];
    }
}

// the source row behind minibatch row i and its action; false (and the status bit) when either is out of range
__device__ __forceinline__ bool dqn_row(const sl_dqn_loss &p, long long i, long long &r, int &a) {
    r = p.index ? p.index[i] : i;
    if (r < 0 || r >= p.N) {
        atomicOr((unsigned long long *)p.status, (unsigned long long)SL_DQN_BAD_INDEX);
        return false;
    }
    const long long act = p.source == SL_DQN_FROM_RING ? (long long)((const int32_t *)p.action)[r]
                                                       : ((const long long *)p.action)[r];
    if (act < 0 || act >= p.n_actions) {
        atomicOr((unsigned long long *)p.status, (unsigned long long)SL_DQN_BAD_ACTION);
        return false;
    }
    a = (int)act;
    return true;
}

// a row's maximum as torch.max gives it (NaN once any element is NaN) and the float64 sum of its elements in index order
__device__ __forceinline__ void row_max_sum(const float *row, int A, float &mx, double &sum) {
    mx = row[0];
    sum = (double)row[0];
    for (int k = 1; k < A; ++k) {
        const float v = row[k];
        if (v > mx || v != v) mx = v;
        sum += (double)v;
    }
}

__device__ __forceinline__ double wave_sum(double x) {
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

__device__ __forceinline__ void write_sums(const sl_dqn_loss &p, const double *total, double *__restrict__ sums_out) {
    const double n = (double)p.n, cells = n * (double)p.n_actions;
    const double loss = total[0] / n;
    sums_out[SL_DQN_SUM_LOSS] = loss;
    sums_out[SL_DQN_SUM_Q_MODEL_MEAN] = total[1] / cells;
    sums_out[SL_DQN_SUM_Q_MODEL_MAX] = total[2] / n;
    sums_out[SL_DQN_SUM_Q_TARGET_MEAN] = total[3] / cells;
    sums_out[SL_DQN_SUM_Q_TARGET_MAX] = total[4] / n;
    sums_out[SL_DQN_SUM_N] = n;
    sums_out[SL_DQN_SUM_RESERVED] = 0.0;
    float *f = (float *)(sums_out + SL_DQN_SUM_LOSS_F32);       // the loss as float32 in the slot's first four bytes
    f[0] = (float)loss;
    f[1] = 0.f;
}

__global__ __launch_bounds__(DQN_THREADS) void k_dqn_rows(sl_dqn_loss p, float *__restrict__ td_out,
                                                          double *__restrict__ partial, double *__restrict__ sums_out) {
    extern __shared__ double lds[];
    double *wave_part = lds;                                // [DQN_WAVES][DQN_PARTS]
    double *total = lds + DQN_WAVES * DQN_PARTS;            // [DQN_PARTS]
    float *tile = (float *)(total + DQN_PARTS + 1);
    const int A = p.n_actions, S = tile_stride(A);
    const long long row0 = (long long)blockIdx.x * DQN_THREADS;
    const int nrows = (int)(p.n - row0 < DQN_THREADS ? p.n - row0 : DQN_THREADS);
    const long long i = row0 + threadIdx.x;
    const bool mine = (int)threadIdx.x < nrows;
    const float *row = tile + threadIdx.x * S;

    tile_load(p.q_values, row0, nrows, A, tile);
    long long r = 0;
    int a = 0;
    const bool good = mine && dqn_row(p, i, r, a);
    float rew = 0.f, done = 0.f;
    if (good) {
        if (p.source == SL_DQN_FROM_RING) {
            rew = (float)((const double *)p.reward)[r];     // the float64 n-step sum, rounded once
            done = (float)((const uint8_t *)p.done)[r];
        } else {
            rew = ((const float *)p.reward)[r];
            done = ((const float *)p.done)[r];
        }
    }
    __syncthreads();
    float q_taken = 0.f, q_max = 0.f;
    double q_sum = 0.0;
    if (mine) {
        row_max_sum(row, A, q_max, q_sum);
        if (good) q_taken = row[a];
    }
    __syncthreads();
    tile_load(p.next_q_values, row0, nrows, A, tile);
    __syncthreads();
    float m = 0.f, sq = 0.f;
    double next_sum = 0.0;
    if (mine) {
        row_max_sum(row, A, m, next_sum);
        float td = 0.f;
        if (good) {
            const float nd = __fsub_rn(1.0f, done);
            const float disc = __fmul_rn((float)p.discount, nd);
            const float expected = __fadd_rn(rew, __fmul_rn(disc, m));
            td = __fsub_rn(q_taken, expected);
            sq = __fmul_rn(td, td);
        } else {
            m = 0.f;                                        // a bad row's maximum is left out of q_target_max
        }
        td_out[i] = td;
    }
    const double s[DQN_PARTS] = {wave_sum((double)sq), wave_sum(q_sum), wave_sum((double)q_max), wave_sum(next_sum),
                                 wave_sum((double)m)};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int k = 0; k < DQN_PARTS; ++k) wave_part[wave * DQN_PARTS + k] = s[k];
    __syncthreads();
    if (threadIdx.x < DQN_PARTS) {
        double t = wave_part[threadIdx.x];
        for (int w = 1; w < DQN_WAVES; ++w) t += wave_part[w * DQN_PARTS + threadIdx.x];
        if (gridDim.x == 1) total[threadIdx.x] = 0.0 + t;   // what k_dqn_finish computes from one partial
        else partial[(long long)blockIdx.x * DQN_PARTS + threadIdx.x] = t;
    }
    if (gridDim.x == 1) {
        __syncthreads();
        if (threadIdx.x == 0) write_sums(p, total, sums_out);
    }
}

__global__ __launch_bounds__(FINISH_CHUNK) void k_dqn_finish(sl_dqn_loss p, const double *__restrict__ partial,
                                                            long long blocks, double *__restrict__ sums_out) {
    __shared__ double stage[FINISH_CHUNK * DQN_PARTS];
    __shared__ double total[DQN_PARTS];
    double s = 0.0;
    for (long long b0 = 0; b0 < blocks; b0 += FINISH_CHUNK) {
        const int nb = (int)(blocks - b0 < FINISH_CHUNK ? blocks - b0 : FINISH_CHUNK);
        for (int j = threadIdx.x; j < nb * DQN_PARTS; j += FINISH_CHUNK) stage[j] = partial[b0 * DQN_PARTS + j];
        __syncthreads();
        if (threadIdx.x < DQN_PARTS)
            for (int b = 0; b < nb; ++b) s += stage[b * DQN_PARTS + threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x < DQN_PARTS) total[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) write_sums(p, total, sums_out);
}

__global__ __launch_bounds__(DQN_THREADS) void k_dqn_backward(sl_dqn_loss p, const float *__restrict__ grad_loss,
                                                              const float *__restrict__ grad_td, const float *__restrict__ td,
                                                              float *__restrict__ d_q) {
    const long long j = (long long)blockIdx.x * DQN_THREADS + threadIdx.x;
    const int A = p.n_actions;
    if (j >= p.n * A) return;
    const long long i = j / A;
    const int k = (int)(j - i * A);
    long long r;
    int a;
    float d = 0.f;
    if (dqn_row(p, i, r, a) && a == k) {
        // mean's backward divides by n, pow's multiplies by 2 * td, gather's scatters
        d = __fmul_rn(__fdiv_rn(*grad_loss, (float)p.n), __fmul_rn(2.0f, td[i]));
        if (grad_td) d = __fadd_rn(d, grad_td[i]);
    }
    d_q[j] = d;
}

inline unsigned dqn_blocks(long long n) { return (unsigned)((n + DQN_THREADS - 1) / DQN_THREADS); }

}  // namespace

size_t dqn_workspace_bytes(long long n) { return (size_t)dqn_blocks(n) * DQN_PARTS * sizeof(double); }

hipError_t launch_dqn_loss_forward(const sl_dqn_loss &p, float *td_out, double *sums_out, void *workspace,
                                   hipStream_t stream) {
    const unsigned blocks = dqn_blocks(p.n);
    const size_t lds = (DQN_WAVES * DQN_PARTS + DQN_PARTS + 1) * sizeof(double) +
                       (size_t)DQN_THREADS * tile_stride(p.n_actions) * sizeof(float);
    hipLaunchKernelGGL(k_dqn_rows, dim3(blocks), dim3(DQN_THREADS), lds, stream, p, td_out, (double *)workspace, sums_out);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || blocks == 1) return err;
    hipLaunchKernelGGL(k_dqn_finish, dim3(1), dim3(FINISH_CHUNK), 0, stream, p, (const double *)workspace, (long long)blocks,
                       sums_out);
    return hipGetLastError();
}

hipError_t launch_dqn_loss_backward(const sl_dqn_loss &p, const float *grad_loss, const float *grad_td, const float *td,
                                    float *d_q, hipStream_t stream) {
    const long long cells = p.n * p.n_actions;
    hipLaunchKernelGGL(k_dqn_backward, dim3((unsigned)((cells + DQN_THREADS - 1) / DQN_THREADS)), dim3(DQN_THREADS), 0, stream,
                       p, grad_loss, grad_td, td, d_q);
    return hipGetLastError();
}

}  // namespace sl
