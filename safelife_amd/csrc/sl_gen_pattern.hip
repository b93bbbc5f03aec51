// sl_gen_pattern.hip -- batched pattern generation: N independent Metropolis chains (the sampler that grows still lifes and
// oscillators into the masked part of a board), one WAVEFRONT per chain, all chains of a launch sharing (rows, cols, depth).
//
// One chain is sequential -- every iteration samples a cell, prices up to 3 * (2 depth + 1)^2 candidate swaps around it, draws
// one and applies it, and the next iteration sees the result -- so a launch gets its width from the number of chains, not from
// inside one.  A chain's state (layers, neighbour counts, violations, oscillation bits, the mask, three index sets, the
// candidates' table: sl_gen_pattern_core.h has the layout) sits in LDS, 12 KiB at 26x26 with one layer, so a CU holds a dozen
// chains; a shape whose state is over 64 KiB (above 60x60 with one layer, 48x48 with four) uses a slice of a global workspace
// through the same code.
//
//   depth 1   the wavefront works together: lane 0 samples the cell and prices the cell types, 27 lanes evaluate the 27
//             candidates side by side from the base state (with one layer a candidate's delta is a function of the 3x3 it
//             reaches, nothing is written: core.h says why that is exact), lane 0 sums, draws, picks and applies.  Two
//             workgroup barriers per iteration, one wavefront wide.
//   depth 2-4 a change runs through the later layers over an area that grows while it is walked and wraps on narrow boards;
//             the swaps and swap-backs also leave their mark in the stored violations.  Lane 0 walks the candidates one after
//             the other exactly as the sampler does; the other lanes help with set-up and with the copy out only.
//
// Bit-exact with the sampler: board, status, iteration count and the generator's six words.  The arithmetic is IEEE double with
// no fusion; exp() is the one call whose last bit may differ from a host libm's, which can change a pick only when the draw
// lands within a few ulps of a cumulative probability.
//
// Bounds: every index into the state is formed by idx3() (wrapped into the layer) or comes out of an index set (values below
// `layer`); slots of the candidates' table are below `cand`; a problem touches its own slices of the inputs and outputs only.
#include "sl_kernels.h"
#include "sl_gen_pattern_core.h"

#pragma clang fp contract(off)

namespace sl {
namespace {

struct GenPatternArgs {
    const uint16_t *layers;     // [N][depth][layer]
    const int32_t *mask;        // [N][layer]
    const int32_t *seeds;       // [N][layer] or null (the mask stands in)
    const double *params;       // [N][N_PARAMS]
    gp::u64 *rng;               // [N][6], advanced in place
    uint16_t *out_board;        // [N][layer]
    int32_t *status;            // [N]
    int32_t *iterations;        // [N]
    unsigned char *workspace;   // [N][layout.bytes] when the state is not in LDS
    gp::Layout layout;
};

template <bool IN_LDS>
__global__ __launch_bounds__(gp::WAVE) void k_gen_pattern(GenPatternArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gp_lds[];
    const int p = blockIdx.x, lane = threadIdx.x;
    const gp::Layout &l = a.layout;
    unsigned char *base = IN_LDS ? gp_lds : a.workspace + (size_t)p * l.bytes;
    const gp::View v = gp::make_view(base, l);
    const size_t cell0 = (size_t)p * l.layer;
    const uint16_t *layers = a.layers + cell0 * l.depth;
    const int32_t *mask = a.mask + cell0;
    const int32_t *seeds = a.seeds ? a.seeds + cell0 : nullptr;
    const double *params = a.params + (size_t)p * gp::N_PARAMS;

    gp::Chain ch = {};
    gp::init_copy(v, layers, mask, lane, gp::WAVE);
    __syncthreads();
    gp::init_counts(v, lane, gp::WAVE);
    __syncthreads();
    if (lane == 0) gp::init_sets(v, ch, mask, seeds, params, a.rng + (size_t)p * gp::N_RNG_WORDS);

    if (l.depth == 1) {
        for (;;) {
            if (lane == 0) gp::iter_head(v, ch, params);
            __syncthreads();
            if (v.ctrl->done) break;                    // the same word for every lane: the branch is uniform
            if (lane < 27) gp::candidate_depth1(v, lane);
            __syncthreads();
            if (lane == 0) gp::iter_tail(v, ch, gp::compact_depth1(v));
        }
    } else {
        if (lane == 0) {
            for (;;) {
                gp::iter_head(v, ch, params);
                if (v.ctrl->done) break;
                gp::iter_tail(v, ch, gp::candidates_serial(v));
            }
        }
        __syncthreads();
    }

    // the new layer 0, or the board as it came where the run failed
    const int status = __shfl(lane == 0 ? gp::chain_status(ch) : 0, 0);
    const uint16_t *src = status == gp::STATUS_OK ? v.board : layers;
    for (int i = lane; i < l.layer; i += gp::WAVE) a.out_board[cell0 + i] = src[i];
    if (lane == 0) {
        gp::u64 *w = a.rng + (size_t)p * gp::N_RNG_WORDS;
        w[0] = ch.rng.hi; w[1] = ch.rng.lo; w[2] = ch.rng.inc_hi; w[3] = ch.rng.inc_lo;
        w[4] = ch.rng.has_uint32; w[5] = ch.rng.uinteger;
        a.status[p] = status;
        a.iterations[p] = ch.it;
    }
}

}  // namespace

size_t gen_pattern_workspace_bytes(int n, int rows, int cols, int depth) { return gp::workspace_bytes(n, rows, cols, depth); }

hipError_t launch_gen_pattern(const uint16_t *layers, const int32_t *mask, const int32_t *seeds, const double *params,
                              unsigned long long *rng, uint16_t *out_board, int32_t *status, int32_t *iterations, int n,
                              int rows, int cols, int depth, void *workspace, hipStream_t stream) {
    GenPatternArgs a;
    a.layers = layers; a.mask = mask; a.seeds = seeds; a.params = params; a.rng = rng;
    a.out_board = out_board; a.status = status; a.iterations = iterations;
    a.workspace = (unsigned char *)workspace;
    a.layout = gp::make_layout(rows, cols, depth);
    if (a.layout.bytes <= gp::LDS_LIMIT)
        hipLaunchKernelGGL(k_gen_pattern<true>, dim3(n), dim3(gp::WAVE), a.layout.bytes, stream, a);
    else
        hipLaunchKernelGGL(k_gen_pattern<false>, dim3(n), dim3(gp::WAVE), 0, stream, a);
    return hipGetLastError();
}

}  // namespace sl
