// sl_partition.hip -- batched region partition of the level generator: N independent partitions (proc_gen.partition: seeded
// regions that grow one cell per turn, never within two cells of each other), one WAVEFRONT per partition, all partitions of a
// launch sharing (rows, cols).
//
// One partition is sequential -- a turn draws a region and a cell of its frontier, looks at the 5x5 around the cell, and the
// next turn sees the result -- so a launch gets its width from the number of partitions.  A partition's state (labels, one
// bitmap and one frontier per region: sl_partition_core.h has the layout) sits in LDS, 4.5 KiB at 26x26 with room for three
// regions, so a CU holds dozens; 64x64 with room for eight regions is over 64 KiB and uses a slice of a global workspace
// through the same code.
//
//   seeding   per region, the lanes test 64 cells at a time for "free" (25 looks each); one ballot per chunk is the chunk's
//             word of the free cells' bitmap, its population counts add up to the number the draw is bounded by, and lane 0
//             finds the j-th set bit: the free list in ascending cell order, never written out.
//   turns     lane 0 draws the region and the cell and pops it; 25 lanes look at the wrapped 5x5 side by side, one ballot
//             says "blocked"; lane 0 labels the cell and pushes its neighbours.  One workgroup barrier per turn, one wavefront
//             wide.
//
// Bit-exact with proc_gen.partition on a numpy Generator(PCG64) set to the same words: labels and the six words afterwards.
// No loop is unbounded: the turns are capped at regions * cells + 1 (a cell enters a region's frontier at most once) and a
// bounded draw at 64 redraws; either cap ends the problem with status -5, its labels and words untouched.
//
// Bounds: every index into the state is a cell index below `cells` -- formed by wrap() from a cell's row and column, read from
// a frontier (which holds only such), or found in a bitmap of ceil(cells / 64) words and checked; region indices are below
// the number drawn, which is within the layout's `regions`; a problem touches its own slices of the inputs and outputs only.
#include "sl_kernels.h"
#include "sl_partition_core.h"

#pragma clang fp contract(off)

namespace sl {
namespace {

struct PartitionArgs {
    pt::u64 *rng;               // [N][6], advanced in place where status is 0
    const int32_t *min_regions; // [N]
    const int32_t *max_regions; // [N]
    int16_t *labels;            // [N][cells], written where status is 0
    int32_t *status;            // [N]
    unsigned char *workspace;   // [N][layout.bytes] when the state is not in LDS
    pt::Layout layout;
    int shape_ok;
};

template <bool IN_LDS>
__global__ __launch_bounds__(pt::WAVE) void k_partition(PartitionArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pt_lds[];
    const int p = blockIdx.x, lane = threadIdx.x;
    const pt::Layout &l = a.layout;
    int lo, hi;
    pt::clamp_bounds(a.min_regions[p], a.max_regions[p], lo, hi);
    if (!a.shape_ok || hi > l.regions) {                // the same for every lane; nothing drawn, nothing written but this
        if (lane == 0) a.status[p] = pt::STATUS_REFUSED;
        return;
    }
    unsigned char *base = IN_LDS ? pt_lds : a.workspace + (size_t)p * l.bytes;
    const pt::View v = pt::make_view(base, l);
    pt::u64 *words = a.rng + (size_t)p * pt::N_RNG_WORDS;

    pt::Run run = {};
    pt::init_clear(v, l.regions, lane, pt::WAVE);
    if (lane == 0) pt::begin(v, run, words, lo, hi);
    __syncthreads();

    // seeding: region k's free cells as a bitmap, 64 cells a ballot
    const int want = v.ctrl->done ? 0 : v.ctrl->want;
    for (int k = 1; k <= want; k++) {
        int count = 0;
        for (int chunk = 0; chunk < v.words; chunk++) {
            const int cell = chunk * pt::WAVE + lane;
            const pt::u64 free = __ballot(cell < v.cells && pt::seed_free(v, cell, k));
            if (lane == 0) v.queued[(size_t)(k - 1) * v.words + chunk] = free;
            count += __popcll(free);
        }
        if (!count) break;                              // no free seed cell is left: fewer regions than drawn
        if (lane == 0) pt::seed_take(v, run, k, count);
        __syncthreads();
        if (v.ctrl->done) break;
    }

    // turns
    for (;;) {
        if (lane == 0) pt::turn_head(v, run);
        __syncthreads();
        if (v.ctrl->done) break;                        // the same word for every lane: the branch is uniform
        const int cell = v.ctrl->cell, k = v.ctrl->k;
        const int r = cell / v.cols, c = cell - r * v.cols;
        const pt::u64 blocked = __ballot(lane < pt::NEAR && pt::near_blocked(v, r, c, k + 1, lane));
        if (!blocked && lane == 0) pt::turn_tail(v, run);
    }

    __syncthreads();
    const int status = v.ctrl->status;
    if (status == pt::STATUS_OK) {
        int16_t *out = a.labels + (size_t)p * v.cells;
        for (int i = lane; i < v.cells; i += pt::WAVE) out[i] = v.label[i];
    }
    if (lane == 0) {
        if (status == pt::STATUS_OK) pt::store_words(run.rng, words);
        a.status[p] = status;
    }
}

}  // namespace

size_t partition_workspace_bytes(int n, int rows, int cols, int regions) { return pt::workspace_bytes(n, rows, cols, regions); }

hipError_t launch_partition(unsigned long long *rng, const int32_t *min_regions, const int32_t *max_regions, int16_t *labels,
                            int32_t *status, int n, int rows, int cols, int regions, void *workspace, hipStream_t stream) {
    PartitionArgs a = {};
    a.rng = rng; a.min_regions = min_regions; a.max_regions = max_regions; a.labels = labels; a.status = status;
    a.workspace = (unsigned char *)workspace;
    a.shape_ok = pt::shape_ok(rows, cols) ? 1 : 0;
    if (a.shape_ok) a.layout = pt::make_layout(rows, cols, regions);
    else a.layout.regions = regions;                    // every problem is refused: no state is touched
    if (!a.shape_ok || a.layout.bytes <= pt::LDS_LIMIT)
        hipLaunchKernelGGL(k_partition<true>, dim3(n), dim3(pt::WAVE), a.shape_ok ? a.layout.bytes : 0, stream, a);
    else
        hipLaunchKernelGGL(k_partition<false>, dim3(n), dim3(pt::WAVE), 0, stream, a);
    return hipGetLastError();
}

}  // namespace sl
