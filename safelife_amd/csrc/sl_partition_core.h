// sl_partition_core.h -- one region partition of the level generator (safelife_amd/proc_gen.py: partition), as functions that
// compile for the device AND for the host.  The kernel in sl_partition.hip calls them from the lanes of one wavefront;
// tests/partition_host_check.cpp calls the very same functions in plain loops on the CPU (under AddressSanitizer), so the
// logic and every index it forms are checked without a GPU.  Nothing here touches HIP.
//
// A partition's whole state lives in ONE flat buffer (LDS on the device when it fits, a slice of a global workspace when not)
// cut up by `Layout`:
//     ctrl      Ctrl                     the frontiers' sizes, what lane 0 hands the other lanes, the status
//     queued    u64    [regions][words]  per region: the cells that have ever been in its frontier (or are its seed), one bit
//                                        each, words = ceil(cells / 64); while a region is being seeded the same words hold
//                                        the bitmap of its free seed cells
//     frontier  uint16 [regions][cells]  per region: its frontier; a cell enters a region's frontier at most once (queued),
//                                        so `cells` entries are enough
//     label     uint8  [cells]           0 = buffer, 1.. = region
// with cells = rows * cols <= 4096 (an index fits 16 bits) and regions <= 8.
//
// The draws are numpy's: Generator.integers(0, n) is Lemire's bounded method on next_uint32 (nothing drawn for n == 1),
// Generator.random() a fresh 64-bit output; sl_gen_pattern_core.h has the generator.  The region pick is IEEE double, one
// rounding per operation, as Python computes it.
#pragma once
#include "sl_gen_pattern_core.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sl {
namespace pt {

typedef gp::u64 u64;
typedef gp::Rng Rng;

constexpr int MIN_SIDE = 3, MAX_SIDE = 64, MAX_REGIONS = 8;
constexpr int N_RNG_WORDS = gp::N_RNG_WORDS;
constexpr int STATUS_OK = 0, STATUS_REFUSED = -4, STATUS_CAPPED = -5;
constexpr int MAX_REDRAWS = 64;         // Lemire's rejection loop redraws with probability below n / 2^32: never, in effect
constexpr int WAVE = 64;
constexpr int NEAR = 25;                // the wrapped 5x5 window of foreign_near
constexpr unsigned LDS_LIMIT = gp::LDS_LIMIT;

struct Ctrl {
    int size[MAX_REGIONS];      // the frontiers' sizes
    int n_regions;              // regions seeded so far
    int want;                   // regions drawn
    int taken;                  // labelled cells
    int cell, k;                // the turn's cell and its region (0-based)
    int done, status;
    int pad;
};

struct Layout {
    int rows, cols, cells, regions, words;
    unsigned off_ctrl, off_queued, off_frontier, off_label, bytes;
};

SLGP_FN bool shape_ok(int rows, int cols) {
    return rows >= MIN_SIDE && rows <= MAX_SIDE && cols >= MIN_SIDE && cols <= MAX_SIDE;
}

// `regions`: how many regions the state has room for, 1 .. MAX_REGIONS
SLGP_FN Layout make_layout(int rows, int cols, int regions) {
    Layout l;
    l.rows = rows; l.cols = cols; l.regions = regions;
    l.cells = rows * cols;
    l.words = (l.cells + 63) / 64;
    unsigned o = 0;
    l.off_ctrl = o;      o += (unsigned)((sizeof(Ctrl) + 7) & ~(size_t)7);
    l.off_queued = o;    o += 8u * regions * l.words;
    l.off_frontier = o;  o += 2u * regions * l.cells;
    l.off_label = o;     o += l.cells;
    l.bytes = (o + 15u) & ~15u;
    return l;
}

// the host's clamping of a problem's bounds: lo = max(1, min), hi = max(max, lo)
SLGP_FN void clamp_bounds(int min_regions, int max_regions, int &lo, int &hi) {
    lo = min_regions > 1 ? min_regions : 1;
    hi = max_regions > lo ? max_regions : lo;
}

// ---- the host side of a launch: what is an error, and how large a workspace it needs ------------------------------------------

constexpr int E_OK = 0, E_ARG = -2;     // SL_OK, SL_E_ARG

// bytes of global workspace for n partitions: 0 where one's state fits a workgroup's LDS (or every problem is refused anyway)
inline size_t workspace_bytes(int n, int rows, int cols, int regions) {
    if (n < 1 || !shape_ok(rows, cols) || regions < 1 || regions > MAX_REGIONS) return 0;
    const Layout l = make_layout(rows, cols, regions);
    return l.bytes <= LDS_LIMIT ? 0 : (size_t)n * l.bytes;
}

// A shape outside the range is no error of the call: its problems are refused one by one (STATUS_REFUSED).
inline int validate(const void *rng, const void *min_regions, const void *max_regions, const void *labels, const void *status,
                    int n, int regions, size_t need, const void *workspace, size_t workspace_size, const char **why) {
    const char *none;
    if (!why) why = &none;
    if (n < 0) return *why = "partition_batch: negative problem count", E_ARG;
    if (regions < 1 || regions > MAX_REGIONS) return *why = "partition_batch: room for 1 to 8 regions", E_ARG;
    if (n == 0) return E_OK;
    if (!rng || !min_regions || !max_regions || !labels || !status) return *why = "partition_batch: null pointer", E_ARG;
    if ((uintptr_t)rng & 7) return *why = "partition_batch: rng not 8-byte aligned", E_ARG;
    if ((uintptr_t)labels & 1) return *why = "partition_batch: labels not 2-byte aligned", E_ARG;
    if (((uintptr_t)min_regions | (uintptr_t)max_regions | (uintptr_t)status) & 3)
        return *why = "partition_batch: min_regions / max_regions / status not 4-byte aligned", E_ARG;
    if (need && (!workspace || workspace_size < need || ((uintptr_t)workspace & 15)))
        return *why = "partition_batch: workspace missing, smaller than slhip_partition_workspace_bytes says, or not 16-byte "
                      "aligned", E_ARG;
    return E_OK;
}

struct View {
    Ctrl *ctrl;
    u64 *queued;
    uint16_t *frontier;
    uint8_t *label;
    int rows, cols, cells, words;
};

SLGP_FN View make_view(unsigned char *base, const Layout &l) {
    View v;
    v.ctrl = (Ctrl *)(base + l.off_ctrl);
    v.queued = (u64 *)(base + l.off_queued);
    v.frontier = (uint16_t *)(base + l.off_frontier);
    v.label = base + l.off_label;
    v.rows = l.rows; v.cols = l.cols; v.cells = l.cells; v.words = l.words;
    return v;
}

// ---- the draws ------------------------------------------------------------------------------------------------------------------

// Generator.integers(0, n), 1 <= n < 2^32.  False: the rejection loop reached its cap (the problem ends STATUS_CAPPED).
SLGP_FN bool bounded(Rng &g, uint32_t n, uint32_t &out) {
    if (n == 1) {
        out = 0;
        return true;
    }
    u64 m = (u64)gp::next32(g) * n;
    if ((uint32_t)m < n) {
        const uint32_t threshold = (0u - n) % n;            // (2^32 - n) % n
        for (int redraws = 0; (uint32_t)m < threshold; redraws++) {
            if (redraws == MAX_REDRAWS) return false;
            m = (u64)gp::next32(g) * n;
        }
    }
    out = (uint32_t)(m >> 32);
    return true;
}

// a turn goes to region k with probability size_k / total: `at` is random() * total
SLGP_FN int pick_region(const int *size, int n, double at) {
    int k = 0;
    while (k < n - 1 && (at >= (double)size[k] || !size[k])) {
        at -= (double)size[k];
        k++;
    }
    for (int tries = 0; !size[k] && tries < n; tries++) k = k + 1 == n ? 0 : k + 1;      // while not frontiers[k]
    return k;
}

// ---- the board --------------------------------------------------------------------------------------------------------------------

// x in [-2, n + 1] wrapped into [0, n), n >= 3: Python's % without a division
SLGP_FN int wrap(int x, int n) {
    x += n;
    if (x >= n) x -= n;
    if (x >= n) x -= n;
    return x;
}

// One of the 25 looks of `label[cell] or foreign_near(r, c, k)` (k 1-based): lane 12 is the cell itself, where any label
// counts.  The turn's cell is taken when no lane says true; the order of the looks does not matter.
SLGP_FN bool near_blocked(const View &v, int r, int c, int k, int lane) {
    const int dy = lane / 5 - 2, dx = lane % 5 - 2;
    const int lab = v.label[wrap(r + dy, v.rows) * v.cols + wrap(c + dx, v.cols)];
    return lab && (lab != k || lane == 12);
}

// is `cell` a free seed cell of region k: not labelled, no other region's cell within two
SLGP_FN bool seed_free(const View &v, int cell, int k) {
    const int r = cell / v.cols, c = cell - r * v.cols;
    for (int lane = 0; lane < NEAR; lane++)
        if (near_blocked(v, r, c, k, lane)) return false;
    return true;
}

SLGP_FN bool is_queued(const u64 *q, int cell) { return (q[cell >> 6] >> (cell & 63)) & 1; }
SLGP_FN void set_queued(u64 *q, int cell) { q[cell >> 6] |= 1ull << (cell & 63); }

// the four neighbours in the order the frontier takes them: (-1,0), (0,-1), (0,1), (1,0)
SLGP_FN int neighbour(const View &v, int r, int c, int which) {
    const int dy = which == 0 ? -1 : which == 3 ? 1 : 0, dx = which == 1 ? -1 : which == 2 ? 1 : 0;
    return wrap(r + dy, v.rows) * v.cols + wrap(c + dx, v.cols);
}

// ---- one partition, in the pieces the wavefront runs ------------------------------------------------------------------------------

struct Run {
    Rng rng;
    int turns, max_turns, room;
};

SLGP_FN void load_words(Rng &g, const u64 *w) {
    g.hi = w[0]; g.lo = w[1]; g.inc_hi = w[2]; g.inc_lo = w[3]; g.has_uint32 = w[4]; g.uinteger = w[5];
}

SLGP_FN void store_words(const Rng &g, u64 *w) {
    w[0] = g.hi; w[1] = g.lo; w[2] = g.inc_hi; w[3] = g.inc_lo; w[4] = g.has_uint32; w[5] = g.uinteger;
}

SLGP_FN void fail(const View &v, int status) {
    v.ctrl->status = status;
    v.ctrl->done = 1;
}

// every lane: the labels and the bitmaps start empty
SLGP_FN void init_clear(const View &v, int regions, int lane, int lanes) {
    for (int i = lane; i < v.cells; i += lanes) v.label[i] = 0;
    for (int i = lane; i < regions * v.words; i += lanes) v.queued[i] = 0;
}

// lane 0: the number of regions -- the partition's first draw.  lo, hi as clamp_bounds leaves them, hi within the layout.
SLGP_FN void begin(const View &v, Run &run, const u64 *words, int lo, int hi) {
    Ctrl *c = v.ctrl;
    for (int i = 0; i < MAX_REGIONS; i++) c->size[i] = 0;
    c->n_regions = c->taken = c->cell = c->k = c->done = c->pad = 0;
    c->status = STATUS_OK;
    load_words(run.rng, words);
    uint32_t extra = 0;
    if (!bounded(run.rng, (uint32_t)(hi - lo + 1), extra)) fail(v, STATUS_CAPPED);
    c->want = lo + (int)extra;
    run.turns = 0;
    run.max_turns = c->want * v.cells + 1;
    run.room = (4 * v.cells) / 5;       // a lone region has no neighbour to stop it: it leaves a fifth as buffer
}

// lane 0, after the free seed cells of region k (1-based) have been written to its bitmap, `count` of them, count >= 1:
// draw one -- the j-th in ascending cell order --, label it and start the region's frontier
SLGP_FN void seed_take(const View &v, Run &run, int k, int count) {
    Ctrl *c = v.ctrl;
    u64 *q = v.queued + (size_t)(k - 1) * v.words;
    uint32_t j = 0;
    if (!bounded(run.rng, (uint32_t)count, j)) return fail(v, STATUS_CAPPED);
    int w = 0;
    for (; w < v.words - 1; w++) {
        const uint32_t here = (uint32_t)__builtin_popcountll(q[w]);
        if (j < here) break;
        j -= here;
    }
    u64 bits = q[w];
    for (; j; j--) bits &= bits - 1;
    const int cell = w * 64 + (bits ? __builtin_ctzll(bits) : 0);
    for (int i = 0; i < v.words; i++) q[i] = 0;
    if (cell >= v.cells) return fail(v, STATUS_CAPPED);             // count was not the bitmap's: cannot happen
    v.label[cell] = (uint8_t)k;
    set_queued(q, cell);
    uint16_t *f = v.frontier + (size_t)(k - 1) * v.cells;
    const int r = cell / v.cols, col = cell - r * v.cols;
    int size = 0;
    for (int which = 0; which < 4; which++) {
        const int nxt = neighbour(v, r, col, which);
        if (!is_queued(q, nxt)) {
            set_queued(q, nxt);
            f[size++] = (uint16_t)nxt;
        }
    }
    c->size[k - 1] = size;
    c->n_regions = k;
    c->taken = k;
}

// lane 0: whose turn it is and which cell of its frontier -- into ctrl->k, ctrl->cell; or ctrl->done
SLGP_FN void turn_head(const View &v, Run &run) {
    Ctrl *c = v.ctrl;
    if (c->done) return;
    const int n = c->n_regions;
    int total = 0;
    for (int i = 0; i < n; i++) total += c->size[i];
    if (!total) {
        c->done = 1;
        return;
    }
    if (run.turns >= run.max_turns) return fail(v, STATUS_CAPPED);
    run.turns++;
    const double at = gp::next_double(run.rng) * (double)total;
    const int k = pick_region(c->size, n, at);
    const int len = c->size[k];
    uint32_t j = 0;
    if (len < 1 || !bounded(run.rng, (uint32_t)len, j)) return fail(v, STATUS_CAPPED);
    uint16_t *f = v.frontier + (size_t)k * v.cells;
    const int cell = f[j];
    f[j] = f[len - 1];                  // swap with the last and pop
    c->size[k] = len - 1;
    c->cell = cell;
    c->k = k;
}

// lane 0, when no lane found the turn's cell blocked: the cell joins region k, its free neighbours the frontier
SLGP_FN void turn_tail(const View &v, Run &run) {
    Ctrl *c = v.ctrl;
    const int k = c->k, cell = c->cell;
    if (c->n_regions == 1 && c->taken >= run.room) {
        c->done = 1;
        return;
    }
    v.label[cell] = (uint8_t)(k + 1);
    c->taken++;
    u64 *q = v.queued + (size_t)k * v.words;
    uint16_t *f = v.frontier + (size_t)k * v.cells;
    const int r = cell / v.cols, col = cell - r * v.cols;
    int size = c->size[k];
    for (int which = 0; which < 4; which++) {
        const int nxt = neighbour(v, r, col, which);
        if (!is_queued(q, nxt) && !v.label[nxt] && size < v.cells) {
            set_queued(q, nxt);
            f[size++] = (uint16_t)nxt;
        }
    }
    c->size[k] = size;
}

}  // namespace pt
}  // namespace sl
