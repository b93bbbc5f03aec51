// sl_gen_pattern_core.h -- one Metropolis chain of the pattern generator, as functions that compile for the device AND for
// the host.  The kernel in sl_gen_pattern.hip calls them from the lanes of one wavefront; tests/gen_pattern_host_check.cpp
// calls the very same functions in a plain loop on the CPU (under AddressSanitizer), so the chain's logic and every index it
// forms are checked without a GPU.  Nothing here touches HIP.
//
// A chain's whole state lives in ONE flat buffer (LDS on the device when it fits, a slice of a global workspace when not)
// cut up by `Layout`:
//     lp     double [cand]            log-probabilities, then cumulative probabilities, of an iteration's candidates
//     ctrl   Ctrl                     what lane 0 hands the other lanes, the cell totals and the three sets' sizes
//     board  uint16 [depth][layer]    the layers
//     sets   uint16 [3][2][layer]     bad / seeds / unmasked index sets: the members' array, then each value's position
//     ctype  uint16 [cand]            candidate's new cell      cidx  uint16 [cand]   candidate's cell index
//     nbr    uint8  [depth][layer]    live cells in the wrapped 3x3 (the cell itself included)
//     viol, osc, mask  uint8 [layer]  violations, oscillation bits, the mask's three low bits
// with layer = rows * cols <= 4096 (so an index fits 16 bits) and cand = 3 * (2 * depth + 1)^2.
//
// Every double operation is written as the sampler it restates writes it, one rounding each (the library is built with
// -ffp-contract=off and the pragma below says it again).  exp() is the one call whose last bit may differ between
// libraries.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define SLGP_FN __host__ __device__ inline
#else
#define SLGP_FN inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace sl {
namespace gp {

typedef unsigned long long u64;

constexpr int MIN_SIDE = 3, MAX_SIDE = 64, MAX_DEPTH = 4;
constexpr int N_PARAMS = 12;            // rel_max_iter, rel_min_fill, temperature, osc_bonus, cell_penalties[8]
constexpr int N_RNG_WORDS = 6;          // PCG64 state hi/lo, inc hi/lo, has_uint32, uinteger
constexpr int STATUS_OK = 0, STATUS_MAX_ITER = -1, STATUS_REFUSED = -4;
constexpr int SET_BAD = 0, SET_SEEDS = 1, SET_UNMASKED = 2;
constexpr int WAVE = 64;
constexpr unsigned LDS_LIMIT = 65536;   // a workgroup's dynamic LDS without asking the runtime for more

constexpr uint16_t ALIVE = 1, DESTRUCTIBLE = 8, FROZEN = 16;
constexpr int NEW_CELL_MASK = 1, CAN_OSCILLATE_MASK = 2, INCLUDE_VIOLATIONS_MASK = 4;
constexpr uint16_t NO_CANDIDATE = 0xFFFF;

struct Ctrl {
    double pen[4];
    double beta, osc_bonus;
    int totals[4];
    int size[3];
    int r0, c0, done;
};

struct Layout {
    int rows, cols, depth, layer, cand;
    unsigned off_lp, off_ctrl, off_board, off_sets, off_ctype, off_cidx, off_nbr, off_viol, off_osc, off_mask, bytes;
};

SLGP_FN bool shape_ok(int rows, int cols, int depth) {
    return rows >= MIN_SIDE && rows <= MAX_SIDE && cols >= MIN_SIDE && cols <= MAX_SIDE && depth >= 1 && depth <= MAX_DEPTH;
}

SLGP_FN Layout make_layout(int rows, int cols, int depth) {
    Layout l;
    l.rows = rows; l.cols = cols; l.depth = depth;
    l.layer = rows * cols;
    l.cand = 3 * (2 * depth + 1) * (2 * depth + 1);
    unsigned o = 0;
    l.off_lp = o;      o += 8u * l.cand;
    l.off_ctrl = o;    o += (unsigned)((sizeof(Ctrl) + 7) & ~(size_t)7);
    l.off_board = o;   o += 2u * depth * l.layer;
    l.off_sets = o;    o += 2u * 6 * l.layer;
    l.off_ctype = o;   o += 2u * l.cand;
    l.off_cidx = o;    o += 2u * l.cand;
    l.off_nbr = o;     o += 1u * depth * l.layer;
    l.off_viol = o;    o += l.layer;
    l.off_osc = o;     o += l.layer;
    l.off_mask = o;    o += l.layer;
    l.bytes = (o + 15u) & ~15u;
    return l;
}

// ---- the host side of a launch: what is refused, and how large a workspace it needs -------------------------------------------

constexpr int E_OK = 0, E_SHAPE = -1, E_ARG = -2, E_UNSUPPORTED = -4;      // SL_OK, SL_E_SHAPE, SL_E_ARG, SL_E_UNSUPPORTED

// bytes of global workspace for n chains: 0 where a chain's state fits a workgroup's LDS (or the shape is refused anyway)
inline size_t workspace_bytes(int n, int rows, int cols, int depth) {
    if (n < 1 || !shape_ok(rows, cols, depth)) return 0;
    const Layout l = make_layout(rows, cols, depth);
    return l.bytes <= LDS_LIMIT ? 0 : (size_t)n * l.bytes;
}

inline int validate(const void *layers, const void *mask, const void *params, const void *rng, const void *out_board,
                    const void *status, const void *iterations, int n, int rows, int cols, int depth, const void *workspace,
                    size_t workspace_size, const char **why) {
    const char *none;
    if (!why) why = &none;
    if (n < 0) return *why = "gen_pattern_batch: negative problem count", E_ARG;
    if (rows < MIN_SIDE || cols < MIN_SIDE) return *why = "Board must be at least 3x3.", E_SHAPE;
    if (depth < 1) return *why = "Pattern period must be larger than 0.", E_ARG;
    if (rows > MAX_SIDE || cols > MAX_SIDE) return *why = "gen_pattern_batch: boards above 64x64 are not supported", E_UNSUPPORTED;
    if (depth > MAX_DEPTH) return *why = "gen_pattern_batch: periods above 4 are not supported", E_UNSUPPORTED;
    if (n == 0) return E_OK;
    if (!layers || !mask || !params || !rng || !out_board || !status || !iterations)
        return *why = "gen_pattern_batch: null pointer", E_ARG;
    if (((uintptr_t)params | (uintptr_t)rng) & 7) return *why = "gen_pattern_batch: params / rng not 8-byte aligned", E_ARG;
    if (((uintptr_t)layers | (uintptr_t)out_board) & 1) return *why = "gen_pattern_batch: boards not 2-byte aligned", E_ARG;
    if (((uintptr_t)mask | (uintptr_t)status | (uintptr_t)iterations) & 3)
        return *why = "gen_pattern_batch: mask / status / iterations not 4-byte aligned", E_ARG;
    const size_t need = workspace_bytes(n, rows, cols, depth);
    if (need && (!workspace || workspace_size < need || ((uintptr_t)workspace & 15)))
        return *why = "gen_pattern_batch: workspace missing, smaller than slhip_gen_pattern_workspace_bytes says, or not "
                      "16-byte aligned", E_ARG;
    return E_OK;
}

struct View {
    double *lp;
    Ctrl *ctrl;
    uint16_t *board, *sets, *ctype, *cidx;
    uint8_t *nbr, *viol, *osc, *mask;
    int rows, cols, depth, layer;
};

SLGP_FN View make_view(unsigned char *base, const Layout &l) {
    View v;
    v.lp = (double *)(base + l.off_lp);
    v.ctrl = (Ctrl *)(base + l.off_ctrl);
    v.board = (uint16_t *)(base + l.off_board);
    v.sets = (uint16_t *)(base + l.off_sets);
    v.ctype = (uint16_t *)(base + l.off_ctype);
    v.cidx = (uint16_t *)(base + l.off_cidx);
    v.nbr = base + l.off_nbr;
    v.viol = base + l.off_viol;
    v.osc = base + l.off_osc;
    v.mask = base + l.off_mask;
    v.rows = l.rows; v.cols = l.cols; v.depth = l.depth; v.layer = l.layer;
    return v;
}

// ---- numpy's PCG64 with the buffered 32-bit half ----------------------------------------------------------------------------

struct Rng {
    u64 hi, lo, inc_hi, inc_lo, has_uint32, uinteger;
};

SLGP_FN u64 mulhi64(u64 a, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (u64)(((unsigned __int128)a * b) >> 64);
#endif
}

SLGP_FN u64 next64(Rng &g) {
    const u64 mh = 0x2360ED051FC65DA4ull, ml = 0x4385DF649FCCF645ull;
    u64 lo = g.lo * ml;
    u64 hi = mulhi64(g.lo, ml) + g.hi * ml + g.lo * mh;
    lo += g.inc_lo;
    hi += g.inc_hi + (lo < g.inc_lo ? 1u : 0u);
    g.hi = hi; g.lo = lo;
    const u64 x = hi ^ lo;
    const unsigned rot = (unsigned)(hi >> 58);
    return (x >> rot) | (x << ((64u - rot) & 63u));
}

// next_uint32: the low half of a fresh 64-bit draw, the high half kept for the next call
SLGP_FN uint32_t next32(Rng &g) {
    if (g.has_uint32) {
        g.has_uint32 = 0;
        return (uint32_t)g.uinteger;
    }
    const u64 n = next64(g);
    g.has_uint32 = 1;
    g.uinteger = n >> 32;
    return (uint32_t)n;
}

// next_double: always a fresh 64-bit draw; the buffered half stays where it is
SLGP_FN double next_double(Rng &g) { return (double)(next64(g) >> 11) * (1.0 / 9007199254740992.0); }

SLGP_FN uint32_t random_int(Rng &g, uint32_t high) {
    if (high == 0) return 0;
    uint32_t mask = high, value;
    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
    do {
        value = mask & next32(g);
    } while (value >= high);
    return value;
}

// ---- index sets: members in set[0 .. size), each value's position in ptr[] ------------------------------------------------

SLGP_FN uint16_t *set_of(const View &v, int s) { return v.sets + s * 2 * v.layer; }

SLGP_FN void iset_add(const View &v, int s, int val) {
    uint16_t *set = set_of(v, s), *ptr = set + v.layer;
    const int size = v.ctrl->size[s], k = ptr[val];
    if (k >= size) {
        const int y = set[size];
        set[size] = (uint16_t)val;
        ptr[val] = (uint16_t)size;
        set[k] = (uint16_t)y;
        ptr[y] = (uint16_t)k;
        v.ctrl->size[s] = size + 1;
    }
}

SLGP_FN void iset_discard(const View &v, int s, int val) {
    uint16_t *set = set_of(v, s), *ptr = set + v.layer;
    int size = v.ctrl->size[s];
    const int k = ptr[val];
    if (k < size) {
        size--;
        const int y = set[size];
        set[size] = (uint16_t)val;
        ptr[val] = (uint16_t)size;
        set[k] = (uint16_t)y;
        ptr[y] = (uint16_t)k;
        v.ctrl->size[s] = size;
    }
}

// ---- the board ----------------------------------------------------------------------------------------------------------------

SLGP_FN int wrap(int j, int n) {
    while (j < 0) j += n;
    while (j >= n) j -= n;
    return j;
}

SLGP_FN int idx3(const View &v, int layer, int r, int c) { return wrap(c, v.cols) + (wrap(r, v.rows) + layer * v.rows) * v.cols; }

SLGP_FN int type_idx(uint16_t cell) { return ((cell & ALIVE) << 1) | ((cell & FROZEN) >> 4); }

SLGP_FN uint16_t cell_of_type(int j) {
    j &= 3;
    return j == 0 ? 0 : j == 1 ? FROZEN : j == 2 ? (uint16_t)(ALIVE | DESTRUCTIBLE) : (uint16_t)(FROZEN | ALIVE);
}

SLGP_FN int violation(uint16_t src, uint16_t dst, int neighbors) {
    if (src & FROZEN) return src != dst;
    if (src & ALIVE) return (neighbors == 3 || neighbors == 4) ^ ((dst & ALIVE) != 0);
    return (neighbors == 3) ^ ((dst & ALIVE) != 0);
}

// 0: nothing changed, 1: only the frozen bit (or other bits), 2: the alive bit
SLGP_FN int swap_single(const View &v, int layer, int row, int col, uint16_t new_cell) {
    const int i0 = idx3(v, layer, row, col);
    const uint16_t old_cell = v.board[i0];
    if (old_cell == new_cell) return 0;
    v.board[i0] = new_cell;
    const int delta_alive = (int)(new_cell & ALIVE) - (int)(old_cell & ALIVE);
    if (!delta_alive) return 1;
    for (int r = row - 1; r <= row + 1; r++)
        for (int c = col - 1; c <= col + 1; c++) {
            const int i = idx3(v, layer, r, c);
            v.nbr[i] = (uint8_t)(v.nbr[i] + delta_alive);
        }
    return 2;
}

struct Delta {
    int oscillations, violations;
};

// Put `new_cell` at (row, col) of layer 0, run the change through the later layers, and bring violations and oscillation bits
// of the area it reached up to date.  The area grows WHILE it is walked and its coordinates wrap, so on a board narrower than
// the area a cell is visited more than once and the later visit sees the earlier one's update: all of that is kept as it is.
SLGP_FN Delta swap_cells(const View &v, int row, int col, uint16_t new_cell, bool track_bad) {
    Delta d = {0, 0};
    int x1 = col, y1 = row, x2 = col, y2 = row;
    int did = swap_single(v, 0, row, col, new_cell);
    if (did == 0) return d;
    if (did == 2) { x1--; y1--; x2++; y2++; }

    for (int layer = 1; layer < v.depth; layer++) {
        int swap_types = 0;
        for (int r = y1; r <= y2; r++) {
            for (int c = x1; c <= x2; c++) {
                const int i1 = idx3(v, layer - 1, r, c);
                const uint16_t b1 = v.board[i1];
                const int n1 = v.nbr[i1];
                uint16_t b2;
                if (b1 & FROZEN) b2 = b1;
                else if (b1 & ALIVE) b2 = (n1 == 3 || n1 == 4) ? b1 : 0;
                else b2 = (n1 == 3) ? ALIVE : b1;
                did = swap_single(v, layer, r, c, b2);
                swap_types |= did;
                if (did) {
                    if (c == x1) x1 -= 1;
                    if (c == x2) x2 += 1;
                    if (r == y1) y1 -= 1;
                    if (r == y2) y2 += 1;
                }
            }
        }
        if (!swap_types) break;
    }

    const int is_osc = 3 * ALIVE;
    for (int r = y1; r <= y2; r++) {
        for (int c = x1; c <= x2; c++) {
            const int i1 = idx3(v, 0, r, c);
            int i2 = i1, osc, viol;
            const uint16_t b1 = v.board[i1];
            if (b1 & FROZEN) {
                osc = 0;
                viol = 0;
            } else {
                uint16_t b2 = b1;
                osc = (b1 & ALIVE) + ALIVE;
                for (int layer = 1; layer < v.depth; layer++) {
                    i2 += v.layer;
                    b2 = v.board[i2];
                    osc |= (b2 & ALIVE) + ALIVE;
                }
                viol = violation(b2, b1, v.nbr[i2]);
            }
            const int m = v.mask[i1];
            if (osc == is_osc && !(m & CAN_OSCILLATE_MASK)) viol += 1;
            d.violations += viol - (int)v.viol[i1];
            d.oscillations += (osc == is_osc);
            d.oscillations -= (v.osc[i1] == is_osc);
            v.viol[i1] = (uint8_t)viol;
            v.osc[i1] = (uint8_t)osc;
            if (track_bad) {
                if (viol && (m & INCLUDE_VIOLATIONS_MASK)) iset_add(v, SET_BAD, i1);
                else iset_discard(v, SET_BAD, i1);
            }
        }
    }
    return d;
}

SLGP_FN double log_prob(const Ctrl *ctrl, int dv, int dosc, int j) {
    double lp = dv;
    lp -= ctrl->osc_bonus * dosc;
    lp += ctrl->pen[j & 3];
    lp *= -ctrl->beta;
    return lp;
}

// ---- what a chain carries in lane 0's registers -------------------------------------------------------------------------------

struct Chain {
    Rng rng;
    double min_fill;
    int max_iter, total_area, it, status;
};

// Set-up, part 1 (lanes side by side, `lane` of `nlanes`): copy in, identity sets.  `seeds` may be null: the mask stands in.
SLGP_FN void init_copy(const View &v, const uint16_t *layers, const int32_t *mask, int lane, int nlanes) {
    const int board_size = v.depth * v.layer;
    for (int i = lane; i < board_size; i += nlanes) v.board[i] = layers[i];
    for (int i = lane; i < v.layer; i += nlanes) {
        v.mask[i] = (uint8_t)(mask[i] & 7);
        for (int s = 0; s < 3; s++) {
            uint16_t *set = set_of(v, s);
            set[i] = (uint16_t)i;
            set[v.layer + i] = (uint16_t)i;
        }
    }
}

// part 2 (after a barrier): neighbour counts and oscillation bits.  On a board of at least 3x3 the wrapped 3x3 window holds
// nine different cells, so the sum over it is what the two wrapped 1-d passes of the sampler give.
SLGP_FN void init_counts(const View &v, int lane, int nlanes) {
    const int board_size = v.depth * v.layer;
    for (int i = lane; i < board_size; i += nlanes) {
        const int layer = i / v.layer, k = i - layer * v.layer, r = k / v.cols, c = k - r * v.cols;
        int n = 0;
        for (int dr = -1; dr <= 1; dr++)
            for (int dc = -1; dc <= 1; dc++) n += v.board[idx3(v, layer, r + dr, c + dc)] & ALIVE;
        v.nbr[i] = (uint8_t)n;
    }
    for (int k = lane; k < v.layer; k += nlanes) {
        int osc = 0;
        for (int layer = 0; layer < v.depth; layer++) osc |= (v.board[k + layer * v.layer] & ALIVE) + ALIVE;
        v.osc[k] = (uint8_t)osc;
    }
}

// part 3 (after a barrier; ONE lane: the order of the adds is the order of the sets): violations, sets, totals, limits
SLGP_FN void init_sets(const View &v, Chain &ch, const int32_t *mask, const int32_t *seeds, const double *params,
                       const u64 *rng_words) {
    Ctrl *ctrl = v.ctrl;
    for (int j = 0; j < 4; j++) ctrl->totals[j] = 0;
    for (int s = 0; s < 3; s++) ctrl->size[s] = 0;
    ctrl->done = 0;
    const int last = (v.depth - 1) * v.layer;
    int total_area = 0;
    for (int i = 0; i < v.layer; i++) {
        const int viol = violation(v.board[i + last], v.board[i], v.nbr[i + last]);
        v.viol[i] = (uint8_t)viol;
        if ((seeds ? seeds : mask)[i]) iset_add(v, SET_SEEDS, i);
        const int m = v.mask[i];
        if (viol && (m & INCLUDE_VIOLATIONS_MASK)) iset_add(v, SET_BAD, i);
        if (m & NEW_CELL_MASK) {
            iset_add(v, SET_UNMASKED, i);
            total_area++;
            ctrl->totals[type_idx(v.board[i])]++;
        }
    }
    ch.rng.hi = rng_words[0]; ch.rng.lo = rng_words[1]; ch.rng.inc_hi = rng_words[2]; ch.rng.inc_lo = rng_words[3];
    ch.rng.has_uint32 = rng_words[4]; ch.rng.uinteger = rng_words[5];
    ch.total_area = total_area;
    ch.it = 0;
    ch.status = STATUS_OK;
    const double limit = params[0] * total_area * v.depth;
    if (!(limit > -2147483649.0 && limit < 2147483648.0)) {      // the C conversion to int is undefined: refuse
        ch.status = STATUS_REFUSED;
        ch.max_iter = 0;
        ctrl->done = 1;
    } else {
        ch.max_iter = (int)limit;
    }
    ch.min_fill = params[1] * total_area;
    ctrl->beta = 1.0 / params[2];
    ctrl->osc_bonus = params[3];
}

// The head of an iteration (ONE lane): done?  Otherwise sample the centre and price the four cell types.
SLGP_FN void iter_head(const View &v, Chain &ch, const double *params) {
    Ctrl *ctrl = v.ctrl;
    if (ctrl->done) return;
    const int not_empty = ch.total_area - ctrl->totals[0];
    if (ch.it >= ch.max_iter || (ctrl->size[SET_BAD] == 0 && not_empty >= ch.min_fill)) {
        ctrl->done = 1;
        return;
    }
    const int s = ctrl->size[SET_BAD] > 0 ? SET_BAD : ctrl->size[SET_SEEDS] > 0 ? SET_SEEDS : SET_UNMASKED;
    const int n = ctrl->size[s] ? ctrl->size[s] : v.layer;      // an empty set: sample its whole backing array
    const int k0 = set_of(v, s)[random_int(ch.rng, (uint32_t)n)];
    iset_discard(v, SET_SEEDS, k0);
    ctrl->r0 = k0 / v.cols;
    ctrl->c0 = k0 % v.cols;
    {
        const double t = not_empty / ch.min_fill;
        ctrl->pen[0] = t < 0.9 ? 2.0 : t < 1 ? 20 * (1 - t) : 0;
    }
    const double *cp = params + 4;
    for (int j = 1; j < 4; j++) {
        const double t = ctrl->totals[j] / (not_empty + 1.0);
        const double base = cp[j * 2], slope = cp[j * 2 + 1];
        ctrl->pen[j] = base + t * slope;
    }
}

// The candidates of an iteration, one after the other with swap and swap-back on the shared state (any depth).  Returns how
// many there are; lp / ctype / cidx hold them in order.
SLGP_FN int candidates_serial(const View &v) {
    const Ctrl *ctrl = v.ctrl;
    int num = 0;
    for (int r = ctrl->r0 - v.depth; r <= ctrl->r0 + v.depth; r++) {
        for (int c = ctrl->c0 - v.depth; c <= ctrl->c0 + v.depth; c++) {
            const int i1 = idx3(v, 0, r, c);
            if (!(v.mask[i1] & NEW_CELL_MASK)) continue;
            const uint16_t current = v.board[i1];
            const int start = type_idx(current) + 1;
            int dv = 0, dosc = 0;
            for (int j = start; j < start + 3; j++) {
                const uint16_t target = cell_of_type(j);
                const Delta d = swap_cells(v, r, c, target, false);
                dv += d.violations;
                dosc += d.oscillations;
                v.lp[num] = log_prob(ctrl, dv, dosc, j);
                v.ctype[num] = target;
                v.cidx[num] = (uint16_t)i1;
                num++;
            }
            swap_cells(v, r, c, current, false);
        }
    }
    return num;
}

// Depth 1 only: candidate `slot` (0 .. 26 = window cell * 3 + type) from the base state alone, writing nothing but its own
// slot.  With one layer a cell's violation is a function of the cell and its count, the stored violations always equal that
// function, and nothing can oscillate, so "swap, read the delta, swap back" is "new minus stored" over the 3x3 the change
// reaches -- and the 27 slots are independent of each other.
SLGP_FN void candidate_depth1(const View &v, int slot) {
    const Ctrl *ctrl = v.ctrl;
    const int w = slot / 3, jj = slot - 3 * w;
    const int r = ctrl->r0 - 1 + w / 3, c = ctrl->c0 - 1 + w % 3;
    const int i1 = idx3(v, 0, r, c);
    if (!(v.mask[i1] & NEW_CELL_MASK)) {
        v.cidx[slot] = NO_CANDIDATE;
        return;
    }
    const uint16_t current = v.board[i1];
    const int j = type_idx(current) + 1 + jj;
    const uint16_t target = cell_of_type(j);
    const int delta_alive = (int)(target & ALIVE) - (int)(current & ALIVE);
    int dv = 0;
    if (delta_alive) {
        for (int rr = r - 1; rr <= r + 1; rr++)
            for (int cc = c - 1; cc <= c + 1; cc++) {
                const int i = idx3(v, 0, rr, cc);
                const uint16_t b = i == i1 ? target : v.board[i];
                const int viol = (b & FROZEN) ? 0 : violation(b, b, v.nbr[i] + delta_alive);
                dv += viol - (int)v.viol[i];
            }
    } else {
        const int viol = (target & FROZEN) ? 0 : violation(target, target, v.nbr[i1]);
        dv = viol - (int)v.viol[i1];
    }
    v.lp[slot] = log_prob(ctrl, dv, 0, j);
    v.ctype[slot] = target;
    v.cidx[slot] = (uint16_t)i1;
}

// ONE lane, behind candidate_depth1 in every slot: close the gaps the masked-out cells left.  Returns the count.
SLGP_FN int compact_depth1(const View &v) {
    int num = 0;
    for (int slot = 0; slot < 27; slot++) {
        if (v.cidx[slot] == NO_CANDIDATE) continue;
        if (num != slot) {
            v.lp[num] = v.lp[slot];
            v.ctype[num] = v.ctype[slot];
            v.cidx[num] = v.cidx[slot];
        }
        num++;
    }
    return num;
}

// The tail of an iteration (ONE lane): cumulative probabilities, the draw, the pick, the swap that stays.
SLGP_FN void iter_tail(const View &v, Chain &ch, int num) {
    Ctrl *ctrl = v.ctrl;
    double max_lp = -1e100;
    for (int k = 0; k < num; k++)
        if (max_lp < v.lp[k]) max_lp = v.lp[k];
    double total = 0.0;
    for (int k = 0; k < num; k++) {
        total += exp(v.lp[k] - max_lp);
        v.lp[k] = total;
    }
    const double target = next_double(ch.rng) * total;
    for (int k = 0; k < num; k++) {
        if (v.lp[k] > target) {
            const int cell = v.cidx[k];
            const uint16_t old_cell = v.board[cell], new_cell = v.ctype[k];
            swap_cells(v, cell / v.cols, cell % v.cols, new_cell, true);
            ctrl->totals[type_idx(old_cell)]--;
            ctrl->totals[type_idx(new_cell)]++;
            break;
        }
    }
    ch.it++;
}

SLGP_FN int chain_status(const Chain &ch) {
    if (ch.status != STATUS_OK) return ch.status;
    return ch.it == ch.max_iter ? STATUS_MAX_ITER : STATUS_OK;
}

}  // namespace gp
}  // namespace sl
