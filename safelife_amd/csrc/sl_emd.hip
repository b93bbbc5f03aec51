// sl_emd.hip -- the earth-mover distances of side_effect_score (safelife/side_effects.py:13-57,132-154) for every
// (entry, key) of a queue of finished episodes, on the device: the EMD-hat of Pele & Werman between the "inaction"
// and the "action" distribution of a cell type, solved exactly.
//
// One (entry, key) problem per workgroup at a time.  `concurrency` workgroups are launched; each owns one slice of
// the workspace and takes problems off a device-side counter until none are left, so heavy problems (hundreds of
// differing cells) and the many trivial ones (key absent, or nothing differs) balance by themselves.
//
// The problem.  a, b: the two [H,W] distributions, as integers over one denominator (occupancy counts over
// num_samples; 0/1 masks over 1).  gap = |a/den - b/den| in float64 exactly as the host forms it; the cells with
// gap > 1e-3 * max(gap) take part, in row-major order.  Ground distance d(i,j) of two participating cells: a table
// look-up by (row_i - row_j, col_i - col_j) -- the table is built by the host (side_effects.ground_table) and
// uploaded, so host and device price every arc with the same bits.  Result:
//     min-cost flow of min(sum a, sum b) from a to b  +  penalty * |sum a - sum b|     (sums over participating cells)
//
// Cancelling min(a_i, b_i) at a cell first.  Every participating cell has a_i != b_i, so after cancelling it is a
// supplier (a_i - b_i units) or a consumer (b_i - a_i units), never both: ns + nd = n, at most n^2/4 arcs.  This
// leaves the optimum unchanged iff d is a quasi-metric with d(i,i) = 0 (a unit routed x -> i and another i -> y can
// be replaced by i -> i and x -> y at no greater cost iff d(x,y) <= d(x,i) + d(i,y)).  The reference's signed-gap
// torus rule is asymmetric but satisfies that: per axis, a move towards larger coordinates costs the plain
// difference, a move towards smaller ones min(g, size - g) <= g; a path's forward legs add up to at least its net
// forward displacement, and a path with net backward displacement g that uses a backward leg l > size/2 (cost
// size - l) pays l - g forward as well, size - g in all -- so no detour beats the direct arc on an axis; the sum of
// two quasi-metrics is one, and tanh is non-decreasing, concave and 0 at 0, hence subadditive, which keeps the
// inequality (up to the rounding of np.tanh, 1 ulp).  tests/test_emd.py checks the device against the FULL host LP.
//
// Unequal masses: a dummy consumer (S > D) or supplier (D > S) with zero-cost arcs takes the excess, which makes the
// problem balanced; the penalty term is added at the end.
//
// Solver: successive shortest paths on the bipartite supplier/consumer graph with node potentials (float64) and
// integer flows -- the Hungarian method for transportation problems.  For each supplier with supply left: a dense
// Dijkstra over the consumers (reduced cost c(i,j) - u_i - v_j from the table, never an n x n matrix), the scan
// spread over the workgroup's 256 lanes with a wave-shuffle arg-min; a consumer without demand left hands the
// search on to the suppliers that feed it (one coalesced read of its flow row); the first consumer with demand left
// ends it; potentials are updated, and the path is augmented by its bottleneck.  All ties break on the smaller
// index, the final sum(flow * cost) runs in a fixed order: results are deterministic.
//
// Loop bounds (a logic error must end as NaN + error flag, never as a hung kernel): every augmentation moves >= 1
// unit, so there are at most max(S, D) of them; a Dijkstra marks one consumer per iteration, at most nd + 1; a path
// has at most ns + nd + 2 arcs.  An exceeded bound writes NaN and the 1-based problem index into the workspace
// header, which slhip_emd_status() reports.
//
// Workspace (caller-owned, slhip_emd_workspace_bytes):
//     256  +  concurrency * ( align256(2 * M * M) + align256(36 * (H*W + 2)) ),   M = H*W/2 + 1
//   header (problem counter, error flag) + per workgroup: the dense uint16 flow matrix [nd+1][ns+1] (a flow never
//   exceeds a cell's supply <= num_samples <= 65535; (ns+1)(nd+1) with at most one dummy <= M*M) and 36 bytes per
//   node (potential, distance: float64; cell, remaining units, tree link, mark, worklist: int32) for when they do not
//   fit in LDS next to the table.  64x64: 8.5 MB per workgroup; 25x25: 218 KB.
// LDS: the table when it fits ((2H-1)(2W-1) float64: 19 KB at 25x25, 126 KB at 64x64), then the node arrays of the
// problem at hand when 36 * (n + 2) bytes fit behind it, else they live in the workspace.
#include <climits>
#include "sl_device.h"
#include "sl_kernels.h"

namespace sl {

namespace {

constexpr int EMD_THREADS = 256;
constexpr int EMD_WAVES = EMD_THREADS / 64;
constexpr int EMD_NODE_BYTES = 36;
constexpr size_t EMD_HEADER_BYTES = 256;
constexpr size_t EMD_LDS_DYNAMIC_MAX = 160 * 1024 - 8 * 1024;     // (static arrays below + slack)

__host__ __device__ inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct EmdHeader {
    int next;       // next problem to hand out
    int error;      // 0, or 1 + index of a problem that ran over a loop bound
};

struct EmdParams {
    sl_episode_queue q;
    int H, W, concurrency, table_lds;
    double den, penalty;
    const int32_t *counts;
    const uint16_t *keys;
    const uint8_t *type_masks;
    const double *ground;
    unsigned char *ws;
    size_t flow_bytes, slot_bytes, lds_bytes;
    double *scores;
    int32_t *n_cells;
};

__device__ __forceinline__ double emd_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double emd_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

__device__ __forceinline__ int block_sum(int v, int *scratch) {
    const int tid = threadIdx.x;
    __syncthreads();
    scratch[tid] = v;
    __syncthreads();
    for (int off = EMD_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) scratch[tid] += scratch[tid + off];
        __syncthreads();
    }
    return scratch[0];
}

__device__ __forceinline__ double block_sum(double v, double *scratch) {      // fixed order: deterministic
    const int tid = threadIdx.x;
    __syncthreads();
    scratch[tid] = v;
    __syncthreads();
    for (int off = EMD_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) scratch[tid] += scratch[tid + off];
        __syncthreads();
    }
    return scratch[0];
}

__device__ __forceinline__ double block_max(double v, double *scratch) {
    const int tid = threadIdx.x;
    __syncthreads();
    scratch[tid] = v;
    __syncthreads();
    for (int off = EMD_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) scratch[tid] = fmax(scratch[tid], scratch[tid + off]);
        __syncthreads();
    }
    return scratch[0];
}

__global__ __launch_bounds__(EMD_THREADS) void k_emd(EmdParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double s_red[EMD_THREADS];
    __shared__ int s_scan[EMD_THREADS];
    __shared__ double s_wm[EMD_WAVES];
    __shared__ int s_wj[EMD_WAVES];
    __shared__ int s_problem, s_wl, s_fail;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = P.H, W = P.W, HW = H * W, K = SL_SE_MAX_KEYS, C = P.q.capacity;
    const int TW = 2 * W - 1, table_len = (2 * H - 1) * TW;
    EmdHeader *hdr = (EmdHeader *)P.ws;
    unsigned char *slot = P.ws + EMD_HEADER_BYTES + (size_t)blockIdx.x * P.slot_bytes;
    u16 *flow = (u16 *)slot;
    const size_t flow_cap = P.flow_bytes / 2;

    const double *tbl = P.ground;
    size_t lds_used = 0;
    if (P.table_lds) {
        double *t = (double *)smem;
        for (int i = tid; i < table_len; i += EMD_THREADS) t[i] = P.ground[i];
        tbl = t;
        lds_used = (size_t)table_len * 8;
    }
    const int n_count = *P.q.count;
    const int valid = n_count < C ? n_count : C;
    const int n_problems = valid * K;
    __syncthreads();

    const int per = (HW + EMD_THREADS - 1) / EMD_THREADS;
    const int c_lo = min(HW, tid * per), c_hi = min(HW, c_lo + per);

    for (;;) {
        __syncthreads();
        if (tid == 0) s_problem = atomicAdd(&hdr->next, 1);
        __syncthreads();
        const int prob = s_problem;
        if (prob >= n_problems) break;
        const int entry = prob / K, k = prob - entry * K;
        double *out = P.scores + (size_t)prob * 2;
        if (P.q.records[entry].n_cell_types > K - 8) {          // keys cut short: the host evaluates this entry
            if (tid == 0) {
                out[0] = out[1] = emd_nan();
                P.n_cells[prob] = -1;
            }
            continue;
        }
        if (P.keys[(size_t)entry * K + k] == 0xFFFFu) {
            if (tid == 0) {
                out[0] = out[1] = emd_nan();
                P.n_cells[prob] = 0;
            }
            continue;
        }
        // a, b of a cell, as integers over `den`
        const int32_t *cnt0 = nullptr, *cnt1 = nullptr;
        const uint8_t *m0 = nullptr, *m1 = nullptr;
        double den = P.den;
        if (k < 8) {
            cnt0 = P.counts + (size_t)entry * HW * 8 + k;
            cnt1 = P.counts + ((size_t)C + entry) * HW * 8 + k;
        } else {
            m0 = P.type_masks + (((size_t)entry * 2 + 0) * (K - 8) + (k - 8)) * HW;
            m1 = P.type_masks + (((size_t)entry * 2 + 1) * (K - 8) + (k - 8)) * HW;
            den = 1.0;
        }
        double gmax = 0.0;
        int mass = 0;
        for (int c = c_lo; c < c_hi; ++c) {
            const int a = cnt0 ? cnt0[(size_t)c * 8] : (int)m0[c], b = cnt0 ? cnt1[(size_t)c * 8] : (int)m1[c];
            gmax = fmax(gmax, fabs((double)a / den - (double)b / den));
            mass += a;
        }
        gmax = block_max(gmax, s_red);
        mass = block_sum(mass, s_scan);
        const double thr = 1e-3 * gmax;
        int my_s = 0, my_d = 0;
        for (int c = c_lo; c < c_hi; ++c) {
            const int a = cnt0 ? cnt0[(size_t)c * 8] : (int)m0[c], b = cnt0 ? cnt1[(size_t)c * 8] : (int)m1[c];
            if (fabs((double)a / den - (double)b / den) > thr) {
                my_s += a > b;
                my_d += b > a;
            }
        }
        // exclusive scan of (suppliers | consumers << 16) over the lanes' cell ranges: row-major order
        __syncthreads();
        s_scan[tid] = my_s | (my_d << 16);
        __syncthreads();
        for (int off = 1; off < EMD_THREADS; off <<= 1) {
            const int v = tid >= off ? s_scan[tid - off] : 0;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        const int incl = s_scan[tid], total = s_scan[EMD_THREADS - 1];
        const int ns = total & 0xFFFF, nd = total >> 16, n = ns + nd;
        if (n == 0) {
            if (tid == 0) {
                out[0] = 0.0;
                out[1] = (double)mass / den;
                P.n_cells[prob] = 0;
            }
            continue;
        }
        // node arrays: suppliers 0..ns (ns = the dummy), consumers ns+1..ns+1+nd (the last = the dummy)
        const int N = n + 2;
        unsigned char *nodes = slot + P.flow_bytes;
        if (lds_used + (size_t)N * EMD_NODE_BYTES <= P.lds_bytes) nodes = smem + lds_used;
        double *pot = (double *)nodes, *dist = pot + N;
        int *pos = (int *)(dist + N), *rem = pos + N, *link = rem + N, *mark = link + N, *list = mark + N;
        const int D0 = ns + 1;                                   // first consumer
        {
            int is = (incl & 0xFFFF) - my_s, id = (incl >> 16) - my_d;
            for (int c = c_lo; c < c_hi; ++c) {
                const int a = cnt0 ? cnt0[(size_t)c * 8] : (int)m0[c], b = cnt0 ? cnt1[(size_t)c * 8] : (int)m1[c];
                if (fabs((double)a / den - (double)b / den) > thr) {
                    const int cell = ((c / W) << 8) | (c % W);
                    if (a > b) {
                        pos[is] = cell, rem[is] = a - b, pot[is] = 0.0;
                        ++is;
                    } else if (b > a) {
                        pos[D0 + id] = cell, rem[D0 + id] = b - a, pot[D0 + id] = 0.0;
                        ++id;
                    }
                }
            }
        }
        int sup = 0, dem = 0;
        __syncthreads();
        for (int i = tid; i < ns; i += EMD_THREADS) sup += rem[i];
        for (int j = tid; j < nd; j += EMD_THREADS) dem += rem[D0 + j];
        const int S = block_sum(sup, s_scan), D = block_sum(dem, s_scan);
        const int nss = ns + (D > S), ndd = nd + (S > D);
        if (tid == 0) {
            pos[ns] = -1, rem[ns] = D > S ? D - S : 0, pot[ns] = 0.0;
            pos[D0 + nd] = -1, rem[D0 + nd] = S > D ? S - D : 0, pot[D0 + nd] = 0.0;
            s_fail = (size_t)nss * ndd > flow_cap;
        }
        const int n_arcs = nss * ndd;
        __syncthreads();
        int fail = s_fail;
        if (!fail) {
            uint32_t *fw = (uint32_t *)flow;
            for (int i = tid; i < (n_arcs + 1) / 2; i += EMD_THREADS) fw[i] = 0u;
        }
        __syncthreads();

        auto cost = [&](int ps, int pd) -> double {
            if ((ps | pd) < 0) return 0.0;
            return tbl[((ps >> 8) - (pd >> 8) + H - 1) * TW + ((ps & 255) - (pd & 255) + W - 1)];
        };
        double *distD = dist + D0, *potD = pot + D0;
        int *posD = pos + D0, *remD = rem + D0, *linkD = link + D0, *markD = mark + D0;

        const int max_aug = S > D ? S : D;
        int augs = 0;
        for (int src = 0; src < nss && !fail; ++src) {
            for (;;) {
                __syncthreads();
                if (rem[src] <= 0) break;
                if (++augs > max_aug) {
                    fail = 1;
                    break;
                }
                for (int j = tid; j < ndd; j += EMD_THREADS) distD[j] = emd_inf(), linkD[j] = -1, markD[j] = 0;
                for (int i = tid; i < nss; i += EMD_THREADS) mark[i] = 0;
                __syncthreads();
                if (tid == 0) {
                    mark[src] = 1, dist[src] = 0.0, link[src] = -1, list[0] = src;
                    s_wl = 1;
                }
                __syncthreads();
                int wl = 1, term = -1;
                double delta = 0.0;
                for (int it = 0; it <= ndd; ++it) {
                    // relax the consumers from the suppliers that joined the tree, and find the nearest unmarked one
                    double bm = emd_inf();
                    int bj = INT_MAX;
                    for (int j = tid; j < ndd; j += EMD_THREADS) {
                        if (markD[j]) continue;
                        double m = distD[j];
                        if (wl > 0) {
                            int w = linkD[j];
                            const int pd = posD[j];
                            const double vj = potD[j];
                            for (int t = 0; t < wl; ++t) {
                                const int i = list[t];
                                const double cand = dist[i] + (cost(pos[i], pd) - pot[i] - vj);
                                if (cand < m || (cand == m && i < w)) m = cand, w = i;
                            }
                            distD[j] = m, linkD[j] = w;
                        }
                        if (m < bm) bm = m, bj = j;
                    }
                    for (int off = 32; off > 0; off >>= 1) {
                        const double om = __shfl_down(bm, off);
                        const int oj = __shfl_down(bj, off);
                        if (om < bm || (om == bm && oj < bj)) bm = om, bj = oj;
                    }
                    if (lane == 0) s_wm[wave] = bm, s_wj[wave] = bj;
                    __syncthreads();
                    bm = s_wm[0], bj = s_wj[0];
                    for (int w = 1; w < EMD_WAVES; ++w)
                        if (s_wm[w] < bm || (s_wm[w] == bm && s_wj[w] < bj)) bm = s_wm[w], bj = s_wj[w];
                    if (bj == INT_MAX) break;                    // (cannot happen: the problem is balanced)
                    delta = bm;
                    if (tid == 0) {
                        markD[bj] = 1;
                        s_wl = 0;
                    }
                    if (remD[bj] > 0) {
                        term = bj;
                        break;
                    }
                    __syncthreads();
                    const u16 *row = flow + (size_t)bj * nss;
                    for (int i = tid; i < nss; i += EMD_THREADS)
                        if (row[i] && !mark[i]) {
                            mark[i] = 1, link[i] = bj, dist[i] = delta;
                            list[atomicAdd(&s_wl, 1)] = i;      // (order-free: the relaxation breaks ties on the index)
                        }
                    __syncthreads();
                    wl = s_wl;
                }
                __syncthreads();
                if (term < 0) {
                    fail = 1;
                    break;
                }
                for (int i = tid; i < nss; i += EMD_THREADS)
                    if (mark[i]) pot[i] += delta - dist[i];
                for (int j = tid; j < ndd; j += EMD_THREADS)
                    if (markD[j]) potD[j] -= delta - distD[j];
                if (tid == 0) {
                    const int max_hops = nss + ndd;
                    int bott = min(rem[src], remD[term]), hops = 0, bad = 0;
                    for (int i = linkD[term]; i != src;) {
                        const int pj = link[i];
                        if (i < 0 || i >= nss || pj < 0 || pj >= ndd || ++hops > max_hops) {
                            bad = 1;
                            break;
                        }
                        bott = min(bott, (int)flow[(size_t)pj * nss + i]);
                        i = linkD[pj];
                    }
                    if (bott <= 0) bad = 1;
                    if (!bad) {
                        for (int j = term;;) {
                            const int i = linkD[j];
                            flow[(size_t)j * nss + i] = (u16)(flow[(size_t)j * nss + i] + bott);
                            if (i == src) break;
                            const int pj = link[i];
                            flow[(size_t)pj * nss + i] = (u16)(flow[(size_t)pj * nss + i] - bott);
                            j = pj;
                        }
                        rem[src] -= bott;
                        remD[term] -= bott;
                    }
                    s_fail = bad;
                }
                __syncthreads();
                if (s_fail) {
                    fail = 1;
                    break;
                }
            }
        }
        __syncthreads();
        double acc = 0.0;
        if (!fail)
            for (int e = tid; e < n_arcs; e += EMD_THREADS) {
                const int f = flow[e];
                if (f) {
                    const int j = e / nss, i = e - j * nss;
                    acc += (double)f * cost(pos[i], posD[j]);
                }
            }
        acc = block_sum(acc, s_red);
        if (tid == 0) {
            if (fail) {
                out[0] = out[1] = emd_nan();
                atomicMax(&hdr->error, prob + 1);
            } else {
                out[0] = acc / den + P.penalty * ((double)(S > D ? S - D : D - S) / den);
                out[1] = (double)mass / den;
            }
            P.n_cells[prob] = n;
        }
    }
}

}  // namespace

size_t emd_workspace_bytes(int H, int W, int concurrency) {
    const size_t HW = (size_t)H * W, M = HW / 2 + 1;
    return EMD_HEADER_BYTES + (size_t)concurrency * (align256(2 * M * M) + align256(EMD_NODE_BYTES * (HW + 2)));
}

hipError_t launch_emd(const sl_episode_queue &q, int H, int W, int num_samples, const int32_t *counts,
                      const uint16_t *keys, const uint8_t *type_masks, const double *ground, double penalty,
                      void *workspace, int concurrency, double *scores, int32_t *n_cells, hipStream_t stream) {
    const size_t HW = (size_t)H * W, M = HW / 2 + 1;
    EmdParams P;
    P.q = q;
    P.H = H, P.W = W, P.concurrency = concurrency;
    P.den = (double)num_samples, P.penalty = penalty;
    P.counts = counts, P.keys = keys, P.type_masks = type_masks, P.ground = ground;
    P.ws = (unsigned char *)workspace;
    P.flow_bytes = align256(2 * M * M);
    P.slot_bytes = P.flow_bytes + align256(EMD_NODE_BYTES * (HW + 2));
    P.scores = scores, P.n_cells = n_cells;
    const size_t table_bytes = (size_t)(2 * H - 1) * (2 * W - 1) * 8;
    P.table_lds = table_bytes <= EMD_LDS_DYNAMIC_MAX;
    // the table, then as much of the node arrays as a board of this shape can need (or as fits)
    size_t lds = (P.table_lds ? table_bytes : 0) + EMD_NODE_BYTES * (HW + 2);
    if (lds > EMD_LDS_DYNAMIC_MAX) lds = EMD_LDS_DYNAMIC_MAX;
    P.lds_bytes = lds;
    hipError_t err = hipFuncSetAttribute((const void *)k_emd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    err = hipMemsetAsync(workspace, 0, EMD_HEADER_BYTES, stream);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_emd, dim3(concurrency), dim3(EMD_THREADS), lds, stream, P);
    return hipGetLastError();
}

}  // namespace sl
