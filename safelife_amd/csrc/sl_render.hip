// sl_render.hip -- boards -> RGB frames on the device (the reference's fast_render.c:33-133 and the view of
// render_graphics.render_game / helper_utils.py:42-75), bit exact with the reference's C blitter.
//
// Every cell becomes a 14x14 sprite: the tile is chosen by the cell's type, tinted with the cell's colour over a
// background of the GOAL's colour.  Per output byte, in fp32, left to right, nothing fused, truncated:
//     (uint8)(255.f * (bg * (1.f - mask) + mask * sprite * fg))          mask = the sheet's 4th channel
// (the library is built with -ffp-contract=off and the pragma below says it again: a fused multiply-add in the blend
// changes 345 of the 752 640 bytes of the tile x fg x bg table).
//
// Shape of the kernel.  The output of a launch is one flat range of N * vh * vw * 588 bytes (always a multiple of 4).
// It is walked in 16-byte chunks, one per lane and iteration: a lane decodes its chunk's first byte into (frame, cell row,
// sprite row, cell column, pixel, channel) once -- 32-bit divisions relative to the workgroup's first byte, whose 64-bit
// decomposition is wave-uniform -- and steps through the 16 bytes incrementally.  Image rows are 42 * vw bytes, not even
// dword aligned for odd vw, so any per-row scheme ends in byte stores; the flat walk stores whole uint4's whatever the
// view's width (dwords for the tail of the range and for an `out` that is not 16-byte aligned).
// A workgroup owns a contiguous run of chunks, hence a contiguous run of view rows.  What a cell decodes to -- tile
// offset, fg, bg: one word -- is needed by 14 image rows x ~3 chunks; two variants provide it:
//   STAGE = true   the workgroup decodes the view rows its run touches into LDS first (one decode per cell and workgroup)
//   STAGE = false  every lane decodes the (at most a few) cells of its chunk itself from global memory (L1 / L2)
// The sprite sheet stays in global memory: 78 KB as floats, read as one float4 per pixel, shared by every workgroup -- it
// lives in L2 / L1; in LDS it would cap a CU at two workgroups.  SAFELIFE_RENDER_VARIANT=direct|stage picks a variant for
// A/B runs (tools/render_bench.py times both).  Default: STAGE -- one decode per cell and workgroup instead of one per
// chunk (with a view, a decode walks the exit table); DESIGN.md section 4.7 records what has been measured.
#include "sl_kernels.h"

#pragma clang fp contract(off)

namespace sl {
namespace {

constexpr int RENDER_THREADS = 256;
constexpr bool RENDER_DEFAULT_STAGE = true;   // 
constexpr int SPRITE = 14;                   // SPRITE_SIZE
constexpr int CELL_ROW_BYTES = SPRITE * 3;   // 42: one sprite row of one cell
constexpr int CELL_BYTES = SPRITE * SPRITE * 3;     // 588
constexpr int SHEET_ROW_FLOATS = 5 * SPRITE * 4;    // 280: one pixel row of the 70 x 70 x 4 sheet

__constant__ float c_fg[8][3] = {{0.4f, 0.4f, 0.4f}, {0.8f, 0.2f, 0.2f}, {0.2f, 0.8f, 0.2f}, {0.8f, 0.8f, 0.2f},
                                 {0.2f, 0.2f, 0.8f}, {0.8f, 0.2f, 0.8f}, {0.2f, 0.8f, 0.8f}, {1.0f, 1.0f, 1.0f}};
__constant__ float c_bg[8][3] = {{0.6f, 0.6f, 0.6f}, {0.9f, 0.6f, 0.6f}, {0.6f, 0.9f, 0.6f}, {0.9f, 0.9f, 0.6f},
                                 {0.5f, 0.5f, 0.9f}, {0.9f, 0.6f, 0.9f}, {0.6f, 0.9f, 0.9f}, {0.9f, 0.9f, 0.9f}};

// tile (row, col) of the sheet for a cell (fast_render.c:43-86) as the float offset of its first pixel
__device__ __forceinline__ u32 tile_offset(u32 cell) {
    const u32 orient = (cell >> 12) & 3u;
    const u32 type = cell & ~((7u << 9) | (3u << 12)) & 0xFFFFu;
    int row = 3, col = 4;                    // unknown; an empty cell that carries colour or orientation bits
    switch (type) {
        case 0: if (cell == 0) row = 0, col = 0; break;
        case 9: row = 1, col = 0; break;     // life
        case 1: row = 1, col = 1; break;     // hard life
        case 53: row = 1, col = 2; break;    // weed
        case 32789: row = 1, col = 3; break; // plant
        case 17: row = 1, col = 4; break;    // tree
        case 32884: row = 2, col = 0; break; // ice cube
        case 48: row = 2, col = 1; break;    // fountain
        case 16: row = 2, col = 2; break;    // wall
        case 32788: row = 2, col = 3; break; // crate
        case 85: row = 2, col = 4; break;    // parasite
        case 152: row = 3, col = 0; break;   // spawner
        case 272: row = 3, col = 1; break;   // exit
        case 144: row = 3, col = 2; break;   // hard spawner
        default: if (type & 2u) row = 0, col = 1 + (int)orient; break;    // agent
    }
    return (u32)(row * SPRITE * SHEET_ROW_FLOATS + col * SPRITE * 4);
}

// what view cell (cy, cx) of output frame n shows: tile offset | fg << 16 | bg << 19
__device__ u32 decode_cell(const sl_render_args &a, int vh, int vw, int n, int cy, int cx) {
    long long f = a.index ? a.index[n] : n;
    if (f < 0 || f >= a.n_source) return 0;                     // (an index outside the source: an empty frame)
    const u16 *board = a.board + f * a.board_stride;
    const u16 *goals = a.goals + f * a.goal_stride;
    const int H = a.H, W = a.W;
    u32 cell, goal;
    if (a.view_h > 0) {
        const long long s = a.aux_by_index ? f : n;
        const int32_t *c = a.centers + s * a.center_stride;
        int y0 = c[0], x0 = c[1];
        if (y0 < 0) y0 = 0, x0 = 0;                             // no agent
        y0 %= H, x0 = pos_mod(x0, W);
        const int src = pos_mod(y0 - vh / 2 + cy, H) * W + pos_mod(x0 - vw / 2 + cx, W);
        cell = board[src], goal = goals[src];
        // helper_utils.py:64-74: every exit's BOARD value goes to its position in the view, clipped to the perimeter;
        // later entries overwrite earlier ones (numpy's fancy assignment); goals are not repainted
        const int32_t *exits = a.exits ? a.exits + s * a.E : nullptr;
        for (int k = 0; exits && k < a.E; ++k) {
            const int ex = exits[k];
            if (ex < 0 || ex >= H * W) continue;
            const int iy = ex / W, ix = ex - iy * W;
            int jy = pos_mod(iy - y0 + H / 2, H) - H / 2 + vh / 2;
            int jx = pos_mod(ix - x0 + W / 2, W) - W / 2 + vw / 2;
            jy = min(max(jy, 0), vh - 1), jx = min(max(jx, 0), vw - 1);
            if (jy == cy && jx == cx) cell = board[ex];
        }
    } else {
        cell = board[cy * W + cx], goal = goals[cy * W + cx];
    }
    if (a.orientation) cell = (cell & ~(3u << 12)) | (((u32)a.orientation[n] & 3u) << 12);
    return tile_offset(cell) | (((cell >> 9) & 7u) << 16) | (((goal >> 9) & 7u) << 19);
}

template <bool STAGE>
__global__ __launch_bounds__(RENDER_THREADS) void k_render(sl_render_args a, int vh, int vw, u64 total_bytes, int iters) {
    extern __shared__ u32 s_cells[];
    const u32 frame_bytes = (u32)vh * vw * CELL_BYTES, row_bytes = (u32)vw * CELL_ROW_BYTES;
    const u32 band_bytes = row_bytes * SPRITE;                 // one view row: 14 image rows
    const u32 run_bytes = (u32)iters * RENDER_THREADS * 16;     // what a workgroup writes
    const u64 p0 = (u64)blockIdx.x * run_bytes;                 // wave-uniform: the 64-bit divisions are scalar
    const int n0 = (int)(p0 / frame_bytes);
    const u32 q0 = (u32)(p0 % frame_bytes);
    const u32 band0 = q0 / band_bytes;                          // first view row of frame n0 the run touches
    const u64 left = total_bytes - p0;
    const u32 len = left < run_bytes ? (u32)left : run_bytes;
    if (STAGE) {
        const u32 n_bands = (q0 - band0 * band_bytes + len + band_bytes - 1) / band_bytes;
        for (u32 s = threadIdx.x; s < n_bands * (u32)vw; s += RENDER_THREADS) {
            const u32 b = band0 + s / vw;
            s_cells[s] = decode_cell(a, vh, vw, n0 + (int)(b / vh), (int)(b % vh), (int)(s % vw));
        }
        __syncthreads();
    }
    const bool wide = (((uintptr_t)a.out) & 15) == 0;
    uint8_t *const out = a.out + p0;
    for (int it = 0; it < iters; ++it) {
        const u32 off = ((u32)it * RENDER_THREADS + threadIdx.x) * 16;
        if (off >= len) break;
        const u32 nbytes = min(16u, len - off);                 // 4, 8 or 12 only at the end of the whole range
        const u32 q = q0 + off;                                 // < 2 * frame_bytes + run_bytes: fits 32 bits
        int n = n0 + (int)(q / frame_bytes);
        const u32 r = q % frame_bytes;
        const u32 iy = r / row_bytes, bx = r - iy * row_bytes;
        int cy = (int)(iy / SPRITE), sr = (int)(iy - (u32)cy * SPRITE);
        int cx = (int)(bx / CELL_ROW_BYTES);
        const int t = (int)(bx - (u32)cx * CELL_ROW_BYTES);
        int px = t / 3, ch = t - px * 3;
        // 16 bytes are less than one sprite row of a cell: a chunk shows its first cell and at most the one after it
        int n1 = n, cy1 = cy, sr1 = sr, cx1 = cx + 1;
        if (cx1 == vw) {
            cx1 = 0;
            if (++sr1 == SPRITE) {
                sr1 = 0;
                if (++cy1 == vh) cy1 = 0, ++n1;
            }
        }
        const bool two = (u32)t + nbytes > (u32)CELL_ROW_BYTES;
        u32 code, code1 = 0;
        if (STAGE) {
            code = s_cells[(((u32)(n - n0) * vh + cy) - band0) * vw + cx];
            if (two) code1 = s_cells[(((u32)(n1 - n0) * vh + cy1) - band0) * vw + cx1];
        } else {
            code = decode_cell(a, vh, vw, n, cy, cx);
            if (two) code1 = decode_cell(a, vh, vw, n1, cy1, cx1);
        }
        float4 pix = make_float4(0.f, 0.f, 0.f, 0.f);
        bool new_pixel = true;
        u32 words[4] = {0, 0, 0, 0};
#pragma unroll
        for (u32 i = 0; i < 16; ++i) {
            if (i < nbytes) {
                if (new_pixel) {
                    pix = *(const float4 *)(a.sprites + (code & 0xFFFFu) + sr * SHEET_ROW_FLOATS + px * 4);
                    new_pixel = false;
                }
                const float fg = c_fg[(code >> 16) & 7u][ch], bg = c_bg[(code >> 19) & 7u][ch];
                const float sp = ch == 0 ? pix.x : (ch == 1 ? pix.y : pix.z), mask = pix.w;
                const float v = 255.f * (bg * (1.f - mask) + mask * sp * fg);
                words[i >> 2] |= ((u32)(int)v & 0xFFu) << (8 * (i & 3));
                if (++ch == 3) {
                    ch = 0, new_pixel = true;
                    if (++px == SPRITE) px = 0, code = code1, sr = sr1;
                }
            }
        }
        if (wide && nbytes == 16) {
            *(uint4 *)(out + off) = make_uint4(words[0], words[1], words[2], words[3]);
        } else {
            for (u32 w = 0; w < nbytes / 4; ++w) *(u32 *)(out + off + 4 * w) = words[w];
        }
    }
}

}  // namespace

hipError_t launch_render(const sl_render_args &a, int variant, hipStream_t stream) {
    const int vh = a.view_h > 0 ? a.view_h : a.H, vw = a.view_h > 0 ? a.view_w : a.W;
    const u64 total = (u64)a.N * vh * vw * CELL_BYTES;
    const u64 chunks = (total + 15) / 16;
    // up to four chunks per lane, fewer while that would leave the chip short of workgroups
    int iters = 4;
    while (iters > 1 && chunks / ((u64)iters * RENDER_THREADS) < 2048) iters >>= 1;
    const u64 per_group = (u64)iters * RENDER_THREADS;
    const u64 grid = (chunks + per_group - 1) / per_group;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    // view rows a run can touch: run / (588 vw) rounded up, plus one at each end
    const size_t lds = 4 * ((size_t)(per_group * 16 / CELL_BYTES) + 3 * (size_t)vw + 4);
    const bool stage = variant == 2 ? true : (variant == 1 ? false : RENDER_DEFAULT_STAGE);
    if (stage && lds <= 48 * 1024)
        hipLaunchKernelGGL(k_render<true>, dim3((unsigned)grid), dim3(RENDER_THREADS), lds, stream, a, vh, vw, total, iters);
    else
        hipLaunchKernelGGL(k_render<false>, dim3((unsigned)grid), dim3(RENDER_THREADS), 0, stream, a, vh, vw, total, iters);
    return hipGetLastError();
}

}  // namespace sl
