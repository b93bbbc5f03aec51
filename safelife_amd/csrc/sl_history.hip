// sl_history.hip -- episode histories on the device: the board frames of selected episodes, what the reference's
// SafeLifeLogWrapper records per step and SafeLifeLogger.log_episode keeps every video_interval-th episode
// (safelife_logger.py:560-592, :338-347).  The model -- watched envs, slots, the free order, the interval rule over the
// episode log's row numbering -- is spelled out in include/safelife_hip.h next to the entry points and restated in
// tests/episode_history_ref.py.  No step kernel changes: these kernels run on the caller's stream behind the fused step.
//
//   k_history_book<REWIND,R> ONE workgroup.  Capture: the done flags of all B envs as 64-bit masks per lane and one workgroup
//                            scan per tile of 16384 envs (the structure of k_episode_log_harvest) give every watched env the
//                            number of done envs below it; the queue entries pushed since the cursor go through LDS a chunk at
//                            a time and the lane of a watched env whose episode ended walks them for its (env, episode_idx)
//                            -- the first hit, so the smallest index; a scan over the K slot states lists the free slots
//                            in ascending order and a scan over the watched envs that need one hands the r-th of them the r-th
//                            free slot.  Nothing is freed inside a call, so that matching IS "ascending env order, lowest free
//                            slot first".  One lane per watched env then writes its own owner / cur_* / entry / slot states
//                            and its copy order.
//                            Rewind: the last two steps only, for the envs the mask names.  The loads that wait for no scan
//                            -- counters, queue end, the lane's watched env and its records, its slot state, its first queue
//                            entry -- are issued first: the kernel is one workgroup's latency chain, and they run under it.
//   k_history_copy           grid (watched env, {frame, goals plane}): carries the orders out.  Source and destination are
//                            boards of H*W 2-byte cells at arbitrary 2-byte alignment (1250 bytes for 25x25); the widest of
//                            16 / 8 / 4 / 2 bytes that divides both addresses moves the bulk, 2-byte accesses the rest.
//
// The pass has ONE body under both env classes: R, the record reader, is all that knows whether `out` holds one record per
// env (records_single) or A per env (records_multi: an episode ends when ALL agents are done, its length is the largest
// of theirs, success a bit per agent, the live frame index comes from num_steps).  Every other line is shared.
//
// Every write goes to a place only its writer owns (a watched env's own records, the slot it owns or was just matched with),
// the counters are written by lane 0 behind the last barrier, and there are no global atomics.
#include "sl_kernels.h"

namespace sl {
namespace {

constexpr int HIST_THREADS = 256;
constexpr int HIST_PER_LANE = 64;                               // envs a lane places per tile of the done scan
constexpr int HIST_TILE = HIST_THREADS * HIST_PER_LANE;
constexpr int NO_ENTRY = 0x7FFFFFFF;
enum { SRC_NONE = 0, SRC_BOARD = 1, SRC_QUEUE = 2 };

// what the lane of watched env i reads of it: issued in front of the scans, so that these round trips run under them
struct watched {
    int e, s, level, episode, length_now, cur_episode, cur_level;
    sl_step_out o;
    bool valid, in;
};

// ---- the record readers: what k_history_book asks of `out`

struct records_single {                                         // out [B]
    static constexpr bool MULTI = false;
    const sl_step_out *__restrict__ out;

    // one byte per env of the tile: 0 / 1 (independent loads, eight in flight per lane: no load stands behind a per-lane
    // condition)
    __device__ __forceinline__ void stage(uint8_t *flag, const uint8_t *__restrict__ mask, int tile, int nt) const {
        if (!mask) {
#pragma unroll 8
            for (int i = threadIdx.x; i < nt; i += HIST_THREADS) flag[i] = out[tile + i].done != 0 ? 1 : 0;
        } else {
#pragma unroll 8
            for (int i = threadIdx.x; i < nt; i += HIST_THREADS)
                flag[i] = ((out[tile + i].done != 0) & (mask[tile + i] != 0)) ? 1 : 0;
        }
    }
    __device__ __forceinline__ bool done(int e) const { return out[e].done != 0; }
    __device__ __forceinline__ sl_step_out episode(int e) const { return out[e]; }
    __device__ __forceinline__ int length_now(const sl_env_scalars *sc) const { return sc->episode_length; }
    __device__ __forceinline__ uint8_t agents() const { return 0; }
};

struct records_multi {                                          // out [B, A]
    static constexpr bool MULTI = true;
    const sl_step_out *__restrict__ out;
    const int A;

    // every env of the tile starts as finished (if the mask lets it count); then the nt * A records come in as one flat,
    // coalesced stream of independent loads (sixteen in flight per lane -- the load is unconditional, only the LDS store hangs
    // on what it brought) and a record that is not done clears its env's flag: every writer of a byte writes the same 0.
    // In a kernel trace at 8192 envs of 2 agents the pass takes 12.6 us this way; 14.4 with eight loads in flight and the
    // record's env a division by the run-time A, and 14.2 with one lane per env ANDing its A records (no clearing pass, no
    // barrier, but loads of 32 bytes a lane apart).
    template <int AC>
    static __device__ __forceinline__ void clear(uint8_t *flag, const sl_step_out *__restrict__ rec, int n) {
#pragma unroll 16
        for (int j = threadIdx.x; j < n; j += HIST_THREADS)
            if (rec[j].done == 0) flag[j / AC] = 0;
    }
    __device__ __forceinline__ void stage(uint8_t *flag, const uint8_t *__restrict__ mask, int tile, int nt) const {
        if (!mask) {
            for (int i = threadIdx.x; i < nt; i += HIST_THREADS) flag[i] = 1;
        } else {
#pragma unroll 8
            for (int i = threadIdx.x; i < nt; i += HIST_THREADS) flag[i] = mask[tile + i] != 0 ? 1 : 0;
        }
        __syncthreads();
        const sl_step_out *rec = out + (long long)tile * A;
        switch (A) {                                            // (uniform: the record's env is a division by a constant)
        case 1: clear<1>(flag, rec, nt); break;
        case 2: clear<2>(flag, rec, nt * 2); break;
        case 3: clear<3>(flag, rec, nt * 3); break;
        case 4: clear<4>(flag, rec, nt * 4); break;
        case 5: clear<5>(flag, rec, nt * 5); break;
        case 6: clear<6>(flag, rec, nt * 6); break;
        case 7: clear<7>(flag, rec, nt * 7); break;
        default: clear<8>(flag, rec, nt * 8); break;
        }
    }
    // SL_MAX_AGENTS loads whatever A is, at a clamped index: agent A - 1 read again changes neither an AND, an OR nor a
    // maximum, so only the success bit asks which agent a load belongs to, and no load waits for a condition
    __device__ __forceinline__ sl_step_out episode(int e) const {
        const sl_step_out *rec = out + (long long)e * A;
        sl_step_out s = rec[0];
        s.done = s.done != 0, s.success = s.success != 0, s.times_up = s.times_up != 0, s.reserved = 0;
#pragma unroll
        for (int a = 1; a < SL_MAX_AGENTS; ++a) {
            const sl_step_out o = rec[min(a, A - 1)];
            s.done &= o.done != 0;
            s.success |= (a < A && o.success != 0) << a;
            s.times_up |= o.times_up != 0;
            s.episode_length = max(s.episode_length, o.episode_length);
        }
        return s;
    }
    __device__ __forceinline__ bool done(int e) const {
        const sl_step_out *rec = out + (long long)e * A;
        bool all = true;
#pragma unroll
        for (int a = 0; a < SL_MAX_AGENTS; ++a) all &= rec[min(a, A - 1)].done != 0;
        return all;
    }
    // (the multi-agent kernels count the env's steps in num_steps and zero it on reload; they keep no env-wide episode_length)
    __device__ __forceinline__ int length_now(const sl_env_scalars *sc) const { return sc->num_steps; }
    __device__ __forceinline__ uint8_t agents() const { return (uint8_t)A; }
};

template <bool REWIND, typename R>
__device__ __forceinline__ watched load_watched(const sl_episode_history &h, const sl_env_scalars *__restrict__ scalars,
                                                const R &rd, const uint8_t *__restrict__ mask, int i) {
    // Every load is made, at a clamped index, and what a lane has no right to is thrown away afterwards: a load under a
    // per-lane condition is a branch with a wait behind it, and these are meant to be in flight together.
    watched w;
    w.valid = i < h.n_watch;
    const int ic = min(i, h.n_watch - 1);
    w.e = h.watch[ic];
    w.s = w.valid ? h.owner[ic] : -1;
    w.cur_level = h.cur_level[ic];
    w.cur_episode = h.cur_episode[ic];
    const int ec = min(max(w.e, 0), h.B - 1);
    const int on = mask ? mask[ec] : 1;                         // (mask is uniform)
    const sl_env_scalars *sc = scalars + ec;
    w.level = sc->level_idx, w.episode = sc->episode_idx, w.length_now = rd.length_now(sc);
    if (!REWIND) {
        w.o = rd.episode(ec);
    } else {
        w.o.reward = w.o.episode_reward = 0.0f;
        w.o.done = w.o.success = w.o.times_up = w.o.reserved = 0, w.o.episode_length = 0;
    }
    w.in = w.valid && w.e == ec && on != 0;
    if (!w.in) w.o.done = 0;
    return w;
}

template <bool REWIND, typename R>
__global__ __launch_bounds__(HIST_THREADS) void k_history_book(sl_episode_history h, const sl_env_scalars *__restrict__ scalars,
                                                               const R rd, sl_episode_queue queue,
                                                               const uint8_t *__restrict__ mask) {
    __shared__ int wave_sum[HIST_THREADS / 64];
    __shared__ uint32_t flags[HIST_TILE / 4];                   // one byte per env of the tile: 0 / 1
    __shared__ unsigned long long lane_mask[HIST_THREADS];
    __shared__ int lane_place[HIST_THREADS];
    __shared__ int rank[SL_HIST_MAX_WATCH];                     // done envs below watched env i
    __shared__ int final_j[SL_HIST_MAX_WATCH];                  // queue entry of its current episode, or NO_ENTRY
    __shared__ int free_list[SL_HIST_MAX_SLOTS];                // the free slots, ascending
    __shared__ int q_env[HIST_THREADS], q_episode[HIST_THREADS];        // a chunk of the queue's new entries
    __shared__ int tally[3];                                    // kept, missed, incomplete
    const int tid = threadIdx.x, n = h.n_watch, K = h.n_slots, B = h.B;
    // Everything that does not depend on a scan is asked for here, first: the counters (written below, behind the last
    // barrier), the queue's end, this lane's watched env of the first chunk, its slot state, its first queue entry.
    const long long episodes = h.counters[0];
    int q_first = 0, q_end = 0;
    if (!REWIND && queue.capacity > 0) {
        q_end = min(max(*queue.count, 0), queue.capacity);
        q_first = (int)min(max(h.counters[4], 0ll), (long long)q_end);
    }
    const watched w0 = load_watched<REWIND>(h, scalars, rd, mask, tid);
    const int state0 = h.slot_state[min(tid, K - 1)];
    int env0 = -1, episode0 = 0;
    if (q_first < q_end) {                                      // (uniform)
        const sl_episode_record *rec = queue.records + min(q_first + tid, q_end - 1);
        env0 = q_first + tid < q_end ? rec->env - queue.env_base : -1, episode0 = rec->episode_idx;
    }
    int total_done = 0;

    for (int i = tid; i < n; i += HIST_THREADS) rank[i] = 0, final_j[i] = NO_ENTRY;
    if (tid < 3) tally[tid] = 0;
    if (!REWIND) {
        uint8_t *flag = (uint8_t *)flags;
        for (int tile = 0; tile < B; tile += HIST_TILE) {
            const int nt = min(HIST_TILE, B - tile);
            __syncthreads();                                    // (the previous tile's flags and places have been read)
            rd.stage(flag, mask, tile, nt);
            for (int i = nt + tid; i < ((nt + 63) & ~63); i += HIST_THREADS) flag[i] = 0;
            __syncthreads();
            const int lo = tid * HIST_PER_LANE;
            unsigned long long m = 0;                           // bit i: env tile + lo + i is done
            if (lo < nt) { SL_FLAG_BYTES_TO_MASK(m, flags, lo, HIST_PER_LANE); }
            int n_tile = 0;
            const int place = block_exclusive_scan<HIST_THREADS>(__popcll(m), wave_sum, n_tile);
            lane_mask[tid] = m;
            lane_place[tid] = place;
            __syncthreads();
            for (int i = tid; i < n; i += HIST_THREADS) {
                const int at = (i == tid ? w0.e : h.watch[i]) - tile;
                if (at >= 0 && at < nt) {
                    const int l = at / HIST_PER_LANE, b = at % HIST_PER_LANE;
                    rank[i] = total_done + lane_place[l] + __popcll(lane_mask[l] & ((1ull << b) - 1ull));
                }
            }
            total_done += n_tile;
        }
        // The queue entries pushed since the recorder last looked, a chunk at a time through LDS; the lane of a watched env
        // whose episode ended walks the chunk for its (env, episode_idx) and keeps the first hit -- chunks and entries in
        // ascending order, so that is the smallest index.  final_j[i] has one writer: no atomics.
        for (int jb = q_first; jb < q_end; jb += HIST_THREADS) {            // (uniform bounds)
            int env = -1, episode = 0;
            if (jb == q_first) {
                env = env0, episode = episode0;
            } else if (jb + tid < q_end) {
                const sl_episode_record *rec = queue.records + jb + tid;
                env = rec->env - queue.env_base, episode = rec->episode_idx;
            }
            __syncthreads();                                    // (the previous chunk has been walked)
            q_env[tid] = env, q_episode[tid] = episode;
            __syncthreads();
            const int cnt = min(HIST_THREADS, q_end - jb);
            for (int base = 0; base < n; base += HIST_THREADS) {
                const int i = base + tid;
                if (i >= n) continue;
                int e = w0.e, ce = w0.cur_episode;
                bool done = w0.in && w0.o.done != 0;
                if (base > 0) {
                    e = h.watch[i], ce = h.cur_episode[i];
                    done = e >= 0 && e < B && (!mask || mask[e] != 0) && rd.done(e);
                }
                if (!done || final_j[i] != NO_ENTRY) continue;
                for (int k = 0; k < cnt; ++k)
                    if (q_env[k] == e && q_episode[k] == ce) {
                        final_j[i] = jb + k;
                        break;
                    }
            }
        }
    }
    // the free slots in ascending order (slot_state as the call found it: it is written behind the barrier below)
    int n_free = 0;
    for (int base = 0; base < K; base += HIST_THREADS) {
        const int s = base + tid;
        const int state = base == 0 ? state0 : h.slot_state[min(s, K - 1)];
        const int is_free = s < K && state == SL_HIST_SLOT_FREE ? 1 : 0;
        int n_here = 0;
        const int p = block_exclusive_scan<HIST_THREADS>(is_free, wave_sum, n_here);
        if (is_free) free_list[n_free + p] = s;
        n_free += n_here;
    }
    __syncthreads();                                            // (free_list, final_j and rank have settled)
    int needers = 0;                                            // watched envs below this chunk that needed a slot
    for (int base = 0; base < n; base += HIST_THREADS) {
        const int i = base + tid;
        const watched w = base == 0 ? w0 : load_watched<REWIND>(h, scalars, rd, mask, i);
        const sl_step_out o = w.o;
        const int e = w.e;
        int s = w.s;
        const bool done = !REWIND && w.in && o.done != 0;
        const bool starts = REWIND ? w.in : done;
        const long long number = episodes + rank[w.valid ? i : 0];
        const bool by_rule = done && number % h.interval == 0;
        const bool kept = by_rule && s >= 0 && s < K;
        const bool need = starts && (kept || s < 0);
        int n_need = 0;
        const int r = needers + block_exclusive_scan<HIST_THREADS>(need ? 1 : 0, wave_sum, n_need);
        needers += n_need;
        if (!w.valid) continue;                                 // (behind the scan: every lane has been through its barriers)
        int src = SRC_NONE, src_index = 0, slot = -1, frame = -1, goals_slot = -1;
        if (!REWIND && w.in && !done && s >= 0 && s < K) src = SRC_BOARD, slot = s, frame = w.length_now - 1;
        if (by_rule && !kept) atomicAdd(&tally[1], 1);
        if (kept) {
            const int j = final_j[i];
            sl_history_entry en;
            en.row = number;
            en.env = e, en.level = w.cur_level, en.episode_idx = w.cur_episode;
            en.length = o.episode_length, en.slot = s;
            en.success = o.success, en.times_up = o.times_up;
            en.flags = SL_HIST_LIVE | (j == NO_ENTRY ? SL_HIST_NO_FINAL : 0), en.reserved = rd.agents();
            h.entries[s] = en;
            h.slot_state[s] = SL_HIST_SLOT_ENTRY;
            atomicAdd(&tally[0], 1);
            if (j == NO_ENTRY)
                atomicAdd(&tally[2], 1);
            else
                src = SRC_QUEUE, src_index = j, slot = s, frame = o.episode_length - 1;
            s = -1;
        }
        if (need) {
            s = r < n_free ? free_list[r] : -1;
            if (s >= 0) h.slot_state[s] = SL_HIST_SLOT_ENV;
        }
        if (starts) {
            h.owner[i] = s;
            h.cur_level[i] = w.level;
            h.cur_episode[i] = w.episode;
            goals_slot = s >= 0 && s < K ? s : -1;
        }
        if (frame < 0 || frame >= h.T) src = SRC_NONE;          // (a frame outside the slot is not written)
        int4 *ord = reinterpret_cast<int4 *>(h.orders + (long long)i * SL_HIST_ORDER_WORDS);
        ord[0] = make_int4(src, src_index, slot, frame);
        ord[1] = make_int4(goals_slot, 0, 0, 0);
    }
    __syncthreads();                                            // (the tallies are complete)
    if (!REWIND && tid == 0) {
        h.counters[0] = episodes + total_done;
        h.counters[1] += tally[0];
        h.counters[2] += tally[1];
        h.counters[3] += tally[2];
        if (queue.capacity > 0) h.counters[4] = q_end;
    }
}

template <typename V>
__device__ __forceinline__ void copy_as(uint16_t *__restrict__ dst, const uint16_t *__restrict__ src, int cells) {
    constexpr int PER = sizeof(V) / 2;                          // cells per access
    const int n_vec = cells / PER;
    const V *s = reinterpret_cast<const V *>(src);
    V *d = reinterpret_cast<V *>(dst);
    for (int k = threadIdx.x; k < n_vec; k += HIST_THREADS) d[k] = s[k];
    for (int k = n_vec * PER + threadIdx.x; k < cells; k += HIST_THREADS) dst[k] = src[k];
}

// `cells` 2-byte cells from src to dst, by the whole workgroup (every condition is uniform over it)
__device__ __forceinline__ void copy_cells(uint16_t *dst, const uint16_t *src, int cells) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src);
    if ((a & 15) == 0)
        copy_as<uint4>(dst, src, cells);
    else if ((a & 7) == 0)
        copy_as<uint2>(dst, src, cells);
    else if ((a & 3) == 0)
        copy_as<uint32_t>(dst, src, cells);
    else
        copy_as<uint16_t>(dst, src, cells);
}

__global__ __launch_bounds__(HIST_THREADS) void k_history_copy(sl_episode_history h, const uint16_t *__restrict__ board,
                                                               const uint16_t *__restrict__ goals,
                                                               const uint16_t *__restrict__ queue_boards, int queue_capacity) {
    const int i = blockIdx.x;
    if (i >= h.n_watch) return;
    const int e = h.watch[i];
    if (e < 0 || e >= h.B) return;
    const int32_t *ord = h.orders + (long long)i * SL_HIST_ORDER_WORDS;
    const size_t HW = (size_t)h.H * h.W;
    if (blockIdx.y == 0) {
        const int src = ord[0], j = ord[1], slot = ord[2], frame = ord[3];
        if (slot < 0 || slot >= h.n_slots || frame < 0 || frame >= h.T) return;
        uint16_t *dst = h.frames + ((size_t)slot * h.T + frame) * HW;
        if (src == SRC_BOARD && board)
            copy_cells(dst, board + (size_t)e * HW, (int)HW);
        else if (src == SRC_QUEUE && queue_boards && j >= 0 && j < queue_capacity)
            copy_cells(dst, queue_boards + (size_t)j * HW, (int)HW);
    } else {
        const int slot = ord[4];
        if (slot < 0 || slot >= h.n_slots || !goals) return;
        copy_cells(h.goals + (size_t)slot * HW, goals + (size_t)e * HW, (int)HW);
    }
}

}  // namespace

hipError_t launch_history_capture(const sl_episode_history &h, const uint16_t *board, const uint16_t *goals,
                                  const sl_env_scalars *scalars, const sl_step_out *out, const sl_episode_queue &queue,
                                  const uint8_t *active, hipStream_t stream) {
    hipLaunchKernelGGL((k_history_book<false, records_single>), dim3(1), dim3(HIST_THREADS), 0, stream, h, scalars,
                       records_single{out}, queue, active);
    if (hipError_t err = hipGetLastError()) return err;
    hipLaunchKernelGGL(k_history_copy, dim3(h.n_watch, 2), dim3(HIST_THREADS), 0, stream, h, board, goals,
                       (const uint16_t *)queue.boards, queue.capacity);
    return hipGetLastError();
}

hipError_t launch_history_capture_multi(const sl_episode_history &h, const uint16_t *board, const uint16_t *goals,
                                        const sl_env_scalars *scalars, const sl_step_out *out, int n_agents,
                                        const sl_episode_queue &queue, const uint8_t *active, hipStream_t stream) {
    hipLaunchKernelGGL((k_history_book<false, records_multi>), dim3(1), dim3(HIST_THREADS), 0, stream, h, scalars,
                       records_multi{out, n_agents}, queue, active);
    if (hipError_t err = hipGetLastError()) return err;
    hipLaunchKernelGGL(k_history_copy, dim3(h.n_watch, 2), dim3(HIST_THREADS), 0, stream, h, board, goals,
                       (const uint16_t *)queue.boards, queue.capacity);
    return hipGetLastError();
}

hipError_t launch_history_rewind(const sl_episode_history &h, const uint16_t *goals, const sl_env_scalars *scalars,
                                 const uint8_t *mask, hipStream_t stream) {
    sl_episode_queue none;
    none.capacity = 0, none.env_base = 0, none.count = nullptr, none.records = nullptr, none.boards = nullptr;
    // (a rewind reads no record: of the env only level_idx, episode_idx and, in the copy pass, goals -- what both env classes keep)
    hipLaunchKernelGGL((k_history_book<true, records_single>), dim3(1), dim3(HIST_THREADS), 0, stream, h, scalars,
                       records_single{nullptr}, none, mask);
    if (hipError_t err = hipGetLastError()) return err;
    hipLaunchKernelGGL(k_history_copy, dim3(h.n_watch, 2), dim3(HIST_THREADS), 0, stream, h, (const uint16_t *)nullptr, goals,
                       (const uint16_t *)nullptr, 0);
    return hipGetLastError();
}

}  // namespace sl
