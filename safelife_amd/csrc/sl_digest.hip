// sl_digest.hip -- a 64-bit integrity checksum of a table of device memory segments, without a host copy: what a checkpoint
// uses to tell that the state it uploaded is the state it saved, and what two runs use to compare their whole state.  NOT a
// cryptographic hash.
//
// The definition (include/safelife_hip.h; all arithmetic mod 2^64, mix = splitmix64's finaliser, G = 0x9E3779B97F4A7C15): a
// segment of n bytes is ceil(n / 8) little-endian words w_i, bytes past n counting as zero, and
//     acc    = sum_i mix(w_i + mix(salt) + (i + 1) * G)
//     digest = mix(acc + mix((salt ^ n) + G))
// The sum is an integer sum: any split of it over lanes and workgroups gives the same bits, so nothing below needs an order.
//
//   k_digest_chunks   a capped grid, grid-stride over the CHUNKS of all segments: chunk g belongs to the segment s with
//                     prefix[s] <= g < prefix[s + 1] (binary search in the host-built prefix table at the head of the
//                     workspace).  A huge segment is thousands of chunks dealt over the whole grid, a 4-byte counter one
//                     chunk: neither waits for the other.  The workgroup's sum of its chunk -- a butterfly over the
//                     wavefront, the four waves through LDS -- is ONE plain store into the chunk's slot of the slab.
//   k_digest_finish   one wavefront per segment: its slots of the slab, the length term, the last mix.
// No atomics and no floating point anywhere; the inputs are only read.
//
// Alignment.  A segment may start at any byte.  With r = ptr & 7 and q_j the ALIGNED 8-byte word at (ptr - r) + 8 j,
//     w_i = q_i                                    (r == 0)
//     w_i = q_i >> 8 r  |  q_(i+1) << (64 - 8 r)   (r != 0)
// A word is INTERIOR when every aligned word it is made of lies wholly inside [ptr, ptr + n); interior words are read with
// aligned loads, 16 bytes (two words) per lane -- plus the one aligned word behind them when r != 0, which the neighbouring
// lane has just pulled into the cache.  The few words that are not interior -- the first when r != 0, the last one or two --
// are put together BYTEWISE, each byte bounds-checked against n: the kernel never reads a byte outside [ptr, ptr + n), not even
// inside the allocation's granule.  Chunks are cut at 16-byte ALIGNED addresses (word i sits in chunk (i + odd) / CHUNK_WORDS,
// odd = bit 3 of the address of q_0), so a segment has n_words / CHUNK_WORDS + 1 chunks whatever its alignment and the prefix
// table depends on the byte counts alone; the last chunk may be empty and then adds zero.
#include "sl_kernels.h"

namespace sl {
namespace {

typedef unsigned long long u64;

constexpr int DIGEST_THREADS = 256;
constexpr int DIGEST_WAVES = DIGEST_THREADS / 64;
constexpr int CHUNK_WORDS = 4096;                               // 32 KiB: 8 rounds of 16 bytes per lane
constexpr int CHUNK_PAIRS = CHUNK_WORDS / 2;
constexpr int CHUNK_ROUNDS = CHUNK_PAIRS / DIGEST_THREADS;
constexpr int DIGEST_GRID = 2048;                               // 8 workgroups for each of the 256 CUs
constexpr u64 GOLDEN = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ u64 mix64(u64 z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

__host__ __device__ __forceinline__ u64 chunks_of(u64 bytes) { return ((bytes + 7) >> 3) / CHUNK_WORDS + 1; }

typedef u64 ulong2_t __attribute__((ext_vector_type(2)));       // one 16-byte load

// The segments' pointers come out of a table in memory, so the compiler cannot know that they point into global memory and
// would emit flat loads; every segment IS device memory, and saying so gives global loads.
#define SL_GLOBAL __attribute__((address_space(1)))
typedef const SL_GLOBAL unsigned char *gbytes;
typedef const SL_GLOBAL u64 *gwords;
typedef const SL_GLOBAL ulong2_t *gpairs;

// word i of the segment, byte by byte; nothing at or past `n` is touched
__device__ __forceinline__ u64 word_bytewise(gbytes p, u64 n, u64 i) {
    u64 w = 0;
    const u64 base = i << 3;
    for (int b = 0; b < 8; ++b)
        if (base + b < n) w |= (u64)p[base + b] << (8 * b);
    return w;
}

__global__ __launch_bounds__(DIGEST_THREADS) void k_digest_chunks(const sl_digest_segment *__restrict__ segments,
                                                                  int n_segments, u64 salt_mix,
                                                                  const u64 *__restrict__ prefix, u64 *__restrict__ slab) {
    __shared__ u64 wave_part[DIGEST_WAVES];
    const u64 total = prefix[n_segments];
    const int t = threadIdx.x;
    for (u64 g = blockIdx.x; g < total; g += gridDim.x) {
        // the segment of chunk g: the last s with prefix[s] <= g.  Every lane makes the same search and reads the same
        // table entry again for every chunk -- on purpose: the addresses are uniform, so the loads are broadcasts out of the
        // cache, about log2(n_segments) of them, and nothing has to be shared through LDS.  For a table of thousands of tiny
        // segments this search IS most of the work of a chunk, and still far below the launch's own cost.
        int lo_s = 0, hi_s = n_segments - 1;
        while (lo_s < hi_s) {
            const int mid = (lo_s + hi_s + 1) >> 1;
            if (prefix[mid] <= g) lo_s = mid; else hi_s = mid - 1;
        }
        const gbytes p = (gbytes)segments[lo_s].ptr;
        const u64 n = segments[lo_s].bytes;
        const u64 c = g - prefix[lo_s];
        const u64 nw = (n + 7) >> 3;
        const unsigned r = (unsigned)((uintptr_t)p & 7);
        const gwords q = (gwords)(p - r);                       // q[j] is dereferenced for interior words only
        const u64 odd = ((uintptr_t)q >> 3) & 1;
        // interior words: [first, last]  (last < first: none)
        const long long first = r ? 1 : 0;
        const long long last = r ? (long long)((n + r) >> 3) - 2 : (long long)(n >> 3) - 1;
        // the chunk's words: i = v - odd for v in [c * CHUNK_WORDS, (c + 1) * CHUNK_WORDS)
        const long long i_begin = (long long)(c * CHUNK_WORDS) - (long long)odd;
        u64 acc = 0;
        if (i_begin >= first && i_begin + CHUNK_WORDS - 1 <= last) {
            // the whole chunk is interior: every load first, then the arithmetic
            ulong2_t v[CHUNK_ROUNDS];
            u64 nx[CHUNK_ROUNDS];
#pragma unroll
            for (int m = 0; m < CHUNK_ROUNDS; ++m) {
                const long long i = i_begin + 2 * (t + m * DIGEST_THREADS);
                v[m] = *(gpairs)(q + i);
                nx[m] = r ? q[i + 2] : 0;
            }
            u64 k = salt_mix + (u64)(i_begin + 2 * t + 1) * GOLDEN;
#pragma unroll
            for (int m = 0; m < CHUNK_ROUNDS; ++m) {
                u64 w0 = v[m].x, w1 = v[m].y;
                if (r) {
                    w0 = (v[m].x >> (8 * r)) | (v[m].y << (64 - 8 * r));
                    w1 = (v[m].y >> (8 * r)) | (nx[m] << (64 - 8 * r));
                }
                acc += mix64(w0 + k) + mix64(w1 + k + GOLDEN);
                k += (u64)(2 * DIGEST_THREADS) * GOLDEN;
            }
        } else {
            for (int m = 0; m < CHUNK_ROUNDS; ++m) {
                const long long i = i_begin + 2 * (t + m * DIGEST_THREADS);
                if (i + 1 < 0 || i >= (long long)nw) continue;
                if (i >= first && i + 1 <= last) {
                    const ulong2_t v = *(gpairs)(q + i);
                    u64 w0 = v.x, w1 = v.y;
                    if (r) {
                        const u64 nx = q[i + 2];
                        w0 = (v.x >> (8 * r)) | (v.y << (64 - 8 * r));
                        w1 = (v.y >> (8 * r)) | (nx << (64 - 8 * r));
                    }
                    const u64 k = salt_mix + (u64)(i + 1) * GOLDEN;
                    acc += mix64(w0 + k) + mix64(w1 + k + GOLDEN);
                } else {
                    for (long long j = i; j <= i + 1; ++j)
                        if (j >= 0 && j < (long long)nw)
                            acc += mix64(word_bytewise(p, n, (u64)j) + salt_mix + (u64)(j + 1) * GOLDEN);
                }
            }
        }
        for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
        if ((t & 63) == 0) wave_part[t >> 6] = acc;
        __syncthreads();
        if (t == 0) {
            u64 sum = 0;
            for (int w = 0; w < DIGEST_WAVES; ++w) sum += wave_part[w];
            slab[g] = sum;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_digest_finish(const sl_digest_segment *__restrict__ segments, u64 salt,
                                                      const u64 *__restrict__ prefix, const u64 *__restrict__ slab,
                                                      u64 *__restrict__ out) {
    const int s = blockIdx.x;
    u64 acc = 0;
    for (u64 g = prefix[s] + threadIdx.x; g < prefix[s + 1]; g += 64) acc += slab[g];
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if (threadIdx.x == 0) out[s] = mix64(acc + mix64((salt ^ segments[s].bytes) + GOLDEN));
}

}  // namespace

size_t digest_workspace_bytes(const unsigned long long *bytes, int n_segments) {
    u64 total = 0;
    for (int s = 0; s < n_segments; ++s) total += chunks_of(bytes[s]);
    return (size_t)((u64)(n_segments + 1) + total) * sizeof(u64);
}

void digest_prefix(const unsigned long long *bytes, int n_segments, unsigned long long *prefix_out) {
    u64 total = 0;
    for (int s = 0; s < n_segments; ++s) {
        prefix_out[s] = total;
        total += chunks_of(bytes[s]);
    }
    prefix_out[n_segments] = total;
}

hipError_t launch_state_digest(const sl_digest_segment *segments, int n_segments, unsigned long long salt,
                               unsigned long long *out, void *workspace, hipStream_t stream) {
    const u64 *prefix = (const u64 *)workspace;
    u64 *slab = (u64 *)workspace + (n_segments + 1);
    hipLaunchKernelGGL(k_digest_chunks, dim3(DIGEST_GRID), dim3(DIGEST_THREADS), 0, stream, segments, n_segments,
                       mix64(salt), prefix, slab);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(k_digest_finish, dim3(n_segments), dim3(64), 0, stream, segments, (u64)salt, prefix,
                       (const u64 *)slab, out);
    return hipGetLastError();
}

}  // namespace sl
