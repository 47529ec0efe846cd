// rhj_stats_batch.hip.h — the column statistics of many columns in the three launches of one
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// The optimiser's statistics of a column (relation_map.c:53-84): l = min, u = max, d = the number of flags set when every
// value sets flag v - l (a range u - l + 1 of 50 000 000 or more: flag (v - l) % 5 000 000).  rhj_column_stats_device
// (csrc/rhj_inter.hip) does that for one column with three launches, two stream waits and one byte per flag;
// rhj_column_stats_batch_device runs N columns as THREE launches and two stream waits per chunk, with one BIT per flag:
//   k_statsbatch_minmax  grid = the 2048-row tiles of the chunk's columns, one behind the other: every workgroup reduces its
//                        tile and issues one atomic min and one atomic max into the column's two words (each only where an
//                        agent-scope load of the word shows that it can move it)
//   (the host reads the extremes back, places every column's bitmap in the arena and zeroes the span the chunk uses)
//   k_statsbatch_mark    the same grid: flag x = v - l (folded) is bit x & 31 of word x >> 5 of the column's bitmap
//   k_statsbatch_count   grid = the 2048-word tiles of the chunk's bitmaps: popcounts, one atomic add a workgroup into the
//                        column's count word
// A workgroup finds its column by a binary search in the chunk's array of tile starts (fbatch_find) and reads the column's
// StatsDesc from a device array; both come through const __restrict__ kernel arguments and are read at a workgroup-uniform
// index, so the fields arrive by scalar loads as kernel arguments do.  What the kernels write — a
// column's min, max and count words — lies outside the descriptors, in the same uploaded block: the block carries ~0, 0
// and 0 for them, so nothing is memset.
//
// A thread's 8 rows are tile * 2048 + round * 256 + thread (8-byte loads), or, where the column starts on a 16-byte boundary
// and the tile is whole, the four pairs tile * 2048 + round * 512 + 2 * thread (16-byte loads).  The branch is
// workgroup-uniform and outside the rounds, so that a thread's loads are in flight together; a row out of bounds reads row 0
// in its place (n >= 1): a value of the column, which changes neither the extremes nor the set of flags.
#pragma once
#include "rhj.h"
#include "rhj_inter.h"
#include "rhj_filter_batch.hip.h"

namespace rhj {

constexpr int STATS_ROUNDS = 8;
constexpr uint32_t STATS_TILE = 2048;                // 256 threads x 8 rows
constexpr uint32_t STATS_WORD_TILE = 2048;           // k_statsbatch_count: 256 threads x 8 bitmap words
constexpr uint64_t STATS_CAP = 50000000;             // a range below this: one flag per value (relation_map.c:66)
constexpr uint64_t STATS_FOLD = 5000000;             // at or above: (v - l) % STATS_FOLD (relation_map.c:74)

struct StatsDesc {
    const uint64_t     *col;
    uint64_t            n;       // >= 1
    unsigned long long *words;   // min, max, count: ~0, 0, 0 at launch
    uint32_t           *bits;    // the column's bitmap in the arena, zero at launch (set after the extremes are known)
    uint64_t            lo;      // the column's minimum (the same)
    uint32_t            fold;    // 0, or STATS_FOLD
    uint32_t            nwords;  // 32-bit words of the bitmap
};

typedef __attribute__((address_space(1))) uint32_t       *sb_gu32;
typedef const __attribute__((address_space(1))) uint32_t *sb_gcu32;

// the 8 rows of this thread of tile `tile`
__device__ __forceinline__ void statsbatch_rows(fb_gcu64 col, uint64_t n, uint32_t tile, uint64_t (&v)[STATS_ROUNDS])
{
    const uint64_t first = (uint64_t)tile * STATS_TILE;
    if (first + STATS_TILE <= n && ((uintptr_t)col & 15) == 0) {      // (workgroup-uniform)
#pragma unroll
        for (int k = 0; k < STATS_ROUNDS / 2; ++k) {
            const fb_u64x2 x = *(fb_gcu64x2)(col + first + (uint64_t)k * 512 + 2 * threadIdx.x);
            v[2 * k] = x.x; v[2 * k + 1] = x.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < STATS_ROUNDS; ++k) {
            const uint64_t i = first + (uint64_t)k * 256 + threadIdx.x;
            v[k] = col[i < n ? i : 0];                                // a row out of bounds reads row 0 in its place
        }
    }
}

__global__ __launch_bounds__(256) void k_statsbatch_minmax(const StatsDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t nc)
{
    __shared__ unsigned long long lo4[4], hi4[4];
    const uint32_t j = fbatch_find(tile_start, nc, blockIdx.x);
    const StatsDesc &d = descs[j];
    uint64_t v[STATS_ROUNDS];
    statsbatch_rows((fb_gcu64)d.col, d.n, blockIdx.x - tile_start[j], v);
    unsigned long long lo = v[0], hi = v[0];
#pragma unroll
    for (int k = 1; k < STATS_ROUNDS; ++k) {
        lo = v[k] < lo ? v[k] : lo;
        hi = v[k] > hi ? v[k] : hi;
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
        const unsigned long long a = __shfl_xor(lo, x, 64), b = __shfl_xor(hi, x, 64);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if ((threadIdx.x & 63) == 0) { lo4[threadIdx.x >> 6] = lo; hi4[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { lo = lo4[w] < lo ? lo4[w] : lo; hi = hi4[w] > hi ? hi4[w] : hi; }
        // A column of many tiles sends them all to the same two words; the minimum only ever falls and the maximum only ever
        // rises during the launch, so a workgroup that cannot move the word it reads (however old its view) leaves it alone.
        unsigned long long *mm = d.words;
        if (lo < __hip_atomic_load(&mm[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            __hip_atomic_fetch_min(&mm[0], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (hi > __hip_atomic_load(&mm[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            __hip_atomic_fetch_max(&mm[1], hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Bits are only ever set during the launch, so the plain load that looks at the word first may be stale at no cost but an
// atomic that was not needed; it never shows a bit that is not there (the words are zero when the launch begins).  (An
// agent-scope load in its place, which goes past the L1, measured slower: DESIGN.md 6.)
__device__ __forceinline__ void statsbatch_set(sb_gu32 bits, uint32_t x)
{
    const uint32_t bit = 1u << (x & 31);
    sb_gu32 w = bits + (x >> 5);
    if ((*w & bit) == 0) __hip_atomic_fetch_or((uint32_t *)w, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_statsbatch_mark(const StatsDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t nc)
{
    const uint32_t j = fbatch_find(tile_start, nc, blockIdx.x);
    const StatsDesc &d = descs[j];
    uint64_t v[STATS_ROUNDS];
    statsbatch_rows((fb_gcu64)d.col, d.n, blockIdx.x - tile_start[j], v);
    const uint64_t lo = d.lo;
    const sb_gu32 bits = (sb_gu32)d.bits;
    if (d.fold) {                                                     // (workgroup-uniform, outside the rounds)
#pragma unroll
        for (int k = 0; k < STATS_ROUNDS; ++k) statsbatch_set(bits, (uint32_t)((v[k] - lo) % STATS_FOLD));
    } else {
#pragma unroll
        for (int k = 0; k < STATS_ROUNDS; ++k) statsbatch_set(bits, (uint32_t)(v[k] - lo));     // below STATS_CAP
    }
}

__global__ __launch_bounds__(256) void k_statsbatch_count(const StatsDesc *__restrict__ descs, const uint32_t *__restrict__ wtile_start, uint32_t nc)
{
    __shared__ uint32_t part[4];
    const uint32_t j = fbatch_find(wtile_start, nc, blockIdx.x);
    const StatsDesc &d = descs[j];
    const sb_gcu32 bits = (sb_gcu32)d.bits;
    const uint32_t nwords = d.nwords;
    const uint32_t first = (blockIdx.x - wtile_start[j]) * STATS_WORD_TILE + threadIdx.x;
    uint32_t w[STATS_ROUNDS];
#pragma unroll
    for (int k = 0; k < STATS_ROUNDS; ++k) {
        const uint32_t i = first + (uint32_t)k * 256;
        w[k] = bits[i < nwords ? i : 0];
    }
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < STATS_ROUNDS; ++k) s += first + (uint32_t)k * 256 < nwords ? (uint32_t)__popc(w[k]) : 0u;
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) s += __shfl_xor(s, x, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long mine = (unsigned long long)part[0] + part[1] + part[2] + part[3];
        if (mine) __hip_atomic_fetch_add(&d.words[2], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace rhj
