// rhj_filter_batch.hip.h — many conjunctive filters in the two launches of one
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// A resident filter (rhj_filter.hip.h) is a mask launch, a write launch and a host round trip whatever its size: the 50
// filters of the contest's `small` batch are 50 round trips for microseconds of HBM time.  Filters on base relations are
// independent, so rhj_filter_batch_device runs N of them as ONE mask launch and ONE write launch and waits for the stream once:
//   k_fbatch_mask    grid = the 4096-element tiles of the chunk's filters, one behind the other
//   k_fbatch_write   one wave per pair of tiles over the filters' tasks, one behind the other, grid-stride
// A workgroup (a wave) finds its filter by a binary search in the chunk's array of tile (task) starts and reads that filter's
// FBatchDesc from a device array uploaded once per chunk.  Both arrays come through const __restrict__ kernel arguments and are
// read at a workgroup- (wave-) uniform index, so the fields arrive by scalar loads as kernel arguments do.
//
// A filter is a conjunction of up to RHJ_FILTER_MAX_TERMS predicates over columns of one relation.  The mask kernel keeps a
// round's two ballot words in SGPRs and ANDs every term's ballots into them, so only one term's 16 values a lane are live at a
// time; the mask layout is k_filter_mask's, and the write pass is k_filter_write<true>'s own body (filter_write_task).
//
// The batch of two-column equalities (rhj_eq2_batch.hip.h) is the same scheme over another descriptor, and what the two have
// in common is written once, here: fbatch_find, the bounds ballots (fbatch_bounds), the loads of one column through its optional
// row-id vector (fbatch_side), the mask store and tile count (fbatch_mask_round, fbatch_mask_count), and the whole write pass (fbatch_write_tasks, a
// template over the descriptor type; k_fbatch_write and k_eq2batch_write are its two instances).  A mask kernel keeps what is
// its own: the term loop with its early-out and three comparisons here, the two sides and one equality there.
#pragma once
#include "rhj.h"
#include "rhj_filter.hip.h"

namespace rhj {

struct FBatchTerm {
    const uint64_t *col;
    uint64_t        value;
    int             op;          // 0 '<', 1 '>', 2 '='
    int             pad;
};

struct FBatchDesc {
    const uint64_t     *sel;         // nullptr: every term scans col[0..n)
    uint64_t            n;
    uint64_t           *out;         // nullptr: count only
    uint64_t           *masks;       // 2 * ceil(n / 128) words, 16-byte aligned
    uint64_t           *tile_count;  // ceil(n / 4096) words
    unsigned long long *h_total;     // the filter's slot in the pinned host array of hit totals
    int                 nterms;
    int                 vec;         // the scanned vector of every term starts on a 16-byte boundary
    FBatchTerm          t[RHJ_FILTER_MAX_TERMS];
};

// A pointer read from a descriptor is a generic pointer to the compiler (flat loads); these name it as what it is, a global one.
typedef const __attribute__((address_space(1))) uint64_t   *fb_gcu64;
typedef __attribute__((address_space(1))) uint64_t         *fb_gu64;
typedef uint64_t fb_u64x2 __attribute__((ext_vector_type(2)));             // (a built-in vector: loadable from any address space)
typedef const __attribute__((address_space(1))) fb_u64x2   *fb_gcu64x2;

// the filter that holds tile (task) x: the largest j < nf with start[j] <= x.  start[0] = 0, strictly ascending (no filter of
// a chunk is empty), start[nf] = the chunk's total.
__device__ __forceinline__ uint32_t fbatch_find(const uint32_t *__restrict__ start, uint32_t nf, uint32_t x)
{
    uint32_t lo = 0, hi = nf;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (start[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// The bounds ballots every mask kernel starts from: me[k] / mo[k] the even / odd rows of round k that lie inside [0, n).
__device__ __forceinline__ void fbatch_bounds(uint64_t n, uint64_t lbase, uint64_t (&me)[FILTER_ROUNDS], uint64_t (&mo)[FILTER_ROUNDS])
{
#pragma unroll
    for (int k = 0; k < FILTER_ROUNDS; ++k) {
        const uint64_t i = lbase + (uint64_t)k * 2 * WAVE;
        me[k] = __ballot(i < n);
        mo[k] = __ballot(i + 1 < n);
    }
}

// One column's values of a wave's eight rounds, read directly or through a row-id vector: v0[k] / v1[k] the even / odd row of
// lane's pair in round k.  fast: 16-byte loads of the scanned vector, the wave's 1024 rows in bounds; otherwise a row whose bit
// in me / mo is clear (out of bounds, or dropped by an earlier term) reads row 0 in its place (n >= 1), and the caller keeps
// its comparison out of the masks.  Every branch is wave-uniform and outside the rounds, so that the eight (sixteen) loads are
// in flight together.
__device__ __forceinline__ void fbatch_side(fb_gcu64 col, fb_gcu64 sel, bool fast, uint64_t lbase, uint32_t lane, const uint64_t (&me)[FILTER_ROUNDS],
                                            const uint64_t (&mo)[FILTER_ROUNDS], uint64_t (&v0)[FILTER_ROUNDS], uint64_t (&v1)[FILTER_ROUNDS])
{
    if (fast) {
        if (sel) {
            fb_u64x2 x[FILTER_ROUNDS];
#pragma unroll
            for (int k = 0; k < FILTER_ROUNDS; ++k) x[k] = *(fb_gcu64x2)(sel + lbase + (uint64_t)k * 2 * WAVE);
#pragma unroll
            for (int k = 0; k < FILTER_ROUNDS; ++k) { v0[k] = col[x[k].x]; v1[k] = col[x[k].y]; }
        } else {
#pragma unroll
            for (int k = 0; k < FILTER_ROUNDS; ++k) {
                const fb_u64x2 x = *(fb_gcu64x2)(col + lbase + (uint64_t)k * 2 * WAVE);
                v0[k] = x.x; v1[k] = x.y;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < FILTER_ROUNDS; ++k) {
            const uint64_t i = lbase + (uint64_t)k * 2 * WAVE;
            v0[k] = (me[k] >> lane) & 1 ? i : 0;
            v1[k] = (mo[k] >> lane) & 1 ? i + 1 : 0;
        }
        if (sel) {
#pragma unroll
            for (int k = 0; k < FILTER_ROUNDS; ++k) { v0[k] = sel[v0[k]]; v1[k] = sel[v1[k]]; }
        }
#pragma unroll
        for (int k = 0; k < FILTER_ROUNDS; ++k) { v0[k] = col[v0[k]]; v1[k] = col[v1[k]]; }
    }
}

// The end of every mask kernel, in k_filter_mask's layout: fbatch_mask_round stores the two mask words of round k and returns
// their hits, fbatch_mask_count sums the four waves' hits into the tile's count.
__device__ __forceinline__ uint32_t fbatch_mask_round(uint64_t n, uint64_t wbase, uint32_t lane, int k, uint64_t me, uint64_t mo, fb_gu64 masks)
{
    if (lane == 0 && wbase + (uint64_t)k * 2 * WAVE < n) {
        masks[(wbase >> 6) + 2 * k] = me;
        masks[(wbase >> 6) + 2 * k + 1] = mo;
    }
    return (uint32_t)__popcll(me) + (uint32_t)__popcll(mo);
}

__device__ __forceinline__ void fbatch_mask_count(uint32_t cnt, uint32_t lane, uint32_t w, uint32_t tile, fb_gu64 tile_count)
{
    __shared__ uint32_t wsum[4];
    if (lane == 0) wsum[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_count[tile] = (uint64_t)wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(256) void k_fbatch_mask(const FBatchDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t nf)
{
    const uint32_t j = fbatch_find(tile_start, nf, blockIdx.x);
    const FBatchDesc &d = descs[j];
    const uint32_t tile = blockIdx.x - tile_start[j];
    const uint32_t lane = threadIdx.x & 63, w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n = d.n;
    const fb_gcu64 sel = (fb_gcu64)d.sel;
    const fb_gu64 masks = (fb_gu64)d.masks, tile_count = (fb_gu64)d.tile_count;
    const int nterms = d.nterms;
    const uint64_t wbase = (uint64_t)tile * FILTER_TILE + (uint64_t)w * FILTER_WAVE_ELEMS;
    const uint64_t lbase = wbase + 2 * lane;                     // this lane's first element of round 0
    const bool fast = d.vec && wbase + FILTER_WAVE_ELEMS <= n;   // 16-byte loads, whole wave range in bounds
    uint64_t me[FILTER_ROUNDS], mo[FILTER_ROUNDS];               // wave-uniform: the rows in bounds, then those every term so far holds on
    fbatch_bounds(n, lbase, me, mo);
    for (int t = 0; t < nterms; ++t) {
        uint64_t live = 0;
#pragma unroll
        for (int k = 0; k < FILTER_ROUNDS; ++k) live |= me[k] | mo[k];
        if (live == 0) break;                                    // nothing left for the further terms to decide
        const fb_gcu64 col = (fb_gcu64)d.t[t].col;
        const uint64_t value = d.t[t].value;
        const int op = d.t[t].op;
        uint64_t v0[FILTER_ROUNDS], v1[FILTER_ROUNDS];
        fbatch_side(col, sel, fast, lbase, lane, me, mo, v0, v1);
        if (op == 0) {
#pragma unroll
            for (int k = 0; k < FILTER_ROUNDS; ++k) { me[k] &= __ballot(v0[k] < value); mo[k] &= __ballot(v1[k] < value); }
        } else if (op == 1) {
#pragma unroll
            for (int k = 0; k < FILTER_ROUNDS; ++k) { me[k] &= __ballot(v0[k] > value); mo[k] &= __ballot(v1[k] > value); }
        } else {
#pragma unroll
            for (int k = 0; k < FILTER_ROUNDS; ++k) { me[k] &= __ballot(v0[k] == value); mo[k] &= __ballot(v1[k] == value); }
        }
    }
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < FILTER_ROUNDS; ++k) cnt += fbatch_mask_round(n, wbase, lane, k, me[k], mo[k], masks);
    fbatch_mask_count(cnt, lane, w, tile, tile_count);
}

// The write pass of a batch, over either descriptor type (it reads n, out, masks, tile_count and h_total).  An item with an
// output has one task per pair of tiles, as in k_filter_write; a count-only item has ONE task, whose wave sums the item's tile
// counts and writes nothing but the total.
template <class D>
__device__ __forceinline__ void fbatch_write_tasks(const D *descs, const uint32_t *task_start, uint32_t nf)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t ntasks_all = task_start[nf];
    const uint32_t stride = gridDim.x * (256 / WAVE);
    const uint64_t lt = lanemask_lt();
    for (uint32_t x = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6))); x < ntasks_all; x += stride) {
        const uint32_t j = fbatch_find(task_start, nf, x);
        const D &d = descs[j];
        const uint64_t n = d.n;
        const uint64_t ntiles = (n + FILTER_TILE - 1) / FILTER_TILE;
        if (d.out == nullptr) {
            uint64_t total = 0;
            for (uint64_t t = lane; t < ntiles; t += WAVE) total += d.tile_count[t];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) total += __shfl_xor(total, s, 64);
            if (lane == 0) __hip_atomic_store(d.h_total, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            continue;
        }
        filter_write_task<true>(n, ntiles, (ntiles + 1) / 2, x - task_start[j], d.masks, d.tile_count, d.out, d.h_total, lane, lt);
    }
}

__global__ __launch_bounds__(256) void k_fbatch_write(const FBatchDesc *__restrict__ descs, const uint32_t *__restrict__ task_start, uint32_t nf)
{
    fbatch_write_tasks(descs, task_start, nf);
}

}  // namespace rhj
