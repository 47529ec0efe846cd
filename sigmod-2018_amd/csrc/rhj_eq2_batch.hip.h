// rhj_eq2_batch.hip.h — many two-column equalities in the two launches of one
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// A join predicate whose two bindings already sit in one intermediate node (SelfJoin and the same-node branch of JoinInterNode,
// inter_res.c:234-263, :363-389) is the filter colA[selA ? selA[i] : i] == colB[selB ? selB[i] : i] over the node's rows.  As a
// single call (rhj_filter_eq2_device) it is a mask launch, a write launch and a host round trip; rhj_filter_eq2_batch_device
// runs N of them as ONE mask launch and ONE write launch, by the scheme of rhj_filter_batch.hip.h:
//   k_eq2batch_mask    grid = the 4096-row tiles of the chunk's items, one behind the other
//   k_eq2batch_write   one wave per pair of tiles over the items' tasks, one behind the other, grid-stride
// The item is found with fbatch_find and its Eq2BatchDesc read through a const __restrict__ array at a workgroup- (wave-)
// uniform index, so the fields arrive by scalar loads.  The mask layout is k_filter_mask's and the write pass
// filter_write_task<true>, as in k_fbatch_write.
//
// The two sides are loaded one after the other by eq2_side(): its branches on the side's form (a vector or none, the 16-byte
// loads or not) are wave-uniform and outside the rounds, so a side's sixteen loads a lane are in flight together.  The
// 16-byte loads are decided per side: a column scanned directly from an odd word beside a vector that starts on a 16-byte
// boundary costs the vector nothing.
#pragma once
#include "rhj.h"
#include "rhj_filter_batch.hip.h"

namespace rhj {

struct Eq2BatchDesc {
    const uint64_t     *colA, *selA;     // sel nullptr: the column's rows 0..n)
    const uint64_t     *colB, *selB;
    uint64_t            n;
    uint64_t           *out;         // nullptr: count only
    uint64_t           *masks;       // 2 * ceil(n / 128) words, 16-byte aligned
    uint64_t           *tile_count;  // ceil(n / 4096) words
    unsigned long long *h_total;     // the item's slot in the pinned host array of hit totals
    int                 vecA, vecB;  // the vector the side scans (its sel, or its column without one) starts on a 16-byte boundary
};

// One side's values of a wave's eight rounds: v0[k] / v1[k] the even / odd row of lane's pair in round k.  fast: 16-byte loads
// of the scanned vector, the wave's 1024 rows in bounds; otherwise a row out of bounds (bit clear in me / mo) reads row 0 in
// its place (n >= 1), and the caller keeps its comparison out of the masks.
__device__ __forceinline__ void eq2_side(fb_gcu64 col, fb_gcu64 sel, bool fast, uint64_t lbase, uint32_t lane, const uint64_t (&me)[FILTER_ROUNDS],
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

__global__ __launch_bounds__(256) void k_eq2batch_mask(const Eq2BatchDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t nf)
{
    __shared__ uint32_t wsum[4];
    const uint32_t j = fbatch_find(tile_start, nf, blockIdx.x);
    const Eq2BatchDesc &d = descs[j];
    const uint32_t tile = blockIdx.x - tile_start[j];
    const uint32_t lane = threadIdx.x & 63, w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n = d.n;
    const fb_gu64 masks = (fb_gu64)d.masks, tile_count = (fb_gu64)d.tile_count;
    const uint64_t wbase = (uint64_t)tile * FILTER_TILE + (uint64_t)w * FILTER_WAVE_ELEMS;
    const uint64_t lbase = wbase + 2 * lane;                     // this lane's first row of round 0
    const bool whole = wbase + FILTER_WAVE_ELEMS <= n;           // the wave's 1024 rows are in bounds
    uint64_t me[FILTER_ROUNDS], mo[FILTER_ROUNDS];               // wave-uniform: the rows in bounds, then those that are equal
#pragma unroll
    for (int k = 0; k < FILTER_ROUNDS; ++k) {
        const uint64_t i = lbase + (uint64_t)k * 2 * WAVE;
        me[k] = __ballot(i < n);
        mo[k] = __ballot(i + 1 < n);
    }
    uint64_t a0[FILTER_ROUNDS], a1[FILTER_ROUNDS], b0[FILTER_ROUNDS], b1[FILTER_ROUNDS];
    eq2_side((fb_gcu64)d.colA, (fb_gcu64)d.selA, d.vecA && whole, lbase, lane, me, mo, a0, a1);
    eq2_side((fb_gcu64)d.colB, (fb_gcu64)d.selB, d.vecB && whole, lbase, lane, me, mo, b0, b1);
    // a row out of bounds read row 0 on both sides and compares equal whenever A[0] == B[0]: the bounds ballots mask it out
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < FILTER_ROUNDS; ++k) {
        me[k] &= __ballot(a0[k] == b0[k]);
        mo[k] &= __ballot(a1[k] == b1[k]);
        if (lane == 0 && wbase + (uint64_t)k * 2 * WAVE < n) {
            masks[(wbase >> 6) + 2 * k] = me[k];
            masks[(wbase >> 6) + 2 * k + 1] = mo[k];
        }
        cnt += (uint32_t)__popcll(me[k]) + (uint32_t)__popcll(mo[k]);
    }
    if (lane == 0) wsum[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_count[tile] = (uint64_t)wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// k_fbatch_write's body over Eq2BatchDesc: an item with an output has one task per pair of tiles; a count-only item has ONE
// task, whose wave sums the item's tile counts and writes nothing but the total.
__global__ __launch_bounds__(256) void k_eq2batch_write(const Eq2BatchDesc *__restrict__ descs, const uint32_t *__restrict__ task_start, uint32_t nf)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t ntasks_all = task_start[nf];
    const uint32_t stride = gridDim.x * (256 / WAVE);
    const uint64_t lt = lanemask_lt();
    for (uint32_t x = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6))); x < ntasks_all; x += stride) {
        const uint32_t j = fbatch_find(task_start, nf, x);
        const Eq2BatchDesc &d = descs[j];
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

}  // namespace rhj
