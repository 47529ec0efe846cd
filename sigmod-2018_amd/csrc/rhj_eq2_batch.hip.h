// rhj_eq2_batch.hip.h — many two-column equalities in the two launches of one
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// A join predicate whose two bindings already sit in one intermediate node (SelfJoin and the same-node branch of JoinInterNode,
// inter_res.c:234-263, :363-389) is the filter colA[selA ? selA[i] : i] == colB[selB ? selB[i] : i] over the node's rows.  As a
// single call (rhj_filter_eq2_device) it is a mask launch, a write launch and a host round trip; rhj_filter_eq2_batch_device
// runs N of them as ONE mask launch and ONE write launch, by the scheme of rhj_filter_batch.hip.h:
//   k_eq2batch_mask    grid = the 4096-row tiles of the chunk's items, one behind the other
//   k_eq2batch_write   one wave per pair of tiles over the items' tasks, one behind the other, grid-stride
// Only the descriptor and the mask kernel's middle are this file's own.  The item is found with fbatch_find and its Eq2BatchDesc
// read through a const __restrict__ array at a workgroup- (wave-) uniform index, so the fields arrive by scalar loads; the bounds
// ballots, the mask store and tile count (k_filter_mask's layout) and the write pass (fbatch_write_tasks: filter_write_task<true>,
// or one wave that sums a count-only item's tile counts) are rhj_filter_batch.hip.h's, shared with the batched filters.
//
// The two sides are loaded one after the other by fbatch_side(): its branches on the side's form (a vector or none, the 16-byte
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

__global__ __launch_bounds__(256) void k_eq2batch_mask(const Eq2BatchDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t nf)
{
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
    fbatch_bounds(n, lbase, me, mo);
    uint64_t a0[FILTER_ROUNDS], a1[FILTER_ROUNDS], b0[FILTER_ROUNDS], b1[FILTER_ROUNDS];
    fbatch_side((fb_gcu64)d.colA, (fb_gcu64)d.selA, d.vecA && whole, lbase, lane, me, mo, a0, a1);
    fbatch_side((fb_gcu64)d.colB, (fb_gcu64)d.selB, d.vecB && whole, lbase, lane, me, mo, b0, b1);
    // a row out of bounds read row 0 on both sides and compares equal whenever A[0] == B[0]: the bounds ballots mask it out
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < FILTER_ROUNDS; ++k) {
        me[k] &= __ballot(a0[k] == b0[k]);
        mo[k] &= __ballot(a1[k] == b1[k]);
        cnt += fbatch_mask_round(n, wbase, lane, k, me[k], mo[k], masks);
    }
    fbatch_mask_count(cnt, lane, w, tile, tile_count);
}

__global__ __launch_bounds__(256) void k_eq2batch_write(const Eq2BatchDesc *__restrict__ descs, const uint32_t *__restrict__ task_start, uint32_t nf)
{
    fbatch_write_tasks(descs, task_start, nf);
}

}  // namespace rhj
