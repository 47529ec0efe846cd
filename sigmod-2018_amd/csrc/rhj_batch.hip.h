// rhj_batch.hip.h — many small joins in the launches of one: the small path's kernels over a third grid dimension
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// A small join (rhj_small.hip.h) is two or three dependent launches and a host round trip, whatever its size: 88 of them, the
// contest's `small` batch, are 88 round trips for microseconds of HBM time.  Independent joins need not wait for each other,
// so rhj_join_batch_device runs N of them as ONE histogram launch (only for the joins that need it), ONE scatter + plan launch
// and ONE fused-join launch per kernel variant, and waits for the stream once:
//   k_batch_hist     grid (8, 2, joins with a relation of more than SM_SELF_TILES tiles)      small_hist_body
//   k_batch_scatter  grid (8 + 1, 2, N): a join's tiles and its plan workgroup                 small_scatter_body
//                    (k_batch_hist_cols, k_batch_scatter_cols: the same bodies reading {col[sel ? sel[i] : i], i} — ColSrc,
//                    rhj_small.hip.h — for rhj_join_cols_batch_device; everything behind the scatter is shared)
//   k_batch_fused    grid (BJ_WGS, joins of the variant): row j's workgroups share join j's     fj_join
//                    ticket, and the last of them out leaves the join's summary and walk count
//                    in slot j of a pinned host array
// The bodies are the single-join kernels' own (device functions; the partition's take their coordinates as arguments, the
// fused join's workgroups are those of one row of the grid either way), so a batched join computes what the single call
// computes.  What differs is where the arguments come from: a BatchJoin per join in a device array uploaded once per call.
// It is read through a const __restrict__ kernel argument at a workgroup-uniform index, so the fields arrive by scalar
// loads as kernel arguments do.
//
// No workgroup of one join ever waits for another join's: a unit's look-back (fj_lookback) waits only on units handed out by
// the SAME join's ticket, and only running workgroups take tickets — so a grid of more workgroups than the chip holds at
// once cannot deadlock, and BJ_WGS may be chosen for the workspace alone (FusedArgs::ovf is 640 KB per workgroup).
#pragma once
#include "rhj_small.hip.h"
#include "rhj_join_fused.hip.h"

namespace rhj {

constexpr uint32_t BJ_MAX_TILES = 8;              // largest relation of a batched join, in SM_TILE tiles: 65 536 tuples
constexpr uint32_t BJ_WGS = 4;                    // fused workgroups per join: a join of this class has at most 2^bits + 32 + 2 units

struct BatchJoin {
    RelArgs   r0, r1;
    PlanArgs  plan;
    FusedArgs f;
    uint64_t *hist, *psum;       // [2][bins] each, R's then S's
    uint64_t *zero_words;        // the join's ticket and status words ...
    uint64_t  n_zero;
    int       bits;
    int       self_hist;         // ... cleared by the scatter launch (1: no histogram launch covers this join) or by the histogram launch
    ColSrc    c0, c1;            // rhj_join_cols_batch_device: where R and S are read (the _cols kernels; r0.in / r1.in are null then)
};

__global__ __launch_bounds__(SM_BLOCK) void k_batch_hist(const BatchJoin *__restrict__ joins, const uint32_t *__restrict__ list)
{
    const BatchJoin &d = joins[list[blockIdx.z]];
    small_hist_body<false>(d.r0, d.r1, d.c0, d.c1, d.bits, d.zero_words, d.n_zero, blockIdx.x, blockIdx.y, gridDim.x, gridDim.y);
}

__global__ __launch_bounds__(SM_BLOCK) void k_batch_hist_cols(const BatchJoin *__restrict__ joins, const uint32_t *__restrict__ list)
{
    const BatchJoin &d = joins[list[blockIdx.z]];
    small_hist_body<true>(d.r0, d.r1, d.c0, d.c1, d.bits, d.zero_words, d.n_zero, blockIdx.x, blockIdx.y, gridDim.x, gridDim.y);
}

__global__ __launch_bounds__(SM_BLOCK) void k_batch_scatter(const BatchJoin *__restrict__ joins)
{
    const BatchJoin &d = joins[blockIdx.z];
    small_scatter_body<false>(d.r0, d.r1, d.c0, d.c1, d.bits, d.hist, d.psum, d.plan, d.self_hist, d.zero_words, d.n_zero, blockIdx.x,
                              blockIdx.y, gridDim.x, gridDim.y);
}

__global__ __launch_bounds__(SM_BLOCK) void k_batch_scatter_cols(const BatchJoin *__restrict__ joins)
{
    const BatchJoin &d = joins[blockIdx.z];
    small_scatter_body<true>(d.r0, d.r1, d.c0, d.c1, d.bits, d.hist, d.psum, d.plan, d.self_hist, d.zero_words, d.n_zero, blockIdx.x,
                             blockIdx.y, gridDim.x, gridDim.y);
}

// 16-byte tuples throughout, like every join of the small path (PlanSummary::wide_row_ids is 1 there)
template <bool MAYRES>
__global__ __launch_bounds__(FJ_BLOCK) void k_batch_fused(const BatchJoin *__restrict__ joins, const uint32_t *__restrict__ list, uint32_t lds_bytes)
{
    const BatchJoin &d = joins[list[blockIdx.y]];
    fj_join<MAYRES, false>(d.f, lds_bytes);
}

}  // namespace rhj
