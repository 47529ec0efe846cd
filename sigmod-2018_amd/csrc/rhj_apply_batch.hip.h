// rhj_apply_batch.hip.h — many row-id rebuilds and view sums in the one launch of one
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// What consumes a join's pair list is a gather per active relation (InsertJoinToInterResults: k_gather_tables over the R
// words, a second launch over the S words) and, after a query's last join, a sum per view (k_sum_views: a launch and a
// stream wait per query).  Behind a join batch of three launches that is two launches a join and a wait a query.
// rhj_apply_batch_device runs N such items as ONE launch per chunk and waits for the stream once:
//   k_apply_batch    grid = the 2048-row tiles of the chunk's items, one behind the other
// An item applies ONE index list to up to RHJ_APPLY_MAX_TERMS terms (include/rhj_inter.h): for row i,
//   p = idx ? idx[i * stride + side_t] : i;   q = src_t ? src_t[p] : p;   dst_t[i] = q (if dst_t);   sum_t += col_t[q] (if col_t)
// A workgroup finds its item by a binary search in the chunk's array of tile starts (fbatch_find) and reads the item's
// ApplyDesc from a device array uploaded once per chunk; both come through const __restrict__ kernel arguments and are read
// at a workgroup-uniform index, so the fields arrive by scalar loads as kernel arguments do.
//
// A thread's 8 rows are tile * 2048 + round * 256 + thread: consecutive lanes read and write consecutive rows.  The index
// words of the 8 rows are loaded once, before the terms, and only the sides some term uses.  Every branch on the item's form
// is workgroup-uniform and outside the rounds, so that a term's 8 loads are in flight together; a row out of bounds reads
// row 0 in its place (n >= 1), so that no load sits behind a per-lane branch.
//
// Sums: per wave by shuffles, the four waves through LDS, then thread 0 adds the workgroup's part of every summing term to the
// item's accumulator words and takes a ticket; the last workgroup out stores the accumulators into the item's slot of the pinned
// host block (system scope) and flags the slot done.  Accumulators and tickets are part of the block the host uploads with
// the descriptors, written as zeros: every chunk starts clean whatever became of the one before.  Items without a summing
// term touch neither.
#pragma once
#include "rhj.h"
#include "rhj_inter.h"
#include "rhj_filter_batch.hip.h"

namespace rhj {

constexpr int APPLY_ROUNDS = 8;
constexpr uint32_t APPLY_TILE = 2048;                // 256 threads x 8 rows
constexpr int APPLY_SLOT_WORDS = RHJ_APPLY_MAX_TERMS + 1;        // an item's words in the pinned host block: the sums, then "done"

struct ApplyTermDesc {
    const uint64_t *src;         // nullptr: q = p
    uint64_t       *dst;         // nullptr: nothing written
    const uint64_t *col;         // nullptr: no sum
    int             side;
    int             pad;
};

struct ApplyDesc {
    const uint64_t     *idx;     // nullptr: p = i
    uint64_t            n;       // >= 1
    unsigned long long *acc;     // RHJ_APPLY_MAX_TERMS accumulator words, zero at launch; nullptr: no summing term
    uint32_t           *ticket;  // zero at launch
    unsigned long long *h_slot;  // APPLY_SLOT_WORDS words of the pinned host block
    int                 stride;  // 1 or 2
    int                 nterms;
    uint32_t            sides;   // bit s: some term reads word s of an index row
    uint32_t            tiles;
    ApplyTermDesc       t[RHJ_APPLY_MAX_TERMS];
};

__global__ __launch_bounds__(256) void k_apply_batch(const ApplyDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    __shared__ unsigned long long part[RHJ_APPLY_MAX_TERMS][4];
    const uint32_t j = fbatch_find(tile_start, ni, blockIdx.x);
    const ApplyDesc &d = descs[j];
    const uint32_t tile = blockIdx.x - tile_start[j];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t n = d.n;
    const fb_gcu64 idx = (fb_gcu64)d.idx;
    const int nterms = d.nterms;
    const uint64_t base = (uint64_t)tile * APPLY_TILE + threadIdx.x;
    // every branch below is workgroup-uniform and outside the rounds
    uint64_t p0[APPLY_ROUNDS], p1[APPLY_ROUNDS];         // word 0 / word 1 of the rows' index entries (p0: the row itself without a list)
#pragma unroll
    for (int k = 0; k < APPLY_ROUNDS; ++k) {
        const uint64_t i = base + (uint64_t)k * 256;
        p0[k] = i < n ? i : 0;                           // a row out of bounds reads row 0 in its place
        p1[k] = 0;
    }
    if (idx) {
        if (d.stride == 1) {
#pragma unroll
            for (int k = 0; k < APPLY_ROUNDS; ++k) p0[k] = idx[p0[k]];
        } else {
            const uint32_t sides = d.sides;
            if (sides == 3u) {
#pragma unroll
                for (int k = 0; k < APPLY_ROUNDS; ++k) { p1[k] = idx[2 * p0[k] + 1]; p0[k] = idx[2 * p0[k]]; }
            } else if (sides == 2u) {
#pragma unroll
                for (int k = 0; k < APPLY_ROUNDS; ++k) p1[k] = idx[2 * p0[k] + 1];
            } else {
#pragma unroll
                for (int k = 0; k < APPLY_ROUNDS; ++k) p0[k] = idx[2 * p0[k]];
            }
        }
    }
    for (int t = 0; t < nterms; ++t) {
        const fb_gcu64 src = (fb_gcu64)d.t[t].src, col = (fb_gcu64)d.t[t].col;
        const fb_gu64 dst = (fb_gu64)d.t[t].dst;
        const bool odd = d.t[t].side != 0;
        uint64_t q[APPLY_ROUNDS];
#pragma unroll
        for (int k = 0; k < APPLY_ROUNDS; ++k) q[k] = odd ? p1[k] : p0[k];
        if (src) {
#pragma unroll
            for (int k = 0; k < APPLY_ROUNDS; ++k) q[k] = src[q[k]];
        }
        if (dst) {
#pragma unroll
            for (int k = 0; k < APPLY_ROUNDS; ++k) {
                const uint64_t i = base + (uint64_t)k * 256;
                if (i < n) dst[i] = q[k];
            }
        }
        if (col) {
            uint64_t v[APPLY_ROUNDS];
#pragma unroll
            for (int k = 0; k < APPLY_ROUNDS; ++k) v[k] = col[q[k]];
            unsigned long long s = 0;
#pragma unroll
            for (int k = 0; k < APPLY_ROUNDS; ++k) s += base + (uint64_t)k * 256 < n ? v[k] : 0;
#pragma unroll
            for (int x = 32; x >= 1; x >>= 1) s += __shfl_xor(s, x, 64);
            if (lane == 0) part[t][w] = s;
        }
    }
    unsigned long long *acc = d.acc;
    if (acc == nullptr) return;                          // (workgroup-uniform) no summing term: no accumulator, no ticket
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 0; t < nterms; ++t) {
            if (d.t[t].col == nullptr) continue;
            const unsigned long long mine = part[t][0] + part[t][1] + part[t][2] + part[t][3];
            if (mine) __hip_atomic_fetch_add(&acc[t], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // release + acquire on the ticket: this workgroup's parts are out before it counts itself, the last one sees everybody's
        if (__hip_atomic_fetch_add(d.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == d.tiles - 1u) {
            unsigned long long *h = d.h_slot;
            for (int t = 0; t < nterms; ++t) {
                if (d.t[t].col == nullptr) continue;
                const unsigned long long total = __hip_atomic_load(&acc[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&h[t], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            __hip_atomic_store(&h[RHJ_APPLY_MAX_TERMS], 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace rhj
