// rhj_fold_self_batch.hip.h — many folds with no child: equalities between two columns of ONE side as a 0/1 factor on its weights
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// A predicate whose two sides are one binding (0.1=0.2) never changes the binding's row space: it is a 0/1 factor on the
// binding's weight, and the fold machinery carries weights already.  One item is one side of n rows, nterms
// equalities and nouts outputs, each a factor P over the side's positions (rhj_join_fold_batch.hip.h's FoldFactor):
//   m(i)      = product over t of [ colA_t[selA_t ? selA_t[i] : i] == colB_t[selB_t ? selB_t[i] : i] ]        (no term: 1)
//   out_o[i]  = m(i) * P_o(i)                  (0 for a masked row: written, not left)
//   total_o   = sum over i of out_o[i]         (mod 2^64)
// rhj_fold_self_batch_device runs N such items in ONE launch per chunk and waits for the stream once:
//   k_fold_self     grid = the 2048-row tiles of every item:   the mask of the thread's 8 rows, term by term; per output load
//                                                              P, store (lane = row) and reduce the total
// There is no table, no flag and no scratch memory, and nobody waits: a workgroup's totals are reduced per wave by shuffles, per
// workgroup through 288 bytes of LDS, and added with one 64-bit atomic per output into the item's words (zero at launch), whose
// results nobody reads in the launch.
//
// A workgroup finds its item by fbatch_find in the launch's array of tile starts and reads the item's FoldSelfDesc through
// const __restrict__ kernel arguments at a workgroup-uniform index.  A thread's 8 rows are tile * 2048 + round * 256 + thread.
// The 16 column loads of one term go out together, outside any per-lane branch (a row out of bounds reads position 0 and takes no
// part); the terms and the outputs are looped over one at a time, uniformly, so the registers hold one term's worth.
#pragma once
#include "rhj.h"
#include "rhj_inter.h"
#include "rhj_join_fold_batch.hip.h"

namespace rhj {

constexpr int FOLD_SELF_WORDS = RHJ_FOLD_MAX_OUTS;   // an item's words: the outputs' totals

struct FoldSelfTerm {
    const uint64_t *col[2];      // the columns A and B
    const uint64_t *sel[2];      // nullptr: q = p
};

struct FoldSelfOutDesc {
    FoldFactor p;
    uint64_t  *out;              // nullptr: the total only
};

struct FoldSelfDesc {
    uint64_t            n;       // >= 1, < 2^32
    unsigned long long *words;   // FOLD_SELF_WORDS words, zero at launch
    int                 nterms, nouts;
    FoldSelfTerm        t[RHJ_FOLD_SELF_MAX_TERMS];
    FoldSelfOutDesc     o[RHJ_FOLD_MAX_OUTS];
};

__global__ __launch_bounds__(256) void k_fold_self(const FoldSelfDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    __shared__ unsigned long long part[RHJ_FOLD_MAX_OUTS][4];
    const uint32_t j = fbatch_find(tile_start, ni, blockIdx.x);
    const FoldSelfDesc &d = descs[j];
    const uint32_t tile = blockIdx.x - tile_start[j];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t n = d.n;
    const uint64_t base = (uint64_t)tile * JSUM_TILE + threadIdx.x;
    const int nterms = d.nterms, nouts = d.nouts;
    uint64_t pos[JSUM_ROUNDS];
    bool m[JSUM_ROUNDS];
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) {
        const uint64_t i = base + (uint64_t)k * 256;
        pos[k] = i < n ? i : 0;
        m[k] = i < n;
    }
    for (int t = 0; t < nterms; ++t) {
        const fb_gcu64 colA = (fb_gcu64)d.t[t].col[0], selA = (fb_gcu64)d.t[t].sel[0];       // (workgroup-uniform, as the branches on them)
        const fb_gcu64 colB = (fb_gcu64)d.t[t].col[1], selB = (fb_gcu64)d.t[t].sel[1];
        uint64_t a[JSUM_ROUNDS], b[JSUM_ROUNDS];
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) a[k] = b[k] = pos[k];
        if (selA) {
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) a[k] = selA[pos[k]];
        }
        if (selB) {
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) b[k] = selB[pos[k]];
        }
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) { a[k] = colA[a[k]]; b[k] = colB[b[k]]; }
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) m[k] = m[k] && a[k] == b[k];
    }
    for (int o = 0; o < nouts; ++o) {
        const fb_gu64 out = (fb_gu64)d.o[o].out;
        uint64_t p[JSUM_ROUNDS];
        fold_factor(d.o[o].p, pos, p);
        unsigned long long total = 0;
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) {
            const uint64_t i = base + (uint64_t)k * 256;
            const uint64_t x = m[k] ? p[k] : 0;           // (m is false for a row out of bounds)
            if (out && i < n) out[i] = x;
            total += x;
        }
        total = jsum_wave_sum(total);
        if (lane == 0) part[o][wv] = total;
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)nouts) {
        const uint32_t o = threadIdx.x;
        const unsigned long long mine = part[o][0] + part[o][1] + part[o][2] + part[o][3];
        if (mine) __hip_atomic_fetch_add(&d.words[o], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace rhj
