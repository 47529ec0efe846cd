// rhj_fold_pred_batch.hip.h — many folds with no child whose mask has constant predicates too: a filter as a 0/1 factor on a
// side's weights, with no hit list
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// A filter's hit list changes a binding's row count, so whoever sizes the next launch has to wait for its length.  As a 0/1 factor
// on the binding's weight (as 4.17 takes 0.1=0.2) it changes nothing: the side stays the whole relation.  One item
// is rhj_fold_self_batch.hip.h's with nconst comparisons against constants in front of its neq equalities:
//   m(i)      = AND over c of [ col_c[sel_c ? sel_c[i] : i]  op_c  value_c ]   AND   over t of [ A_t == B_t ]      (no term: 1)
//   out_o[i]  = m(i) * P_o(i)                  (0 for a masked row: written, not left)
//   total_o   = sum over i of out_o[i]         (mod 2^64)
// op is <, > or =, compared UNSIGNED (rhj_filter.hip.h's filter_pred).  rhj_fold_pred_batch_device runs N such items in ONE launch
// per chunk:
//   k_fold_pred     grid = the 2048-row tiles of every item:   the mask of the thread's 8 rows, term by term; per output load
//                                                              P, store (lane = row) and reduce the total
// Everything else is k_fold_self's: no table, no flag, no scratch memory, nobody waits; a workgroup's totals are reduced per wave
// by shuffles, per workgroup through 288 bytes of LDS, and added with one 64-bit atomic per output into the item's words (zero at
// launch); the item is found by fbatch_find in the tile starts and its descriptor read at a workgroup-uniform index; the 8 (or 16)
// column loads of one term go out together, outside any per-lane branch (a row out of bounds reads position 0 and takes no part);
// terms and outputs are looped over uniformly, so the registers hold one term's worth.
#pragma once
#include "rhj.h"
#include "rhj_inter.h"
#include "rhj_filter.hip.h"
#include "rhj_fold_self_batch.hip.h"

namespace rhj {

constexpr int FOLD_PRED_WORDS = RHJ_FOLD_MAX_OUTS;   // an item's words: the outputs' totals

struct FoldPredConst {
    const uint64_t *col;
    const uint64_t *sel;         // nullptr: q = p
    uint64_t        value;
    int             op;          // filter_pred's: 0 <, 1 >, 2 =
    int             pad_;
};

struct FoldPredDesc {
    uint64_t            n;       // >= 1, < 2^32
    unsigned long long *words;   // FOLD_PRED_WORDS words, zero at launch
    int                 nconst, neq, nouts, pad_;
    FoldPredConst       c[RHJ_FILTER_MAX_TERMS];
    FoldSelfTerm        t[RHJ_FOLD_SELF_MAX_TERMS];
    FoldSelfOutDesc     o[RHJ_FOLD_MAX_OUTS];
};

__global__ __launch_bounds__(256) void k_fold_pred(const FoldPredDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    __shared__ unsigned long long part[RHJ_FOLD_MAX_OUTS][4];
    const uint32_t j = fbatch_find(tile_start, ni, blockIdx.x);
    const FoldPredDesc &d = descs[j];
    const uint32_t tile = blockIdx.x - tile_start[j];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t n = d.n;
    const uint64_t base = (uint64_t)tile * JSUM_TILE + threadIdx.x;
    const int nconst = d.nconst, neq = d.neq, nouts = d.nouts;
    uint64_t pos[JSUM_ROUNDS];
    bool m[JSUM_ROUNDS];
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) {
        const uint64_t i = base + (uint64_t)k * 256;
        pos[k] = i < n ? i : 0;
        m[k] = i < n;
    }
    for (int c = 0; c < nconst; ++c) {
        const fb_gcu64 col = (fb_gcu64)d.c[c].col, sel = (fb_gcu64)d.c[c].sel;               // (workgroup-uniform, as the branches on them)
        const uint64_t value = d.c[c].value;
        const int op = d.c[c].op;
        uint64_t a[JSUM_ROUNDS];
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) a[k] = pos[k];
        if (sel) {
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) a[k] = sel[pos[k]];
        }
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) a[k] = col[a[k]];
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) m[k] = m[k] && filter_pred(a[k], value, op);
    }
    for (int t = 0; t < neq; ++t) {
        const fb_gcu64 colA = (fb_gcu64)d.t[t].col[0], selA = (fb_gcu64)d.t[t].sel[0];
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
