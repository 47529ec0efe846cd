// rhj_join_fold_batch.hip.h — many weighted join folds: a child side folded into its parent side as per-row u64 weights
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// The sums of a query whose join predicates form a tree over its bindings need no intermediate result: sums and products
// modulo 2^64 form a ring, so a subtree is folded into its parent binding as one u64 per parent row.  One
// item folds a child side S into a parent side R over keyR(i) == keyS(j).  A factor {w, src, col} stands for
//   f(p) = (w ? w[p] : 1) * (col ? col[src ? src[p] : p] : 1)                    (mod 2^64, p the row's position in its side)
// The item has nvalues child values V_c (factors over S) and nouts outputs {value index c, factor P over R}:
//   A_c(k)    = sum of V_c(j) over the rows j of S with keyS(j) == k
//   out_o[i]  = P_o(i) * A_c(keyR(i))        (0 where R's key is not in S: written, not left)
//   total_o   = sum over i of out_o[i]
// rhj_join_fold_batch_device runs N such items in at most THREE launches per chunk and waits for the stream once:
//   k_fold_claim    grid = R's 2048-row tiles of the items where R builds:   find or claim the key's slot, add nothing
//   k_fold_add      grid = S's tiles of every item:   find the slot (claim it only where S builds); per value one 64-bit
//                                                     atomic add of V_c(j) into the slot; where R builds a miss adds nothing
//   k_fold_apply    grid = R's tiles of every item:   find the slot once per row; per output load A_c, multiply by P(i),
//                                                     store (lane = row) and reduce the total
// The table and its protocol are rhj_join_sum_batch.hip.h's (jsum_hash, jsum_slots, jsum_build_side, jsum_find, jsum_claim; read
// there why nobody waits) with slots of 1 + nvalues u64 words {key, A_0 ...}: the slot size is per item.  The side that
// jsum_build_side names claims the slots, and the slot count comes from that side's rows, so a table is bounded by twice the
// smaller side's rows.  The adds into a slot are atomics whose results nobody reads in the same launch.
//
// Rows whose key is JSUM_EMPTY never enter the table: S's such rows add their values to nvalues words of the item's own
// (words FOLD_W_EMPTY + c), R's such rows read those words in the apply launch.
//
// A workgroup finds its item by fbatch_find in the launch's array of tile starts (an item without a tile in a launch has an
// empty range there, which the search never lands on) and reads the item's JoinFoldDesc through const __restrict__ kernel
// arguments at a workgroup-uniform index.  A thread's 8 rows are tile * 2048 + round * 256 + thread.  The eight rows' loads of
// one value or one output factor go out together, outside any per-lane branch (a row out of bounds reads position 0 and takes
// no part); the values and the outputs are looped over one at a time, so the registers hold one value's worth.  When all rows
// of a wave's round that have a slot have the SAME slot (an item on one hot key), the wave adds their values up by shuffles and
// one lane issues the atomic; any other mix of keys adds per lane.  With the descriptor's `combine` field set
// (rhj_set_fold_combine) a tile with enough rows on shared slots sends those adds into LDS entries instead and one
// atomic per (tile, slot, value) to the table (rhj_slot_combine.hip.h; fold_add_values below, shared with the tuple-key folds).
#pragma once
#include "rhj.h"
#include "rhj_inter.h"
#include "rhj_join_sum_batch.hip.h"

namespace rhj {

constexpr int FOLD_W_EMPTY = 0;                      // an item's words: the empty key's A_c ...
constexpr int FOLD_W_TOTAL = RHJ_FOLD_MAX_VALUES;    // ... then the outputs' totals
constexpr int FOLD_W_COMBINE = RHJ_FOLD_MAX_VALUES + RHJ_FOLD_MAX_OUTS;      // ... then the combiner's two counters
constexpr int FOLD_WORDS = FOLD_W_COMBINE + (int)COMBINE_WORDS;
constexpr uint64_t FOLD_OUTSIDE = JSUM_NONE - 1;     // no slot: the empty key, kept in the item's words

struct FoldFactor {
    const uint64_t *w;           // nullptr: 1
    const uint64_t *src;         // nullptr: q = p
    const uint64_t *col;         // nullptr: 1
};

struct FoldOutDesc {
    FoldFactor p;
    uint64_t  *out;              // nullptr: the total only
    int        value;
    int        pad;
};

struct JoinFoldDesc {
    const uint64_t     *col[2];  // key column of R, of S
    const uint64_t     *sel[2];  // nullptr: the column's rows 0..n)
    uint64_t            n[2];    // >= 1, < 2^32
    unsigned long long *table;   // slot_words words a slot: the key, then A_0 ...
    unsigned long long *words;   // FOLD_WORDS words, zero at launch
    uint32_t            log2_slots;
    uint32_t            slot_words;          // 1 + nvalues
    int                 build;   // the side that claims the slots
    int                 nvalues, nouts;
    int                 combine; // 1: the add launch combines equal slots per tile in LDS (rhj_slot_combine.hip.h)
    FoldFactor          v[RHJ_FOLD_MAX_VALUES];
    FoldOutDesc         o[RHJ_FOLD_MAX_OUTS];
};

// a factor over the thread's 8 rows: the loads of a stage go out together (pos[k] is in bounds for every k)
__device__ __forceinline__ void fold_factor(const FoldFactor &f, const uint64_t (&pos)[JSUM_ROUNDS], uint64_t (&v)[JSUM_ROUNDS])
{
    const fb_gcu64 w = (fb_gcu64)f.w, src = (fb_gcu64)f.src, col = (fb_gcu64)f.col;      // (workgroup-uniform, as the branches on them)
    uint64_t q[JSUM_ROUNDS];
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) { q[k] = pos[k]; v[k] = 1; }
    if (w) {
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) v[k] = w[pos[k]];
    }
    if (col) {
        if (src) {
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) q[k] = src[pos[k]];
        }
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) v[k] *= col[q[k]];
    }
}

// one add of x into the word `at` of slot `slot`: into the slot's LDS entry when the row has one (`entry`: the tile combines and
// the row is the entry's owner or a rider), else the device-scope atomic, which `adds` counts
__device__ __forceinline__ void fold_slot_add(jsum_gull at, uint64_t slot, unsigned long long x, bool entry, uint32_t &adds)
{
    if (entry) { combine_add(combine_lds<unsigned long long>(), slot, x); return; }
    __hip_atomic_fetch_add(at, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ++adds;
}

// the end of a value in a combining tile: behind a barrier every owner takes its entry's sum and adds a non-zero one to the table;
// a second barrier keeps the next value's adds behind the zero the owner left.  Every thread of the workgroup comes here.
__device__ __forceinline__ void fold_flush(jsum_gull table, uint32_t sw, int c, const uint64_t (&slot)[JSUM_ROUNDS], uint32_t roles, uint32_t &adds)
{
    CombineLds<unsigned long long> &L = combine_lds<unsigned long long>();
    __syncthreads();
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) {
        if (combine_role(roles, k) != COMBINE_OWNER) continue;
        const unsigned long long sum = combine_take(L, slot[k]);
        if (sum) {
            __hip_atomic_fetch_add(&table[sw * slot[k] + 1 + c], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ++adds;
        }
    }
    __syncthreads();
}

// The value loop of an add launch's tile, behind the slot resolution (slot[k] >= FOLD_OUTSIDE: no slot in the table; lead[k]: the
// lane that adds for the wave when the round's slots are one, else 64), for the folds on one key (OUTSIDE: the empty key's rows add
// to the item's words) and on tuple keys.  COMBINED (a tile that combines, rhj_slot_combine.hip.h): a row whose slot has an entry
// adds into it, the wave's sum of a hot round first as ever, and the entry's owner adds the tile's sum to the table.
template <bool COMBINED, bool OUTSIDE, class Desc>
__device__ __forceinline__ void fold_add_loop(const Desc &d, jsum_gull table, uint32_t sw, const uint64_t (&slot)[JSUM_ROUNDS], const uint64_t (&pos)[JSUM_ROUNDS],
                                              const uint32_t (&lead)[JSUM_ROUNDS], uint32_t roles, uint32_t &adds)
{
    const uint32_t lane = threadIdx.x & 63;
    const int nvalues = d.nvalues;
    for (int c = 0; c < nvalues; ++c) {
        uint64_t v[JSUM_ROUNDS];
        fold_factor(d.v[c], pos, v);
        unsigned long long outside = 0;
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) {
            const bool in_table = slot[k] < FOLD_OUTSIDE;
            const bool entry = COMBINED && combine_role(roles, k) != COMBINE_BYPASS;
            if (OUTSIDE && slot[k] == FOLD_OUTSIDE) outside += v[k];
            if (lead[k] < 64u) {                         // (wave-uniform)
                const unsigned long long sum = jsum_wave_sum(in_table ? v[k] : 0);
                if (lane == lead[k] && sum) fold_slot_add(&table[sw * slot[k] + 1 + c], slot[k], sum, entry, adds);
            } else if (in_table && v[k]) {
                fold_slot_add(&table[sw * slot[k] + 1 + c], slot[k], (unsigned long long)v[k], entry, adds);
            }
        }
        if (OUTSIDE) {
            outside = jsum_wave_sum(outside);
            if (lane == 0 && outside) __hip_atomic_fetch_add(&d.words[FOLD_W_EMPTY + c], outside, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (COMBINED) fold_flush(table, sw, c, slot, roles, adds);
    }
}

// the values of a tile under the descriptor's switch: off, the per-lane adds alone; on, the tile's claims, the loop in the form
// the riders' count chose (workgroup-uniform: combine_claim), and the counters into the item's words from `w_combine` on
template <bool OUTSIDE, class Desc>
__device__ __forceinline__ void fold_add_values(const Desc &d, jsum_gull table, uint32_t sw, int w_combine, const uint64_t (&slot)[JSUM_ROUNDS],
                                                const uint64_t (&pos)[JSUM_ROUNDS], const uint32_t (&lead)[JSUM_ROUNDS])
{
    uint32_t roles = 0, adds = 0;
    if (!d.combine) {                                    // (workgroup-uniform)
        fold_add_loop<false, OUTSIDE>(d, table, sw, slot, pos, lead, roles, adds);
        return;
    }
    CombineLds<unsigned long long> &L = combine_lds<unsigned long long>();
    const bool combined = combine_claim(L, slot, FOLD_OUTSIDE, roles);
    if (combined) fold_add_loop<true, OUTSIDE>(d, table, sw, slot, pos, lead, roles, adds);
    else fold_add_loop<false, OUTSIDE>(d, table, sw, slot, pos, lead, roles, adds);
    combine_report(L, d.words + w_combine, combined, adds);
}

// the lane that adds for the wave when the rows of one round that have a slot are two or more and all in ONE slot, else 64
__device__ __forceinline__ uint32_t fold_wave_lead(uint64_t slot)
{
    const uint64_t have = __ballot(slot < FOLD_OUTSIDE);
    const uint32_t first = have ? (uint32_t)__ffsll((unsigned long long)have) - 1u : 0u;
    const uint64_t s0 = __shfl(slot, (int)first, 64);
    const uint64_t same = __ballot(slot == s0);
    return (have & (have - 1)) && (have & ~same) == 0 ? first : 64u;
}

__global__ __launch_bounds__(256) void k_fold_claim(const JoinFoldDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    const uint32_t j = fbatch_find(tile_start, ni, blockIdx.x);
    const JoinFoldDesc &d = descs[j];
    const uint32_t tile = blockIdx.x - tile_start[j];
    const uint64_t n = d.n[0];
    const uint64_t base = (uint64_t)tile * JSUM_TILE + threadIdx.x;
    const uint32_t log2_slots = d.log2_slots, sw = d.slot_words;
    const jsum_gull table = (jsum_gull)d.table;
    uint64_t key[JSUM_ROUNDS];
    jsum_keys((fb_gcu64)d.col[0], (fb_gcu64)d.sel[0], n, base, key);
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) {
        if (base + (uint64_t)k * 256 >= n || key[k] == JSUM_EMPTY) continue;
        (void)jsum_claim(table, sw, log2_slots, key[k]);
    }
}

__global__ __launch_bounds__(256) void k_fold_add(const JoinFoldDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    const uint32_t j = fbatch_find(tile_start, ni, blockIdx.x);
    const JoinFoldDesc &d = descs[j];
    const uint32_t tile = blockIdx.x - tile_start[j];
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n = d.n[1];
    const uint64_t base = (uint64_t)tile * JSUM_TILE + threadIdx.x;
    const uint32_t log2_slots = d.log2_slots, sw = d.slot_words;
    const jsum_gull table = (jsum_gull)d.table;
    const bool claims = d.build == 1;                    // (workgroup-uniform)
    uint64_t slot[JSUM_ROUNDS], pos[JSUM_ROUNDS];
    uint32_t lead[JSUM_ROUNDS];                          // the lane that adds for the wave when the round's slots are one, else 64
    {
        uint64_t key[JSUM_ROUNDS];
        jsum_keys((fb_gcu64)d.col[1], (fb_gcu64)d.sel[1], n, base, key);
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) {
            const uint64_t i = base + (uint64_t)k * 256;
            pos[k] = i < n ? i : 0;
            slot[k] = JSUM_NONE;
            if (i < n) {
                if (key[k] == JSUM_EMPTY) slot[k] = FOLD_OUTSIDE;
                else slot[k] = claims ? jsum_claim(table, sw, log2_slots, key[k]) : jsum_find(table, sw, log2_slots, key[k]);
            }
            lead[k] = fold_wave_lead(slot[k]);
        }
    }
    fold_add_values<true>(d, table, sw, FOLD_W_COMBINE, slot, pos, lead);
}

__global__ __launch_bounds__(256) void k_fold_apply(const JoinFoldDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    __shared__ unsigned long long part[RHJ_FOLD_MAX_OUTS][4];
    const uint32_t j = fbatch_find(tile_start, ni, blockIdx.x);
    const JoinFoldDesc &d = descs[j];
    const uint32_t tile = blockIdx.x - tile_start[j];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t n = d.n[0];
    const uint64_t base = (uint64_t)tile * JSUM_TILE + threadIdx.x;
    const uint32_t log2_slots = d.log2_slots, sw = d.slot_words;
    const jsum_gull table = (jsum_gull)d.table;
    const int nouts = d.nouts;
    uint64_t slot[JSUM_ROUNDS], pos[JSUM_ROUNDS];
    {
        uint64_t key[JSUM_ROUNDS];
        jsum_keys((fb_gcu64)d.col[0], (fb_gcu64)d.sel[0], n, base, key);
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) {
            const uint64_t i = base + (uint64_t)k * 256;
            pos[k] = i < n ? i : 0;
            slot[k] = JSUM_NONE;
            if (i < n) slot[k] = key[k] == JSUM_EMPTY ? FOLD_OUTSIDE : jsum_find(table, sw, log2_slots, key[k]);
        }
    }
    for (int o = 0; o < nouts; ++o) {
        const int c = d.o[o].value;
        const fb_gu64 out = (fb_gu64)d.o[o].out;
        const uint64_t a_outside = d.words[FOLD_W_EMPTY + c];        // written by the launch before this one
        uint64_t p[JSUM_ROUNDS], a[JSUM_ROUNDS];
        fold_factor(d.o[o].p, pos, p);
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) a[k] = table[sw * (slot[k] < FOLD_OUTSIDE ? slot[k] : 0) + 1 + c];     // (slot 0 exists)
        unsigned long long total = 0;
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) {
            const uint64_t i = base + (uint64_t)k * 256;
            const uint64_t x = p[k] * (slot[k] < FOLD_OUTSIDE ? a[k] : slot[k] == FOLD_OUTSIDE ? a_outside : 0);
            if (i < n) {
                if (out) out[i] = x;
                total += x;
            }
        }
        total = jsum_wave_sum(total);
        if (lane == 0) part[o][wv] = total;
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)nouts) {
        const uint32_t o = threadIdx.x;
        const unsigned long long mine = part[o][0] + part[o][1] + part[o][2] + part[o][3];
        if (mine) __hip_atomic_fetch_add(&d.words[FOLD_W_TOTAL + o], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace rhj
