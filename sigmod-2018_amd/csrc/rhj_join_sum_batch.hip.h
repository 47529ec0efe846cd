// rhj_join_sum_batch.hip.h — the row count and the view sums of many final joins, without their pairs
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// A query's last join is followed by nothing but sums over its pairs.  For a join on keyR(i) == keyS(j) they need no pair:
//   rows                       = sum over keys k of cntR(k) * cntS(k)
//   sum of a view on R's side  = sum over i of cntS(keyR(i)) * val(i)
//   sum of a view on S's side  = sum over j of cntR(keyS(j)) * val(j)           (all modulo 2^64)
// rhj_join_sum_batch_device runs N such items in THREE launches per chunk and waits for the stream once:
//   k_jsum_insert    grid = the 2048-row tiles of the items' build sides:   find or claim the key's slot, build count += 1
//   k_jsum_count     grid = the tiles of the other sides:                   find the key's slot; if there, other count += 1
//   k_jsum_sum       grid = the tiles of R, then of S, of every item:       w = the opposite side's count of the row's key;
//                                                                            matches += w (R's rows), sum_t += w * col_t[src_t[i]]
// Every item has an open-addressing table of 16-byte slots {key, build count, other count} in a device arena, cleared by the
// chunk's first step (one memset of the chunk's tables: the empty key is 0 and so are fresh counts).  The smaller side builds
// (R on a tie), the table has jsum_slots(build rows) slots: a power of two, at least twice the build rows, so at least one
// slot in two stays empty and every probe sequence ends.
//
// Nobody waits.  A slot is claimed by ONE 64-bit compare-and-swap on its key word: a thread that loses the exchange has been
// handed the winner's key, which is final (a key word changes once, from empty), and goes on by itself — to the slot's count
// if the key is its own, to the next slot if not.  Counts are separate atomic adds whose results nobody reads in the same
// launch.  What a phase needs of the phase before it has by the launch boundary; there are no flags.  Every probe loop runs
// at most `slots` steps.
//
// JSUM_EMPTY is a legal key.  Rows that carry it never enter the table: they are counted, per side, in two words of the
// item's own (words JSUM_W_EMPTY + side), and the sum phase reads the opposite side's word as their w.
//
// A workgroup finds its item by fbatch_find in the launch's array of tile starts and reads the item's JoinSumDesc from a device
// array uploaded once per chunk; both come through const __restrict__ kernel arguments and are read at a workgroup-uniform
// index.  A thread's 8 rows are tile * 2048 + round * 256 + thread.  In the sum phase the loads of
// a term's 8 rows go out together, outside any per-lane branch; a row out of bounds reads row 0 and has w = 0.  Sums go per
// wave by shuffles, per workgroup through LDS, then one atomic add per word and workgroup into the item's accumulator words,
// which the host copies back, the whole chunk's in one copy, behind the third launch.
//
// With the descriptor's `combine` field set (rhj_set_fold_combine) the two count launches run the combiner of
// rhj_slot_combine.hip.h: a tile's rows of one slot count up in LDS and the slot's count word takes ONE add a tile
// (jsum_combine_counts); with it clear they add 1 a row, as written below.  The counts, and so every answer, are the same.
#pragma once
#include "rhj.h"
#include "rhj_inter.h"
#include "rhj_filter_batch.hip.h"
#include "rhj_slot_combine.hip.h"

namespace rhj {

constexpr int JSUM_ROUNDS = 8;
constexpr uint32_t JSUM_TILE = 2048;                 // 256 threads x 8 rows
constexpr uint64_t JSUM_EMPTY = 0;                   // the key word of an empty slot; rows with this key are counted outside the table
constexpr uint64_t JSUM_HASH_MUL = 0x9E3779B97F4A7C15ull;       // odd: key -> key * MUL is a bijection of the 64-bit keys
constexpr uint64_t JSUM_SLOTS_PER_ROW = 2;           // slots >= this many times the build side's rows
constexpr uint64_t JSUM_SLOT_BYTES = 16;             // {u64 key, u32 build count, u32 other count}
constexpr uint32_t JSUM_SLOT_WORDS = 2;              // the same in u64 words: what these kernels pass the table's functions
constexpr uint64_t JSUM_NONE = ~(uint64_t)0;         // no slot: the key is not in the table
constexpr int JSUM_W_MATCHES = 0, JSUM_W_SUM = 1, JSUM_W_EMPTY = 1 + RHJ_JOIN_SUM_MAX_TERMS;
constexpr int JSUM_WORDS = 11 + (int)COMBINE_WORDS;   // an item's accumulator words: matches, the sums, the empty key's rows of R and of S, the combiner's two counters
constexpr int JSUM_W_COMBINE = JSUM_WORDS - (int)COMBINE_WORDS;
static_assert(JSUM_ROUNDS == COMBINE_ROWS && JSUM_TILE == COMBINE_ENTRIES && JSUM_W_COMBINE == JSUM_W_EMPTY + 2, "the combiner's tile is this file's, its counters follow the words above");

// log2 of the slots of a table built from `rows` rows: the smallest power of two that is >= JSUM_SLOTS_PER_ROW * rows, at least 2
constexpr uint32_t jsum_log2_slots(uint64_t rows)
{
    uint32_t l = 1;
    while (((uint64_t)1 << l) < JSUM_SLOTS_PER_ROW * rows) ++l;
    return l;
}
constexpr uint64_t jsum_slots(uint64_t rows) { return (uint64_t)1 << jsum_log2_slots(rows); }
// the home slot: the top log2_slots bits of the multiplicative hash of all 64 key bits (1 <= log2_slots <= 63)
constexpr uint64_t jsum_hash(uint64_t key, uint32_t log2_slots) { return (key * JSUM_HASH_MUL) >> (64 - log2_slots); }
// R builds unless S is strictly smaller
constexpr int jsum_build_side(uint64_t nR, uint64_t nS) { return nS < nR ? 1 : 0; }
static_assert(jsum_slots(1) == 2 && jsum_slots(1024) == 2048 && jsum_slots(1025) == 4096 && jsum_build_side(5, 5) == 0, "the table's rule");
static_assert(JSUM_SLOT_WORDS * 8 == JSUM_SLOT_BYTES, "one slot size");

struct JoinSumTermDesc {
    const uint64_t *src;         // nullptr: q = p
    const uint64_t *col;
    int             side;        // 0: p = i of R, 1: p = j of S
    int             pad;
};

struct JoinSumDesc {
    const uint64_t     *col[2];  // key column of R, of S
    const uint64_t     *sel[2];  // nullptr: the column's rows 0..n)
    uint64_t            n[2];    // >= 1, < 2^32
    unsigned long long *table;   // 2 words a slot: the key, then the two counts
    unsigned long long *words;   // JSUM_WORDS accumulator words, zero at launch
    uint32_t            log2_slots;
    int                 build;   // the side that builds
    uint32_t            tilesR;  // the sum phase: the item's tiles below this one are R's, the others S's
    int                 nterms;
    int                 combine; // 1: the two count launches combine equal slots per tile in LDS (rhj_slot_combine.hip.h)
    int                 pad;
    JoinSumTermDesc     t[RHJ_JOIN_SUM_MAX_TERMS];
};

typedef __attribute__((address_space(1))) unsigned long long *jsum_gull;
typedef __attribute__((address_space(1))) uint32_t *jsum_gu32;
typedef __attribute__((address_space(3))) unsigned long long *jsum_lull;     // a table in LDS (rhj_fold_lds.hip.h)

// the keys of a thread's 8 rows of one side; a row out of bounds reads row 0 in its place (n >= 1)
__device__ __forceinline__ void jsum_keys(fb_gcu64 col, fb_gcu64 sel, uint64_t n, uint64_t base, uint64_t (&key)[JSUM_ROUNDS])
{
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) {
        const uint64_t i = base + (uint64_t)k * 256;
        key[k] = i < n ? i : 0;
    }
    if (sel) {                                           // (workgroup-uniform)
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) key[k] = sel[key[k]];
    }
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) key[k] = col[key[k]];
}

// The table's two functions, over slots of `sw` u64 words whose first is the key (`key` != JSUM_EMPTY).  Table: jsum_gull, a
// table in the arena, or jsum_lull, one in LDS, whose claims are atomics of SCOPE workgroup: one hash and one protocol for both.
// jsum_find: the slot that holds `key`, or JSUM_NONE when the table has none: at most `slots` steps
template <class Table>
__device__ __forceinline__ uint64_t jsum_find(Table table, uint32_t sw, uint32_t log2_slots, uint64_t key)
{
    const uint64_t mask = ((uint64_t)1 << log2_slots) - 1;
    uint64_t s = jsum_hash(key, log2_slots);
    for (uint64_t step = 0; step <= mask; ++step, s = (s + 1) & mask) {
        const uint64_t k = table[sw * s];
        if (k == key) return s;
        if (k == JSUM_EMPTY) break;
    }
    return JSUM_NONE;
}

// jsum_claim: the slot of `key`, found or claimed, at most `slots` steps (a free slot is always met: at most half are taken);
// JSUM_NONE only if the table were full
template <int SCOPE = __HIP_MEMORY_SCOPE_AGENT, class Table>
__device__ __forceinline__ uint64_t jsum_claim(Table table, uint32_t sw, uint32_t log2_slots, uint64_t key)
{
    const uint64_t mask = ((uint64_t)1 << log2_slots) - 1;
    uint64_t s = jsum_hash(key, log2_slots);
    for (uint64_t step = 0; step <= mask; ++step, s = (s + 1) & mask) {
        unsigned long long seen = __hip_atomic_load(&table[sw * s], __ATOMIC_RELAXED, SCOPE);
        if (seen == JSUM_EMPTY) {
            // one exchange; on failure `seen` is the key somebody else put there, which stays
            if (__hip_atomic_compare_exchange_strong(&table[sw * s], &seen, (unsigned long long)key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) seen = key;
        }
        if (seen == key) return s;
    }
    return JSUM_NONE;
}

// the sum of a wave's 64 values of x, in every lane (T: the 32-bit sums shuffle one register, the 64-bit ones two)
template <class T>
__device__ __forceinline__ T jsum_wave_sum(T x)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

// adds a side's rows with the empty key to the item's word of that side: one atomic a wave
__device__ __forceinline__ void jsum_count_empty(unsigned long long *words, int side, uint32_t mine)
{
    mine = jsum_wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) __hip_atomic_fetch_add(&words[JSUM_W_EMPTY + side], (unsigned long long)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a count launch's tile with the combiner on: the tile's rows of one slot meet in LDS and the slot's count word (`word`: 0 the
// build side's, 1 the other's) takes one add a tile; a bypassing row and a bailed-out tile add 1 a row, as without it
__device__ __forceinline__ void jsum_combine_counts(jsum_gull table, int word, const uint64_t (&slot)[JSUM_ROUNDS], unsigned long long *words)
{
    CombineLds<uint32_t> &L = combine_lds<uint32_t>();
    uint32_t roles, adds = 0;
    const bool combined = combine_claim(L, slot, JSUM_NONE, roles);          // (workgroup-uniform)
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) {
        if (slot[k] == JSUM_NONE) continue;
        if (combined && combine_role(roles, k) != COMBINE_BYPASS) { combine_add(L, slot[k], 1u); continue; }
        __hip_atomic_fetch_add((jsum_gu32)(table + JSUM_SLOT_WORDS * slot[k] + 1) + word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ++adds;
    }
    if (combined) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) {
            if (combine_role(roles, k) != COMBINE_OWNER) continue;
            __hip_atomic_fetch_add((jsum_gu32)(table + JSUM_SLOT_WORDS * slot[k] + 1) + word, combine_take(L, slot[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ++adds;                                      // (an owner counts itself: never 0)
        }
    }
    combine_report(L, words + JSUM_W_COMBINE, combined, adds);
}

__global__ __launch_bounds__(256) void k_jsum_insert(const JoinSumDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    const uint32_t j = fbatch_find(tile_start, ni, blockIdx.x);
    const JoinSumDesc &d = descs[j];
    const uint32_t tile = blockIdx.x - tile_start[j];
    const int side = d.build;
    const uint64_t n = d.n[side];
    const uint64_t base = (uint64_t)tile * JSUM_TILE + threadIdx.x;
    const uint32_t log2_slots = d.log2_slots;
    const jsum_gull table = (jsum_gull)d.table;
    uint64_t key[JSUM_ROUNDS];
    jsum_keys((fb_gcu64)d.col[side], (fb_gcu64)d.sel[side], n, base, key);
    uint32_t empty = 0;
    if (d.combine) {                                     // (workgroup-uniform)
        uint64_t slot[JSUM_ROUNDS];
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) {
            slot[k] = JSUM_NONE;
            if (base + (uint64_t)k * 256 >= n) continue;
            if (key[k] == JSUM_EMPTY) { ++empty; continue; }
            slot[k] = jsum_claim(table, JSUM_SLOT_WORDS, log2_slots, key[k]);
        }
        jsum_combine_counts(table, 0, slot, d.words);
        jsum_count_empty(d.words, side, empty);
        return;
    }
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) {
        if (base + (uint64_t)k * 256 >= n) continue;
        const uint64_t mine = key[k];
        if (mine == JSUM_EMPTY) { ++empty; continue; }
        const uint64_t s = jsum_claim(table, JSUM_SLOT_WORDS, log2_slots, mine);
        if (s != JSUM_NONE) __hip_atomic_fetch_add((jsum_gu32)(table + JSUM_SLOT_WORDS * s + 1), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    jsum_count_empty(d.words, side, empty);
}

__global__ __launch_bounds__(256) void k_jsum_count(const JoinSumDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    const uint32_t j = fbatch_find(tile_start, ni, blockIdx.x);
    const JoinSumDesc &d = descs[j];
    const uint32_t tile = blockIdx.x - tile_start[j];
    const int side = d.build ^ 1;
    const uint64_t n = d.n[side];
    const uint64_t base = (uint64_t)tile * JSUM_TILE + threadIdx.x;
    const uint32_t log2_slots = d.log2_slots;
    const jsum_gull table = (jsum_gull)d.table;
    uint64_t key[JSUM_ROUNDS];
    jsum_keys((fb_gcu64)d.col[side], (fb_gcu64)d.sel[side], n, base, key);
    uint32_t empty = 0;
    if (d.combine) {                                     // (workgroup-uniform)
        uint64_t slot[JSUM_ROUNDS];
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) {
            slot[k] = JSUM_NONE;
            if (base + (uint64_t)k * 256 >= n) continue;
            if (key[k] == JSUM_EMPTY) { ++empty; continue; }
            slot[k] = jsum_find(table, JSUM_SLOT_WORDS, log2_slots, key[k]);
        }
        jsum_combine_counts(table, 1, slot, d.words);
        jsum_count_empty(d.words, side, empty);
        return;
    }
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) {
        if (base + (uint64_t)k * 256 >= n) continue;
        const uint64_t mine = key[k];
        if (mine == JSUM_EMPTY) { ++empty; continue; }
        const uint64_t s = jsum_find(table, JSUM_SLOT_WORDS, log2_slots, mine);
        if (s != JSUM_NONE) __hip_atomic_fetch_add((jsum_gu32)(table + JSUM_SLOT_WORDS * s + 1) + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    jsum_count_empty(d.words, side, empty);
}

__global__ __launch_bounds__(256) void k_jsum_sum(const JoinSumDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    __shared__ unsigned long long part[1 + RHJ_JOIN_SUM_MAX_TERMS][4];
    const uint32_t j = fbatch_find(tile_start, ni, blockIdx.x);
    const JoinSumDesc &d = descs[j];
    uint32_t tile = blockIdx.x - tile_start[j];
    const int side = tile >= d.tilesR;                   // (workgroup-uniform, as every branch outside the lookups)
    if (side) tile -= d.tilesR;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t n = d.n[side];
    const uint64_t base = (uint64_t)tile * JSUM_TILE + threadIdx.x;
    const uint32_t log2_slots = d.log2_slots;
    const jsum_gull table = (jsum_gull)d.table;
    const int nterms = d.nterms;
    // the opposite side's count sits in the build word when the opposite side built
    const int opposite = (d.build == side) ? 1 : 0;      // word of a slot's counts: 0 build, 1 other
    const uint64_t w_empty = d.words[JSUM_W_EMPTY + (side ^ 1)];      // written by the two launches before this one
    uint64_t key[JSUM_ROUNDS], w[JSUM_ROUNDS];
    jsum_keys((fb_gcu64)d.col[side], (fb_gcu64)d.sel[side], n, base, key);
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) {
        w[k] = 0;
        if (base + (uint64_t)k * 256 >= n) continue;
        const uint64_t mine = key[k];
        if (mine == JSUM_EMPTY) { w[k] = w_empty; continue; }
        const uint64_t s = jsum_find(table, JSUM_SLOT_WORDS, log2_slots, mine);
        if (s != JSUM_NONE) w[k] = ((jsum_gu32)(table + JSUM_SLOT_WORDS * s + 1))[opposite];
    }
    if (side == 0) {
        unsigned long long m = 0;
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) m += w[k];
        m = jsum_wave_sum(m);
        if (lane == 0) part[0][wv] = m;
    }
    for (int t = 0; t < nterms; ++t) {
        if (d.t[t].side != side) continue;
        const fb_gcu64 src = (fb_gcu64)d.t[t].src, col = (fb_gcu64)d.t[t].col;
        uint64_t q[JSUM_ROUNDS], v[JSUM_ROUNDS];
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) {
            const uint64_t i = base + (uint64_t)k * 256;
            q[k] = i < n ? i : 0;
        }
        if (src) {
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) q[k] = src[q[k]];
        }
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) v[k] = col[q[k]];
        unsigned long long s = 0;
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) s += w[k] * v[k];          // (w = 0 out of bounds)
        s = jsum_wave_sum(s);
        if (lane == 0) part[1 + t][wv] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long *words = d.words;
        if (side == 0) {
            const unsigned long long mine = part[0][0] + part[0][1] + part[0][2] + part[0][3];
            if (mine) __hip_atomic_fetch_add(&words[JSUM_W_MATCHES], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        for (int t = 0; t < nterms; ++t) {
            if (d.t[t].side != side) continue;
            const unsigned long long mine = part[1 + t][0] + part[1 + t][1] + part[1 + t][2] + part[1 + t][3];
            if (mine) __hip_atomic_fetch_add(&words[JSUM_W_SUM + t], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace rhj
