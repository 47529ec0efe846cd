// rhj_join_foldk_batch.hip.h — many weighted join folds on TUPLE keys: the folds of rhj_join_fold_batch.hip.h over up to four columns
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// An item is rhj_join_fold_batch.hip.h's — child values V_c summed per key into A_c, outputs P_o(i) * A_c(keyR(i)) and their totals,
// everything modulo 2^64 — with keyR(i) == keyS(j) read as the equality of all nkeys words, word t of R against word t of S
// (DESIGN.md 4.16).  The words of a side are nkeys columns read through the side's ONE row-id vector.  The launches are the same
// three per chunk:
//   k_foldk_claim   grid = R's 2048-row tiles of the items where R builds:   find or claim the tuple's slot, add nothing
//   k_foldk_add     grid = S's tiles of every item:   find the slot (claim it only where S builds); per value one 64-bit atomic add
//   k_foldk_apply   grid = R's tiles of every item:   find the slot once per row; per output load A_c, multiply, store, reduce
//
// The table.  One compare-and-swap cannot claim 256 bits, and a key filled word after word would need somebody to wait.  So a slot
// does not hold its key: it holds WHO OWNS IT.  A slot is 1 + nvalues u64 words {owner, A_0 ...}; the owner word is
//   low 32 bits    the claiming row's position in the build side + 1 (sides are below 2^32 rows; 0 is "empty", what the memset gives)
//   high 32 bits   foldk_tag of the tuple's hash: bits the comparison may use to pass a foreign slot without a gather
// and it is claimed by the one 64-bit exchange jsum_claim uses.  A thread that meets a taken slot (its own exchange lost, or the slot
// was taken before) reads the owner's position from the word, gathers the owner's nkeys words from the build side's own columns
// through that side's row-id vector, and compares all of them with its own.  Those columns are inputs nobody writes during the
// call, so a slot's meaning is final the moment its exchange lands: nobody waits, there are no flags, and what a launch needs of the
// launch before it has by the launch boundary.  Equal tuples all land in the first slot of their probe sequence whose owner
// carries their tuple; different tuples move on.  The tag only spares gathers: equality is always decided on the gathered words.
// Every probe loop runs at most `slots` steps, and at most half the slots are taken (jsum_slots).
//
// No key value is special: the all-zero tuple and the all-2^64-1 tuple enter the table like any other, so there is no
// outside-the-table case and an item's words are its outputs' totals alone.
//
// The home slot is foldk_home: jsum_hash's multiplier chained over the words, h = (h + word) * JSUM_HASH_MUL from h = 0, and of
// that the top log2_slots bits; at one key it is jsum_hash.
//
// The tiles, fbatch_find, a thread's 8 rows, the one-value-at-a-time loop, the hot-slot rule (all rows of a wave's round that have
// a slot have the SAME slot: the wave adds by shuffles and one lane issues the atomic) and the apply's reduction are
// rhj_join_fold_batch.hip.h's.  nkeys is workgroup-uniform; the loops over the words are unrolled to RHJ_FOLD_MAX_KEYS with a
// uniform test inside, so that every word sits in a register of its own, and the key loads of the eight rows go out together.
#pragma once
#include "rhj.h"
#include "rhj_inter.h"
#include "rhj_join_fold_batch.hip.h"

namespace rhj {

constexpr int FOLDK_W_COMBINE = RHJ_FOLD_MAX_OUTS;       // an item's words: the outputs' totals, then the combiner's two counters
constexpr int FOLDK_WORDS = FOLDK_W_COMBINE + (int)COMBINE_WORDS;
static_assert(RHJ_FOLD_MAX_KEYS == 4, "the kernels name a tuple's four words");

// the hash of a tuple, one word at a time (h = 0 before the first), and the two things read off it
constexpr uint64_t foldk_mix(uint64_t h, uint64_t word) { return (h + word) * JSUM_HASH_MUL; }
constexpr uint64_t foldk_home(uint64_t h, uint32_t log2_slots) { return h >> (64 - log2_slots); }
constexpr uint32_t foldk_tag(uint64_t h) { return (uint32_t)(h >> 16); }
static_assert(foldk_home(foldk_mix(0, 12345), 7) == jsum_hash(12345, 7), "at one key the home slot is the fold batch's");

struct JoinFoldKDesc {
    const uint64_t     *col[2][RHJ_FOLD_MAX_KEYS];       // key columns of R, of S: the first nkeys
    const uint64_t     *sel[2];  // nullptr: the columns' rows 0..n)
    uint64_t            n[2];    // >= 1, < 2^32
    unsigned long long *table;   // slot_words words a slot: the owner, then A_0 ...
    unsigned long long *words;   // FOLDK_WORDS words, zero at launch
    uint32_t            log2_slots;
    uint32_t            slot_words;          // 1 + nvalues
    int                 build;   // the side that claims the slots
    int                 nvalues, nouts;
    int                 nkeys;
    int                 combine; // 1: the add launch combines equal slots per tile in LDS (rhj_slot_combine.hip.h)
    int                 pad;
    FoldFactor          v[RHJ_FOLD_MAX_VALUES];
    FoldOutDesc         o[RHJ_FOLD_MAX_OUTS];
};

struct FoldKSide {                                       // a side's key columns and row-id vector (workgroup-uniform)
    fb_gcu64 col[RHJ_FOLD_MAX_KEYS];
    fb_gcu64 sel;
};

__device__ __forceinline__ FoldKSide foldk_side(const JoinFoldKDesc &d, int side)
{
    FoldKSide s;
#pragma unroll
    for (int t = 0; t < RHJ_FOLD_MAX_KEYS; ++t) s.col[t] = (fb_gcu64)d.col[side][t];
    s.sel = (fb_gcu64)d.sel[side];
    return s;
}

// the key words of a thread's 8 rows of one side (a word beyond nkeys is 0); a row out of bounds reads row 0 in its place (n >= 1)
__device__ __forceinline__ void foldk_keys(const FoldKSide &side, int nkeys, uint64_t n, uint64_t base, uint64_t (&key)[RHJ_FOLD_MAX_KEYS][JSUM_ROUNDS])
{
    uint64_t row[JSUM_ROUNDS];
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) {
        const uint64_t i = base + (uint64_t)k * 256;
        row[k] = i < n ? i : 0;
    }
    if (side.sel) {                                      // (workgroup-uniform)
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) row[k] = side.sel[row[k]];
    }
#pragma unroll
    for (int t = 0; t < RHJ_FOLD_MAX_KEYS; ++t) {
        if (t < nkeys) {                                 // (workgroup-uniform)
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) key[t][k] = side.col[t][row[k]];
        } else {
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) key[t][k] = 0;
        }
    }
}

__device__ __forceinline__ uint64_t foldk_hash(const uint64_t (&mine)[RHJ_FOLD_MAX_KEYS], int nkeys)
{
    uint64_t h = 0;
#pragma unroll
    for (int t = 0; t < RHJ_FOLD_MAX_KEYS; ++t)
        if (t < nkeys) h = foldk_mix(h, mine[t]);
    return h;
}

// whether the build side's row at position `owner` carries the tuple `mine`: the gather that decides every equality
__device__ __forceinline__ bool foldk_owner_is(const FoldKSide &build, int nkeys, uint32_t owner, const uint64_t (&mine)[RHJ_FOLD_MAX_KEYS])
{
    const uint64_t row = build.sel ? build.sel[owner] : (uint64_t)owner;
    uint64_t theirs[RHJ_FOLD_MAX_KEYS];
#pragma unroll
    for (int t = 0; t < RHJ_FOLD_MAX_KEYS; ++t) theirs[t] = t < nkeys ? build.col[t][row] : 0;        // (the loads go out together)
    bool same = true;
#pragma unroll
    for (int t = 0; t < RHJ_FOLD_MAX_KEYS; ++t) same &= theirs[t] == mine[t];                         // (mine is 0 beyond nkeys)
    return same;
}

// foldk_find: the slot whose owner carries `mine`, or JSUM_NONE when the table has none: at most `slots` steps.  (Side: FoldKSide,
// or rhj_join_foldn_batch.hip.h's side with a row-id vector per word; the table protocol is stated here once for both.  Table:
// jsum_gull, a table in the arena, or jsum_lull, one in LDS, rhj_fold_keys_lds.hip.h, whose claims are atomics of SCOPE workgroup.)
template <class Table, class Side>
__device__ __forceinline__ uint64_t foldk_find(Table table, uint32_t sw, uint32_t log2_slots, const Side &build, int nkeys,
                                               const uint64_t (&mine)[RHJ_FOLD_MAX_KEYS])
{
    const uint64_t mask = ((uint64_t)1 << log2_slots) - 1;
    const uint64_t h = foldk_hash(mine, nkeys);
    const uint32_t tag = foldk_tag(h);
    uint64_t s = foldk_home(h, log2_slots);
    for (uint64_t step = 0; step <= mask; ++step, s = (s + 1) & mask) {
        const uint64_t seen = table[sw * s];
        if (seen == 0) break;
        if ((uint32_t)(seen >> 32) == tag && foldk_owner_is(build, nkeys, (uint32_t)seen - 1u, mine)) return s;
    }
    return JSUM_NONE;
}

// foldk_claim: the slot of the tuple `mine` of the build side's row at position `pos`, found or claimed, at most `slots` steps (a
// free slot is always met: at most half are taken); JSUM_NONE only if the table were full
template <int SCOPE = __HIP_MEMORY_SCOPE_AGENT, class Table, class Side>
__device__ __forceinline__ uint64_t foldk_claim(Table table, uint32_t sw, uint32_t log2_slots, const Side &build, int nkeys,
                                                const uint64_t (&mine)[RHJ_FOLD_MAX_KEYS], uint64_t pos)
{
    const uint64_t mask = ((uint64_t)1 << log2_slots) - 1;
    const uint64_t h = foldk_hash(mine, nkeys);
    const uint32_t tag = foldk_tag(h);
    const unsigned long long me = ((unsigned long long)tag << 32) | (unsigned long long)(pos + 1);
    uint64_t s = foldk_home(h, log2_slots);
    for (uint64_t step = 0; step <= mask; ++step, s = (s + 1) & mask) {
        unsigned long long seen = __hip_atomic_load(&table[sw * s], __ATOMIC_RELAXED, SCOPE);
        if (seen == 0) {
            // one exchange; on failure `seen` is the owner word somebody else put there, which stays
            if (__hip_atomic_compare_exchange_strong(&table[sw * s], &seen, me, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) return s;
        }
        if ((uint32_t)(seen >> 32) == tag && foldk_owner_is(build, nkeys, (uint32_t)seen - 1u, mine)) return s;
    }
    return JSUM_NONE;
}

template <class Desc>
__device__ __forceinline__ void foldk_claim_tile(const Desc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    const uint32_t j = fbatch_find(tile_start, ni, blockIdx.x);
    const Desc &d = descs[j];
    const uint32_t tile = blockIdx.x - tile_start[j];
    const uint64_t n = d.n[0];
    const uint64_t base = (uint64_t)tile * JSUM_TILE + threadIdx.x;
    const uint32_t log2_slots = d.log2_slots, sw = d.slot_words;
    const jsum_gull table = (jsum_gull)d.table;
    const int nkeys = d.nkeys;
    const auto R = foldk_side(d, 0);
    uint64_t key[RHJ_FOLD_MAX_KEYS][JSUM_ROUNDS];
    foldk_keys(R, nkeys, n, base, key);
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) {
        const uint64_t i = base + (uint64_t)k * 256;
        if (i >= n) continue;
        const uint64_t mine[RHJ_FOLD_MAX_KEYS] = {key[0][k], key[1][k], key[2][k], key[3][k]};
        (void)foldk_claim(table, sw, log2_slots, R, nkeys, mine, i);
    }
}

template <class Desc>
__device__ __forceinline__ void foldk_add_tile(const Desc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    const uint32_t j = fbatch_find(tile_start, ni, blockIdx.x);
    const Desc &d = descs[j];
    const uint32_t tile = blockIdx.x - tile_start[j];
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n = d.n[1];
    const uint64_t base = (uint64_t)tile * JSUM_TILE + threadIdx.x;
    const uint32_t log2_slots = d.log2_slots, sw = d.slot_words;
    const jsum_gull table = (jsum_gull)d.table;
    const bool claims = d.build == 1;                    // (workgroup-uniform)
    const int nkeys = d.nkeys;
    uint64_t slot[JSUM_ROUNDS], pos[JSUM_ROUNDS];
    uint32_t lead[JSUM_ROUNDS];                          // the lane that adds for the wave when the round's slots are one, else 64
    {
        const auto S = foldk_side(d, 1), B = foldk_side(d, d.build);
        uint64_t key[RHJ_FOLD_MAX_KEYS][JSUM_ROUNDS];
        foldk_keys(S, nkeys, n, base, key);
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) {
            const uint64_t i = base + (uint64_t)k * 256;
            pos[k] = i < n ? i : 0;
            slot[k] = JSUM_NONE;
            if (i < n) {
                const uint64_t mine[RHJ_FOLD_MAX_KEYS] = {key[0][k], key[1][k], key[2][k], key[3][k]};
                slot[k] = claims ? foldk_claim(table, sw, log2_slots, B, nkeys, mine, i) : foldk_find(table, sw, log2_slots, B, nkeys, mine);
            }
            const uint64_t have = __ballot(slot[k] != JSUM_NONE);
            const uint32_t first = have ? (uint32_t)__ffsll((unsigned long long)have) - 1u : 0u;
            const uint64_t s0 = __shfl(slot[k], (int)first, 64);
            const uint64_t same = __ballot(slot[k] == s0);
            lead[k] = (have & (have - 1)) && (have & ~same) == 0 ? first : 64u;       // two or more rows, all in one slot
        }
    }
    fold_add_values<false>(d, table, sw, FOLDK_W_COMBINE, slot, pos, lead);     // (a tuple's slot is below FOLD_OUTSIDE wherever it is not JSUM_NONE)
}

template <class Desc>
__device__ __forceinline__ void foldk_apply_tile(const Desc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    __shared__ unsigned long long part[RHJ_FOLD_MAX_OUTS][4];
    const uint32_t j = fbatch_find(tile_start, ni, blockIdx.x);
    const Desc &d = descs[j];
    const uint32_t tile = blockIdx.x - tile_start[j];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t n = d.n[0];
    const uint64_t base = (uint64_t)tile * JSUM_TILE + threadIdx.x;
    const uint32_t log2_slots = d.log2_slots, sw = d.slot_words;
    const jsum_gull table = (jsum_gull)d.table;
    const int nouts = d.nouts, nkeys = d.nkeys;
    uint64_t slot[JSUM_ROUNDS], pos[JSUM_ROUNDS];
    {
        const auto R = foldk_side(d, 0), B = foldk_side(d, d.build);
        uint64_t key[RHJ_FOLD_MAX_KEYS][JSUM_ROUNDS];
        foldk_keys(R, nkeys, n, base, key);
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) {
            const uint64_t i = base + (uint64_t)k * 256;
            pos[k] = i < n ? i : 0;
            slot[k] = JSUM_NONE;
            if (i < n) {
                const uint64_t mine[RHJ_FOLD_MAX_KEYS] = {key[0][k], key[1][k], key[2][k], key[3][k]};
                slot[k] = foldk_find(table, sw, log2_slots, B, nkeys, mine);
            }
        }
    }
    for (int o = 0; o < nouts; ++o) {
        const int c = d.o[o].value;
        const fb_gu64 out = (fb_gu64)d.o[o].out;
        uint64_t p[JSUM_ROUNDS], a[JSUM_ROUNDS];
        fold_factor(d.o[o].p, pos, p);
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) a[k] = table[sw * (slot[k] != JSUM_NONE ? slot[k] : 0) + 1 + c];     // (slot 0 exists)
        unsigned long long total = 0;
#pragma unroll
        for (int k = 0; k < JSUM_ROUNDS; ++k) {
            const uint64_t i = base + (uint64_t)k * 256;
            const uint64_t x = slot[k] != JSUM_NONE ? p[k] * a[k] : 0;
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
        if (mine) __hip_atomic_fetch_add(&d.words[o], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the three launches of a chunk (the bodies above are shared with rhj_join_foldn_batch.hip.h's kernels)
__global__ __launch_bounds__(256) void k_foldk_claim(const JoinFoldKDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    foldk_claim_tile(descs, tile_start, ni);
}

__global__ __launch_bounds__(256) void k_foldk_add(const JoinFoldKDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    foldk_add_tile(descs, tile_start, ni);
}

__global__ __launch_bounds__(256) void k_foldk_apply(const JoinFoldKDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    foldk_apply_tile(descs, tile_start, ni);
}

}  // namespace rhj
