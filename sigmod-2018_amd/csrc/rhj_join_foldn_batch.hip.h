// rhj_join_foldn_batch.hip.h — many weighted join folds on tuple keys whose WORDS EACH HAVE A ROW-ID VECTOR OF THEIR OWN
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// An item is rhj_join_foldk_batch.hip.h's, except for where a side's key words come from: word t of a side's row at position p is
//   col[t][sel[t] ? sel[t][p] : p]
// with one vector per word.  That is the key of a MATERIALISED NODE: the node's rows are positions, every member
// binding has a row-id vector over them, and the words of one key belong to different members.  The table, the slot
// {owner, A_0 ...} claimed by one 64-bit exchange, "a slot holds who owns it", the hash, the build side, the hot-slot rule, the
// values, the outputs and the three launches are that file's, through the same functions: foldk_find, foldk_claim and the three
// tile bodies are templates over the side, and only the two functions that READ a side's words are written here:
//   foldk_keys       the words of a thread's 8 rows
//   foldk_owner_is   the gather of a slot owner's words
//
// The key load.  A row's distinct vectors are loaded first, all of them before any column: a word without a vector takes the
// position itself, a word whose vector is the previous word's takes the previous word's row id (loaded once), any other word
// loads its own; then the columns are loaded through the row ids.  The three cases are decided on pointers of the descriptor, so
// every test is workgroup-uniform and no load sits under a per-lane branch; a row out of bounds reads position 0 in its place
// (n >= 1), as there.  With every vector of a side the same (or none) the loads are exactly foldk_keys's.
//
//   k_foldn_claim   grid = R's 2048-row tiles of the items where R builds
//   k_foldn_add     grid = S's tiles of every item
//   k_foldn_apply   grid = R's tiles of every item
#pragma once
#include "rhj.h"
#include "rhj_inter.h"
#include "rhj_join_foldk_batch.hip.h"

namespace rhj {

struct JoinFoldNDesc {
    const uint64_t     *col[2][RHJ_FOLD_MAX_KEYS];       // key columns of R, of S: the first nkeys
    const uint64_t     *sel[2][RHJ_FOLD_MAX_KEYS];       // word t's row-id vector; nullptr: the column's rows 0..n)
    uint64_t            n[2];    // >= 1, < 2^32: the sides' positions
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

struct FoldNSide {                                       // a side's key columns and their row-id vectors (workgroup-uniform)
    fb_gcu64 col[RHJ_FOLD_MAX_KEYS];
    fb_gcu64 sel[RHJ_FOLD_MAX_KEYS];
};

__device__ __forceinline__ FoldNSide foldk_side(const JoinFoldNDesc &d, int side)
{
    FoldNSide s;
#pragma unroll
    for (int t = 0; t < RHJ_FOLD_MAX_KEYS; ++t) { s.col[t] = (fb_gcu64)d.col[side][t]; s.sel[t] = (fb_gcu64)d.sel[side][t]; }
    return s;
}

// the key words of a thread's 8 rows of one side (a word beyond nkeys is 0); a row out of bounds reads position 0 in its place
__device__ __forceinline__ void foldk_keys(const FoldNSide &side, int nkeys, uint64_t n, uint64_t base, uint64_t (&key)[RHJ_FOLD_MAX_KEYS][JSUM_ROUNDS])
{
    uint64_t pos[JSUM_ROUNDS];
#pragma unroll
    for (int k = 0; k < JSUM_ROUNDS; ++k) {
        const uint64_t i = base + (uint64_t)k * 256;
        pos[k] = i < n ? i : 0;
    }
    // the row ids, in key[t][] until the columns replace them: every distinct vector is loaded once, before any column
#pragma unroll
    for (int t = 0; t < RHJ_FOLD_MAX_KEYS; ++t) {
        if (t >= nkeys || !side.sel[t]) {                // (workgroup-uniform, as every test here)
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) key[t][k] = pos[k];
        } else if (t > 0 && side.sel[t] == side.sel[t - 1]) {           // the previous word's vector: its row ids are here already
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) key[t][k] = key[t - 1][k];
        } else {
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) key[t][k] = side.sel[t][pos[k]];
        }
    }
#pragma unroll
    for (int t = 0; t < RHJ_FOLD_MAX_KEYS; ++t) {
        if (t < nkeys) {
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) key[t][k] = side.col[t][key[t][k]];
        } else {
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) key[t][k] = 0;
        }
    }
}

// whether the build side's row at position `owner` carries the tuple `mine`: the row id of every word through the word's own
// vector (the loads go out together), then the words
__device__ __forceinline__ bool foldk_owner_is(const FoldNSide &build, int nkeys, uint32_t owner, const uint64_t (&mine)[RHJ_FOLD_MAX_KEYS])
{
    uint64_t row[RHJ_FOLD_MAX_KEYS];
#pragma unroll
    for (int t = 0; t < RHJ_FOLD_MAX_KEYS; ++t) {
        if (t >= nkeys || !build.sel[t]) row[t] = owner;
        else if (t > 0 && build.sel[t] == build.sel[t - 1]) row[t] = row[t - 1];
        else row[t] = build.sel[t][owner];
    }
    uint64_t theirs[RHJ_FOLD_MAX_KEYS];
#pragma unroll
    for (int t = 0; t < RHJ_FOLD_MAX_KEYS; ++t) theirs[t] = t < nkeys ? build.col[t][row[t]] : 0;
    bool same = true;
#pragma unroll
    for (int t = 0; t < RHJ_FOLD_MAX_KEYS; ++t) same &= theirs[t] == mine[t];                         // (mine is 0 beyond nkeys)
    return same;
}

__global__ __launch_bounds__(256) void k_foldn_claim(const JoinFoldNDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    foldk_claim_tile(descs, tile_start, ni);
}

__global__ __launch_bounds__(256) void k_foldn_add(const JoinFoldNDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    foldk_add_tile(descs, tile_start, ni);
}

__global__ __launch_bounds__(256) void k_foldn_apply(const JoinFoldNDesc *__restrict__ descs, const uint32_t *__restrict__ tile_start, uint32_t ni)
{
    foldk_apply_tile(descs, tile_start, ni);
}

}  // namespace rhj
