// rhj_slot_combine.hip.h — a tile's adds to one table slot meet in LDS, and one atomic per (tile, slot, value) goes to the table
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// The table batches (rhj_join_sum_batch.hip.h, rhj_join_fold_batch.hip.h and the two on tuple keys) add into the slot of a row's
// key with one device-scope atomic a row and value.  Every row of one key adds to ONE address, and one address takes about 80 adds
// a microsecond whoever sends them: a side whose join column has few distinct values costs its rows' multiplicity,
// not its bytes.  This file is the workgroup-level combiner the four add kernels share: k_fold_add,
// foldk_add_tile (k_foldk_add, k_foldn_add), k_jsum_insert and k_jsum_count, behind the descriptors' `combine` field
// (rhj_set_fold_combine).  Sums modulo 2^64 and counts do not depend on the order of their terms, so the answers are bit for bit
// those of the per-row adds.
//
// A tile (256 threads x 8 rows) has COMBINE_ENTRIES entries in LDS, each a tag and an accumulator.  A row's entry is the low
// COMBINE_LOG2_ENTRIES bits of its slot index (slot indices are the top bits of a multiplicative hash, so their low bits are
// mixed); the tag is the REST of the slot index plus one, 0 being "free": entry and tag together are the slot, for any table
// below 2^43 slots (the batches allow fewer than 2^33), in a 32-bit word.
//
// Once a tile, after the slots are resolved (combine_claim): the tags are cleared; behind a barrier every row with a slot in the
// table tries ONE LDS compare-and-swap on its entry's tag.  A row that finds the entry free is its OWNER (and zeroes the
// accumulator), a row that finds its own slot there is a RIDER, a row that finds another slot BYPASSES: it adds to the table
// itself, as without the combiner, so correctness never depends on the entries.  A tag is written once, so all rows of one slot
// agree on what its entry holds.  Rows outside the table (no slot, the empty key, out of bounds) take no part.
//
// The bail-out.  The tile's riders are counted in LDS (one LDS atomic a wave).  Behind the second barrier every thread reads
// that one word: with fewer than COMBINE_MIN_RIDERS riders the whole workgroup takes the plain per-lane adds for this tile.  The
// choice comes from LDS behind a barrier, so it is workgroup-uniform, and every thread reaches every barrier whatever its rows.
//
// Per value, in a combining tile: owners and riders add into the entry with an LDS atomic (combine_add), a barrier, every owner
// takes its entry's sum, leaves 0 for the next value and issues ONE device-scope atomic of a non-zero sum (combine_take), a
// barrier.  Bypassing rows add directly.
//
// The counters (combine_report): the table adds a tile issued (owners' flushes, bypasses, a bailed-out tile's per-lane adds) go
// per wave by shuffles, per workgroup through LDS, then one atomic a workgroup into the item's word; a combining tile adds 1 to
// the word before it.  With the switch off nothing of this file runs and the kernels are launched without its LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rhj {

constexpr int COMBINE_ROWS = 8;                          // a thread's rows of a tile (JSUM_ROUNDS)
constexpr uint32_t COMBINE_LOG2_ENTRIES = 11;
constexpr uint32_t COMBINE_ENTRIES = 2048;               // a tile's entries: JSUM_TILE, one a row
constexpr uint32_t COMBINE_MIN_RIDERS = 64;              // a tile with fewer riders adds per lane: below a wave's worth of saved adds the barriers cost more
constexpr uint32_t COMBINE_W_TILES = 0, COMBINE_W_ADDS = 1, COMBINE_WORDS = 2;      // the counters: the LAST words of an item's accumulator words
constexpr uint32_t COMBINE_OWNER = 1, COMBINE_RIDER = 2, COMBINE_BYPASS = 3;        // a row's role, two bits a row (0: no slot)
static_assert(COMBINE_ENTRIES == 1u << COMBINE_LOG2_ENTRIES, "a row's entry is its slot's low bits");
static_assert(COMBINE_MIN_RIDERS >= 1, "a tile without a rider has nothing to combine");

// A: the accumulator, u64 sums (the folds) or u32 counts (the join sums): 24 KB or 16 KB of LDS a workgroup
template <class A>
struct CombineLds {
    uint32_t tag[COMBINE_ENTRIES];
    A        acc[COMBINE_ENTRIES];
    uint32_t riders, adds;
};
static_assert(sizeof(CombineLds<unsigned long long>) <= 32 * 1024, "a workgroup's LDS stays at or below 32 KB");

// the launch's dynamic LDS (sizeof(CombineLds<A>) bytes with the switch on, none with it off)
template <class A>
__device__ __forceinline__ CombineLds<A> &combine_lds()
{
    extern __shared__ __align__(8) unsigned char combine_raw[];
    return *reinterpret_cast<CombineLds<A> *>(combine_raw);
}

__device__ __forceinline__ uint32_t combine_wave_sum(uint32_t x)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

__device__ __forceinline__ uint32_t combine_entry(uint64_t slot) { return (uint32_t)slot & (COMBINE_ENTRIES - 1); }
__device__ __forceinline__ uint32_t combine_role(uint32_t roles, int k) { return (roles >> (2 * k)) & 3u; }

// the tile's claims: `roles` gets every row's role (a row has a slot in the table when slot < limit); returns whether the tile
// combines, the same in every thread.  Two barriers.
template <class A>
__device__ __forceinline__ bool combine_claim(CombineLds<A> &L, const uint64_t (&slot)[COMBINE_ROWS], uint64_t limit, uint32_t &roles)
{
    for (uint32_t e = threadIdx.x; e < COMBINE_ENTRIES; e += 256) L.tag[e] = 0;
    if (threadIdx.x == 0) { L.riders = 0; L.adds = 0; }
    __syncthreads();
    roles = 0;
    uint32_t riders = 0;
#pragma unroll
    for (int k = 0; k < COMBINE_ROWS; ++k) {
        if (slot[k] >= limit) continue;
        const uint32_t e = combine_entry(slot[k]);
        const uint32_t mine = (uint32_t)(slot[k] >> COMBINE_LOG2_ENTRIES) + 1u;
        uint32_t seen = 0, role;
        if (__hip_atomic_compare_exchange_strong(&L.tag[e], &seen, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
            role = COMBINE_OWNER;
            L.acc[e] = 0;
        } else {
            role = seen == mine ? COMBINE_RIDER : COMBINE_BYPASS;
        }
        riders += role == COMBINE_RIDER;
        roles |= role << (2 * k);
    }
    riders = combine_wave_sum(riders);
    if ((threadIdx.x & 63) == 0 && riders) __hip_atomic_fetch_add(&L.riders, riders, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    return L.riders >= COMBINE_MIN_RIDERS;
}

// an owner's or a rider's add into the entry of its slot
template <class A>
__device__ __forceinline__ void combine_add(CombineLds<A> &L, uint64_t slot, A x)
{
    __hip_atomic_fetch_add(&L.acc[combine_entry(slot)], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the owner's: the entry's sum, and 0 left for the next value (between the barrier behind the adds and the one before the next)
template <class A>
__device__ __forceinline__ A combine_take(CombineLds<A> &L, uint64_t slot)
{
    const uint32_t e = combine_entry(slot);
    const A x = L.acc[e];
    L.acc[e] = 0;
    return x;
}

// the tile's counters into counters[COMBINE_W_TILES] and counters[COMBINE_W_ADDS]: one atomic a workgroup and counter.  One barrier.
template <class A>
__device__ __forceinline__ void combine_report(CombineLds<A> &L, unsigned long long *counters, bool combined, uint32_t adds)
{
    adds = combine_wave_sum(adds);
    if ((threadIdx.x & 63) == 0 && adds) __hip_atomic_fetch_add(&L.adds, adds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (combined) __hip_atomic_fetch_add(&counters[COMBINE_W_TILES], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (L.adds) __hip_atomic_fetch_add(&counters[COMBINE_W_ADDS], (unsigned long long)L.adds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace rhj
