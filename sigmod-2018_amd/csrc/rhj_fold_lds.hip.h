// rhj_fold_lds.hip.h — the weighted join folds whose table fits a workgroup's LDS: one workgroup, one item, one launch
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// rhj_join_fold_batch.hip.h folds an item in up to three launches over a table in HBM: right for sides of millions of rows,
// where the launches' grids fill the device, and the wrong shape for an item of a few thousand rows, whose every claim, add
// and lookup is a device-scope atomic or a dependent round trip to L2 between launches that each wait for the one before.
// With rhj_set_fold_resident on an item that fold_resident_rule names RESIDENT runs here instead:
//   k_fold_lds      grid = the chunk's resident items, one workgroup each, found through an index array uploaded with the chunk
// The table is the same table — jsum_slots(build rows) slots of 1 + nvalues u64 words {key, A_0 ...}, the home slot jsum_hash,
// linear probing, key word JSUM_EMPTY free, the side jsum_build_side names claims — in dynamic LDS, behind the item's fixed
// words: the empty key's A_c (FOLD_LDS_W_EMPTY + c) and the four waves' partial totals (FOLD_LDS_W_PART + 4 * o + wave).  The
// item needs no arena bytes, no memset and no claim launch; its JoinFoldDesc is the table form's with `table` unused.
//
// The workgroup walks the phases the three launches are, over the sides' 2048-row tiles as jsum_keys lays them out (a thread's
// 8 rows are tile * 2048 + round * 256 + thread), with a barrier where the table form has a launch boundary:
//   1  clear the fixed words and the table
//   2  where R builds, R's rows claim their keys (one 64-bit LDS compare-and-swap, workgroup scope; nobody waits, as in
//      jsum_claim); barrier; S's rows find their slot, claiming it only where S builds, and add V_c(j) per value with one
//      64-bit LDS atomic add.  A miss where R builds adds nothing, a row with the key JSUM_EMPTY adds to the empty key's
//      words, and a wave's round whose rows with a slot all have the SAME slot adds up by shuffles and lets one lane add
//      (fold_wave_lead, the add launch's shortcut)
//   3  R's rows find the slot once; per output x = P(i) * A_c (or the empty key's sum, or 0 where the key is not in S), stored
//      when d_out is given (0 is written, not left; nothing at or beyond d_out[nR]) and summed per wave into the wave's word
//   4  one thread per output adds the four waves' words and stores words[FOLD_W_TOTAL + o]: the workgroup owns the item, so a
//      plain store, no atomic.  The combiner's words stay 0: there is no table launch and no tile to count.
// Everything is a sum modulo 2^64, so the answers are the table form's bit for bit.
#pragma once
#include "rhj.h"
#include "rhj_inter.h"
#include "rhj_join_fold_batch.hip.h"

namespace rhj {

constexpr uint64_t FOLD_LDS_WORDS = 16384;           // the most u64 words of a resident table: 128 KiB
constexpr uint64_t FOLD_LDS_MAX_ROWS = 16384;        // the most rows of the side that does not build: the largest power of two at which eight items, one workgroup each, measured no slower than the table form
constexpr int FOLD_LDS_W_EMPTY = 0;                  // the fixed words in front of the table: the empty key's A_c ...
constexpr int FOLD_LDS_W_PART = RHJ_FOLD_MAX_VALUES; // ... then every output's partial totals, one a wave
constexpr int FOLD_LDS_FIXED_WORDS = FOLD_LDS_W_PART + 4 * RHJ_FOLD_MAX_OUTS;

// 1 when an item of these sizes is resident: both sides have rows, the table of the build side fits FOLD_LDS_WORDS, and the
// other side, which one workgroup walks alone, has at most FOLD_LDS_MAX_ROWS rows
constexpr int fold_resident_rule(uint64_t nR, uint64_t nS, int nvalues)
{
    if (nR == 0 || nS == 0 || nvalues < 0 || nvalues > RHJ_FOLD_MAX_VALUES) return 0;
    const int build = jsum_build_side(nR, nS);
    const uint64_t nb = build ? nS : nR, no = build ? nR : nS;
    if (nb > FOLD_LDS_WORDS) return 0;               // (so the product below stays small)
    return jsum_slots(nb) * (uint64_t)(1 + nvalues) <= FOLD_LDS_WORDS && no <= FOLD_LDS_MAX_ROWS;
}
static_assert(fold_resident_rule(4096, 4096, 1) && !fold_resident_rule(4097, 4097, 1) && fold_resident_rule(409, 500, 9) && !fold_resident_rule(513, 600, 9), "the resident rule");
// the dynamic LDS of an item that is resident, in bytes
constexpr size_t fold_lds_bytes(uint64_t nR, uint64_t nS, int nvalues)
{
    return (size_t)(FOLD_LDS_FIXED_WORDS + jsum_slots(jsum_build_side(nR, nS) ? nS : nR) * (uint64_t)(1 + nvalues)) * 8;
}

__device__ __forceinline__ void fold_lds_add(jsum_lull at, unsigned long long x)
{
    __hip_atomic_fetch_add(at, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(256) void k_fold_lds(const JoinFoldDesc *__restrict__ descs, const uint32_t *__restrict__ resident)
{
    extern __shared__ __align__(8) unsigned long long fold_lds_raw[];
    const jsum_lull fixed = (jsum_lull)fold_lds_raw, table = fixed + FOLD_LDS_FIXED_WORDS;
    const JoinFoldDesc &d = descs[resident[blockIdx.x]];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t nR = d.n[0], nS = d.n[1];
    const uint32_t log2_slots = d.log2_slots, sw = d.slot_words;
    const int nvalues = d.nvalues, nouts = d.nouts;
    const bool claims = d.build == 1;                    // (workgroup-uniform, as every branch outside the lookups)

    // phase 1
    const uint32_t words = (uint32_t)FOLD_LDS_FIXED_WORDS + (sw << log2_slots);
    for (uint32_t w = threadIdx.x; w < words; w += 256) fixed[w] = 0;
    __syncthreads();

    // phase 2: R's claims where R builds, then S's adds
    if (!claims) {
        for (uint64_t tile = 0; tile < nR; tile += JSUM_TILE) {
            const uint64_t base = tile + threadIdx.x;
            uint64_t key[JSUM_ROUNDS];
            jsum_keys((fb_gcu64)d.col[0], (fb_gcu64)d.sel[0], nR, base, key);
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) {
                if (base + (uint64_t)k * 256 >= nR || key[k] == JSUM_EMPTY) continue;
                (void)jsum_claim<__HIP_MEMORY_SCOPE_WORKGROUP>(table, sw, log2_slots, key[k]);
            }
        }
        __syncthreads();
    }
    for (uint64_t tile = 0; tile < nS; tile += JSUM_TILE) {
        const uint64_t base = tile + threadIdx.x;
        uint64_t slot[JSUM_ROUNDS], pos[JSUM_ROUNDS];
        uint32_t lead[JSUM_ROUNDS];
        {
            uint64_t key[JSUM_ROUNDS];
            jsum_keys((fb_gcu64)d.col[1], (fb_gcu64)d.sel[1], nS, base, key);
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) {
                const uint64_t i = base + (uint64_t)k * 256;
                pos[k] = i < nS ? i : 0;
                slot[k] = JSUM_NONE;
                if (i < nS) {
                    if (key[k] == JSUM_EMPTY) slot[k] = FOLD_OUTSIDE;
                    else slot[k] = claims ? jsum_claim<__HIP_MEMORY_SCOPE_WORKGROUP>(table, sw, log2_slots, key[k])
                                          : jsum_find(table, sw, log2_slots, key[k]);
                }
                lead[k] = fold_wave_lead(slot[k]);
            }
        }
        for (int c = 0; c < nvalues; ++c) {
            uint64_t v[JSUM_ROUNDS];
            fold_factor(d.v[c], pos, v);
            unsigned long long outside = 0;
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) {
                const bool in_table = slot[k] < FOLD_OUTSIDE;
                if (slot[k] == FOLD_OUTSIDE) outside += v[k];
                if (lead[k] < 64u) {                     // (wave-uniform)
                    const unsigned long long sum = jsum_wave_sum(in_table ? v[k] : 0);
                    if (lane == lead[k] && sum) fold_lds_add(&table[sw * slot[k] + 1 + c], sum);
                } else if (in_table && v[k]) {
                    fold_lds_add(&table[sw * slot[k] + 1 + c], (unsigned long long)v[k]);
                }
            }
            outside = jsum_wave_sum(outside);
            if (lane == 0 && outside) fold_lds_add(&fixed[FOLD_LDS_W_EMPTY + c], outside);
        }
    }
    __syncthreads();

    // phase 3
    for (uint64_t tile = 0; tile < nR; tile += JSUM_TILE) {
        const uint64_t base = tile + threadIdx.x;
        uint64_t slot[JSUM_ROUNDS], pos[JSUM_ROUNDS];
        {
            uint64_t key[JSUM_ROUNDS];
            jsum_keys((fb_gcu64)d.col[0], (fb_gcu64)d.sel[0], nR, base, key);
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) {
                const uint64_t i = base + (uint64_t)k * 256;
                pos[k] = i < nR ? i : 0;
                slot[k] = JSUM_NONE;
                if (i < nR) slot[k] = key[k] == JSUM_EMPTY ? FOLD_OUTSIDE : jsum_find(table, sw, log2_slots, key[k]);
            }
        }
        for (int o = 0; o < nouts; ++o) {
            const int c = d.o[o].value;
            const fb_gu64 out = (fb_gu64)d.o[o].out;
            const uint64_t a_outside = fixed[FOLD_LDS_W_EMPTY + c];
            uint64_t p[JSUM_ROUNDS];
            fold_factor(d.o[o].p, pos, p);
            unsigned long long total = 0;
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) {
                const uint64_t i = base + (uint64_t)k * 256;
                const uint64_t a = table[sw * (slot[k] < FOLD_OUTSIDE ? slot[k] : 0) + 1 + c];        // (slot 0 exists)
                const uint64_t x = p[k] * (slot[k] < FOLD_OUTSIDE ? a : slot[k] == FOLD_OUTSIDE ? a_outside : 0);
                if (i < nR) {
                    if (out) out[i] = x;
                    total += x;
                }
            }
            total = jsum_wave_sum(total);
            if (lane == 0) fixed[FOLD_LDS_W_PART + 4 * o + wv] += total;      // (the wave's own word)
        }
    }
    __syncthreads();

    // phase 4
    if (threadIdx.x < (uint32_t)nouts) {
        const uint32_t o = threadIdx.x;
        const jsum_lull part = fixed + FOLD_LDS_W_PART + 4 * o;
        ((jsum_gull)d.words)[FOLD_W_TOTAL + o] = part[0] + part[1] + part[2] + part[3];
    }
}

}  // namespace rhj
