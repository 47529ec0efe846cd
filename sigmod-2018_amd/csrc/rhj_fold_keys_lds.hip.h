// rhj_fold_keys_lds.hip.h — the weighted join folds on TUPLE keys whose table fits a workgroup's LDS: one workgroup, one item, one launch
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// rhj_fold_lds.hip.h gave the folds on one key a resident form; this file is that form for the two batches on tuple keys,
// rhj_join_foldk_batch.hip.h (one row-id vector a side) and rhj_join_foldn_batch.hip.h (one a key word).  With
// rhj_set_fold_resident_keys on an item that fold_keys_resident_rule names RESIDENT runs here instead of in the
// memset and the three launches of its chunk:
//   k_foldk_lds     grid = the chunk's resident items of rhj_join_foldk_batch_device, one workgroup each
//   k_foldn_lds     the same for rhj_join_foldn_batch_device
// Both are ONE body, fold_keys_lds_item<Desc>, over the descriptor, as that file's three tile bodies are: only foldk_side,
// foldk_keys and foldk_owner_is know where a side's words come from.
//
// The table is the same table — jsum_slots(build rows) slots of 1 + nvalues u64 words {owner, A_0 ...}, the owner word
// tag << 32 | (position + 1), the home slot foldk_home, linear probing, owner word 0 free, the side jsum_build_side names
// claims — in dynamic LDS, behind the item's fixed words: the four waves' partial totals per output (4 * o + wave).  Tuples have
// no special key, so there are no empty-key words.  A slot holds WHO OWNS IT, not a key: a thread that meets a taken slot
// whose tag matches gathers the owner row's words from the build side's columns in global memory (foldk_owner_is) and
// compares them with its own.  Only the owner words and the sums are in LDS; foldk_find and foldk_claim are templates on the
// table pointer's address space (and the claim on the atomics' scope, workgroup here), so both forms share one hash and one
// protocol.  The item needs no arena bytes, no memset and no claim launch; its descriptor is the table form's with `table`
// unused.
//
// The phases are k_fold_lds's, over the sides' 2048-row tiles as foldk_keys lays them out (a thread's 8 rows are
// tile * 2048 + round * 256 + thread), with a barrier where the table form has a launch boundary:
//   1  clear the fixed words and the table
//   2  where R builds, R's rows claim their tuples (one 64-bit LDS compare-and-swap; nobody waits); barrier
//   3  S's rows find their slot, claiming it only where S builds, and add V_c(j) per value with one 64-bit LDS atomic add.  A
//      miss where R builds adds nothing; a wave's round whose rows with a slot all have the SAME slot adds up by shuffles and
//      lets one lane add (fold_wave_lead)
//   4  barrier; R's rows find the slot once; per output x = P(i) * A_c (0 where the tuple is not in S), stored when d_out is
//      given (0 is written, not left; nothing at or beyond d_out[nR]) and summed per wave into the wave's word
//   5  barrier; one thread per output adds the four waves' words and stores words[o]: the workgroup owns the item, so a plain
//      store, no atomic.  The combiner's two words stay 0: there is no table launch and no tile to count.
// Everything is a sum modulo 2^64, so the answers are the table form's bit for bit.  Every branch outside the lookups is
// workgroup-uniform, and a thread's key words (four words times eight rows) live in a scope that ends before the value or
// output loops start.
#pragma once
#include "rhj.h"
#include "rhj_inter.h"
#include "rhj_fold_lds.hip.h"
#include "rhj_join_foldk_batch.hip.h"
#include "rhj_join_foldn_batch.hip.h"

namespace rhj {

constexpr uint64_t FOLDK_LDS_MAX_ROWS = 4096;        // the most rows of the side that does not build: the largest power of two at which eight items, one workgroup each, measured no slower than the table form (0.84 x at 2^12 rows, 1.15 x at 2^13)
constexpr int FOLDK_LDS_FIXED_WORDS = 4 * RHJ_FOLD_MAX_OUTS;          // the fixed words in front of the table: every output's partial totals, one a wave

// 1 when an item of these sizes is resident: both sides have rows, the table of the build side fits FOLD_LDS_WORDS (nkeys does
// not enter: a slot holds an owner, not a key), and the other side, which one workgroup walks alone, has at most
// FOLDK_LDS_MAX_ROWS rows
constexpr int fold_keys_resident_rule(uint64_t nR, uint64_t nS, int nvalues)
{
    if (nR == 0 || nS == 0 || nvalues < 0 || nvalues > RHJ_FOLD_MAX_VALUES) return 0;
    const int build = jsum_build_side(nR, nS);
    const uint64_t nb = build ? nS : nR, no = build ? nR : nS;
    if (nb > FOLD_LDS_WORDS) return 0;               // (so the product below stays small)
    return jsum_slots(nb) * (uint64_t)(1 + nvalues) <= FOLD_LDS_WORDS && no <= FOLDK_LDS_MAX_ROWS;
}
static_assert(fold_keys_resident_rule(4096, 4096, 1) && !fold_keys_resident_rule(4097, 4097, 1) && fold_keys_resident_rule(409, 500, 9) && !fold_keys_resident_rule(513, 600, 9),
              "the resident rule of the tuple-key folds");
// the dynamic LDS of an item that is resident, in bytes
constexpr size_t fold_keys_lds_bytes(uint64_t nR, uint64_t nS, int nvalues)
{
    return (size_t)(FOLDK_LDS_FIXED_WORDS + jsum_slots(jsum_build_side(nR, nS) ? nS : nR) * (uint64_t)(1 + nvalues)) * 8;
}

template <class Desc>
__device__ __forceinline__ void fold_keys_lds_item(const Desc &d)
{
    extern __shared__ __align__(8) unsigned long long fold_keys_lds_raw[];
    const jsum_lull fixed = (jsum_lull)fold_keys_lds_raw, table = fixed + FOLDK_LDS_FIXED_WORDS;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t nR = d.n[0], nS = d.n[1];
    const uint32_t log2_slots = d.log2_slots, sw = d.slot_words;
    const int nvalues = d.nvalues, nouts = d.nouts, nkeys = d.nkeys;
    const bool claims = d.build == 1;                    // (workgroup-uniform, as every branch outside the lookups)

    // phase 1
    const uint32_t words = (uint32_t)FOLDK_LDS_FIXED_WORDS + (sw << log2_slots);
    for (uint32_t w = threadIdx.x; w < words; w += 256) fixed[w] = 0;
    __syncthreads();

    // phase 2: R's claims where R builds
    if (!claims) {
        const auto R = foldk_side(d, 0);
        for (uint64_t tile = 0; tile < nR; tile += JSUM_TILE) {
            const uint64_t base = tile + threadIdx.x;
            uint64_t key[RHJ_FOLD_MAX_KEYS][JSUM_ROUNDS];
            foldk_keys(R, nkeys, nR, base, key);
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) {
                const uint64_t i = base + (uint64_t)k * 256;
                if (i >= nR) continue;
                const uint64_t mine[RHJ_FOLD_MAX_KEYS] = {key[0][k], key[1][k], key[2][k], key[3][k]};
                (void)foldk_claim<__HIP_MEMORY_SCOPE_WORKGROUP>(table, sw, log2_slots, R, nkeys, mine, i);
            }
        }
        __syncthreads();
    }

    // phase 3: S's adds
    for (uint64_t tile = 0; tile < nS; tile += JSUM_TILE) {
        const uint64_t base = tile + threadIdx.x;
        uint64_t slot[JSUM_ROUNDS], pos[JSUM_ROUNDS];
        uint32_t lead[JSUM_ROUNDS];
        {
            const auto S = foldk_side(d, 1), B = foldk_side(d, d.build);
            uint64_t key[RHJ_FOLD_MAX_KEYS][JSUM_ROUNDS];
            foldk_keys(S, nkeys, nS, base, key);
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) {
                const uint64_t i = base + (uint64_t)k * 256;
                pos[k] = i < nS ? i : 0;
                slot[k] = JSUM_NONE;
                if (i < nS) {
                    const uint64_t mine[RHJ_FOLD_MAX_KEYS] = {key[0][k], key[1][k], key[2][k], key[3][k]};
                    slot[k] = claims ? foldk_claim<__HIP_MEMORY_SCOPE_WORKGROUP>(table, sw, log2_slots, B, nkeys, mine, i)
                                     : foldk_find(table, sw, log2_slots, B, nkeys, mine);
                }
                lead[k] = fold_wave_lead(slot[k]);       // (a tuple's slot is below FOLD_OUTSIDE wherever it is not JSUM_NONE)
            }
        }
        for (int c = 0; c < nvalues; ++c) {
            uint64_t v[JSUM_ROUNDS];
            fold_factor(d.v[c], pos, v);
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) {
                const bool in_table = slot[k] != JSUM_NONE;
                if (lead[k] < 64u) {                     // (wave-uniform)
                    const unsigned long long sum = jsum_wave_sum(in_table ? v[k] : 0);
                    if (lane == lead[k] && sum) fold_lds_add(&table[sw * slot[k] + 1 + c], sum);
                } else if (in_table && v[k]) {
                    fold_lds_add(&table[sw * slot[k] + 1 + c], (unsigned long long)v[k]);
                }
            }
        }
    }
    __syncthreads();

    // phase 4
    for (uint64_t tile = 0; tile < nR; tile += JSUM_TILE) {
        const uint64_t base = tile + threadIdx.x;
        uint64_t slot[JSUM_ROUNDS], pos[JSUM_ROUNDS];
        {
            const auto R = foldk_side(d, 0), B = foldk_side(d, d.build);
            uint64_t key[RHJ_FOLD_MAX_KEYS][JSUM_ROUNDS];
            foldk_keys(R, nkeys, nR, base, key);
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) {
                const uint64_t i = base + (uint64_t)k * 256;
                pos[k] = i < nR ? i : 0;
                slot[k] = JSUM_NONE;
                if (i < nR) {
                    const uint64_t mine[RHJ_FOLD_MAX_KEYS] = {key[0][k], key[1][k], key[2][k], key[3][k]};
                    slot[k] = foldk_find(table, sw, log2_slots, B, nkeys, mine);
                }
            }
        }
        for (int o = 0; o < nouts; ++o) {
            const int c = d.o[o].value;
            const fb_gu64 out = (fb_gu64)d.o[o].out;
            uint64_t p[JSUM_ROUNDS];
            fold_factor(d.o[o].p, pos, p);
            unsigned long long total = 0;
#pragma unroll
            for (int k = 0; k < JSUM_ROUNDS; ++k) {
                const uint64_t i = base + (uint64_t)k * 256;
                const uint64_t a = table[sw * (slot[k] != JSUM_NONE ? slot[k] : 0) + 1 + c];          // (slot 0 exists)
                const uint64_t x = slot[k] != JSUM_NONE ? p[k] * a : 0;
                if (i < nR) {
                    if (out) out[i] = x;
                    total += x;
                }
            }
            total = jsum_wave_sum(total);
            if (lane == 0) fixed[4 * o + wv] += total;   // (the wave's own word)
        }
    }
    __syncthreads();

    // phase 5
    if (threadIdx.x < (uint32_t)nouts) {
        const uint32_t o = threadIdx.x;
        const jsum_lull part = fixed + 4 * o;
        ((jsum_gull)d.words)[o] = part[0] + part[1] + part[2] + part[3];
    }
}

__global__ __launch_bounds__(256) void k_foldk_lds(const JoinFoldKDesc *__restrict__ descs, const uint32_t *__restrict__ resident)
{
    fold_keys_lds_item(descs[resident[blockIdx.x]]);
}

__global__ __launch_bounds__(256) void k_foldn_lds(const JoinFoldNDesc *__restrict__ descs, const uint32_t *__restrict__ resident)
{
    fold_keys_lds_item(descs[resident[blockIdx.x]]);
}

}  // namespace rhj
