// rhj_subbucket.hip.h — a canonical join on 9..13 radix bits whose buckets are beyond the LDS index: the low-radix argument
// (rhj_lowradix.hip.h) on the two-pass partition's own r-bit layout
// (part of the device code of librhj.so; rhj_kernels.hip.h includes all of it)
//
// At r <= 8 the low-radix path gets the canonical order of every bucket for free from pass 1 running on exactly r bits.  At
// 9..13 bits the ordinary two-pass partition already leaves every r-bit bucket contiguous and in input order, so:
//   partition   the r-bit partition as every join runs it (run_partition: the range drop of a share included);
//   pass B      a stable split of every bucket on key bits [r, r + k): sub-bucket s of bucket b lands at T-bit bucket
//               (s << r) | b, T = r + k — the layout (and hist / psum) the low-radix path hands to k_plan and
//               k_join_fused<false, true>.  A bucket is cut into chunks of SB_CHUNK tuples (never across a bucket's end):
//               k_sb_count counts per (chunk, digit), one exclusive scan (launch_offsets) over [relation][digit][chunk] gives
//               every chunk its place among its bucket's chunks, k_sb_hist / k_scan_psum the T-bit histogram and offsets,
//               k_sb_scatter moves the tuples with stable in-chunk ranks (wave match-any, per-wave counters).  For the probe
//               relation of its bucket (R when histR >= histS, rhjoin.c:86) it also records where every tuple went: emap[e]
//               = T-bit position | (S probes) << 31, e = the tuple's place in the EMIT sequence — bucket by bucket, each
//               bucket's probe side in canonical order (ebase[b] = the probe tuples of the buckets in front of b);
//   join        unchanged: k_lr_parent, k_plan, k_join_fused<false, true> (lr_mode) — equal keys share a sub-bucket, so the
//               matches of a probe tuple and their descending build positions are those of the r-bit join;
//   emit        walks the emit sequence SB_CHUNK positions a workgroup: the match count of a tuple from stash_cnt at its
//               T-bit position, the chunks' totals (k_sb_totals) scanned by launch_offsets, a single match from stash_row,
//               several copied from the internal join's list (k_sb_emit) — every pair once, at its canonical place.
// Row ids are 12-byte intermediates here (Tuple12); a wide input leaves every count zero and the host refuses after the join.
#pragma once
#include "rhj_common.hip.h"
#include "rhj_partition.hip.h"
#include "rhj_join_tiled.hip.h"

namespace rhj {

constexpr int SB_BLOCK = 512;
constexpr int SB_V = 8;
constexpr uint32_t SB_CHUNK = SB_BLOCK * SB_V;    // 4096 tuples a chunk (pass B) and a slot of the emit sequence
constexpr int SB_WAVES = SB_BLOCK / WAVE;
constexpr int SB_MAX_K = 5;                       // r >= 9 and r + k < MAX_BITS (15)
constexpr uint32_t SB_MAX_DIGITS = 1u << SB_MAX_K;

struct SbArgs {
    const Tuple12  *in[2];           // R, S in the r-bit canonical layout (run_partition's final arrays)
    Tuple12        *out[2];          // R, S in the T-bit layout
    const uint64_t *histr, *psumr;   // [2][2^r] of the r-bit partition
    const uint64_t *psumT;           // [2][2^T] (scatter)
    uint64_t       *histT;           // [2][2^T] (k_sb_hist)
    uint32_t       *cbase;           // [2][2^r + 1] first chunk of every bucket; [2^r] = the relation's chunks
    uint64_t       *ebase;           // [2^r + 1] first emit position of every bucket; [2^r] = the emit sequence's length
    uint64_t       *ccnt;            // [2][digits][rowlen] tuples per (chunk, digit), then their exclusive prefix over the array
    uint32_t       *emap;            // [emit sequence] T-bit position of the probe tuple | (S probes) << 31
    const PlanSummary *summary;
    uint32_t        r_bits, k_bits;
    uint32_t        rowlen;          // chunk slots per (relation, digit): >= every relation's chunks + 1
};

// Chunk bases and the emit sequence's bucket bases; one workgroup.
__global__ __launch_bounds__(1024) void k_sb_meta(SbArgs a)
{
    __shared__ uint64_t sm[3 * (1024 / 64 + 1)];
    const uint32_t bins = 1u << a.r_bits;
    const uint32_t per = (bins + 1023) / 1024;
    const uint32_t b0 = threadIdx.x * per, b1 = min(b0 + per, bins);
    uint64_t v[3] = {0, 0, 0};
    for (uint32_t b = b0; b < b1; ++b) {
        const uint64_t hR = a.histr[b], hS = a.histr[bins + b];
        v[0] += (hR + SB_CHUNK - 1) / SB_CHUNK;
        v[1] += (hS + SB_CHUNK - 1) / SB_CHUNK;
        v[2] += (hR != 0 && hS != 0) ? (hR < hS ? hS : hR) : 0;     // the probe side (rhjoin.c:82, :86)
    }
    uint64_t ex[3], tot[3];
    block_excl_scan_n<1024, 3>(v, ex, tot, sm);
    for (uint32_t b = b0; b < b1; ++b) {
        const uint64_t hR = a.histr[b], hS = a.histr[bins + b];
        a.cbase[b] = (uint32_t)ex[0];
        a.cbase[bins + 1 + b] = (uint32_t)ex[1];
        a.ebase[b] = ex[2];
        ex[0] += (hR + SB_CHUNK - 1) / SB_CHUNK;
        ex[1] += (hS + SB_CHUNK - 1) / SB_CHUNK;
        ex[2] += (hR != 0 && hS != 0) ? (hR < hS ? hS : hR) : 0;
    }
    if (threadIdx.x == 0) {
        a.cbase[bins] = (uint32_t)tot[0];
        a.cbase[2 * bins + 1] = (uint32_t)tot[1];
        a.ebase[bins] = tot[2];
    }
}

// The chunk of a workgroup: relation blockIdx.y, bucket b, chunk j of the bucket, its first tuple and length.
struct SbChunk {
    uint32_t b, j, count;
    uint64_t first;
    bool     active;
};
__device__ __forceinline__ SbChunk sb_chunk(const SbArgs &a, uint32_t rel, uint32_t c)
{
    SbChunk ch;
    const uint32_t bins = 1u << a.r_bits;
    const uint32_t *cb = a.cbase + (size_t)rel * (bins + 1);
    ch.active = c < cb[bins] && a.summary->wide_row_ids == 0;
    ch.b = 0; ch.j = 0; ch.count = 0; ch.first = 0;
    if (!ch.active) return ch;
    uint32_t b = 0;                                   // the last bucket whose first chunk is <= c (it has tuples: cb[b + 1] > c)
    for (uint32_t s = bins >> 1; s >= 1; s >>= 1)
        if (cb[b + s] <= c) b += s;
    ch.b = b;
    ch.j = c - cb[b];
    const uint64_t h = a.histr[(size_t)rel * bins + b];
    ch.first = a.psumr[(size_t)rel * bins + b] + (uint64_t)ch.j * SB_CHUNK;
    ch.count = (uint32_t)min((uint64_t)SB_CHUNK, h - (uint64_t)ch.j * SB_CHUNK);
    return ch;
}

// The digits of a chunk's tuples, (wave, round, lane) = chunk order, and their stable ranks among the wave's tuples of the
// same digit; wcnt[w][d] ends as wave w's count of digit d.
__device__ __forceinline__ void sb_rank(const SbArgs &a, const SbChunk &ch, const Tuple12 *in, uint32_t *wcnt, Tuple12 (&t)[SB_V],
                                        uint32_t (&d)[SB_V], uint32_t (&rk)[SB_V], bool load_all)
{
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t dmask = (1u << a.k_bits) - 1u;
    const uint64_t lt = lanemask_lt();
    uint32_t *mycnt = wcnt + w * SB_MAX_DIGITS;
#pragma unroll
    for (int k = 0; k < SB_V; ++k) {
        const uint32_t i = w * (WAVE * SB_V) + k * WAVE + lane;
        const bool ok = i < ch.count;
        t[k] = Tuple12{0u, 0u, 0u};
        if (ok) {
            if (load_all) t[k] = in[ch.first + i];
            else t[k].klo = in[ch.first + i].klo;
        }
        d[k] = ok ? (t[k].klo >> a.r_bits) & dmask : 0u;      // key bits [r, r + k): r + k <= 14 < 32
    }
#pragma unroll
    for (int k = 0; k < SB_V; ++k) {
        const bool ok = w * (WAVE * SB_V) + k * WAVE + lane < ch.count;
        const uint64_t peers = digit_peers(d[k], ok, (int)a.k_bits);
        const uint32_t rank = (uint32_t)__popcll(peers & lt);
        const uint32_t old = mycnt[d[k]];             // the whole group reads its counter, its lowest lane adds the group
        if (ok && rank == 0) mycnt[d[k]] = old + (uint32_t)__popcll(peers);
        rk[k] = old + rank;
    }
}

// ccnt[rel][d][c] = tuples of chunk c with digit d (0 for the slots behind the relation's last chunk).
__global__ __launch_bounds__(SB_BLOCK) void k_sb_count(SbArgs a)
{
    __shared__ uint32_t wcnt[SB_WAVES * SB_MAX_DIGITS];
    const uint32_t rel = blockIdx.y, c = blockIdx.x;
    const uint32_t digits = 1u << a.k_bits;
    uint64_t *cnt = a.ccnt + (size_t)rel * digits * a.rowlen;
    const SbChunk ch = sb_chunk(a, rel, c);
    if (!ch.active) {
        if (threadIdx.x < digits) cnt[(size_t)threadIdx.x * a.rowlen + c] = 0;
        return;
    }
    for (uint32_t i = threadIdx.x; i < SB_WAVES * SB_MAX_DIGITS; i += SB_BLOCK) wcnt[i] = 0;
    __syncthreads();
    Tuple12 t[SB_V];
    uint32_t d[SB_V], rk[SB_V];
    sb_rank(a, ch, a.in[rel], wcnt, t, d, rk, false);
    __syncthreads();
    if (threadIdx.x < digits) {
        uint32_t sum = 0;
        for (int w = 0; w < SB_WAVES; ++w) sum += wcnt[w * SB_MAX_DIGITS + threadIdx.x];
        cnt[(size_t)threadIdx.x * a.rowlen + c] = sum;
    }
}

// histT[rel][(d << r) | b] = tuples of bucket b with digit d: the scanned counts at the bucket's chunk bounds.
__global__ __launch_bounds__(256) void k_sb_hist(SbArgs a)
{
    const uint32_t rel = blockIdx.y;
    const uint32_t bins = 1u << a.r_bits, binsT = bins << a.k_bits;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= binsT) return;
    const uint32_t b = t & (bins - 1u), d = t >> a.r_bits;
    const uint32_t *cb = a.cbase + (size_t)rel * (bins + 1);
    const uint64_t *row = a.ccnt + ((size_t)rel * (1u << a.k_bits) + d) * a.rowlen;
    a.histT[(size_t)rel * binsT + t] = row[cb[b + 1]] - row[cb[b]];
}

// Pass B proper: every chunk's tuples to their T-bit places, in chunk order inside every (bucket, digit); the probe
// relation's tuples leave their T-bit position in the emit map.
__global__ __launch_bounds__(SB_BLOCK) void k_sb_scatter(SbArgs a)
{
    __shared__ uint32_t wcnt[SB_WAVES * SB_MAX_DIGITS];
    __shared__ uint64_t base[SB_MAX_DIGITS];
    const uint32_t rel = blockIdx.y, c = blockIdx.x;
    const SbChunk ch = sb_chunk(a, rel, c);
    if (!ch.active) return;
    const uint32_t bins = 1u << a.r_bits, binsT = bins << a.k_bits, digits = 1u << a.k_bits;
    for (uint32_t i = threadIdx.x; i < SB_WAVES * SB_MAX_DIGITS; i += SB_BLOCK) wcnt[i] = 0;
    __syncthreads();
    Tuple12 t[SB_V];
    uint32_t d[SB_V], rk[SB_V];
    sb_rank(a, ch, a.in[rel], wcnt, t, d, rk, true);
    __syncthreads();
    if (threadIdx.x < digits) {                       // per digit: exclusive prefix over the waves; where this chunk's run starts
        uint32_t run = 0;
        for (int w = 0; w < SB_WAVES; ++w) {
            const uint32_t v = wcnt[w * SB_MAX_DIGITS + threadIdx.x];
            wcnt[w * SB_MAX_DIGITS + threadIdx.x] = run;
            run += v;
        }
        const uint32_t cb0 = a.cbase[(size_t)rel * (bins + 1) + ch.b];
        const uint64_t *row = a.ccnt + ((size_t)rel * digits + threadIdx.x) * a.rowlen;
        base[threadIdx.x] = a.psumT[(size_t)rel * binsT + ((threadIdx.x << a.r_bits) | ch.b)] + (row[c] - row[cb0]);
    }
    __syncthreads();
    const uint64_t hR = a.histr[ch.b], hS = a.histr[bins + ch.b];
    const uint32_t flip = hR < hS ? 1u : 0u;
    const bool probe = hR != 0 && hS != 0 && rel == flip;
    uint32_t *emap = a.emap + (probe ? a.ebase[ch.b] + (uint64_t)ch.j * SB_CHUNK : 0);
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    Tuple12 *out = a.out[rel];
#pragma unroll
    for (int k = 0; k < SB_V; ++k) {
        const uint32_t i = w * (WAVE * SB_V) + k * WAVE + lane;
        if (i < ch.count) {
            const uint64_t dest = base[d[k]] + wcnt[w * SB_MAX_DIGITS + d[k]] + rk[k];
            out[dest] = t[k];
            if (probe) emap[i] = (uint32_t)dest | (flip << 31);
        }
    }
}

struct SbEmitArgs {
    const uint32_t *emap;
    uint64_t        n;               // length of the emit sequence
    const uint8_t  *stash_cnt;       // [nR + nS] match count per probe tuple of the internal join, S behind R
    const uint2    *stash_row;       // [nR + nS] {build row id of the only match | place of the tuple's pairs in tmp, probe row id}
    const uint4    *tmp;             // the internal join's pairs
    uint64_t        nR;
    uint64_t       *ctotal;          // [slots] pairs of every slot (k_sb_totals), then their exclusive prefix
    uint4          *out;
    uint64_t        out_capacity;
};

__device__ __forceinline__ uint64_t sb_stash_at(const SbEmitArgs &a, uint32_t m, bool &flip)
{
    flip = (m >> 31) != 0;
    return (flip ? a.nR : 0) + (m & 0x7fffffffu);
}

// ctotal[slot] = pairs of the emit sequence's positions [slot * SB_CHUNK, (slot + 1) * SB_CHUNK).
__global__ __launch_bounds__(SB_BLOCK) void k_sb_totals(SbEmitArgs a)
{
    __shared__ uint64_t sm[SB_BLOCK / 64 + 1];
    const uint64_t e0 = (uint64_t)blockIdx.x * SB_CHUNK;
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < SB_V; ++k) {
        const uint64_t e = e0 + (uint64_t)k * SB_BLOCK + threadIdx.x;
        if (e < a.n) {
            bool flip;
            sum += a.stash_cnt[sb_stash_at(a, a.emap[e], flip)] & 0x7fu;
        }
    }
    uint64_t tot;
    block_excl_scan<SB_BLOCK>(sum, &tot, sm);
    if (threadIdx.x == 0) a.ctotal[blockIdx.x] = tot;
}

// The pairs of one slot at ctotal[slot]: (row_idR, row_idS), rhjoin.c:169-178.
__global__ __launch_bounds__(SB_BLOCK) void k_sb_emit(SbEmitArgs a)
{
    __shared__ uint32_t wsum[SB_WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t e0 = (uint64_t)blockIdx.x * SB_CHUNK + w * (WAVE * SB_V);
    uint32_t c[SB_V], off[SB_V];
    uint2 row[SB_V];
    bool flip[SB_V];
#pragma unroll
    for (int k = 0; k < SB_V; ++k) {
        const uint64_t e = e0 + (uint64_t)k * WAVE + lane;
        c[k] = 0; row[k] = make_uint2(0, 0); flip[k] = false;
        if (e < a.n) {
            const uint64_t at = sb_stash_at(a, a.emap[e], flip[k]);
            c[k] = a.stash_cnt[at] & 0x7fu;
            row[k] = a.stash_row[at];                 // (not behind the count: both loads wait on the map entry only)
        }
    }
    uint32_t wrun = 0;
#pragma unroll
    for (int k = 0; k < SB_V; ++k) {
        uint32_t tot;
        off[k] = wrun + wave_excl_scan_u32(c[k], &tot);
        wrun += tot;
    }
    if (lane == 0) wsum[w] = wrun;
    __syncthreads();
    uint32_t wbase = 0;
#pragma unroll
    for (int i = 0; i < SB_WAVES; ++i)
        if ((uint32_t)i < w) wbase += wsum[i];
    const uint64_t at0 = a.ctotal[blockIdx.x] + wbase;
    const uint64_t cap = a.out_capacity;
#pragma unroll
    for (int k = 0; k < SB_V; ++k) {
        const uint64_t at = at0 + off[k];
        if (c[k] == 1u) {
            if (at < cap) a.out[at] = make_pair(flip[k], row[k].y, 0u, row[k].x, 0u);
        } else if (c[k] >= 2u) {
            for (uint32_t i = 0; i < c[k]; ++i)
                if (at + i < cap) a.out[at + i] = a.tmp[(uint64_t)row[k].x + i];
        }
    }
}

}  // namespace rhj
