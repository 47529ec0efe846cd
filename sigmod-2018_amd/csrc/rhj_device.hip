// rhj_device.hip — launch orchestration, device workspace and staging behind the
// C-ABI of include/rhj.h.  The host-facing reference signatures (RadixHashJoin,
// Filter, result lists) live in rhj_abi.c and call the rhj_host_* helpers below.
//
// There is no CPU fallback: any HIP failure is reported on stderr and returned as
// an error; a missing GPU makes every entry point fail.
#include "rhj_kernels.hip.h"
#include "rhj_shard_kernels.hip.h"
#include "rhj_internal.h"
#include "rhj_block.h"
#include <mutex>
#include <thread>
#include <atomic>
#include <type_traits>
#include <vector>
#include <array>
#include <climits>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <utility>

using namespace rhj;

#define HIP_TRY(x)                                                                          \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) {                                                             \
            fprintf(stderr, "rhj: %s -> %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, \
                    __LINE__);                                                              \
            return -1;                                                                      \
        }                                                                                   \
    } while (0)

namespace {

// RHJ_DEBUG_SYNC=1: synchronise after every launch and name it on stderr (the last name printed before
// a "Memory access fault" is the kernel that faulted).  Diagnostic runs only.
static int g_debug_sync = -1;
static void debug_after_launch(const char *what, hipStream_t s)
{
    if (g_debug_sync < 0) g_debug_sync = getenv("RHJ_DEBUG_SYNC") ? 1 : 0;
    if (!g_debug_sync) return;
    fprintf(stderr, "rhj: launched %s\n", what);
    fflush(stderr);
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) fprintf(stderr, "rhj: %s -> %s\n", what, hipGetErrorString(e));
}
#define RHJ_LAUNCH(kernel, grid, block, lds, stream, ...)                       \
    do {                                                                         \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);       \
        debug_after_launch(#kernel, stream);                                     \
    } while (0)

// kernels compiled apart for sharded joins (template <bool RANGED>): the ordinary form when the range is the whole radix
#define RHJ_LAUNCH_RANGED(kernel, ranged, grid, block, lds, stream, ...)        \
    do {                                                                         \
        if (ranged) RHJ_LAUNCH((kernel<true>), grid, block, lds, stream, __VA_ARGS__);   \
        else        RHJ_LAUNCH((kernel<false>), grid, block, lds, stream, __VA_ARGS__);  \
    } while (0)

struct Buf {
    void  *p = nullptr;
    size_t cap = 0;
};

constexpr int MAX_BITS = 15;
constexpr uint32_t LDS_BUDGET = 160 * 1024;       // bytes per workgroup on gfx950
constexpr uint32_t FUSED_LDS = LDS_BUDGET - FJ_LDS_EXTRA;                     // dynamic LDS of the fused kernels
constexpr uint32_t LDS_MAX_SLOTS = LDS_BUDGET / 4 / 4 * 4;                    // tiled path: k_build_lds owns the whole LDS
constexpr uint32_t FUSED_LDS_CAP = (FUSED_LDS - 128) * 2 / 9;                 // fused: 4 B entry + >= 0.5 B of slot starts per build tuple
static_assert(LDS_MAX_SLOTS * 4 / 5 <= 65534 && FUSED_LDS_CAP <= 65534, "LDS-indexed build sides: 16-bit position + 1");
constexpr uint32_t FOLD_LDS_MAX_BYTES = (uint32_t)(FOLD_LDS_FIXED_WORDS + FOLD_LDS_WORDS) * 8;        // k_fold_lds: the largest resident table and the fixed words
static_assert(FOLD_LDS_MAX_BYTES <= LDS_BUDGET, "a resident fold's table and its fixed words fit a workgroup's LDS");
constexpr uint32_t FOLDK_LDS_MAX_BYTES = (uint32_t)(FOLDK_LDS_FIXED_WORDS + FOLD_LDS_WORDS) * 8;      // k_foldk_lds, k_foldn_lds: the same for the folds on tuple keys
static_assert(FOLDK_LDS_MAX_BYTES <= LDS_BUDGET, "a resident tuple-key fold's table and its fixed words fit a workgroup's LDS");
constexpr uint32_t BUILD_CHUNK = 4096;            // build tuples per 64-bit-table build unit

enum Stage { ST_HIST, ST_SCAN, ST_SCATTER, ST_PLAN, ST_BUILD, ST_COUNT, ST_OFFSETS, ST_PROBE, ST_END, ST_N };

// The workspace buffers of a context, listed once: Ctx declares them and rhj_release() frees them from this list.
#define RHJ_WORKSPACE(X)                                                                                                   \
    X(partR) X(partS) X(tmpR) X(tmpS) X(cntR) X(cntS) X(chunk) X(histpsum) X(passhp) X(units) X(bunits) X(ldsb) X(meta)   \
    X(summary) X(ucount) X(ubase) X(uflag) X(tab32) X(tab64) X(stash_cnt) X(stash_row) X(status) X(dbg) X(bsum) X(digR)  \
    X(digS) X(ovf) X(ovf_base) X(runR) X(runS) X(walk) X(xrows) X(lr_tmp) X(lr_words) X(lr_status) X(stripR) X(stripS)   \
    X(slice_tot) X(sbase) X(sb_cnt) X(sb_meta) X(sb_map) X(batch_arena) X(batch_desc) X(fbatch_arena) X(stats_arena)      \
    X(jsum_arena)                                                                                                          \
    X(inR) X(inS) X(out) X(fcol_sel) X(fmask) X(ftile) X(fbase) X(fout)                                                    \
    X(fcol)                                                      /* staging of an unregistered column (host Filter()) */

// The small pinned host block the device's answers are read back into, one member per kind of read-back.
struct Pinned {
    PlanSummary summary;        // a join's or a partition's plan summary (the small path's k_join_fused stores it here itself)
    uint64_t    walk_units;     // k_join_fused, behind the summary: the units it left to k_join_walk
    uint32_t    ticket[8];      // the fused kernels' ticket words (FusedArgs::ticket; word 4: the speculation failed)
    uint32_t    lr_words[4];    // the split paths' words 0..3 (word 0: a pass-2 tile beyond one batch)
    uint64_t    emit_len;       // sub-bucket path: the emit sequence's length
    uint64_t    hits;           // filter (k_filter_write<true> stores it itself) and select_range: the count
};
static_assert(offsetof(Pinned, walk_units) == sizeof(PlanSummary), "k_join_fused stores the walk count at host_summary + sizeof(PlanSummary) / 8");

struct Ctx {
    bool        ready = false;
    int         device = 0;
    hipStream_t stream = nullptr;
    bool        own_stream = false;
    bool        stream_set = false;  // rhj_set_stream() was called (possibly with the null stream)
    int         bits = 4;
    int         null_on_empty = 0;
    int         force_hbm = 0;
    int         order_any = 0;       // 1: pair order not needed, the library picks the radix (env RHJ_ORDER=any, rhj_set_order(1))
    int         no_fused = 0;
    int         force_fused = 0;     // rhj_set_fused(2): the fused path even where the tiled one is expected to be faster (tiny buckets)
    int         no_resident = 0;
    int         wide_row_ids = 0;    // 1: never use 12-byte intermediates (env RHJ_WIDE_ROW_IDS)
    int         timing = 2;          // 0: no events, rhj_get_stats() times are zero; 1: whole join only; 2: per stage (env RHJ_TIMING, rhj_set_timing)
    bool        stamps = false;      // env RHJ_STAMPS (diagnostics build): in-kernel phase stamps of the fused kernel, read once at load time
    int         no_count_in_pass1 = 0;   // 1: pass 2's counts from the digit bytes (k_hist_runs) at every radix width (env RHJ_NO_COUNT_IN_PASS1; A/B)
    int         no_spec = 0;         // 1: never try the foreign-key speculation (env RHJ_NO_SPEC; rhj_set_spec(0))
    int         spec_score = 2;      // > 0: try it (a speculation that holds adds 1, up to 4; one that fails takes 2 off)
    int         spec_skipped = 0;    // joins not speculated on since the score went to zero: every 16th tries again
    int         last_spec = 0;       // the last join: 0 not tried, 1 held, 2 failed (rhj_last_spec)
    int         no_exact = 1;        // 1: never launch k_join_exact (the default: it measured slower than the gather kernels, profiles/README.md r04a; env RHJ_EXACT=1 / rhj_set_exact(1) turn it on)
    int         exact_score = 2;     // > 0: launch it where it applies (a join it did adds 1, up to 4; one it handed back for its input takes 2 off)
    int         exact_skipped = 0;   // eligible joins not given to it since the score went to zero: every 16th tries again
    int         last_exact = 0;      // the last join: 0 not launched, 1 k_join_exact did the join, 2 it handed over (rhj_last_exact)
    int         walk_count = 0;      // 1: the two-pass fused path reads the ticket words back after every join (rhj_set_walk_count; tests)
    int64_t     last_walk_units = -1;    // the last join or batch: units k_join_walk took, -1 where the number was not fetched (rhj_last_walk_units)
    int         msd = 0;             // RHJ_MSD=1: pass 1 of the two-pass partition takes the HIGH bits of the radix, pass 2 the low ones (A/B)
    int         lo_override = 0;     // RHJ_LO_BITS: pass-1 digit bits of the two-pass partition (experiments; default bits / 2)
    int         seen_wide = 0;       // a join of this process needed 16-byte intermediates: launch those kernels from now on
    int         no_lowradix = 0;     // 1: never take the low-radix path (env RHJ_NO_LOWRADIX; rhj_set_lowradix(0)): big joins on few bits go tiled
    int         no_small = 0;        // 1: never take the three-launch path for small joins (env RHJ_NO_SMALL, rhj_set_small(0))
    uint32_t    small_tiles = 512;   // largest relation, in 8192-tuple tiles, the small path takes (env RHJ_SMALL_TILES; at most SM_MAX_TILES)
    int         cus = 256;           // compute units of the device (one fused workgroup each)
    uint64_t    node_pairs = 65535;
    hipEvent_t  ev[ST_N + 1] = {};
    hipEvent_t  ev_x[4] = {};
    hipEvent_t  ev_batch[2] = {};    // every batched entry point but the query batch: the whole call (what they run alone records the stage events)
    void       *batch_pin = nullptr; // every batched entry point: pinned host block of a chunk's answers and of what is uploaded for it (rhj_block.h)
    size_t      batch_pin_cap = 0;
#define RHJ_BUF(name) Buf name;
    RHJ_WORKSPACE(RHJ_BUF)
#undef RHJ_BUF
    Pinned *pin = nullptr;          // 4 KiB pinned block for read-backs
    void *pin_ring[4] = {nullptr, nullptr, nullptr, nullptr};   // D2H staging of result pairs (16 MiB each)
    hipEvent_t ev_ring[4] = {};
    // REGISTERED host columns (rhj_register_relation_map / the resident InitRelationMap) -> device copy.
    // Nothing else is cached: an unregistered column is uploaded on every call that names it, so a caller
    // that frees a column and gets the same address back never meets the old contents.
    struct Column { void *dev; size_t rows; };
    std::map<const void *, Column> columns;
    std::map<const void *, size_t> pinned;                       // hipHostRegister'ed host ranges (base -> bytes)
    int pin_refusals = 0;                                        // ranges of 64 KiB or more the host refused to pin
    std::multimap<size_t, void *> free_blocks;                  // rhj_dev_alloc: cached blocks by size
    std::map<void *, size_t> live_blocks;                       // rhj_dev_alloc: blocks handed out
    rhj_stats stats = {};
};

// One context per device.  g_all[0] is the library's context (every entry point of round 1..3 works on it); g_all[1..] belong to
// the further devices of rhj_set_devices(n) and are only ever touched by the worker threads of a multi-device join, each of
// which makes its device's context the current one of ITS thread.  `g` stays the name of "the context this thread works on".
constexpr int MAX_DEVICES = 8;
Ctx g_all[MAX_DEVICES];
thread_local Ctx *g_cur = &g_all[0];
#define g (*g_cur)
int g_ndev = 1;                      // devices a join is sharded over (rhj_set_devices, env RHJ_DEVICES)
int g_ndev_env = 0;                  // RHJ_DEVICES as read at load time (applied by the first call that can shard)
int g_balance = 0;                   // rhj_join_devices: 1 cuts the bucket ranges by histR + histS instead of equal widths, 2 also cuts INSIDE hot buckets (rhj_set_devices_balance, env RHJ_DEVICES_BALANCE=hist / slice)
int g_same_device = 0;               // RHJ_DEVICES_SAME=1 (tests): every context on the library's own device — n streams and workspaces on one GPU
int g_query_fold = 0;                // 1: rhj_query_batch_device sums the queries whose predicates are a tree by rounds of rhj_join_fold_batch_device items (rhj_set_query_fold, env RHJ_QUERY_FOLD)
int g_query_fold_keys = 0;           // 1: with g_query_fold, the queries whose predicates are a tree once parallel predicates are grouped fold too, the groups as rhj_join_foldk_batch_device items (rhj_set_query_fold_keys, env RHJ_QUERY_FOLD_KEYS)
int g_query_fold_self = 0;           // 1: with g_query_fold, the queries that fold once one-binding and implied predicates are taken care of fold too, after one rhj_fold_self_batch_device call (rhj_set_query_fold_self, env RHJ_QUERY_FOLD_SELF)
int g_query_fold_nodes = 0;          // 1: with the three fold switches above all on, a query none of them takes runs by levels only until its merged nodes and remaining predicates are a tree, and folds over the nodes from there (rhj_set_query_fold_nodes, env RHJ_QUERY_FOLD_NODES)
uint64_t g_query_fold_node_rows = 1ull << 32;            // a query hands over only while every merged node has fewer rows than this (rhj_set_query_fold_node_rows; a fold's sides are below 2^32 rows)
int g_query_fold_one_wait = 0;       // 1: with g_query_fold, the folding queries over relations of 1..g_query_fold_one_wait_rows rows run as fold programs with one wait each, their filters 0/1 weights (rhj_set_query_fold_one_wait, env RHJ_QUERY_FOLD_ONE_WAIT)
uint64_t g_query_fold_one_wait_rows = 4096;              // the most rows of a relation on that route (rhj_set_query_fold_one_wait_rows): the largest size at which whole relations under weights measured no slower than hit lists
int g_query_sum_last = 0;            // 1: rhj_query_batch_device takes a query's last join as a rhj_join_sum_batch_device item (rhj_set_query_sum_last, env RHJ_QUERY_SUM_LAST)
int g_fold_combine = 1;              // 1: the add launches of the four table batches combine a tile's adds to one slot in LDS and send one atomic per (tile, slot, value) (rhj_slot_combine.hip.h; rhj_set_fold_combine, env RHJ_FOLD_COMBINE)
int g_fold_resident = 0;             // 1: an item of rhj_join_fold_batch_device whose table fits a workgroup's LDS (fold_resident_rule) is folded by one workgroup in one k_fold_lds launch, with no table in the arena (rhj_fold_lds.hip.h; rhj_set_fold_resident, env RHJ_FOLD_RESIDENT)
int g_fold_resident_keys = 0;        // 1: the same for an item of rhj_join_foldk_batch_device or rhj_join_foldn_batch_device (fold_keys_resident_rule): one workgroup, one k_foldk_lds / k_foldn_lds launch, the table of owners in LDS (rhj_fold_keys_lds.hip.h; rhj_set_fold_resident_keys, env RHJ_FOLD_RESIDENT_KEYS); independent of g_fold_resident
int g_query_products = 0;            // 1: rhj_query_batch_device takes a query whose bindings end in several nodes (a cross product) as one query per component and multiplies their answers on the host (rhj_set_query_products, env RHJ_QUERY_PRODUCTS)

// environment defaults are read once at load time; the rhj_set_* calls override them
struct EnvDefaults {
    EnvDefaults()
    {
        const char *e;
        if ((e = getenv("RHJ_DEVICE"))) g.device = atoi(e);
        if ((e = getenv("RHJ_DEVICES"))) g_ndev_env = atoi(e);
        if ((e = getenv("RHJ_DEVICES_SAME"))) g_same_device = atoi(e);
        if ((e = getenv("RHJ_DEVICES_BALANCE"))) g_balance = strcmp(e, "slice") == 0 ? 2 : strcmp(e, "hist") == 0 ? 1 : 0;
        if ((e = getenv("RHJ_RADIX_BITS"))) { int b = atoi(e); if (b >= 1 && b <= 15) g.bits = b; }
        if ((e = getenv("RHJ_EMPTY"))) g.null_on_empty = (strcmp(e, "null") == 0);
        if ((e = getenv("RHJ_FORCE_HBM_TABLE"))) g.force_hbm = atoi(e);
        if ((e = getenv("RHJ_ORDER"))) g.order_any = (strcmp(e, "any") == 0);
        if ((e = getenv("RHJ_NO_FUSED"))) g.no_fused = atoi(e);
        if ((e = getenv("RHJ_FORCE_FUSED"))) g.force_fused = atoi(e);
        if ((e = getenv("RHJ_NO_RESIDENT"))) g.no_resident = atoi(e);
        if ((e = getenv("RHJ_WIDE_ROW_IDS"))) g.wide_row_ids = atoi(e);
        if ((e = getenv("RHJ_NODE_PAIRS"))) g.node_pairs = strtoull(e, nullptr, 10);
        if ((e = getenv("RHJ_NO_SMALL"))) g.no_small = atoi(e);
        if ((e = getenv("RHJ_NO_LOWRADIX"))) g.no_lowradix = atoi(e);
        if ((e = getenv("RHJ_NO_SPEC"))) g.no_spec = atoi(e);
        if ((e = getenv("RHJ_EXACT"))) g.no_exact = !atoi(e);
        if ((e = getenv("RHJ_LO_BITS"))) g.lo_override = atoi(e);
        if ((e = getenv("RHJ_MSD"))) g.msd = atoi(e);
        if ((e = getenv("RHJ_NO_COUNT_IN_PASS1"))) g.no_count_in_pass1 = atoi(e);
        g.stamps = getenv("RHJ_STAMPS") != nullptr;
        if ((e = getenv("RHJ_TIMING"))) g.timing = atoi(e);
        if ((e = getenv("RHJ_QUERY_SUM_LAST"))) g_query_sum_last = atoi(e) != 0;
        if ((e = getenv("RHJ_QUERY_FOLD"))) g_query_fold = atoi(e) != 0;
        if ((e = getenv("RHJ_QUERY_FOLD_KEYS"))) g_query_fold_keys = atoi(e) != 0;
        if ((e = getenv("RHJ_QUERY_FOLD_SELF"))) g_query_fold_self = atoi(e) != 0;
        if ((e = getenv("RHJ_QUERY_FOLD_NODES"))) g_query_fold_nodes = atoi(e) != 0;
        if ((e = getenv("RHJ_QUERY_FOLD_ONE_WAIT"))) g_query_fold_one_wait = atoi(e) != 0;
        if ((e = getenv("RHJ_QUERY_PRODUCTS"))) g_query_products = atoi(e) != 0;
        if ((e = getenv("RHJ_FOLD_COMBINE"))) g_fold_combine = atoi(e) != 0;
        if ((e = getenv("RHJ_FOLD_RESIDENT"))) g_fold_resident = atoi(e) != 0;
        if ((e = getenv("RHJ_FOLD_RESIDENT_KEYS"))) g_fold_resident_keys = atoi(e) != 0;
        if ((e = getenv("RHJ_SMALL_TILES"))) { g.small_tiles = (uint32_t)atoi(e); if (g.small_tiles > SM_MAX_TILES) g.small_tiles = SM_MAX_TILES; }
    }
} env_defaults;

// Stage events by timing level (rhj_set_timing): 2 = all of them, 1 = first and last of a join only, 0 = none.  A record
// between two kernels keeps the second from being fed while the first drains (~6 us, tools/timeline.sh).
static inline bool stage_on(int st) { return g.timing >= 2 || (g.timing >= 1 && (st == ST_HIST || st == ST_END)); }
#define RHJ_STAGE(st) do { if (stage_on(st)) HIP_TRY(hipEventRecord(g.ev[st], g.stream)); } while (0)

int ensure(Buf &b, size_t bytes)
{
    if (bytes <= b.cap) return 0;
    static const bool trace = getenv("RHJ_TRACE") != nullptr;
    if (trace) fprintf(stderr, "rhj-trace:   workspace buffer grows %zu -> %zu bytes (hipFree + hipMalloc)\n", b.cap, bytes);
    const size_t was = b.cap;
    if (b.p) HIP_TRY(hipFree(b.p));
    b.p = nullptr; b.cap = 0;
    // first allocation: what is asked for and an eighth; after that at least double — a query plan's joins come in every
    // size and each regrowth is a hipFree + hipMalloc (two device-wide synchronisations): 41 of them in the `small` run
    size_t want = bytes + bytes / 8 + 4096;
    if (was && was < ((size_t)1 << 30) && want < 2 * was) want = 2 * was;     // (above 1 GiB a regrowth is not a per-query event: no doubling)
    if (hipMalloc(&b.p, want) != hipSuccess) {
        // the generous size does not fit: what was asked for, exactly (a C4-scale buffer of 16 GB must not fail for its slack)
        (void)hipGetLastError();
        b.p = nullptr;
        want = bytes;
        HIP_TRY(hipMalloc(&b.p, want));
    }
    b.cap = want;
    return 0;
}

int ctx_init()
{
    // HIP's current device is per thread: every entry point (all of them come through here under the API
    // lock) selects the library's device on the calling thread before it allocates, records or launches
    if (g.ready) { HIP_TRY(hipSetDevice(g.device)); return 0; }
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (count <= 0) { fprintf(stderr, "rhj: no HIP device visible; this library has no CPU path\n"); return -1; }
    HIP_TRY(hipSetDevice(g.device));
    HIP_TRY(hipDeviceGetAttribute(&g.cus, hipDeviceAttributeMultiprocessorCount, g.device));
    if (g.cus <= 0) g.cus = 256;
    if (!g.stream_set) { HIP_TRY(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking)); g.own_stream = true; }
    for (auto &ev : g.ev) HIP_TRY(hipEventCreate(&ev));
    for (auto &ev : g.ev_x) HIP_TRY(hipEventCreate(&ev));
    for (auto &ev : g.ev_batch) HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(hipHostMalloc((void **)&g.pin, 4096, hipHostMallocDefault));
    // dynamic LDS above 64 KiB has to be requested per kernel
    HIP_TRY(hipFuncSetAttribute((const void *)k_build_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BUDGET));
    {
        const void *fused[6] = {(const void *)k_join_fused<false, false>, (const void *)k_join_fused<false, true>,
                                (const void *)k_join_fused<true, false>, (const void *)k_join_fused<true, true>,
                                (const void *)k_join_spec<false>, (const void *)k_join_spec<true>};
        for (const void *k : fused)
            HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_BUDGET - FJ_LDS_EXTRA)));
        HIP_TRY(hipFuncSetAttribute((const void *)k_join_walk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_BUDGET - FJ_LDS_EXTRA)));
        HIP_TRY(hipFuncSetAttribute((const void *)k_join_exact, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_BUDGET - FJ_LDS_EXTRA)));
    }
    HIP_TRY(hipFuncSetAttribute((const void *)k_small_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)small_lds_bytes(PT_MAX_BITS)));
    HIP_TRY(hipFuncSetAttribute((const void *)k_batch_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)small_lds_bytes(PT_MAX_BITS)));
    HIP_TRY(hipFuncSetAttribute((const void *)k_small_scatter_cols, hipFuncAttributeMaxDynamicSharedMemorySize, (int)small_lds_bytes(PT_MAX_BITS)));
    HIP_TRY(hipFuncSetAttribute((const void *)k_batch_scatter_cols, hipFuncAttributeMaxDynamicSharedMemorySize, (int)small_lds_bytes(PT_MAX_BITS)));
    HIP_TRY(hipFuncSetAttribute((const void *)k_batch_fused<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_BUDGET - FJ_LDS_EXTRA)));
    HIP_TRY(hipFuncSetAttribute((const void *)k_batch_fused<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_BUDGET - FJ_LDS_EXTRA)));
    HIP_TRY(hipFuncSetAttribute((const void *)k_bucket_hist, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4u << MAX_BITS)));
    HIP_TRY(hipFuncSetAttribute((const void *)k_bucket_psum<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(8u << 14)));
    HIP_TRY(hipFuncSetAttribute((const void *)k_scatter_lds<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BUDGET));
    HIP_TRY(hipFuncSetAttribute((const void *)k_scatter_lds<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BUDGET));
    {
        const void *lp[] = {(const void *)k_local_part<false, true, false>, (const void *)k_local_part<false, true, true>,
                            (const void *)k_local_part<false, false, true>, (const void *)k_local_part<true, true, false>,
                            (const void *)k_local_part<true, true, true>,   (const void *)k_local_part<true, false, true>,
                            (const void *)k_local_part<false, true, false, true>, (const void *)k_local_part<false, true, true, true>,
                            (const void *)k_local_part<false, false, true, true>};
        for (const void *k : lp) HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BUDGET));
    }
    HIP_TRY(hipFuncSetAttribute((const void *)k_scatter_runs<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BUDGET));
    HIP_TRY(hipFuncSetAttribute((const void *)k_scatter_runs<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BUDGET));
    HIP_TRY(hipFuncSetAttribute((const void *)k_scatter_runs<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BUDGET));
    HIP_TRY(hipFuncSetAttribute((const void *)k_lr_emit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lr_lds_bytes(PT_MAX_BITS)));
    HIP_TRY(hipFuncSetAttribute((const void *)k_fold_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FOLD_LDS_MAX_BYTES));
    HIP_TRY(hipFuncSetAttribute((const void *)k_foldk_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FOLDK_LDS_MAX_BYTES));
    HIP_TRY(hipFuncSetAttribute((const void *)k_foldn_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FOLDK_LDS_MAX_BYTES));
    g.ready = true;
    return 0;
}

struct PartState {
    bool     launch_wide = false;    // the 16-byte kernels of the two-pass partition were launched (else only the 12-byte ones)
    RelArgs  p2[2];          // two-pass partition: the relations as pass 2 saw them (runs, digit bytes, scanned tile counts) —
                             // the low-radix path replays pass 2's order when it emits (rhj_lowradix.hip.h)
    int      lo_bits = 0;    // two-pass partition: digit bits of pass 1 (0: half of the radix); the low-radix path passes the caller's radix
    RelArgs  r[2];           // in = caller's input, out = final partitioned array
    rhj_tuple *tmp[2];       // intermediate of the two-pass path
    uint64_t *hist, *psum;   // [2][bins] of the join's radix (filled by run_partition)
    const PlanArgs *plan = nullptr;   // the join's plan arguments: a small one-pass partition runs the plan in its scan launch
    bool plan_done = false;
    int      cols_input = 0;  // the inputs are key columns (rhj_join_keys_device): pass 1 of the two-pass partition reads 8 bytes a tuple
};

uint32_t tiles_for(uint64_t n)
{
    const uint64_t t = (n + PT_TILE - 1) / PT_TILE;
    return (uint32_t)(t ? t : 1);
}

size_t scatter_lds_bytes(int bits)
{
    const size_t bins = (size_t)1 << bits;
    return (size_t)PT_TILE * 16 + (PT_WAVES + 2) * bins * 4 + (PT_BLOCK / 64 + 1) * 8 + 16;
}

size_t scatter_runs_lds_bytes(int bits)
{
    const size_t bins = (size_t)1 << bits;
    return (size_t)SR_TILE * 16 + (PT_WAVES + 3) * bins * 4 + (PT_BLOCK / 64 + 2) * 8 + 2 * (SR_RUNOFF + PT_MAX_GROUP) * 4 + 16;   // (run tables double-buffered)
}

// one stable pass over both relations (radix bits <= 8): per-tile histogram, scan, LDS-staged scatter
int partition_pass(RelArgs r0, RelArgs r1, int nrel, int bits, uint64_t *hist, uint64_t *psum, const PlanArgs *plan = nullptr,
                   bool *plan_done = nullptr)
{
    const uint32_t bins = 1u << bits;
    uint32_t max_tiles = r0.tiles;
    if (nrel > 1 && r1.tiles > max_tiles) max_tiles = r1.tiles;
    if (plan && nrel == 2 && max_tiles <= SMALL_TILES) {
        // small join: histogram, {scans + plan} in one single-workgroup launch, scatter — three launches instead of seven
        RHJ_STAGE(ST_HIST);
        RHJ_LAUNCH_RANGED(k_hist_tiles, r0.range_span, dim3(max_tiles, nrel), dim3(256), (size_t)bins * 4, g.stream, r0, r1, 0, bits);
        RHJ_STAGE(ST_SCAN);
        RHJ_LAUNCH(k_small_scan_plan, dim3(1), dim3(1024), 0, g.stream, r0, r1, bits, hist, psum, *plan);
        RHJ_STAGE(ST_SCATTER);
        RHJ_LAUNCH_RANGED(k_scatter_lds, r0.range_span, dim3(max_tiles, nrel), dim3(PT_BLOCK), scatter_lds_bytes(bits), g.stream, r0, r1, 0, bits);
        HIP_TRY(hipGetLastError());
        *plan_done = true;
        return 0;
    }
    uint32_t chunks = (max_tiles + 15) / 16;                  // >= 16 tiles per chunk, at most 512 chunks
    if (chunks > 512) chunks = 512;
    if (chunks < 1) chunks = 1;
    if (ensure(g.chunk, (size_t)2 * chunks * bins * 8)) return -1;
    const uint32_t hist_grid = max_tiles < 2048 ? max_tiles : 2048;
    RHJ_STAGE(ST_HIST);
    RHJ_LAUNCH_RANGED(k_hist_tiles, r0.range_span, dim3(hist_grid, nrel), dim3(256), (size_t)bins * 4, g.stream, r0, r1, 0, bits);
    RHJ_STAGE(ST_SCAN);
    RHJ_LAUNCH(k_scan_chunks, dim3((bins + 255) / 256, chunks, nrel), dim3(256), 0, g.stream, r0, r1, bits,
                       chunks, (uint64_t *)g.chunk.p);
    RHJ_LAUNCH(k_scan_bins, dim3(bins, nrel), dim3(WAVE), 0, g.stream, bits, chunks, (uint64_t *)g.chunk.p, hist);
    RHJ_LAUNCH(k_scan_psum, dim3(nrel), dim3(1024), 0, g.stream, bits, (const uint64_t *)hist, psum);
    RHJ_LAUNCH(k_scan_apply, dim3((bins + 255) / 256, chunks, nrel), dim3(256), 0, g.stream, r0, r1, bits,
                       chunks, (const uint64_t *)g.chunk.p, (const uint64_t *)psum);
    RHJ_STAGE(ST_SCATTER);
    RHJ_LAUNCH_RANGED(k_scatter_lds, r0.range_span, dim3(max_tiles, nrel), dim3(PT_BLOCK), scatter_lds_bytes(bits), g.stream, r0, r1, 0, bits);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Stable radix partition of one or two relations on the low `bits` bits.  bits <= 8: one pass
// (per-tile histogram, scan, LDS-staged scatter).  bits 9..15: two LSD passes in run form — pass 1
// partitions every tile in place on the low half of the bits (no histogram, no offsets), pass 2
// moves the runs to their final places on the high half; the bucket histogram of the full radix is
// the column sum of pass 2's per-tile counts.
// Stage events: one pass  ST_HIST..ST_SCAN histogram, ST_SCAN..ST_SCATTER scan, ST_SCATTER..ST_PLAN scatter;
//               two passes ST_HIST..ST_SCAN pass 1, ST_SCAN..ST_SCATTER pass-2 histogram + scan,
//                          ST_SCATTER..ST_PLAN pass-2 scatter.
// final12: with 12-byte intermediates (row ids below 2^32) the FINAL arrays hold Tuple12 as well — the join's own
// partition on its fused path; rhj_partition_device() hands out rhj_tuple and passes false.
int run_partition(PartState &ps, int bits, int nrel, bool force_wide, bool final12)
{
    const uint32_t bins = 1u << bits;
    if (ensure(g.histpsum, (size_t)4 * bins * 8) || ensure(g.passhp, (size_t)4 * 256 * 8)) return -1;
    ps.hist = (uint64_t *)g.histpsum.p;
    ps.psum = ps.hist + 2 * bins;
    RelArgs none = RelArgs{};
    for (int i = 0; i < nrel; ++i) ps.r[i].tiles = tiles_for(ps.r[i].n);
    if (ensure(g.summary, sizeof(PlanSummary))) return -1;
    if (ensure(g.cntR, (size_t)ps.r[0].tiles * 256 * 4)) return -1;
    ps.r[0].cnt = (uint32_t *)g.cntR.p;
    if (nrel > 1) {
        if (ensure(g.cntS, (size_t)ps.r[1].tiles * 256 * 4)) return -1;
        ps.r[1].cnt = (uint32_t *)g.cntS.p;
    }
    if (bits <= PT_MAX_BITS && !ps.lo_bits) {
        // one pass: no 12-byte intermediates and nothing that checks the row ids, so everything downstream stays wide
        HIP_TRY(hipMemsetAsync(&((PlanSummary *)g.summary.p)->wide_row_ids, 0, 8, g.stream));    // wide_row_ids, row_id_overflow
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)&((PlanSummary *)g.summary.p)->wide_row_ids, 1, 1, g.stream));
        ps.launch_wide = true;
        return partition_pass(ps.r[0], nrel > 1 ? ps.r[1] : none, nrel, bits, ps.hist, ps.psum, ps.plan, &ps.plan_done);
    }

    // ---- two passes in run form (k_local_part .. k_scatter_runs in rhj_kernels.hip.h)
    int lo = ps.lo_bits ? ps.lo_bits : bits / 2;
    if (!ps.lo_bits && g.lo_override > 0 && g.lo_override < bits && bits - g.lo_override <= PT_MAX_BITS && g.lo_override <= PT_MAX_BITS) lo = g.lo_override;   // (RHJ_LO_BITS: experiments)
    const int hi = bits - lo;
    // which end of the radix pass 1 takes: the low `lo` bits (pass 2 then gathers by them and scatters by the high `hi`), or —
    // msd — the high `lo` bits, pass 2 the low `hi` (same buckets, same order inside them: either pass is stable and a pass-2
    // tile reads its runs in tile order).  The low-radix path counts on pass 1 taking the caller's own low bits.
    const bool msd = g.msd && !ps.lo_bits;
    const int sh1 = msd ? hi : 0, sh2 = msd ? 0 : lo;
    const uint32_t bins1 = 1u << lo, bins2 = 1u << hi;
    if (ensure(g.slice_tot, (size_t)2 * bins * FH_SLICES * 4) || ensure(g.sbase, (size_t)2 * bins * FH_SLICES * 4)) return -1;
    RelArgs a0 = ps.r[0], a1 = nrel > 1 ? ps.r[1] : none;
    Buf *digb[2] = {&g.digR, &g.digS}, *runb[2] = {&g.runR, &g.runS}, *cntb[2] = {&g.cntR, &g.cntS}, *partb[2] = {&g.stripR, &g.stripS};
    // pass 1 counts pass 2's digits itself while the (digit, digit) cells fit beside its staging tile (k_local_part); the
    // digit bytes then serve the low-radix emit only
    const bool count_in_pass1 = bits <= 12 && !g.no_count_in_pass1;
    const bool want_dig = !count_in_pass1 || ps.lo_bits != 0;
    RelArgs *ar[2] = {&a0, &a1};
    uint32_t group = 15u * bins1 / 16u;               // a pass-2 tile averages 15/16 of 4096 tuples on uniform keys
    // (the low-radix path replays pass 2 one batch per tile and gives up on a tile beyond 4096 tuples: 7/8 of a batch on
    // average puts the limit 8 standard deviations away on uniform keys — at 15/16 it was 4, and 100 M tuples have 49 K tiles)
    if (ps.lo_bits) group = 7u * bins1 / 8u;
    if (group < 1) group = 1;
    if (group > PT_MAX_GROUP - 1) group = PT_MAX_GROUP - 1;
    uint32_t most_tiles = 0;
    for (int i = 0; i < nrel; ++i) most_tiles = ps.r[i].tiles > most_tiles ? ps.r[i].tiles : most_tiles;
    const uint32_t strip_tiles = most_tiles >= 2048 ? PT_STRIP : most_tiles >= 1024 ? (PT_STRIP < 2 ? PT_STRIP : 2u) : 1u;
    for (int i = 0; i < nrel; ++i) {
        RelArgs &a = *ar[i];
        a.tiles1 = a.tiles;
        a.group = group;
        a.groups = (a.tiles1 + group - 1) / group;
        // strips of 4 tiles when there are enough of them to fill the chip twice over; small relations keep one tile a workgroup
        // (200 K .. 1 M tuples lost 3-6 % of the join to strips of 4: 75 workgroups of four tiles each instead of 245 of one)
        a.strip = strip_tiles;
        a.parts = (group + a.strip - 1) / a.strip;
        a.per = (a.groups + FH_SLICES - 1) / FH_SLICES;
        a.sbase = (uint32_t *)g.sbase.p + (size_t)i * bins * FH_SLICES;
        if ((want_dig && ensure(*digb[i], a.n + 64)) || ensure(*runb[i], (size_t)a.tiles1 * (bins1 + 1) * 2 + 64) ||
            ensure(*cntb[i], (size_t)bins1 * a.groups * bins2 * 4) ||
            (count_in_pass1 && ensure(*partb[i], (size_t)bins * a.groups * a.parts * 2)))
            return -1;
        a.out = ps.tmp[i];
        a.part = count_in_pass1 ? (uint16_t *)partb[i]->p : nullptr;
        a.dig_out = want_dig ? (uint8_t *)digb[i]->p : nullptr;
        a.runs = (uint16_t *)runb[i]->p;
        a.cnt = (uint32_t *)cntb[i]->p;
    }
    RelArgs b0 = a0, b1 = a1;
    RelArgs *br[2] = {&b0, &b1};
    uint32_t max1 = 0, max2 = 0;
    for (int i = 0; i < nrel; ++i) {
        RelArgs &b = *br[i];
        b.in = ps.tmp[i];
        b.out = ps.r[i].out;
        b.dig_in = want_dig ? (const uint8_t *)digb[i]->p : nullptr;
        b.dig_out = nullptr;
        b.tiles = bins1 * b.groups;                   // pass-2 tiles
        if (ar[i]->tiles > max1) max1 = ar[i]->tiles;
        if (b.tiles > max2) max2 = b.tiles;
    }
    // 12-byte intermediates when the row ids fit 32 bits: a sample decides on the device and the pass
    // kernels read the decision there (no host round trip; pass 2 is compiled once per format).  The host
    // launches the 12-byte kernels alone until a join of this process turned out to need the 16-byte ones
    // (g.seen_wide): the sample then reports a wide input as an overflow and the caller runs again wide.
    const bool launch_narrow = !force_wide;
    ps.launch_wide = force_wide || g.seen_wide;
    PlanSummary *dsum = (PlanSummary *)g.summary.p;
    RHJ_STAGE(ST_HIST);
    RHJ_LAUNCH(k_rowid_sample, dim3(1), dim3(1024), 0, g.stream, a0, a1, nrel, force_wide ? 1 : 0, ps.launch_wide ? 0 : 1, dsum, ps.cols_input);
    {
        const uint32_t h2_off = (uint32_t)((scatter_lds_bytes(lo) + 15) & ~(size_t)15);
        const size_t lds1 = count_in_pass1 ? h2_off + ((size_t)2 << bits) : scatter_lds_bytes(lo);
        uint32_t strips = 0;
        for (int i = 0; i < nrel; ++i) strips = ar[i]->groups * ar[i]->parts > strips ? ar[i]->groups * ar[i]->parts : strips;
        const dim3 grid1(count_in_pass1 ? strips : max1, nrel);
        const bool ranged = a0.range_span != 0;
#define RHJ_LP(R, H, D) RHJ_LAUNCH((k_local_part<R, H, D>), grid1, dim3(PT_BLOCK), lds1, g.stream, a0, a1, sh1, lo, sh2, hi, dsum, h2_off)
#define RHJ_LPC(H, D) RHJ_LAUNCH((k_local_part<false, H, D, true>), grid1, dim3(PT_BLOCK), lds1, g.stream, a0, a1, sh1, lo, sh2, hi, dsum, h2_off)
        if (ps.cols_input) { if (!count_in_pass1) RHJ_LPC(false, true); else if (want_dig) RHJ_LPC(true, true); else RHJ_LPC(true, false); }   // (never ranged: join_keys)
        else if (ranged)  { if (!count_in_pass1) RHJ_LP(true, false, true); else if (want_dig) RHJ_LP(true, true, true); else RHJ_LP(true, true, false); }
        else              { if (!count_in_pass1) RHJ_LP(false, false, true); else if (want_dig) RHJ_LP(false, true, true); else RHJ_LP(false, true, false); }
#undef RHJ_LPC
#undef RHJ_LP
    }
    RHJ_STAGE(ST_SCAN);
    if (count_in_pass1)
        RHJ_LAUNCH((k_group_scan<true>), dim3(bins1, nrel, FH_SLICES), dim3(1024), 0, g.stream, b0, b1, hi, (uint32_t *)g.slice_tot.p, msd ? 1 : 0);
    else {
        const uint32_t hw = (max2 + HR_BLOCK / WAVE - 1) / (HR_BLOCK / WAVE);    // one wave per pass-2 tile
        RHJ_LAUNCH(k_hist_runs, dim3(hw < 4096 ? hw : 4096, nrel), dim3(HR_BLOCK), (size_t)bins2 * 4 * (HR_BLOCK / WAVE), g.stream,
                   b0, b1, hi);
        RHJ_LAUNCH((k_group_scan<false>), dim3(bins1, nrel, FH_SLICES), dim3(1024), 0, g.stream, b0, b1, hi, (uint32_t *)g.slice_tot.p, msd ? 1 : 0);
    }
    const int staged = bits >= 13;
#define RHJ_BP(P) RHJ_LAUNCH((k_bucket_psum<P>), dim3(nrel, FH_SLICES), dim3(1024), staged ? (size_t)(bins < 16384u ? bins : 16384u) * 8 : 0, g.stream, lo, hi, \
                            (const uint32_t *)g.slice_tot.p, (uint32_t *)g.sbase.p, ps.hist, ps.psum, staged, msd ? 1 : 0)
    if (bits <= 10) RHJ_BP(1); else if (bits == 11) RHJ_BP(2); else if (bits == 12) RHJ_BP(4); else RHJ_BP(0);
#undef RHJ_BP
    RHJ_STAGE(ST_SCATTER);
    uint32_t search0 = 1;                             // largest power of two <= group: first step of the run search
    while (search0 * 2 <= group) search0 *= 2;
    {
        uint32_t per_cu = (uint32_t)(LDS_BUDGET / scatter_runs_lds_bytes(hi));   // the workgroups that are resident together
        if (per_cu > (uint32_t)SR_MINW * 256u / PT_BLOCK) per_cu = (uint32_t)SR_MINW * 256u / PT_BLOCK;
        if (per_cu < 1) per_cu = 1;
        const uint32_t sgrid = (uint32_t)g.cus * per_cu;
        const uint32_t want = ((max2 < sgrid ? max2 : sgrid) + 7u) & ~7u;     // a multiple of the 8 XCDs
        if (launch_narrow && final12)
            RHJ_LAUNCH((k_scatter_runs<true, true>), dim3(want, nrel), dim3(PT_BLOCK), scatter_runs_lds_bytes(hi), g.stream, b0, b1,
                       sh2, hi, search0, (const PlanSummary *)dsum);
        else if (launch_narrow)
            RHJ_LAUNCH((k_scatter_runs<true, false>), dim3(want, nrel), dim3(PT_BLOCK), scatter_runs_lds_bytes(hi), g.stream, b0, b1,
                       sh2, hi, search0, (const PlanSummary *)dsum);
        if (ps.launch_wide)
            RHJ_LAUNCH((k_scatter_runs<false, false>), dim3(want, nrel), dim3(PT_BLOCK), scatter_runs_lds_bytes(hi), g.stream, b0, b1,
                       sh2, hi, search0, (const PlanSummary *)dsum);
    }
    ps.p2[0] = b0; ps.p2[1] = b1;
    HIP_TRY(hipGetLastError());
    return 0;
}

// exclusive scan of up to max_n u64 counts (device-side count in *n_ptr when given)
int launch_offsets(const uint64_t *cnt, uint64_t *base, const uint64_t *n_ptr, uint64_t n_fixed, uint64_t max_n,
                   uint64_t *total_out)
{
    const uint32_t nblocks = (uint32_t)((max_n + 1023) / 1024 ? (max_n + 1023) / 1024 : 1);
    if (ensure(g.bsum, (size_t)nblocks * 8)) return -1;
    RHJ_LAUNCH(k_offsets_local, dim3(nblocks), dim3(1024), 0, g.stream, cnt, base, n_ptr, n_fixed, (uint64_t *)g.bsum.p);
    RHJ_LAUNCH(k_offsets_blocks, dim3(1), dim3(1024), 0, g.stream, (uint64_t *)g.bsum.p, nblocks, total_out);
    RHJ_LAUNCH(k_offsets_add, dim3(nblocks), dim3(1024), 0, g.stream, base, n_ptr, n_fixed, (const uint64_t *)g.bsum.p);
    return 0;
}

float ev_ms(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0.f;
    return ms;
}
float stage_ms(int a, int b) { return stage_on(a) && stage_on(b) ? ev_ms(g.ev[a], g.ev[b]) : 0.f; }

// ---- one join ----------------------------------------------------------------------------------------------------------------

// A join as an entry point asks for it.  out == nullptr: the pairs are only counted, or with use_ctx_out they land in the
// context's own buffer (grown as needed) and come back through *ctx_out.
struct JoinReq {
    const rhj_tuple   *R;
    uint64_t           nR;
    const rhj_tuple   *S;
    uint64_t           nS;
    rhj_result_tuple  *out;
    uint64_t           out_capacity;
    bool               use_ctx_out;
    rhj_result_tuple **ctx_out;
    uint64_t          *matches;
    int                bits;                           // the radix (RHJ_ORDER=any: join_device picks it)
    uint32_t           range_lo = 0, range_span = 0;   // rhj_join_device_range: the buckets this call joins (span 0: all of them)
    uint64_t           slice_skip = 0, slice_end = 0;  // rhj_join_device_slice: the first bucket's probe tuples from slice_skip on, the last bucket's before slice_end (0: all)
    int                cols_input = 0;                 // R and S are key columns (rhj_join_keys_device): pass 1 of the two-pass partition reads 8 bytes a tuple
    bool               via_sel = false;                // R and S are not there yet (rhj_join_cols_device): tuple i is {col[sel ? sel[i] : i], i} of srcR / srcS, which the
    ColSrc             srcR = {}, srcS = {};           // small path reads itself; every other path materialises them first (materialise)

    bool count_only() const { return !use_ctx_out && out == nullptr; }
};

// every attempt at a join starts here: the stats of this attempt alone (the upload's time, taken before the call, stays)
static int begin_join(const JoinReq &q)
{
    if (ctx_init()) return -1;
    rhj_stats &st = g.stats;
    const float keep_h2d = st.ms_h2d;
    memset(&st, 0, sizeof(st));
    st.ms_h2d = keep_h2d;
    st.n_r = q.nR; st.n_s = q.nS; st.radix_bits = q.bits;
    g.last_spec = g.last_exact = 0;                    // (only the fused path tries them: a join on another path says "not tried")
    g.last_walk_units = -1;                            // (the small and fused paths, and a batch, leave the number)
    *q.matches = 0;
    if (q.ctx_out) *q.ctx_out = nullptr;
    return 0;
}

// the resident variant of the fused kernels: only when an average bucket could fit beside the index (~7.4 K tuples)
static bool resident(uint64_t nmin, uint32_t bins) { return nmin / bins <= 7000 && !g.no_resident; }

// fused kernels: workgroups are persistent (ticket loop) and the LDS request leaves room for one per CU
static unsigned fused_grid(uint64_t unit_bound) { return (unsigned)(unit_bound < (uint64_t)g.cus ? unit_bound : (uint64_t)g.cus); }

// The plan's workspace (grown here, the histograms last) and its and the join kernels' arguments: 2^bits buckets over partR /
// partS with histograms and offsets in hb ([2][bins] each, R's then S's), LDS-indexed build sides of up to lds_cap tuples, span
// probe tuples a unit, and on the split paths the side choice of the caller's bucket (parent_mask / parent_flip, else 0 / null).
static int plan_args(uint64_t nR, uint64_t nS, int bits, Buf &hb, uint32_t lds_cap, uint32_t span, uint32_t parent_mask,
                     const uint8_t *parent_flip, PlanArgs &pa, JoinArgs &ja)
{
    const uint32_t bins = 1u << bits;
    const uint64_t nmin = nR < nS ? nR : nS;
    const uint64_t max_units = (uint64_t)bins + (nR + nS) / PR_UNIT + 2;
    const uint64_t max_bunits = (uint64_t)bins + nmin / BUILD_CHUNK + 2;
    if (ensure(g.units, max_units * sizeof(Unit)) || ensure(g.bunits, max_bunits * sizeof(Unit)) || ensure(g.ldsb, (size_t)bins * 4) ||
        ensure(g.meta, (size_t)bins * sizeof(BucketMeta)) || ensure(g.summary, sizeof(PlanSummary) + 64) ||
        ensure(g.ucount, max_units * 8) || ensure(g.ubase, max_units * 8) || ensure(g.uflag, max_units * 4) ||
        ensure(hb, (size_t)4 * bins * 8))
        return -1;
    uint64_t *hist = (uint64_t *)hb.p, *psum = hist + 2 * bins;
    pa.histR = hist; pa.histS = hist + bins;
    pa.units = (Unit *)g.units.p; pa.build_units = (Unit *)g.bunits.p; pa.lds_buckets = (uint32_t *)g.ldsb.p;
    pa.meta = (BucketMeta *)g.meta.p; pa.summary = (PlanSummary *)g.summary.p;
    pa.lds_cap = lds_cap; pa.lds_max_slots = LDS_MAX_SLOTS; pa.build_chunk = BUILD_CHUNK; pa.span_lds = span;
    pa.parent_mask = parent_mask; pa.parent_flip = parent_flip; pa.zero = nullptr; pa.zero_words = 0;
    ja.partR = (const rhj_tuple *)g.partR.p; ja.partS = (const rhj_tuple *)g.partS.p;
    ja.histR = hist; ja.histS = hist + bins; ja.psumR = psum; ja.psumS = psum + bins;
    ja.units = (const Unit *)g.units.p; ja.meta = (const BucketMeta *)g.meta.p; ja.summary = (const PlanSummary *)g.summary.p;
    ja.tab32 = nullptr; ja.tab64 = nullptr;
    ja.unit_count = (uint64_t *)g.ucount.p; ja.unit_base = (const uint64_t *)g.ubase.p; ja.unit_flag = (uint32_t *)g.uflag.p;
    ja.out = nullptr; ja.out_capacity = 0;
    ja.parent_mask = parent_mask; ja.parent_flip = parent_flip;
    ja.stash_cnt = nullptr; ja.stash_row = nullptr; ja.stash_nR = nR;
    return 0;
}

// The fused kernels' workspace (grown in this order: stash, status_bytes of ticket and status words, overflow lists, walk list)
// and their arguments but fa.j.  lr_mode: the split paths' form; host_summary: the small path's pinned summary (else null).
static int fused_args(uint64_t nR, uint64_t nS, int bits, uint64_t unit_bound, uint64_t status_bytes, uint32_t lr_mode,
                      uint64_t *host_summary, FusedArgs &fa)
{
    if (ensure(g.stash_cnt, nR + nS + 64) || ensure(g.stash_row, (nR + nS + 8) * 8) || ensure(g.status, status_bytes) ||
        ensure(g.ovf, fj_ovf_bytes((size_t)g.cus)) || ensure(g.ovf_base, (size_t)g.cus * 2 * FJ_GROUPS * 16 * 4) ||
        ensure(g.walk, (unit_bound + 1) * sizeof(FjWalkItem)))
        return -1;
    fa.stash_cnt = (uint8_t *)g.stash_cnt.p; fa.stash_row = (uint64_t *)g.stash_row.p;
    fa.status = (uint64_t *)g.status.p + 8;               // words 0..7 hold the ticket
    fa.ticket = (uint32_t *)g.status.p;
    fa.nR = nR;
    fa.allow_resident = lr_mode ? 0 : !g.no_resident; fa.radix_bits = (uint32_t)bits; fa.lr_mode = lr_mode; fa.spec = 0; fa.xrows = nullptr;
    fa.unit_bound = unit_bound; fa.host_summary = host_summary; fa.dbg = nullptr;
    fa.ovf = (uint64_t *)g.ovf.p; fa.ovf_base = (uint32_t *)g.ovf_base.p; fa.walk = (FjWalkItem *)g.walk.p;
    return 0;
}

// The pairs' buffer of the small and fused paths, whose join kernel counts them itself: the caller's, or with use_ctx_out the
// context's own, of at least max(nR, nS) + 1024 pairs before the kernel ...
static int out_guess(const JoinReq &q, rhj_result_tuple *&out, uint64_t &cap)
{
    out = q.out; cap = q.out_capacity;
    if (!q.use_ctx_out) return 0;
    if (ensure(g.out, ((q.nR > q.nS ? q.nR : q.nS) + 1024) * sizeof(rhj_result_tuple))) return -1;
    out = (rhj_result_tuple *)g.out.p;
    cap = g.out.cap / sizeof(rhj_result_tuple);
    return 0;
}

// ... and grown to the kernel's M when that was short: 1 = launch the kernel again, 0 = the pairs are in place, -1 = error
static int out_grow(const JoinReq &q, uint64_t M, rhj_result_tuple *&out, uint64_t &cap)
{
    if (!q.use_ctx_out || M <= cap) return 0;
    if (ensure(g.out, M * sizeof(rhj_result_tuple))) return -1;    // rare: fan-out above the guess
    out = (rhj_result_tuple *)g.out.p;
    cap = M;
    return 1;
}

// The pairs' buffer of the paths that learn M before they write: the context's own, grown to M pairs (use_ctx_out), or the
// caller's, rc 1 when M passes its capacity (the first out_capacity pairs are written).
static int out_exact(const JoinReq &q, uint64_t M, rhj_result_tuple *&out, uint64_t &cap, int &rc)
{
    out = q.out; cap = q.out_capacity; rc = 0;
    if (q.use_ctx_out) {
        if (ensure(g.out, (M ? M : 1) * sizeof(rhj_result_tuple))) return -1;
        out = (rhj_result_tuple *)g.out.p;
        cap = M;
        if (q.ctx_out) *q.ctx_out = out;
    } else if (M > cap) {
        rc = 1;
    }
    return 0;
}

// the end of a small (path 3) or fused (path 1) join: stats, *matches, *ctx_out; rc 1 when the caller's buffer was short
static int fused_epilogue(const JoinReq &q, const PlanSummary &plan, uint64_t M, rhj_result_tuple *out, uint64_t cap, int path)
{
    rhj_stats &st = g.stats;
    st.units = plan.units; st.hbm_units = 0; st.max_build = plan.max_build;
    st.reserved = path;                                // path id (stats()["path"])
    *q.matches = M;
    st.matches = M;
    if (q.ctx_out) *q.ctx_out = out;
    if (path == 3) {
        st.ms_hist = stage_ms(ST_HIST, ST_SCATTER);
        st.ms_scan = 0.f;                              // no scan launch: every scatter workgroup sums the columns it needs
        st.ms_scatter = stage_ms(ST_SCATTER, ST_PROBE);
    } else {
        st.ms_hist = stage_ms(ST_HIST, ST_SCAN);
        st.ms_scan = stage_ms(ST_SCAN, ST_SCATTER);
        st.ms_scatter = stage_ms(ST_SCATTER, ST_PLAN);
        st.ms_plan = stage_ms(ST_PLAN, ST_PROBE);
    }
    st.ms_probe = stage_ms(ST_PROBE, ST_END);
    st.ms_total = stage_ms(ST_HIST, ST_END);
    return (!q.use_ctx_out && out && M > cap) ? 1 : 0;
}

// The relations of a join given by columns and row-id vectors, built in inR / inS as GetRelation builds them
// (rhj_build_relation_device): from here on the join is one on rhj_tuple arrays.
static int materialise(JoinReq &q)
{
    if (!q.via_sel) return 0;
    if (ctx_init() || ensure(g.inR, (q.nR ? q.nR : 1) * sizeof(rhj_tuple)) || ensure(g.inS, (q.nS ? q.nS : 1) * sizeof(rhj_tuple))) return -1;
    if (rhj_build_relation_device(q.srcR.col, q.srcR.sel, q.nR, (rhj_tuple *)g.inR.p) ||
        rhj_build_relation_device(q.srcS.col, q.srcS.sel, q.nS, (rhj_tuple *)g.inS.p))
        return -1;
    q.R = (const rhj_tuple *)g.inR.p; q.S = (const rhj_tuple *)g.inS.p;
    q.via_sel = false;
    return 0;
}

// What the small, fused and tiled paths of one join share (join_setup): decisions on its sizes, partition state, kernel arguments
struct JoinSetup {
    int       bits;
    uint32_t  bins;
    uint64_t  nmin;
    bool      small;           // the small path takes the join
    bool      want_fused;      // the fused path runs behind the partition (else the tiled path)
    bool      wide;            // the partition keeps 16-byte tuples (forced, or for the tiled path, which reads rhj_tuple)
    uint64_t  unit_bound;      // fused path: the host-side bound on the unit count
    uint64_t  status_bytes;    // fused path: its ticket and status words
    PartState ps;
    PlanArgs  pa;
    JoinArgs  ja;
};

// What the small and fused paths return besides 0 / 1 (done; 1: the caller's buffer was short) and -1: RUN_WIDE, wide row ids
// met the 12-byte kernels (the join runs again wide), or the tiled path's handover — the plan in place, or a plan of fused-sized
// units after the small path (which recorded no partition stages) or the fused path, to be made again with tile-granular ones.
enum { RUN_WIDE = 3, TILED_PLANNED, TILED_AFTER_SMALL, TILED_AFTER_FUSED };

static uint32_t sm_tiles(uint64_t n) { return (uint32_t)((n + SM_TILE - 1) / SM_TILE); }

// probe tuples per fused unit: whole buckets when there are plenty of them, smaller spans (each unit
// rebuilds its bucket's index) when a low radix would otherwise leave most CUs idle
static uint32_t fused_span_for(uint32_t bins, uint64_t nR, uint64_t nS)
{
    uint32_t fused_span = FJ_SPAN;
    if (bins < 256) {                                         // fewer buckets than CUs
        uint64_t want = ((nR > nS ? nR : nS) / 512 + FJ_BATCH - 1) / FJ_BATCH * FJ_BATCH;
        if (want < FJ_BATCH) want = FJ_BATCH;
        if (want < fused_span) fused_span = (uint32_t)want;
    }
    return fused_span;
}

static int join_setup(const JoinReq &q, bool force_wide, JoinSetup &s)
{
    const uint64_t nR = q.nR, nS = q.nS;
    const int bits = s.bits = q.bits;
    const uint32_t bins = s.bins = 1u << bits;
    PartState &ps = s.ps;
    if (ensure(g.partR, nR * sizeof(rhj_tuple)) || ensure(g.partS, nS * sizeof(rhj_tuple))) return -1;
    ps.r[0] = RelArgs{q.R, (rhj_tuple *)g.partR.p, nullptr, nR, 0, 0, nullptr, nullptr};
    ps.r[1] = RelArgs{q.S, (rhj_tuple *)g.partS.p, nullptr, nS, 0, 0, nullptr, nullptr};
    for (int i = 0; i < 2; ++i) { ps.r[i].range_lo = q.range_lo; ps.r[i].range_span = q.range_span; }   // a rank's share of a sharded join: the partition drops the other buckets
    ps.tmp[0] = ps.tmp[1] = nullptr;
    ps.cols_input = q.cols_input;
    if (bits > PT_MAX_BITS) {
        if (ensure(g.tmpR, nR * sizeof(rhj_tuple)) || ensure(g.tmpS, nS * sizeof(rhj_tuple))) return -1;
        ps.tmp[0] = (rhj_tuple *)g.tmpR.p; ps.tmp[1] = (rhj_tuple *)g.tmpS.p;
    }
    // Thousands of buckets of a few hundred tuples: a fused unit costs ~15 us whatever its size (a dozen barriers and
    // dependent round trips, one unit per CU at a time), the tiled path's 256-thread probe units run eight to a CU —
    // 1M x 1M at 15 bits 2.2 ms fused, 0.88 ms tiled; from ~512 tuples per bucket on the fused path is ahead again
    // (tools/exp_twopass_sizes.py).  rhj_set_fused(2) keeps the fused path regardless.
    const bool tiny_buckets = bins >= 4096 && (nR > nS ? nR : nS) < (uint64_t)512 * bins;
    s.want_fused = !g.no_fused && !g.force_hbm && (g.force_fused || !tiny_buckets);
    // the fused path reads 12-byte partitioned tuples when the row ids fit 32 bits; the tiled path reads rhj_tuple
    s.wide = force_wide || !s.want_fused;
    s.nmin = nR < nS ? nR : nS;
    const uint32_t fused_span = fused_span_for(bins, nR, nS);
    const uint32_t lds_cap = s.want_fused ? FUSED_LDS_CAP : g.force_hbm ? 0 : LDS_MAX_SLOTS * 4 / 5;     // tiled: load factor <= 0.8
    if (plan_args(nR, nS, bits, g.histpsum, lds_cap, s.want_fused ? fused_span : PR_UNIT, 0, nullptr, s.pa, s.ja)) return -1;
    // the plan runs behind the partition (a small one-pass partition runs it in its scan launch)
    ps.hist = (uint64_t *)g.histpsum.p;
    ps.psum = ps.hist + 2 * bins;
    ps.plan = &s.pa;
    if (q.slice_skip) { s.pa.slice_b0 = q.range_lo; s.pa.slice_o0 = q.slice_skip; }      // (a slice is always a share: join_range)
    if (q.slice_end) { s.pa.slice_b1 = q.range_lo + q.range_span - 1u; s.pa.slice_o1 = q.slice_end; }
    s.unit_bound = (uint64_t)bins + (nR + nS) / fused_span + 2;
    s.status_bytes = (s.unit_bound + 1) * 8 + 64;
    s.small = s.want_fused && bits <= PT_MAX_BITS && !g.no_small && !q.range_span && sm_tiles(nR) <= g.small_tiles &&
              sm_tiles(nS) <= g.small_tiles && !g.stamps;
    return 0;
}

// ---- small joins (rhj_small.hip.h): two launches for the partition — the plan rides in the second — and the fused join
// third; no host memset, no total kernel, no read-back copy.
static int join_small(const JoinReq &q, JoinSetup &s)
{
    const int bits = s.bits;
    const uint64_t status_words = s.unit_bound + 1 + 8;                 // 8 ticket words in front
    RelArgs a0 = s.ps.r[0], a1 = s.ps.r[1];
    a0.tiles = sm_tiles(q.nR); a1.tiles = sm_tiles(q.nS);
    FusedArgs fa;
    if (ensure(g.cntR, (size_t)a0.tiles * 256 * 4) || ensure(g.cntS, (size_t)a1.tiles * 256 * 4) ||
        fused_args(q.nR, q.nS, bits, s.unit_bound, status_words * 8 + 64, 0, (uint64_t *)&g.pin->summary, fa))
        return -1;
    a0.cnt = (uint32_t *)g.cntR.p; a1.cnt = (uint32_t *)g.cntS.p;
    rhj_result_tuple *out;
    uint64_t cap;
    if (out_guess(q, out, cap)) return -1;
    const uint32_t max_tiles = a0.tiles > a1.tiles ? a0.tiles : a1.tiles;
    const unsigned fgrid = fused_grid(s.unit_bound);
    // relations of one or two tiles: the scatter workgroups count the digits themselves, two launches in all
    const int self_hist = max_tiles <= SM_SELF_TILES;
    PlanSummary plan;
    uint64_t M = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        s.ja.out = out; s.ja.out_capacity = out ? cap : 0;
        fa.j = s.ja;
        RHJ_STAGE(ST_HIST);
        if (!self_hist) {
            if (q.via_sel)
                RHJ_LAUNCH(k_small_hist_cols, dim3(max_tiles, 2), dim3(SM_BLOCK), 0, g.stream, a0, a1, q.srcR, q.srcS, bits,
                           (uint64_t *)g.status.p, status_words);
            else
                RHJ_LAUNCH(k_small_hist, dim3(max_tiles, 2), dim3(SM_BLOCK), 0, g.stream, a0, a1, bits, (uint64_t *)g.status.p, status_words);
        }
        RHJ_STAGE(ST_SCATTER);
        if (q.via_sel)
            RHJ_LAUNCH(k_small_scatter_cols, dim3(max_tiles + 1, 2), dim3(SM_BLOCK), small_lds_bytes(bits), g.stream, a0, a1, q.srcR, q.srcS,
                       bits, s.ps.hist, s.ps.psum, s.pa, self_hist, (uint64_t *)g.status.p, status_words);
        else
            RHJ_LAUNCH(k_small_scatter, dim3(max_tiles + 1, 2), dim3(SM_BLOCK), small_lds_bytes(bits), g.stream, a0, a1, bits, s.ps.hist,
                       s.ps.psum, s.pa, self_hist, (uint64_t *)g.status.p, status_words);
        RHJ_STAGE(ST_PROBE);
        if (resident(s.nmin, s.bins))
            RHJ_LAUNCH((k_join_fused<true, false>), dim3(fgrid), dim3(FJ_BLOCK), FUSED_LDS, g.stream, fa, FUSED_LDS);
        else
            RHJ_LAUNCH((k_join_fused<false, false>), dim3(fgrid), dim3(FJ_BLOCK), FUSED_LDS, g.stream, fa, FUSED_LDS);
        RHJ_STAGE(ST_END);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g.stream));
        plan = g.pin->summary;                         // written by the join kernel's last workgroup (system-scope stores)
        g.last_walk_units = plan.fused_ok && out ? (int64_t)g.pin->walk_units : -1;   // (what the launch below is decided by)
        if (plan.fused_ok && out && g.pin->walk_units != 0) {
            // some unit's pairs need the index walked again (a probe tuple with more than 16 matches, ...): the host is
            // waiting on this stream anyway, so the second kernel is launched only now — a launch that returns at once
            // costs a 0.08 ms join 5 % (the fused path, whose joins are milliseconds, always enqueues it)
            RHJ_LAUNCH(k_join_walk, dim3(fgrid), dim3(FJ_BLOCK), FUSED_LDS, g.stream, fa, FUSED_LDS);
            RHJ_STAGE(ST_END);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(g.stream));
        }
        if (plan.fused_ok && plan.matches == FJ_NO_TOTAL) { fprintf(stderr, "rhj: fused join left no match total (chained scan incomplete)\n"); return -1; }
        if (!plan.fused_ok) return TILED_AFTER_SMALL;  // partitioned and planned, but some bucket needs the tiled path
        M = plan.matches;
        const int again = out_grow(q, M, out, cap);
        if (again < 0) return -1;
        if (!again) break;
    }
    return fused_epilogue(q, plan, M, out, cap, 3);
}

// The partition of both relations and the plan behind it, which clears the fused path's ticket and status words on the way
// (a memset does when a small one-pass partition ran the plan in its scan launch).
static int partition_plan(JoinSetup &s)
{
    if (run_partition(s.ps, s.bits, 2, s.wide, s.want_fused && !s.wide)) return -1;
    RHJ_STAGE(ST_PLAN);
    PlanArgs pa = s.pa;
    if (s.want_fused) {
        if (ensure(g.status, s.status_bytes)) return -1;
        pa.zero = (uint32_t *)g.status.p; pa.zero_words = (uint32_t)(s.status_bytes / 4);
    }
    if (!s.ps.plan_done) RHJ_LAUNCH(k_plan, dim3(s.bits >= 11 ? 8 : 1), dim3(1024), 0, g.stream, pa, s.bits);
    else if (s.want_fused) HIP_TRY(hipMemsetAsync(g.status.p, 0, s.status_bytes, g.stream));
    return 0;
}

// ---- fused LDS path: build + probe + emit in one kernel, chained output offsets.  Launched without waiting for the plan:
// the grid is the host-side upper bound on the unit count, the LDS allocation the maximum, and the kernel itself returns when
// the plan found a bucket that does not fit LDS (then the tiled path takes over).  One host sync per join.
static int join_fused(const JoinReq &q, JoinSetup &s)
{
    const uint64_t nR = q.nR, nS = q.nS;
    const int bits = s.bits;
    FusedArgs fa;
    if (fused_args(nR, nS, bits, s.unit_bound, s.status_bytes, 0, nullptr, fa)) return -1;
    if (g.stamps) {                                       // diagnostic runs only
        if (ensure(g.dbg, (s.unit_bound + 1) * 64)) return -1;
        fa.dbg = (uint64_t *)g.dbg.p;
    }
    rhj_result_tuple *out;
    uint64_t cap;
    if (out_guess(q, out, cap)) return -1;
    RHJ_STAGE(ST_PROBE);                          // (no separate build / count / offsets stages on this path)
    const unsigned fgrid = fused_grid(s.unit_bound);
    const bool res = resident(s.nmin, s.bins);
    // The stash width follows the partition's row-id decision (summary->wide_row_ids, known only on the device):
    // the instantiation that does not match returns at once, and the 16-byte one is launched only when the
    // partition's 16-byte kernels were (one-pass partitions, forced-wide runs, a process that has seen wide row ids).
    const bool maybe_narrow = bits > PT_MAX_BITS && !s.wide;
    const bool maybe_wide = !maybe_narrow || s.ps.launch_wide;
    PlanSummary plan;
    uint64_t M = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        s.ja.out = out; s.ja.out_capacity = out ? cap : 0;
        fa.j = s.ja;
        if (attempt) HIP_TRY(hipMemsetAsync(g.status.p, 0, s.status_bytes, g.stream));   // (first: cleared by the plan)
        // The foreign-key speculation (k_join_spec): the bigger relation's tuples have one match each?  Then nothing is
        // stashed for the units that relation probes and nothing is chained.  Tried while it keeps holding; a failed try
        // costs the time to the first unit that notices (tens of microseconds), so after failures only every 16th join tries.
        // (A buffer below the relation's size is no obstacle: pairs beyond it are dropped as on every path and the caller hears
        // the count.  A rank's share of a sharded join — rhj_join_device_range — has a buffer for its share and buckets of the
        // whole join's size: the per-bucket rule is the same.)
        // (Not on a slice: a bucket cut between two devices has units that start inside it, and the last workgroup's check
        // adds up to the whole relation.)
        bool try_spec = attempt == 0 && maybe_narrow && out != nullptr && g.no_spec <= 0 && !q.slice_skip && !q.slice_end &&
                        (nS >= nR ? nS : nR) / s.bins >= 4096;     // (units of 2.4 K tuples: 10M x 10M at 12 bits lost 7 % to its per-unit extras)
        if (try_spec && g.spec_score <= 0 && g.no_spec >= 0 && ++g.spec_skipped < 16) try_spec = false;   // (RHJ_NO_SPEC=-1: always try — to time a failing one)
        fa.spec = try_spec ? (nS >= nR ? 1u : 2u) : 0u;
        // k_join_exact (rhj_join_exact.hip.h) runs the speculation over an index that needs no verifying gather: build sides
        // the gather kernels would take (beyond the LDS-resident ones), enough radix bits for its slots to make the 40 stored
        // hash bits exact.  It hands over (ticket[4], reason in ticket[5]) what it does not take; a join it handed back for
        // its INPUT (row ids that do not increase, a bucket beyond its index) makes the next eligible joins skip it.
        bool try_exact = try_spec && g.no_exact <= 0 && !res && bits >= 10 && s.nmin / s.bins <= XJ_MAX_BUILD;
        if (try_exact && g.exact_score <= 0 && g.no_exact >= 0 && ++g.exact_skipped < 16) try_exact = false;
        if (try_exact) {
            if (ensure(g.xrows, (size_t)g.cus * XJ_SCRATCH * 4)) return -1;
            fa.xrows = (uint32_t *)g.xrows.p;
            g.exact_skipped = 0;
        }
        if (try_spec) {
            g.spec_skipped = 0;
            if (try_exact)
                RHJ_LAUNCH(k_join_exact, dim3(fgrid), dim3(FJ_BLOCK), FUSED_LDS, g.stream, fa, FUSED_LDS);
            else if (res)
                RHJ_LAUNCH((k_join_spec<true>), dim3(fgrid), dim3(FJ_BLOCK), FUSED_LDS, g.stream, fa, FUSED_LDS);
            else
                RHJ_LAUNCH((k_join_spec<false>), dim3(fgrid), dim3(FJ_BLOCK), FUSED_LDS, g.stream, fa, FUSED_LDS);
        }
        if (res) {
            if (maybe_narrow)
                RHJ_LAUNCH((k_join_fused<true, true>), dim3(fgrid), dim3(FJ_BLOCK), FUSED_LDS, g.stream, fa, FUSED_LDS);
            if (maybe_wide)
                RHJ_LAUNCH((k_join_fused<true, false>), dim3(fgrid), dim3(FJ_BLOCK), FUSED_LDS, g.stream, fa, FUSED_LDS);
        } else {
            if (maybe_narrow)
                RHJ_LAUNCH((k_join_fused<false, true>), dim3(fgrid), dim3(FJ_BLOCK), FUSED_LDS, g.stream, fa, FUSED_LDS);
            if (maybe_wide)
                RHJ_LAUNCH((k_join_fused<false, false>), dim3(fgrid), dim3(FJ_BLOCK), FUSED_LDS, g.stream, fa, FUSED_LDS);
        }
        RHJ_LAUNCH(k_join_walk, dim3(fgrid), dim3(FJ_BLOCK), FUSED_LDS, g.stream, fa, FUSED_LDS);   // returns at once when no unit needs it
        RHJ_STAGE(ST_END);
        HIP_TRY(hipMemcpyAsync(&g.pin->summary, g.summary.p, sizeof(PlanSummary), hipMemcpyDeviceToHost, g.stream));
        const bool fetch_ticket = try_spec || g.walk_count;   // (rhj_set_walk_count(1): word 2, the walk list's length, for the tests)
        if (fetch_ticket) HIP_TRY(hipMemcpyAsync(g.pin->ticket, g.status.p, sizeof(g.pin->ticket), hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g.stream));
        plan = g.pin->summary;
        g.last_walk_units = fetch_ticket && plan.fused_ok && out ? (int64_t)g.pin->ticket[2] : -1;
        g.last_spec = 0;
        g.last_exact = 0;
        if (try_spec) {
            const bool held = g.pin->ticket[4] == 0;                          // word 4: the speculation failed
            const bool not_taken = try_exact && !held && g.pin->ticket[5] == 2;   // k_join_exact's input, not the hypothesis
            g.last_spec = held ? 1 : 2;
            if (try_exact) {
                g.last_exact = held ? 1 : 2;
                g.exact_score = not_taken ? g.exact_score - 2 : (g.exact_score < 4 ? g.exact_score + 1 : 4);
                if (g.exact_score < -2) g.exact_score = -2;
            }
            if (!not_taken) {
                g.spec_score = held ? (g.spec_score < 4 ? g.spec_score + 1 : 4) : g.spec_score - 2;
                if (g.spec_score < -2) g.spec_score = -2;
            }
        }
        if (plan.row_id_overflow) return RUN_WIDE;     // (also: wide row ids met the 12-byte kernels alone)
        if (plan.fused_ok && plan.matches == FJ_NO_TOTAL) { fprintf(stderr, "rhj: fused join left no match total (chained scan incomplete)\n"); return -1; }
        // a bucket needs the tiled path, which reads 16-byte tuples: partition again wide if this one was narrow
        if (!plan.fused_ok) return bits > PT_MAX_BITS && !s.wide && !plan.wide_row_ids ? RUN_WIDE : TILED_AFTER_FUSED;
        M = plan.matches;
        const int again = out_grow(q, M, out, cap);
        if (again < 0) return -1;
        if (!again) break;
    }
    return fused_epilogue(q, plan, M, out, cap, 1);
}

// ---- tiled path: the tables (LDS- or HBM-built), a count pass, the output offsets, the emit pass.  `from`: how the plan
// stands (the outcomes above).
static int join_tiled(const JoinReq &q, JoinSetup &s, int from)
{
    if (from == TILED_AFTER_SMALL)
        for (int e = ST_HIST; e <= ST_PLAN; ++e) RHJ_STAGE(e);
    if (from != TILED_PLANNED) {
        s.pa.span_lds = PR_UNIT;                       // plan again with tile-granular units
        RHJ_LAUNCH(k_plan, dim3(1), dim3(1024), 0, g.stream, s.pa, s.bits);
    }
    rhj_stats &st = g.stats;
    PlanSummary *hs = &g.pin->summary;
    HIP_TRY(hipMemcpyAsync(hs, g.summary.p, sizeof(PlanSummary), hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));                  // launch geometry
    const PlanSummary plan = *hs;
    st.units = plan.units; st.hbm_units = plan.build_units; st.max_build = plan.max_build;
    st.table_slots = plan.hbm_slots + plan.tab32_slots;

    JoinArgs &ja = s.ja;
    const uint64_t max_tab32 = s.nmin + s.nmin / 2 + (uint64_t)80 * s.bins + 64;
    if (ensure(g.tab32, max_tab32 * 4) || ensure(g.stash_cnt, q.nR + q.nS + 64) || ensure(g.stash_row, (q.nR + q.nS + 8) * 8)) return -1;
    ja.tab32 = (uint32_t *)g.tab32.p;
    ja.stash_cnt = (uint8_t *)g.stash_cnt.p; ja.stash_row = (uint64_t *)g.stash_row.p;
    RHJ_STAGE(ST_BUILD);
    if (plan.hbm_slots) {
        if (ensure(g.tab64, plan.hbm_slots * 8)) return -1;
        ja.tab64 = (uint64_t *)g.tab64.p;
        HIP_TRY(hipMemsetAsync(g.tab64.p, 0, plan.hbm_slots * 8, g.stream));
        RHJ_LAUNCH(k_build_hbm, dim3((unsigned)plan.build_units), dim3(256), 0, g.stream, ja, (const Unit *)g.bunits.p);
    }
    if (plan.lds_buckets)
        RHJ_LAUNCH(k_build_lds, dim3((unsigned)plan.lds_buckets), dim3(BL_BLOCK), (size_t)plan.max_lds_slots * 4,
                   g.stream, ja, (const uint32_t *)g.ldsb.p);

    const unsigned probe_grid = (unsigned)((plan.units + 7) / 8 * 8);
    RHJ_STAGE(ST_COUNT);
    if (plan.units)
        RHJ_LAUNCH((k_probe<false>), dim3(probe_grid), dim3(PR_BLOCK), 0, g.stream, ja);
    RHJ_STAGE(ST_OFFSETS);
    if (launch_offsets((const uint64_t *)g.ucount.p, (uint64_t *)g.ubase.p, (const uint64_t *)&((PlanSummary *)g.summary.p)->units, 0,
                       plan.units, &((PlanSummary *)g.summary.p)->matches))
        return -1;
    HIP_TRY(hipMemcpyAsync(hs, g.summary.p, sizeof(PlanSummary), hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));                  // sync #2: match count -> output size
    if (hs->row_id_overflow) return RUN_WIDE;
    const uint64_t M = hs->matches;
    *q.matches = M;
    st.matches = M;

    rhj_result_tuple *out;
    uint64_t cap;
    int rc;
    if (out_exact(q, M, out, cap, rc)) return -1;
    RHJ_STAGE(ST_PROBE);
    if (plan.units && M && out && cap) {
        ja.out = out; ja.out_capacity = cap;
        RHJ_LAUNCH((k_probe<true>), dim3(probe_grid), dim3(PR_BLOCK), 0, g.stream, ja);
    }
    RHJ_STAGE(ST_END);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g.stream));
    st.ms_hist = stage_ms(ST_HIST, ST_SCAN);
    st.ms_scan = stage_ms(ST_SCAN, ST_SCATTER);
    st.ms_scatter = stage_ms(ST_SCATTER, ST_PLAN);
    st.ms_plan = stage_ms(ST_PLAN, ST_BUILD);
    st.ms_build = stage_ms(ST_BUILD, ST_COUNT);
    st.ms_count = stage_ms(ST_COUNT, ST_OFFSETS);
    st.ms_offsets = stage_ms(ST_OFFSETS, ST_PROBE);
    st.ms_probe = stage_ms(ST_PROBE, ST_END);
    st.ms_total = stage_ms(ST_HIST, ST_END);
    return rc;
}

// ---- the low-radix and sub-bucket paths (rhj_lowradix.hip.h, rhj_subbucket.hip.h) -------------------------------------
// A canonical join on r <= 13 radix bits whose buckets' build sides are beyond the LDS index runs on r + k bits and is
// emitted in the order of r bits.  Both return 2 when the path does not apply or gave up (the caller takes the tiled path).
static int lowradix_sub_bits(int r, uint64_t nR, uint64_t nS)
{
    const uint64_t nmin = nR < nS ? nR : nS;
    if (r + 1 >= MAX_BITS || (nmin >> r) <= 33000) return 0;            // the fused path takes such buckets as they are (its LDS index holds 36 K build tuples)
    const int kmax = r <= PT_MAX_BITS ? PT_MAX_BITS : MAX_BITS - 1 - r;   // the sub-bucket path stays below the widest radix
    int k = 1;
    while (k < kmax && r + k < MAX_BITS && (nmin >> (r + k)) > 20000) ++k;
    if ((nmin >> (r + k)) > 30000) return 0;                              // even the widest split leaves the build sides too big
    return k;
}

// The split width k a join takes (0: none): few radix bits over big inputs, canonical order wanted — run on finer buckets,
// emit in the caller's order.  Also for a rank's share of a sharded join (the partition's first pass, on the caller's bits,
// drops the other buckets), but not for a share cut inside a bucket: that is a matter of the plan's units, and these are
// sub-buckets.
static int split_bits(const JoinReq &q)
{
    if (g.no_lowradix || g.no_fused || g.force_hbm || g.wide_row_ids || q.slice_skip || q.slice_end || q.nR >= (1ull << 32) ||
        q.nS >= (1ull << 32))
        return 0;
    return lowradix_sub_bits(q.bits, q.nR, q.nS);
}

// The part both paths share: the caller's r-bit buckets split into 2^kb sub-buckets each, hist / psum of the r + kb-bit layout
// in hb (sub-bucket s of bucket b at (s << r) | b) and the partitioned relations in partR / partS.  Chooses every caller's bucket's
// probe side (k_lr_parent), plans and runs the fused kernel in its low-radix form: the pairs go to lr_tmp, every probe tuple's
// count and stash row to stash_cnt / stash_row.  Returns 2 for what these paths refuse — wide row ids, a build side beyond the
// LDS index, a unit that needed the index walk (its tuples' pairs are not where their stash rows say), a pass-2 tile of
// several batches (words[0]), 2^32 pairs or more — and otherwise fills ja (out = lr_tmp), *M and the path's (4 / 5) stats.
static int lr_internal_join(const JoinReq &q, int kb, Buf &hb, uint32_t *words, int path, JoinArgs &ja, uint64_t *M_out)
{
    rhj_stats &st = g.stats;
    const uint64_t nR = q.nR, nS = q.nS;
    const int r = q.bits, T = r + kb;
    const uint32_t bins = 1u << T;
    const bool count_only = q.count_only();
    uint8_t *parent_flip = (uint8_t *)(words + 16);            // [2 << r]
    RHJ_LAUNCH(k_lr_parent, dim3(1u << r), dim3(256), 0, g.stream, (const uint64_t *)hb.p, (const uint64_t *)hb.p + bins, r, kb, parent_flip);

    const uint64_t unit_bound = (uint64_t)bins + (nR + nS) / FJ_SPAN + 2;
    const uint64_t status_bytes = (unit_bound + 1) * 8 + 64;
    PlanArgs pa;
    FusedArgs fa;
    if (plan_args(nR, nS, T, hb, FUSED_LDS_CAP, FJ_SPAN, (1u << r) - 1u, parent_flip, pa, ja) ||
        fused_args(nR, nS, T, unit_bound, status_bytes, 1, nullptr, fa))
        return -1;
    RHJ_LAUNCH(k_plan, dim3(T >= 11 ? 8 : 1), dim3(1024), 0, g.stream, pa, T);

    const unsigned fgrid = fused_grid(unit_bound);
    const Pinned &hp = *g.pin;
    uint64_t M = 0;
    RHJ_STAGE(ST_PROBE);
    for (int attempt = 0; attempt < 2; ++attempt) {
        // the internal join's pairs: a scratch list of their own (the emit pass reads it while it writes the caller's)
        if (!count_only) {
            const uint64_t guess = attempt ? M : (nR > nS ? nR : nS) + 1024;
            if (ensure(g.lr_tmp, guess * sizeof(rhj_result_tuple))) return -1;
        }
        ja.out = count_only ? nullptr : (rhj_result_tuple *)g.lr_tmp.p;
        ja.out_capacity = count_only ? 0 : g.lr_tmp.cap / sizeof(rhj_result_tuple);
        fa.j = ja;
        HIP_TRY(hipMemsetAsync(g.status.p, 0, status_bytes, g.stream));
        HIP_TRY(hipMemsetAsync(g.stash_cnt.p, 0, nR + nS, g.stream));      // probe tuples of sub-buckets without a build side match nothing
        RHJ_LAUNCH((k_join_fused<false, true>), dim3(fgrid), dim3(FJ_BLOCK), FUSED_LDS, g.stream, fa, FUSED_LDS);
        RHJ_LAUNCH(k_join_walk, dim3(fgrid), dim3(FJ_BLOCK), FUSED_LDS, g.stream, fa, FUSED_LDS);
        HIP_TRY(hipMemcpyAsync(&g.pin->summary, g.summary.p, sizeof(PlanSummary), hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipMemcpyAsync(g.pin->ticket, g.status.p, 16, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipMemcpyAsync(g.pin->lr_words, words, 16, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g.stream));
        const PlanSummary &p = hp.summary;
        if (p.wide_row_ids || p.row_id_overflow || !p.fused_ok || hp.ticket[2] != 0 || hp.lr_words[0] != 0 ||
            p.matches == FJ_NO_TOTAL || p.matches >= (1ull << 32)) {
            static const bool trace = getenv("RHJ_TRACE") != nullptr;
            if (trace) fprintf(stderr, "rhj-trace:   %s path gives up: wide ids %u/%u, fused_ok %llu, walk units %u, big tile %u, matches %llu\n",
                               path == 4 ? "low-radix" : "sub-bucket", p.wide_row_ids, p.row_id_overflow, (unsigned long long)p.fused_ok,
                               hp.ticket[2], hp.lr_words[0],
                               (unsigned long long)p.matches);
            return 2;
        }
        M = p.matches;
        if (count_only || M * sizeof(rhj_result_tuple) <= g.lr_tmp.cap) break;
    }
    st.units = hp.summary.units; st.hbm_units = 0; st.max_build = hp.summary.max_build;
    st.reserved = path;                                        // path id: 4 low-radix, 5 sub-bucket
    *q.matches = M;
    st.matches = M;
    *M_out = M;
    return 0;
}

static int join_lowradix(const JoinReq &q, int kb)
{
    rhj_stats &st = g.stats;
    const uint64_t nR = q.nR, nS = q.nS;
    const int r = q.bits, T = r + kb;
    PartState ps;
    if (ensure(g.partR, nR * sizeof(rhj_tuple)) || ensure(g.partS, nS * sizeof(rhj_tuple)) ||
        ensure(g.tmpR, nR * sizeof(rhj_tuple)) || ensure(g.tmpS, nS * sizeof(rhj_tuple)) || ensure(g.lr_words, 64 + ((size_t)2 << r) + 4096))
        return -1;
    ps.r[0] = RelArgs{q.R, (rhj_tuple *)g.partR.p, nullptr, nR, 0, 0, nullptr, nullptr};
    ps.r[1] = RelArgs{q.S, (rhj_tuple *)g.partS.p, nullptr, nS, 0, 0, nullptr, nullptr};
    ps.tmp[0] = (rhj_tuple *)g.tmpR.p; ps.tmp[1] = (rhj_tuple *)g.tmpS.p;
    for (int i = 0; i < 2; ++i) { ps.r[i].range_lo = q.range_lo; ps.r[i].range_span = q.range_span; ps.r[i].range_bits = (uint32_t)r; }   // (a share: the CALLER's buckets)
    ps.lo_bits = r;                                            // pass 1 on exactly the caller's bits: pass 2 reads in canonical order
    uint32_t *words = (uint32_t *)g.lr_words.p;                // word 0: a pass-2 tile / chunk beyond one batch; word 1: k_lr_emit's ticket
    HIP_TRY(hipMemsetAsync(words, 0, 64, g.stream));
    if (run_partition(ps, T, 2, false, true)) return -1;
    RHJ_STAGE(ST_PLAN);
    JoinArgs ja;
    uint64_t M = 0;
    const int rj = lr_internal_join(q, kb, g.histpsum, words, 4, ja, &M);
    if (rj) return rj;
    int rc = 0;
    if (!q.count_only() && M) {
        rhj_result_tuple *out;
        uint64_t cap;
        if (out_exact(q, M, out, cap, rc)) return -1;
        LrArgs la;
        la.j = ja; la.j.out = out; la.j.out_capacity = cap;
        la.p2R = ps.p2[0]; la.p2S = ps.p2[1];
        la.stash_cnt = (const uint8_t *)g.stash_cnt.p; la.stash_row = (const uint2 *)g.stash_row.p;
        la.tmp = (const uint4 *)g.lr_tmp.p;
        la.nR = nR; la.r_bits = (uint32_t)r; la.k_bits = (uint32_t)kb;
        la.slots_per_bucket = ps.p2[0].groups > ps.p2[1].groups ? ps.p2[0].groups : ps.p2[1].groups;
        uint32_t search0 = 1;
        while (search0 * 2 <= ps.p2[0].group) search0 *= 2;
        la.search0 = search0;
        const uint32_t nslots = la.slots_per_bucket << r;
        if (ensure(g.lr_status, (size_t)nslots * 8 + 64)) return -1;
        la.ctotal = (uint64_t *)g.lr_status.p;
        la.bad = words;
        RHJ_LAUNCH(k_lr_totals, dim3(nslots), dim3(256), 0, g.stream, la);
        if (launch_offsets((const uint64_t *)g.lr_status.p, (uint64_t *)g.lr_status.p, nullptr, nslots, nslots,
                           (uint64_t *)(words + 4)))
            return -1;
        const unsigned egrid = (unsigned)(nslots < (uint32_t)g.cus * 8u ? nslots : (uint32_t)g.cus * 8u);
        RHJ_LAUNCH(k_lr_emit, dim3(egrid), dim3(LR_BLOCK), lr_lds_bytes(kb), g.stream, la, nslots);
        RHJ_STAGE(ST_END);
        HIP_TRY(hipMemcpyAsync(g.pin->lr_words, words, 16, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g.stream));
        if (g.pin->lr_words[0] != 0) return 2;
    } else {
        RHJ_STAGE(ST_END);
        HIP_TRY(hipStreamSynchronize(g.stream));
    }
    st.ms_hist = stage_ms(ST_HIST, ST_SCAN);
    st.ms_scan = stage_ms(ST_SCAN, ST_SCATTER);
    st.ms_scatter = stage_ms(ST_SCATTER, ST_PLAN);
    st.ms_plan = stage_ms(ST_PLAN, ST_PROBE);
    st.ms_probe = stage_ms(ST_PROBE, ST_END);
    st.ms_total = stage_ms(ST_HIST, ST_END);
    return rc;
}

// The sub-bucket path (rhj_subbucket.hip.h): r = 9..13.  The r-bit partition lands in tmpR / tmpS (pass 1's intermediate in
// partR / partS), pass B splits it into partR / partS on the next kb bits; the internal join is the low-radix path's.
// Stage times: ms_hist / ms_scan / ms_scatter the r-bit partition's, ms_build pass B, ms_plan parent choice + plan, ms_probe the
// internal join, ms_offsets the emit.
static int join_subbucket(const JoinReq &q, int kb)
{
    rhj_stats &st = g.stats;
    const uint64_t nR = q.nR, nS = q.nS;
    const int r = q.bits, T = r + kb;
    if (kb > SB_MAX_K || nR >= (1ull << 31) || nS >= (1ull << 31)) return 2;      // (the emit map keeps 31-bit positions)
    const uint32_t bins_r = 1u << r, binsT = 1u << T, digits = 1u << kb;
    PartState ps;
    if (ensure(g.partR, nR * sizeof(rhj_tuple)) || ensure(g.partS, nS * sizeof(rhj_tuple)) ||
        ensure(g.tmpR, nR * sizeof(rhj_tuple)) || ensure(g.tmpS, nS * sizeof(rhj_tuple)) || ensure(g.lr_words, 64 + ((size_t)2 << r) + 4096))
        return -1;
    ps.r[0] = RelArgs{q.R, (rhj_tuple *)g.tmpR.p, nullptr, nR, 0, 0, nullptr, nullptr};
    ps.r[1] = RelArgs{q.S, (rhj_tuple *)g.tmpS.p, nullptr, nS, 0, 0, nullptr, nullptr};
    ps.tmp[0] = (rhj_tuple *)g.partR.p; ps.tmp[1] = (rhj_tuple *)g.partS.p;
    for (int i = 0; i < 2; ++i) { ps.r[i].range_lo = q.range_lo; ps.r[i].range_span = q.range_span; ps.r[i].range_bits = (uint32_t)r; }
    uint32_t *words = (uint32_t *)g.lr_words.p;                // word 0: (nothing raises it on this path); words 4..5: the emit scan's total
    HIP_TRY(hipMemsetAsync(words, 0, 64, g.stream));
    if (run_partition(ps, r, 2, false, true)) return -1;
    RHJ_STAGE(ST_BUILD);

    // ---- pass B
    const uint32_t rowlen = (uint32_t)(((nR > nS ? nR : nS) + SB_CHUNK - 1) / SB_CHUNK) + bins_r + 1;
    const size_t ncnt = (size_t)2 * digits * rowlen;
    const size_t meta_bytes = (size_t)4 * binsT * 8 + (size_t)2 * (bins_r + 1) * 4 + (size_t)(bins_r + 1) * 8 + 64;
    if (ensure(g.sb_cnt, ncnt * 8) || ensure(g.sb_meta, meta_bytes) || ensure(g.sb_map, (nR + nS) * 4 + 64)) return -1;
    SbArgs sa;
    sa.in[0] = (const Tuple12 *)g.tmpR.p; sa.in[1] = (const Tuple12 *)g.tmpS.p;
    sa.out[0] = (Tuple12 *)g.partR.p; sa.out[1] = (Tuple12 *)g.partS.p;
    sa.histr = ps.hist; sa.psumr = ps.psum;
    uint64_t *histT = (uint64_t *)g.sb_meta.p, *psumT = histT + 2 * (size_t)binsT;
    sa.histT = histT; sa.psumT = psumT;
    sa.ebase = psumT + 2 * (size_t)binsT;
    sa.cbase = (uint32_t *)(sa.ebase + bins_r + 1);
    sa.ccnt = (uint64_t *)g.sb_cnt.p;
    sa.emap = (uint32_t *)g.sb_map.p;
    sa.summary = (const PlanSummary *)g.summary.p;
    sa.r_bits = (uint32_t)r; sa.k_bits = (uint32_t)kb; sa.rowlen = rowlen;
    RHJ_LAUNCH(k_sb_meta, dim3(1), dim3(1024), 0, g.stream, sa);
    RHJ_LAUNCH(k_sb_count, dim3(rowlen, 2), dim3(SB_BLOCK), 0, g.stream, sa);
    if (launch_offsets(sa.ccnt, sa.ccnt, nullptr, ncnt, ncnt, (uint64_t *)(words + 4))) return -1;
    RHJ_LAUNCH(k_sb_hist, dim3((binsT + 255) / 256, 2), dim3(256), 0, g.stream, sa);
    RHJ_LAUNCH(k_scan_psum, dim3(2), dim3(1024), 0, g.stream, T, (const uint64_t *)histT, psumT);
    RHJ_LAUNCH(k_sb_scatter, dim3(rowlen, 2), dim3(SB_BLOCK), 0, g.stream, sa);
    // the emit sequence's length, read back with the join's summary
    HIP_TRY(hipMemcpyAsync(&g.pin->emit_len, sa.ebase + bins_r, 8, hipMemcpyDeviceToHost, g.stream));
    RHJ_STAGE(ST_PLAN);

    JoinArgs ja;
    uint64_t M = 0;
    const int rj = lr_internal_join(q, kb, g.sb_meta, words, 5, ja, &M);
    if (rj) return rj;
    int rc = 0;
    RHJ_STAGE(ST_OFFSETS);
    if (!q.count_only() && M) {
        rhj_result_tuple *out;
        uint64_t cap;
        if (out_exact(q, M, out, cap, rc)) return -1;
        const uint64_t E = g.pin->emit_len;
        const uint64_t nslots = (E + SB_CHUNK - 1) / SB_CHUNK;
        if (ensure(g.lr_status, (size_t)nslots * 8 + 64)) return -1;
        SbEmitArgs ea;
        ea.emap = sa.emap; ea.n = E;
        ea.stash_cnt = (const uint8_t *)g.stash_cnt.p; ea.stash_row = (const uint2 *)g.stash_row.p;
        ea.tmp = (const uint4 *)g.lr_tmp.p; ea.nR = nR;
        ea.ctotal = (uint64_t *)g.lr_status.p;
        ea.out = (uint4 *)out; ea.out_capacity = cap;
        RHJ_LAUNCH(k_sb_totals, dim3((unsigned)nslots), dim3(SB_BLOCK), 0, g.stream, ea);
        if (launch_offsets(ea.ctotal, ea.ctotal, nullptr, nslots, nslots, (uint64_t *)(words + 4))) return -1;
        RHJ_LAUNCH(k_sb_emit, dim3((unsigned)nslots), dim3(SB_BLOCK), 0, g.stream, ea);
    }
    RHJ_STAGE(ST_END);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g.stream));
    static const bool trace = getenv("RHJ_TRACE") != nullptr;
    if (trace) fprintf(stderr, "rhj-trace:   sub-bucket path: %d + %d bits, %llu pairs, emit sequence %llu\n", r, kb,
                       (unsigned long long)M, (unsigned long long)g.pin->emit_len);
    st.ms_hist = stage_ms(ST_HIST, ST_SCAN);
    st.ms_scan = stage_ms(ST_SCAN, ST_SCATTER);
    st.ms_scatter = stage_ms(ST_SCATTER, ST_BUILD);
    st.ms_build = stage_ms(ST_BUILD, ST_PLAN);
    st.ms_plan = stage_ms(ST_PLAN, ST_PROBE);
    st.ms_probe = stage_ms(ST_PROBE, ST_OFFSETS);
    st.ms_offsets = stage_ms(ST_OFFSETS, ST_END);
    st.ms_total = stage_ms(ST_HIST, ST_END);
    return rc;
}

static int auto_radix_bits(uint64_t nR, uint64_t nS)
{
    const uint64_t nmin = nR < nS ? nR : nS, nmax = nR < nS ? nS : nR;
    const uint64_t target = nmax >= 4 * nmin ? 6500 : 16000;
    int b = 0;
    while (b < MAX_BITS && (nmin >> b) > target) ++b;
    while (b < PT_MAX_BITS && (nmin >> (b + 1)) >= 512) ++b;
    // 13 bits only where 12 would leave buckets beyond the gather kernels' LDS index: up to 12 bits pass 1 counts pass 2's digits
    // itself, and since the speculative kernel writes every unit's pairs from phase 1 (round 4) 100M x 100M is faster on 12 bits
    // (24.4 K a bucket: 4.13 ms) than on 13 (4.27) or 14 (4.54); tools/exp_auto_bits.py: 10M / 30M / 50M best on 10 / 11 / 12
    if (b == 13 && nmax < 4 * nmin && (nmin >> 12) <= 28000) b = 12;
    return b < 1 ? 1 : b;
}

// The device-side join.  A split path goes first where it applies (r <= 8 the low-radix path, 9..13 the sub-bucket path) and
// hands back 2 when it refuses.  Then the small path, or the partition and plan followed by the fused path; the tiled path
// where either hands over, and behind the plan when the fused path is not wanted.  A narrow partition that met wide row ids
// makes the whole join run again wide.  Relations still given by columns and row-id vectors (q.via_sel) are read as they
// are by the small path alone: every other route materialises them first.
static int join_device(JoinReq q)
{
    if (g.order_any && q.nR && q.nS) q.bits = auto_radix_bits(q.nR, q.nS);    // RHJ_ORDER=any: the library picks the radix
    if (const int kb = split_bits(q)) {
        if (materialise(q) || begin_join(q)) return -1;
        const int rc = q.bits <= PT_MAX_BITS ? join_lowradix(q, kb) : join_subbucket(q, kb);
        if (rc != 2) return rc;
    }
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (begin_join(q)) return -1;
        if (q.nR == 0 || q.nS == 0) return 0;                         // rhjoin.c:15-16
        if (q.nR >= (1ull << 32) || q.nS >= (1ull << 32)) {
            fprintf(stderr, "rhj: relations of 2^32 tuples or more are not supported (offsets are 32-bit; the reference "
                            "itself is limited to 2^31-1, SURVEY.md finding 9)\n");
            return -2;
        }
        JoinSetup s;
        if (join_setup(q, attempt > 0 || g.wide_row_ids, s)) return -1;
        if (q.via_sel && !s.small) {                                  // only the small path reads columns through row-id vectors
            if (materialise(q)) return -1;
            s.ps.r[0].in = q.R; s.ps.r[1].in = q.S;
        }
        int rc = TILED_PLANNED;
        if (s.small) rc = join_small(q, s);
        else if (partition_plan(s)) return -1;
        else if (s.want_fused) rc = join_fused(q, s);
        if (rc >= TILED_PLANNED) rc = join_tiled(q, s, rc);
        if (rc != RUN_WIDE) return rc;
        g.seen_wide = 1;                                              // from now on the 16-byte kernels are launched as well
    }
    return 0;
}

// ---- batched small joins (rhj_batch.hip.h) -------------------------------------------------------------------------------
// rhj_join_batch_device: the joins batch_takes() names run as chunks of three launches and one stream synchronisation each;
// the others, and the taken ones whose plan found a bucket beyond the LDS index, go through join_device one by one.
//
// A chunk's joins live side by side in ONE arena (every join its partitioned relations, tile counts, histograms and offsets,
// units and their totals, summary, ticket and status words, stash, overflow regions for BJ_WGS workgroups and walk list:
// 2.7 MB + 25 bytes a tuple), which never exceeds BATCH_ARENA_BUDGET: a batch whose joins need more is cut into chunks that
// fit, in call order.
constexpr size_t BATCH_ARENA_BUDGET = (size_t)1 << 30;
constexpr uint64_t BATCH_MAX_JOINS = 65535;               // grid y / z of one chunk
constexpr size_t BATCH_SLOT_WORDS = 16;                   // u64 words of a join's slot in the pinned block: PlanSummary, walk count
static_assert(sizeof(PlanSummary) / 8 + 1 <= BATCH_SLOT_WORDS, "a join's pinned slot holds its summary and its walk count");

// what an item's `path` and rhj_stats::reserved say of the batched launches (include/rhj.h, include/rhj_inter.h)
enum { PATH_BATCH_JOIN = 6, PATH_BATCH_FILTER = 7, PATH_BATCH_APPLY = 8, PATH_BATCH_EQ2 = 9, PATH_QUERY_BATCH = 10, PATH_BATCH_STATS = 11, PATH_BATCH_JOIN_SUM = 12, PATH_BATCH_JOIN_FOLD = 13, PATH_BATCH_JOIN_FOLDK = 14, PATH_BATCH_FOLD_SELF = 15, PATH_BATCH_JOIN_FOLDN = 16, PATH_BATCH_FOLD_PRED = 17, PATH_BATCH_JOIN_FOLD_LDS = 18, PATH_BATCH_JOIN_FOLDK_LDS = 19 };

static int batch_takes(int bits, uint64_t nR, uint64_t nS)
{
    if (bits < 1 || bits > PT_MAX_BITS || nR == 0 || nS == 0) return 0;
    if (nR > (uint64_t)BJ_MAX_TILES * SM_TILE || nS > (uint64_t)BJ_MAX_TILES * SM_TILE) return 0;
    if (sm_tiles(nR) > g.small_tiles || sm_tiles(nS) > g.small_tiles) return 0;
    return !g.no_small && !g.no_fused && !g.force_hbm && !g.stamps;
}

struct BatchPlace {                                       // byte offsets of one join's buffers in the arena
    size_t partR, partS, cntR, cntS, hp, units, ucount, summary, status, stash_cnt, stash_row, ovf, ovf_base, walk, end;
    uint64_t unit_bound, status_words;
    uint32_t span;
};

static size_t batch_place(int bits, uint64_t nR, uint64_t nS, size_t at, BatchPlace &L)
{
    const uint32_t bins = 1u << bits;
    auto take = [&at](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    L.span = fused_span_for(bins, nR, nS);
    L.unit_bound = (uint64_t)bins + (nR + nS) / L.span + 2;
    L.status_words = L.unit_bound + 1 + 8;                // 8 ticket words in front
    L.partR = take(nR * sizeof(rhj_tuple));
    L.partS = take(nS * sizeof(rhj_tuple));
    L.cntR = take((size_t)sm_tiles(nR) * 256 * 4);
    L.cntS = take((size_t)sm_tiles(nS) * 256 * 4);
    L.hp = take((size_t)4 * bins * 8);
    L.units = take(L.unit_bound * sizeof(Unit));
    L.ucount = take(L.unit_bound * 8);                    // JoinArgs::unit_count: the fused kernel leaves every unit's total there
    L.summary = take(sizeof(PlanSummary) + 64);
    L.status = take(L.status_words * 8 + 64);
    L.stash_cnt = take(nR + nS + 64);
    L.stash_row = take((nR + nS + 8) * 8);
    L.ovf = take(fj_ovf_bytes(BJ_WGS));
    L.ovf_base = take((size_t)BJ_WGS * 2 * FJ_GROUPS * 16 * 4);
    L.walk = take((L.unit_bound + 1) * sizeof(FjWalkItem));
    return L.end = at;
}

// an arena grows to what a chunk needs, at least doubling, and never beyond its budget (ensure() adds slack of its own)
static int batch_arena(Buf &b, size_t bytes, size_t budget)
{
    if (bytes <= b.cap) return 0;
    size_t want = 2 * b.cap > bytes ? 2 * b.cap : bytes;
    if (want > budget) want = budget;
    if (want < bytes) want = bytes;                       // (one item alone never needs more than a few MB)
    if (b.p) HIP_TRY(hipFree(b.p));
    b.p = nullptr; b.cap = 0;
    HIP_TRY(hipMalloc(&b.p, want));
    b.cap = want;
    return 0;
}

// the pinned host block of a chunk (every batched entry point; every chunk ends in a stream synchronisation before the next
// one writes the block again)
static int batch_pinned(size_t bytes)
{
    if (bytes <= g.batch_pin_cap) return 0;
    if (g.batch_pin) HIP_TRY(hipHostFree(g.batch_pin));
    g.batch_pin = nullptr; g.batch_pin_cap = 0;
    HIP_TRY(hipHostMalloc(&g.batch_pin, 2 * bytes, hipHostMallocDefault));
    g.batch_pin_cap = 2 * bytes;
    return 0;
}

// a chunk's block (rhj_block.h): pieces(b) declares it, once for the sizes, then over the pinned side and g.batch_desc
template <class Pieces>
static int batch_block(Block &blk, Pieces pieces)
{
    Block sizes;
    pieces(sizes);
    if (batch_pinned(sizes.bytes()) || ensure(g.batch_desc, sizes.up_bytes())) return -1;
    blk = Block(g.batch_pin, g.batch_desc.p);
    pieces(blk);
    return 0;
}

// one copy: the uploaded pieces whose host side is [first, end)
static int batch_upload(const Block &blk, const void *first, const void *end)
{
    HIP_TRY(hipMemcpyAsync(blk.mirror(first), first, (size_t)((const char *)end - (const char *)first), hipMemcpyHostToDevice, g.stream));
    return 0;
}

// Cuts items [0, n) into chunks [lo, hi) in call order and runs them.  use(i, used) is what a chunk that uses `used` so far uses
// once item i has joined it (0: an empty chunk); a chunk takes its first item whatever that uses, then at most max_count - 1
// more, each only if the chunk stays within `limit` with it.  run(lo, hi, used) runs a chunk.
template <class Use, class Run>
static int batch_cut(size_t n, size_t max_count, uint64_t limit, Use use, Run run)
{
    for (size_t lo = 0, hi; lo < n; lo = hi) {
        uint64_t used = use(lo, 0);
        for (hi = lo + 1; hi < n && hi - lo < max_count; ++hi) {
            const uint64_t next = use(hi, used);
            if (next > limit) break;
            used = next;
        }
        if (run(lo, hi, used)) return -1;
    }
    return 0;
}

// The frame of every batched entry point.  batch_open: reset(q) clears item q's results and says whether q is valid; the whole
// batch is validated before anything is launched, an invalid item gets rc -3 and the call returns -3.  Then the context, and
// with timing on the event the call starts at.  batch_close: st becomes the call's rhj_last_stats(), with the time between the
// two events (what a batch runs alone records the stage events).
template <class D, class Reset>
static int batch_open(D *items, uint64_t n, Reset reset, bool &timed)
{
    if (!items) return -1;
    bool invalid = false;
    for (uint64_t i = 0; i < n; ++i)
        if (!reset(items[i])) { items[i].rc = -3; invalid = true; }
    if (invalid) return -3;
    if (ctx_init()) return -1;
    timed = g.timing >= 1;
    if (timed) HIP_TRY(hipEventRecord(g.ev_batch[0], g.stream));
    return 0;
}

static int batch_close(bool timed, const rhj_stats &st)
{
    g.stats = st;
    if (timed) {
        HIP_TRY(hipEventRecord(g.ev_batch[1], g.stream));
        HIP_TRY(hipEventSynchronize(g.ev_batch[1]));
        g.stats.ms_total = ev_ms(g.ev_batch[0], g.ev_batch[1]);
    }
    return 0;
}

struct BatchItem {
    uint64_t   idx;                                       // the join's place in the caller's array
    int        bits;
    BatchPlace L;
};

// What the batch code reads of a join's descriptor.  Both entry points share it (templates over the descriptor type):
// rhj_join_desc names two rhj_tuple arrays, rhj_join_cols_desc two columns with optional row-id vectors (ColSrc).
static inline const rhj_tuple *batch_in(const rhj_join_desc &q, int side) { return side ? q.d_S : q.d_R; }
static inline const rhj_tuple *batch_in(const rhj_join_cols_desc &, int) { return nullptr; }
static inline ColSrc batch_src(const rhj_join_desc &, int) { return ColSrc{nullptr, nullptr}; }
static inline ColSrc batch_src(const rhj_join_cols_desc &q, int side) { return side ? ColSrc{q.d_colS, q.d_selS} : ColSrc{q.d_colR, q.d_selR}; }
static inline bool batch_valid(const rhj_join_desc &) { return true; }
static inline bool batch_valid(const rhj_join_cols_desc &q) { return (q.nR == 0 || q.d_colR) && (q.nS == 0 || q.d_colS); }
template <class D> constexpr bool batch_cols = std::is_same<D, rhj_join_cols_desc>::value;

// One chunk: items[lo, hi).  Joins whose plan refused the fused path are appended to `alone`.
template <class D>
static int batch_chunk(D *joins, const std::vector<BatchItem> &items, size_t lo, size_t hi, std::vector<uint64_t> &alone, uint64_t &units,
                       int64_t &walked_units)
{
    const size_t n = hi - lo;
    if (batch_arena(g.batch_arena, items[hi - 1].L.end, BATCH_ARENA_BUDGET)) return -1;
    // the block: [n summary slots] read back; [n descriptors][3 lists of n join numbers] uploaded in one copy
    Block blk;
    uint64_t *slots; BatchJoin *hd, *dd; uint32_t *hl, *dl;           // hl: [0, n) histogram, [n, 2n) resident, [2n, 3n) gathering
    if (batch_block(blk, [&](Block &b) { b.back(slots, n * BATCH_SLOT_WORDS); b.up(hd, dd, n); b.up(hl, dl, 3 * n); })) return -1;
    memset(slots, 0xff, n * BATCH_SLOT_WORDS * 8);                    // (a slot nobody wrote reads as "no match total": an error, not an answer)
    char *A = (char *)g.batch_arena.p;
    uint32_t n_hist = 0, n_res = 0, n_gat = 0;
    int max_bits = 1;
    for (size_t k = 0; k < n; ++k) {
        const BatchItem &it = items[lo + k];
        const D &q = joins[it.idx];
        const BatchPlace &L = it.L;
        const uint32_t bins = 1u << it.bits;
        BatchJoin d;
        memset((void *)&d, 0, sizeof(d));
        d.r0 = RelArgs{batch_in(q, 0), (rhj_tuple *)(A + L.partR), (uint32_t *)(A + L.cntR), q.nR, sm_tiles(q.nR), 0, nullptr, nullptr};
        d.r1 = RelArgs{batch_in(q, 1), (rhj_tuple *)(A + L.partS), (uint32_t *)(A + L.cntS), q.nS, sm_tiles(q.nS), 0, nullptr, nullptr};
        d.c0 = batch_src(q, 0); d.c1 = batch_src(q, 1);
        uint64_t *hist = (uint64_t *)(A + L.hp), *psum = hist + 2 * bins;
        d.hist = hist; d.psum = psum;
        PlanArgs pa;
        memset((void *)&pa, 0, sizeof(pa));
        pa.histR = hist; pa.histS = hist + bins;
        pa.units = (Unit *)(A + L.units); pa.summary = (PlanSummary *)(A + L.summary);
        pa.lds_cap = FUSED_LDS_CAP; pa.lds_max_slots = LDS_MAX_SLOTS; pa.build_chunk = BUILD_CHUNK; pa.span_lds = L.span;
        pa.slice_b0 = pa.slice_b1 = 0xffffffffu;
        d.plan = pa;
        FusedArgs &fa = d.f;
        JoinArgs &ja = fa.j;
        ja.partR = d.r0.out; ja.partS = d.r1.out;
        ja.histR = hist; ja.histS = hist + bins; ja.psumR = psum; ja.psumS = psum + bins;
        ja.units = pa.units; ja.summary = pa.summary; ja.unit_count = (uint64_t *)(A + L.ucount);
        ja.out = q.d_out; ja.out_capacity = q.d_out ? q.out_capacity : 0;
        ja.stash_nR = q.nR;
        fa.stash_cnt = (uint8_t *)(A + L.stash_cnt); fa.stash_row = (uint64_t *)(A + L.stash_row);
        fa.ticket = (uint32_t *)(A + L.status); fa.status = (uint64_t *)(A + L.status) + 8;
        fa.nR = q.nR; fa.allow_resident = !g.no_resident; fa.radix_bits = (uint32_t)it.bits;
        fa.unit_bound = L.unit_bound; fa.host_summary = slots + k * BATCH_SLOT_WORDS;
        fa.ovf = (uint64_t *)(A + L.ovf); fa.ovf_base = (uint32_t *)(A + L.ovf_base); fa.walk = (FjWalkItem *)(A + L.walk);
        d.zero_words = (uint64_t *)(A + L.status); d.n_zero = L.status_words;
        d.bits = it.bits;
        const uint32_t max_tiles = d.r0.tiles > d.r1.tiles ? d.r0.tiles : d.r1.tiles;
        d.self_hist = max_tiles <= SM_SELF_TILES;
        if (!d.self_hist) hl[n_hist++] = (uint32_t)k;
        if (resident(q.nR < q.nS ? q.nR : q.nS, bins)) hl[n + n_res++] = (uint32_t)k;
        else hl[2 * n + n_gat++] = (uint32_t)k;
        if (it.bits > max_bits) max_bits = it.bits;
        memcpy((void *)&hd[k], (const void *)&d, sizeof(d));
    }
    if (batch_upload(blk, hd, blk.host_end())) return -1;
    if constexpr (batch_cols<D>) {
        if (n_hist) RHJ_LAUNCH(k_batch_hist_cols, dim3(BJ_MAX_TILES, 2, n_hist), dim3(SM_BLOCK), 0, g.stream, dd, dl);
        RHJ_LAUNCH(k_batch_scatter_cols, dim3(BJ_MAX_TILES + 1, 2, (unsigned)n), dim3(SM_BLOCK), small_lds_bytes(max_bits), g.stream, dd);
    } else {
        if (n_hist) RHJ_LAUNCH(k_batch_hist, dim3(BJ_MAX_TILES, 2, n_hist), dim3(SM_BLOCK), 0, g.stream, dd, dl);
        RHJ_LAUNCH(k_batch_scatter, dim3(BJ_MAX_TILES + 1, 2, (unsigned)n), dim3(SM_BLOCK), small_lds_bytes(max_bits), g.stream, dd);
    }
    if (n_res) RHJ_LAUNCH((k_batch_fused<true>), dim3(BJ_WGS, n_res), dim3(FJ_BLOCK), FUSED_LDS, g.stream, dd, dl + n, FUSED_LDS);
    if (n_gat) RHJ_LAUNCH((k_batch_fused<false>), dim3(BJ_WGS, n_gat), dim3(FJ_BLOCK), FUSED_LDS, g.stream, dd, dl + 2 * n, FUSED_LDS);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g.stream));
    bool walked = false;
    for (size_t k = 0; k < n; ++k) {
        D &q = joins[items[lo + k].idx];
        PlanSummary plan;
        memcpy(&plan, slots + k * BATCH_SLOT_WORDS, sizeof(plan));    // written by the join's last workgroup out (system-scope stores)
        const uint64_t walk_units = slots[k * BATCH_SLOT_WORDS + sizeof(PlanSummary) / 8];
        if (plan.fused_ok && q.d_out) walked_units += (int64_t)walk_units;
        if (!plan.fused_ok) { alone.push_back(items[lo + k].idx); continue; }   // a bucket's build side beyond the LDS index
        if (plan.matches == FJ_NO_TOTAL) { fprintf(stderr, "rhj: batched join %zu left no match total (chained scan incomplete)\n", (size_t)items[lo + k].idx); return -1; }
        if (q.d_out && walk_units != 0) {
            // rare (a probe tuple with more than 16 matches, ...): this join's listed units, with its own arguments
            RHJ_LAUNCH(k_join_walk, dim3(BJ_WGS), dim3(FJ_BLOCK), FUSED_LDS, g.stream, hd[k].f, FUSED_LDS);
            walked = true;
        }
        q.matches = plan.matches;
        q.rc = q.d_out && plan.matches > q.out_capacity ? 1 : 0;
        q.path = PATH_BATCH_JOIN;
        units += plan.units;
    }
    if (walked) {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g.stream));
    }
    return 0;
}

template <class D>
static int join_batch(D *joins, uint64_t n)
{
    g.last_walk_units = -1;                                            // (a batch that fails leaves no earlier join's number behind)
    if (n == 0) return 0;
    bool timed = false;
    if (const int rc = batch_open(joins, n, [](D &q) { q.matches = 0; q.rc = 0; q.path = 0; return batch_valid(q); }, timed)) return rc;
    std::vector<BatchItem> items;
    std::vector<uint64_t> alone;
    uint64_t sum_r = 0, sum_s = 0, sum_m = 0, units = 0;
    int64_t walked_units = 0;                                          // rhj_last_walk_units: the sum over the batch's joins
    bool walked_known = true;
    for (uint64_t i = 0; i < n; ++i) {
        const D &q = joins[i];
        sum_r += q.nR; sum_s += q.nS;
        if (q.nR == 0 || q.nS == 0) continue;                         // rhjoin.c:15-16: nothing to launch
        const int bits = g.order_any ? auto_radix_bits(q.nR, q.nS) : g.bits;
        if (!batch_takes(bits, q.nR, q.nS)) { alone.push_back(i); continue; }
        BatchItem it;
        it.idx = i; it.bits = bits;
        items.push_back(it);
    }
    // (a join that does not fit is placed again, first in the next chunk)
    const auto place = [&](size_t k, uint64_t at) { return batch_place(items[k].bits, joins[items[k].idx].nR, joins[items[k].idx].nS, (size_t)at, items[k].L); };
    if (batch_cut(items.size(), BATCH_MAX_JOINS, BATCH_ARENA_BUDGET, place,
                  [&](size_t lo, size_t hi, uint64_t) { return batch_chunk(joins, items, lo, hi, alone, units, walked_units); })) return -1;
    // the joins that run alone, through the single-join code (which keeps its own stats: summed up below); relations given by
    // columns are materialised first
    for (const uint64_t i : alone) {
        D &q = joins[i];
        uint64_t m = 0;
        JoinReq req = {batch_in(q, 0), q.nR, batch_in(q, 1), q.nS, q.d_out, q.d_out ? q.out_capacity : 0, false, nullptr, &m, g.bits};
        req.via_sel = batch_cols<D>; req.srcR = batch_src(q, 0); req.srcS = batch_src(q, 1);
        if (materialise(req)) return -1;
        const int rc = join_device(req);
        // (counting only, nothing was short: the tiled path says 1 whenever M passes the capacity, the small and fused paths
        // only when there is a buffer — a batch says the latter for every join)
        q.matches = m; q.rc = rc == 1 && !q.d_out ? 0 : rc; q.path = g.stats.reserved & 0xff;
        if (rc < 0) return rc;
        units += g.stats.units;
        if (g.last_walk_units < 0) walked_known = false; else walked_units += g.last_walk_units;
    }
    g.last_walk_units = walked_known ? walked_units : -1;
    int any_short = 0;
    for (uint64_t i = 0; i < n; ++i) { sum_m += joins[i].matches; any_short |= joins[i].rc == 1; }
    rhj_stats st = {};
    st.n_r = sum_r; st.n_s = sum_s; st.matches = sum_m; st.units = units; st.radix_bits = g.bits;
    st.reserved = PATH_BATCH_JOIN;
    if (batch_close(timed, st)) return -1;
    return any_short;
}

// k_filter_write is grid-stride, one wave per two tiles: enough workgroups to fill the chip a few times over
unsigned filter_write_grid(uint64_t tiles)
{
    const uint64_t want = (tiles + 7) / 8, cap = (uint64_t)g.cus * 32;
    return (unsigned)(want < cap ? want : cap);
}

int op_code(char op)
{
    return op == '<' ? 0 : op == '>' ? 1 : op == '=' ? 2 : -1;
}

// masks + tile counts -> the ascending index list and the hit total (both filters end here)
int filter_write_out(uint64_t n, uint64_t tiles, uint64_t *total, uint64_t *d_out, uint64_t *hits)
{
    if (tiles <= FILTER_SELF_TILES) {                  // the write waves sum the tile counts themselves, the total lands in pinned memory:
        RHJ_LAUNCH((k_filter_write<true>), dim3(filter_write_grid(tiles)), dim3(256), 0, g.stream, n, (const uint64_t *)g.fmask.p,   // no scan
                   (const uint64_t *)g.ftile.p, d_out, (unsigned long long *)&g.pin->hits);                                           // launches, no copy
        RHJ_STAGE(ST_END);
    } else {
        if (launch_offsets((const uint64_t *)g.ftile.p, (uint64_t *)g.fbase.p, nullptr, tiles, tiles, total)) return -1;
        RHJ_LAUNCH((k_filter_write<false>), dim3(filter_write_grid(tiles)), dim3(256), 0, g.stream, n, (const uint64_t *)g.fmask.p,
                   (const uint64_t *)g.fbase.p, d_out, (unsigned long long *)nullptr);
        RHJ_STAGE(ST_END);
        HIP_TRY(hipMemcpyAsync(&g.pin->hits, total, 8, hipMemcpyDeviceToHost, g.stream));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g.stream));
    *hits = *(volatile uint64_t *)&g.pin->hits;
    return 0;
}

// tile counts -> the hit total alone (a count-only item that runs outside its batch): the scan, and its total copied back
int filter_count_out(uint64_t tiles, uint64_t *total, uint64_t *hits)
{
    if (launch_offsets((const uint64_t *)g.ftile.p, (uint64_t *)g.fbase.p, nullptr, tiles, tiles, total)) return -1;
    HIP_TRY(hipMemcpyAsync(&g.pin->hits, total, 8, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g.stream));
    *hits = *(volatile uint64_t *)&g.pin->hits;
    return 0;
}

// What an item that runs alone inside a batch works in, the single calls' buffers: mask words, tile counts, their scan and the
// total.  The mask bytes are what k_filter_mask and k_filter_mask_eq2 need, n / 8 + 576 or more; k_fbatch_mask's
// fbatch_mask_bytes(n) is at most n / 8 + 16, so this covers it for every n.
int filter_workspace(uint64_t n, uint64_t tiles)
{
    return ensure(g.fmask, ((n + 63) / 64 + FILTER_ROUNDS * 8 + 8) * 8) || ensure(g.ftile, tiles * 8) || ensure(g.fbase, tiles * 8) ||
           ensure(g.summary, sizeof(PlanSummary)) ? -1 : 0;
}

int filter_device(const uint64_t *d_col, const uint64_t *d_sel, uint64_t n, char op, uint64_t value, uint64_t *d_out,
                  bool use_ctx_out, uint64_t **ctx_out, uint64_t *hits)
{
    if (ctx_init()) return -1;
    *hits = 0;
    if (ctx_out) *ctx_out = nullptr;
    const int oc = op_code(op);
    if (oc < 0) return -3;
    if (n == 0) return 0;
    const uint64_t tiles = (n + FILTER_TILE - 1) / FILTER_TILE;
    if (ensure(g.fmask, ((n + 63) / 64 + FILTER_ROUNDS * 8 + 8) * 8) || ensure(g.ftile, tiles * 8) ||
        ensure(g.fbase, tiles * 8) || ensure(g.summary, sizeof(PlanSummary)))
        return -1;
    if (use_ctx_out) {
        if (ensure(g.fout, n * 8)) return -1;
        d_out = (uint64_t *)g.fout.p;
        if (ctx_out) *ctx_out = d_out;
    }
    uint64_t *total = &((PlanSummary *)g.summary.p)->matches;
    RHJ_STAGE(ST_HIST);
    const bool vec = ((uintptr_t)(d_sel ? d_sel : d_col) & 15u) == 0;     // the mask pass's 16-byte loads need an aligned base
    RHJ_LAUNCH(k_filter_mask, dim3((unsigned)tiles), dim3(256), 0, g.stream, d_col, d_sel, n, oc, value, vec,
                       (uint64_t *)g.fmask.p, (uint64_t *)g.ftile.p);
    if (filter_write_out(n, tiles, total, d_out, hits)) return -1;
    memset(&g.stats, 0, sizeof(g.stats));
    g.stats.n_r = n; g.stats.matches = *hits;
    g.stats.ms_total = g.stats.ms_probe = stage_ms(ST_HIST, ST_END);
    return 0;
}

int filter_eq2_device(const uint64_t *colA, const uint64_t *selA, const uint64_t *colB, const uint64_t *selB, uint64_t n,
                      uint64_t *d_out, uint64_t *hits)
{
    if (ctx_init()) return -1;
    *hits = 0;
    if (n == 0) return 0;
    const uint64_t tiles = (n + FILTER_TILE - 1) / FILTER_TILE;
    if (ensure(g.fmask, ((n + 63) / 64 + FILTER_ROUNDS * 8 + 8) * 8) || ensure(g.ftile, tiles * 8) ||
        ensure(g.fbase, tiles * 8) || ensure(g.summary, sizeof(PlanSummary)))
        return -1;
    uint64_t *total = &((PlanSummary *)g.summary.p)->matches;
    RHJ_STAGE(ST_HIST);
    RHJ_LAUNCH(k_filter_mask_eq2, dim3((unsigned)tiles), dim3(256), 0, g.stream, colA, selA, colB, selB, n,
               (uint64_t *)g.fmask.p, (uint64_t *)g.ftile.p);
    if (filter_write_out(n, tiles, total, d_out, hits)) return -1;
    memset(&g.stats, 0, sizeof(g.stats));
    g.stats.n_r = n; g.stats.matches = *hits;
    g.stats.ms_total = g.stats.ms_probe = stage_ms(ST_HIST, ST_END);
    return 0;
}

// ---- batched filters and two-column equalities (rhj_filter_batch.hip.h, rhj_eq2_batch.hip.h) --------------------------------
// rhj_filter_batch_device and rhj_filter_eq2_batch_device are ONE scheme over two descriptors (templates over rhj_filter_desc /
// rhj_eq2_desc, as join_batch is over its two): the items filter_batch_takes() names run as chunks of two launches and one stream
// synchronisation each; a larger one is run alone (fbatch_alone).
//
// A chunk's items live side by side in ONE arena (every item its mask words, 16 bytes per 128 rows, and its tile counts), which
// never exceeds BATCH_ARENA_BUDGET, and a chunk never holds more than FBATCH_MAX_FILTERS items: a batch beyond either is cut into
// chunks, in call order.  The arena is the batches' own: g.fmask / g.ftile / g.fbase stay what the single calls made them.
constexpr uint64_t FBATCH_MAX_ROWS = FILTER_SELF_TILES * FILTER_TILE;
constexpr size_t FBATCH_MAX_FILTERS = 4096;

static int filter_batch_takes(uint64_t rows) { return rows >= 1 && rows <= FBATCH_MAX_ROWS; }

static size_t fbatch_mask_bytes(uint64_t n) { return (size_t)((n + 2 * WAVE - 1) / (2 * WAVE)) * 16; }

struct FBatchItem {
    uint64_t idx;                                         // the item's place in the caller's array
    size_t   masks, counts, end;                          // byte offsets in the arena
};

static size_t fbatch_place(uint64_t rows, size_t at, FBatchItem &it)
{
    auto take = [&at](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    it.masks = take(fbatch_mask_bytes(rows));
    it.counts = take((size_t)((rows + FILTER_TILE - 1) / FILTER_TILE) * 8);
    return it.end = at;
}

// What differs between the two: the device descriptor and how it is filled, the validity rule, the two kernels, the path id,
// the noun of the error text, and how an item beyond FBATCH_MAX_ROWS runs alone.
template <class D> using fbatch_dev = std::conditional_t<std::is_same<D, rhj_filter_desc>::value, FBatchDesc, Eq2BatchDesc>;

static void fbatch_desc(const rhj_filter_desc &q, uint64_t *masks, uint64_t *counts, uint64_t *h_total, FBatchDesc &d)
{
    memset((void *)&d, 0, sizeof(d));
    d.sel = q.d_sel; d.n = q.n; d.out = q.d_out; d.masks = masks; d.tile_count = counts; d.h_total = (unsigned long long *)h_total;
    d.nterms = q.nterms;
    uintptr_t scanned = (uintptr_t)q.d_sel;               // the mask pass's 16-byte loads need every scanned vector's base aligned
    for (int t = 0; t < q.nterms; ++t) {
        d.t[t].col = q.terms[t].d_col; d.t[t].value = q.terms[t].value; d.t[t].op = op_code(q.terms[t].op);
        if (!q.d_sel) scanned |= (uintptr_t)q.terms[t].d_col;
    }
    d.vec = (scanned & 15u) == 0;
}

static void fbatch_desc(const rhj_eq2_desc &q, uint64_t *masks, uint64_t *counts, uint64_t *h_total, Eq2BatchDesc &d)
{
    memset((void *)&d, 0, sizeof(d));
    d.colA = q.d_colA; d.selA = q.d_selA; d.colB = q.d_colB; d.selB = q.d_selB;
    d.n = q.n; d.out = q.d_out; d.masks = masks; d.tile_count = counts; d.h_total = (unsigned long long *)h_total;
    d.vecA = ((uintptr_t)(q.d_selA ? q.d_selA : q.d_colA) & 15u) == 0;      // the 16-byte loads need the scanned vector's base aligned
    d.vecB = ((uintptr_t)(q.d_selB ? q.d_selB : q.d_colB) & 15u) == 0;
}

static bool fbatch_valid(const rhj_filter_desc &q)
{
    bool ok = q.nterms >= 1 && q.nterms <= RHJ_FILTER_MAX_TERMS;
    for (int t = 0; ok && t < q.nterms; ++t) ok = op_code(q.terms[t].op) >= 0 && (q.n == 0 || q.terms[t].d_col != nullptr);
    return ok;
}
static bool fbatch_valid(const rhj_eq2_desc &q) { return q.n == 0 || (q.d_colA && q.d_colB); }

static inline int fbatch_path(const rhj_filter_desc &) { return PATH_BATCH_FILTER; }
static inline int fbatch_path(const rhj_eq2_desc &) { return PATH_BATCH_EQ2; }
static inline const char *fbatch_noun(const rhj_filter_desc &) { return "filter"; }
static inline const char *fbatch_noun(const rhj_eq2_desc &) { return "equality"; }

static void fbatch_launch(const FBatchDesc *dd, uint32_t nf, const uint32_t *tile_start, uint32_t tiles, const uint32_t *task_start, uint32_t write_grid)
{
    RHJ_LAUNCH(k_fbatch_mask, dim3(tiles), dim3(256), 0, g.stream, dd, tile_start, nf);
    RHJ_LAUNCH(k_fbatch_write, dim3(write_grid), dim3(256), 0, g.stream, dd, task_start, nf);
}
static void fbatch_launch(const Eq2BatchDesc *dd, uint32_t nf, const uint32_t *tile_start, uint32_t tiles, const uint32_t *task_start, uint32_t write_grid)
{
    RHJ_LAUNCH(k_eq2batch_mask, dim3(tiles), dim3(256), 0, g.stream, dd, tile_start, nf);
    RHJ_LAUNCH(k_eq2batch_write, dim3(write_grid), dim3(256), 0, g.stream, dd, task_start, nf);
}

// One chunk: items[lo, hi), every one with 1..FBATCH_MAX_ROWS rows.
template <class D>
static int fbatch_chunk(D *qs, const std::vector<FBatchItem> &items, size_t lo, size_t hi)
{
    using Dev = fbatch_dev<D>;
    const size_t nf = hi - lo;
    if (batch_arena(g.fbatch_arena, items[hi - 1].end, BATCH_ARENA_BUDGET)) return -1;
    // the block: [nf hit totals] read back; [nf descriptors][nf + 1 tile starts][nf + 1 task starts] uploaded in one copy
    Block blk;
    uint64_t *totals; Dev *hd, *dd; uint32_t *tile_start, *d_tile_start, *task_start, *d_task_start;
    if (batch_block(blk, [&](Block &b) { b.back(totals, nf); b.up(hd, dd, nf); b.up(tile_start, d_tile_start, nf + 1); b.up(task_start, d_task_start, nf + 1); })) return -1;
    memset(totals, 0xff, nf * 8);                         // (a slot nobody wrote reads as "no total": an error, not an answer)
    char *A = (char *)g.fbatch_arena.p;
    uint32_t tiles = 0, tasks = 0;
    for (size_t k = 0; k < nf; ++k) {
        const FBatchItem &it = items[lo + k];
        const D &q = qs[it.idx];
        Dev d;
        fbatch_desc(q, (uint64_t *)(A + it.masks), (uint64_t *)(A + it.counts), totals + k, d);
        memcpy((void *)&hd[k], (const void *)&d, sizeof(d));
        const uint32_t t = (uint32_t)((q.n + FILTER_TILE - 1) / FILTER_TILE);
        tile_start[k] = tiles; task_start[k] = tasks;
        tiles += t;
        tasks += q.d_out ? (t + 1) / 2 : 1;               // count only: one wave sums the tile counts, nothing else to do
    }
    tile_start[nf] = tiles; task_start[nf] = tasks;
    if (batch_upload(blk, hd, blk.host_end())) return -1;
    const uint32_t want = (tasks + 256 / WAVE - 1) / (256 / WAVE), cap = (uint32_t)g.cus * 32;      // grid-stride, as filter_write_grid
    fbatch_launch(dd, (uint32_t)nf, d_tile_start, tiles, d_task_start, want < cap ? want : cap);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g.stream));
    for (size_t k = 0; k < nf; ++k) {
        D &q = qs[items[lo + k].idx];
        const uint64_t h = ((volatile uint64_t *)totals)[k];            // written by the wave of the item's last task (system-scope store)
        if (h > q.n) { fprintf(stderr, "rhj: batched %s %zu left no hit total\n", fbatch_noun(q), (size_t)items[lo + k].idx); return -1; }
        q.hits = h; q.path = fbatch_path(q);
    }
    return 0;
}

// a filter beyond FBATCH_MAX_ROWS, alone: k_fbatch_mask over its one descriptor, then the scan and k_filter_write<false>
static int fbatch_alone(rhj_filter_desc &q)
{
    const uint64_t n = q.n, tiles = (n + FILTER_TILE - 1) / FILTER_TILE;
    if (tiles >= (1ull << 32)) return -2;
    Block blk;                                            // [the descriptor][2 tile starts], nothing read back
    FBatchDesc *hd, *dd; uint32_t *tile_start, *d_tile_start;
    if (filter_workspace(n, tiles) || batch_block(blk, [&](Block &b) { b.up(hd, dd, 1); b.up(tile_start, d_tile_start, 2); })) return -1;
    FBatchDesc d;
    fbatch_desc(q, (uint64_t *)g.fmask.p, (uint64_t *)g.ftile.p, nullptr, d);
    memcpy((void *)hd, (const void *)&d, sizeof(d));
    tile_start[0] = 0; tile_start[1] = (uint32_t)tiles;
    uint64_t *total = &((PlanSummary *)g.summary.p)->matches;
    if (batch_upload(blk, hd, blk.host_end())) return -1;
    RHJ_LAUNCH(k_fbatch_mask, dim3((unsigned)tiles), dim3(256), 0, g.stream, dd, d_tile_start, 1u);
    uint64_t h = 0;
    if (q.d_out ? filter_write_out(n, tiles, total, q.d_out, &h) : filter_count_out(tiles, total, &h)) return -1;
    q.hits = h; q.path = 0;
    return 0;
}

// an equality beyond FBATCH_MAX_ROWS, alone: the single call as it is, or, counting only, its mask launch and the scan's total
static int fbatch_alone(rhj_eq2_desc &q)
{
    uint64_t h = 0;
    if (q.d_out) {
        const int rc = filter_eq2_device(q.d_colA, q.d_selA, q.d_colB, q.d_selB, q.n, q.d_out, &h);
        if (rc) return rc;
    } else {
        const uint64_t n = q.n, tiles = (n + FILTER_TILE - 1) / FILTER_TILE;
        if (tiles >= (1ull << 32)) return -2;
        if (filter_workspace(n, tiles)) return -1;
        uint64_t *total = &((PlanSummary *)g.summary.p)->matches;
        RHJ_LAUNCH(k_filter_mask_eq2, dim3((unsigned)tiles), dim3(256), 0, g.stream, q.d_colA, q.d_selA, q.d_colB, q.d_selB, n,
                   (uint64_t *)g.fmask.p, (uint64_t *)g.ftile.p);
        if (filter_count_out(tiles, total, &h)) return -1;
    }
    q.hits = h; q.path = 0;
    return 0;
}

template <class D>
static int filter_batch(D *qs, uint64_t n)
{
    if (n == 0) return 0;
    bool timed = false;
    if (const int rc = batch_open(qs, n, [](D &q) { q.hits = 0; q.rc = 0; q.path = 0; return fbatch_valid(q); }, timed)) return rc;
    std::vector<FBatchItem> items;
    std::vector<uint64_t> alone;
    uint64_t rows = 0, hits = 0;
    for (uint64_t i = 0; i < n; ++i) {
        rows += qs[i].n;
        if (qs[i].n == 0) continue;                       // nothing to launch
        if (!filter_batch_takes(qs[i].n)) { alone.push_back(i); continue; }
        FBatchItem it;
        it.idx = i; it.masks = it.counts = it.end = 0;
        items.push_back(it);
    }
    const auto place = [&](size_t k, uint64_t at) { return fbatch_place(qs[items[k].idx].n, (size_t)at, items[k]); };
    if (batch_cut(items.size(), FBATCH_MAX_FILTERS, BATCH_ARENA_BUDGET, place,
                  [&](size_t lo, size_t hi, uint64_t) { return fbatch_chunk(qs, items, lo, hi); })) return -1;
    for (const uint64_t i : alone) {
        const int rc = fbatch_alone(qs[i]);
        if (rc < 0) { qs[i].rc = rc; return rc; }
    }
    for (uint64_t i = 0; i < n; ++i) hits += qs[i].hits;
    rhj_stats st = {};
    st.n_r = rows; st.matches = hits; st.units = items.size();
    st.reserved = fbatch_path(qs[0]);
    return batch_close(timed, st);
}

// ---- batched rebuilds and view sums (rhj_apply_batch.hip.h) ----------------------------------------------------------------
// rhj_apply_batch_device: every item of at least one row runs in the launch of its chunk (path 8); there is no run-alone class.
// A chunk holds at most APPLY_MAX_ITEMS items and APPLY_MAX_TILES tiles (both conditions, not measurements: the first bounds
// the uploaded block, the second keeps a chunk's tile starts far inside 32 bits), and a batch beyond either is cut in call
// order.  A chunk is one upload, one launch and one stream synchronisation; it shares the pinned block and g.batch_desc with
// the join and filter batches, and ends in that synchronisation before the block is written again.
constexpr size_t APPLY_MAX_ITEMS = 4096;
constexpr uint64_t APPLY_MAX_TILES = 1ull << 24;
constexpr uint64_t APPLY_MAX_ROWS = APPLY_MAX_TILES * APPLY_TILE;       // 2^35

static bool apply_valid(const rhj_apply_desc &q)
{
    if ((q.idx_stride != 1 && q.idx_stride != 2) || q.nterms < 1 || q.nterms > RHJ_APPLY_MAX_TERMS || q.n > APPLY_MAX_ROWS) return false;
    for (int t = 0; t < q.nterms; ++t) {
        const rhj_apply_term &a = q.terms[t];
        if (a.side < 0 || a.side >= q.idx_stride || (a.side != 0 && !q.d_idx) || (!a.d_dst && !a.d_col)) return false;
    }
    return true;
}

static bool apply_sums(const rhj_apply_desc &q)
{
    for (int t = 0; t < q.nterms; ++t) if (q.terms[t].d_col) return true;
    return false;
}

// One chunk: items[which[lo, hi)], every one valid and of at least one row.
static int apply_chunk(rhj_apply_desc *items, const std::vector<uint64_t> &which, size_t lo, size_t hi)
{
    const size_t ni = hi - lo;
    size_t nsum = 0;
    for (size_t k = lo; k < hi; ++k) nsum += apply_sums(items[which[k]]);
    // the block: [ni sum slots] read back; [ni descriptors][ni + 1 tile starts][accumulator and ticket words of the summing
    // items, zero] uploaded in one copy
    constexpr size_t WORDS = RHJ_APPLY_MAX_TERMS + 1;     // an item's accumulators and its ticket
    static_assert(sizeof(ApplyDesc) % 8 == 0, "the words' padding is that of the tile starts alone");
    Block blk;
    uint64_t *slots; ApplyDesc *hd, *dd; uint32_t *tile_start, *d_tile_start; unsigned long long *words, *d_words;
    if (batch_block(blk, [&](Block &b) { b.back(slots, ni * APPLY_SLOT_WORDS); b.up(hd, dd, ni); b.up(tile_start, d_tile_start, ni + 1); b.up(words, d_words, nsum * WORDS); })) return -1;
    memset(slots, 0, ni * APPLY_SLOT_WORDS * 8);          // (a summing item whose slot is not flagged done left no sums: an error)
    memset(words, 0, nsum * WORDS * 8);
    uint32_t tiles = 0;
    size_t s = 0;
    for (size_t k = 0; k < ni; ++k) {
        const rhj_apply_desc &q = items[which[lo + k]];
        ApplyDesc d;
        memset((void *)&d, 0, sizeof(d));
        d.idx = q.d_idx; d.n = q.n; d.stride = q.idx_stride; d.nterms = q.nterms;
        d.tiles = (uint32_t)((q.n + APPLY_TILE - 1) / APPLY_TILE);
        for (int t = 0; t < q.nterms; ++t) {
            d.t[t].src = q.terms[t].d_src; d.t[t].dst = q.terms[t].d_dst; d.t[t].col = q.terms[t].d_col; d.t[t].side = q.terms[t].side;
            d.sides |= 1u << q.terms[t].side;
        }
        if (apply_sums(q)) {
            d.acc = d_words + s * WORDS;
            d.ticket = (uint32_t *)(d.acc + RHJ_APPLY_MAX_TERMS);
            d.h_slot = (unsigned long long *)slots + k * APPLY_SLOT_WORDS;
            ++s;
        }
        memcpy((void *)&hd[k], (const void *)&d, sizeof(d));
        tile_start[k] = tiles;
        tiles += d.tiles;
    }
    tile_start[ni] = tiles;
    if (batch_upload(blk, hd, blk.host_end())) return -1;
    RHJ_LAUNCH(k_apply_batch, dim3(tiles), dim3(256), 0, g.stream, dd, d_tile_start, (uint32_t)ni);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g.stream));
    for (size_t k = 0; k < ni; ++k) {
        rhj_apply_desc &q = items[which[lo + k]];
        q.path = PATH_BATCH_APPLY;
        if (!apply_sums(q)) continue;
        const volatile uint64_t *h = (const volatile uint64_t *)slots + k * APPLY_SLOT_WORDS;     // written by the item's last workgroup out (system scope)
        if (h[RHJ_APPLY_MAX_TERMS] != 1) { fprintf(stderr, "rhj: batched apply item %zu left no sums\n", (size_t)which[lo + k]); return -1; }
        for (int t = 0; t < q.nterms; ++t) if (q.terms[t].d_col) q.terms[t].sum = h[t];
    }
    return 0;
}

static int apply_batch(rhj_apply_desc *items, uint64_t n)
{
    if (n == 0) return 0;
    bool timed = false;
    const auto reset = [](rhj_apply_desc &q) {
        q.rc = 0; q.path = 0;
        if (!apply_valid(q)) return false;
        for (int t = 0; t < q.nterms; ++t) q.terms[t].sum = 0;
        return true;
    };
    if (const int rc = batch_open(items, n, reset, timed)) return rc;
    std::vector<uint64_t> which;
    uint64_t rows = 0;
    for (uint64_t i = 0; i < n; ++i) {
        rows += items[i].n;
        if (items[i].n) which.push_back(i);               // an empty item: nothing to launch
    }
    const auto tiles = [&](size_t k, uint64_t t) { return t + (items[which[k]].n + APPLY_TILE - 1) / APPLY_TILE; };   // (one item never has more than the limit: apply_valid)
    if (batch_cut(which.size(), APPLY_MAX_ITEMS, APPLY_MAX_TILES, tiles,
                  [&](size_t lo, size_t hi, uint64_t) { return apply_chunk(items, which, lo, hi); })) return -1;
    rhj_stats st = {};
    st.n_r = rows; st.units = which.size();
    st.reserved = PATH_BATCH_APPLY;
    return batch_close(timed, st);
}

// ---- batched column statistics (rhj_stats_batch.hip.h) ---------------------------------------------------------------------
// rhj_column_stats_batch_device: every column of at least one row runs in the launches of its chunk (path 11); there is no
// run-alone class.  A chunk holds at most STATS_MAX_COLUMNS columns and STATS_MAX_TILES tiles (conditions, as the apply
// batch's) and STATS_ARENA_BYTES of bitmaps (the widest column's is 6.25 MB), and a batch beyond any of them is cut in call
// order.  How many bitmap bytes a column needs is known only after pass 1, so stats_group runs k_statsbatch_minmax over the
// columns the first two limits admit, and then marks and counts them in runs that fit the arena: the first run
// is the chunk that pass 1 belongs to (three launches, two stream waits), and the columns that did not fit keep their
// extremes and make up the following chunks (two launches, one wait each).  The uploaded block is
//   [3 words a column: ~0, 0, 0][descriptors][columns + 1 row-tile starts][columns + 1 word-tile starts]
// in g.batch_desc; the descriptors and both arrays of tile starts are uploaded once more with the placement of every run.
constexpr size_t STATS_MAX_COLUMNS = 4096;
constexpr uint64_t STATS_MAX_TILES = 1ull << 24;
constexpr uint64_t STATS_MAX_ROWS = STATS_MAX_TILES * STATS_TILE;       // 2^35
constexpr size_t STATS_ARENA_BYTES = 256ull * 1024 * 1024;

rhj_colstats_batch_info g_stats_info = {};

static uint64_t stats_flags(uint64_t l, uint64_t u)
{
    if (l > u) return 0;
    const uint64_t size = u - l + 1;                      // 0: the full range, wrapped
    return size == 0 || size >= STATS_CAP ? STATS_FOLD : size;
}

static inline size_t stats_bitmap_bytes(uint64_t flags) { return (size_t)((flags + 31) / 32) * 4; }

// One group: the nc columns cols[which[0, nc)], every one valid and of at least one row.  Pass 1 leaves their extremes in the
// caller's descriptors; passes 2 and 3 then take them in runs whose bitmaps fit the arena together, one chunk a run.
static int stats_group(rhj_colstats_desc *cols, const uint64_t *which, size_t nc)
{
    static_assert(sizeof(StatsDesc) % 8 == 0, "the tile starts follow the descriptors without padding");
    const size_t starts = (nc + 2) & ~(size_t)1;          // uint32_t elements of either array of nc + 1 tile starts: an even number, as this block has always had them
    Block blk;
    unsigned long long *back, *words, *d_words; StatsDesc *hd, *dd; uint32_t *tile_start, *d_tile_start, *wtile_start, *d_wtile_start;
    const auto pieces = [&](Block &b) { b.back(back, 3 * nc); b.up(words, d_words, 3 * nc); b.up(hd, dd, nc); b.up(tile_start, d_tile_start, starts); b.up(wtile_start, d_wtile_start, starts); };
    if (batch_block(blk, pieces)) return -1;
    uint32_t tiles = 0;
    for (size_t k = 0; k < nc; ++k) {
        const rhj_colstats_desc &q = cols[which[k]];
        words[3 * k] = ~0ull; words[3 * k + 1] = 0; words[3 * k + 2] = 0;
        StatsDesc d;
        memset((void *)&d, 0, sizeof(d));
        d.col = q.d_col; d.n = q.n; d.words = d_words + 3 * k;
        memcpy((void *)&hd[k], (const void *)&d, sizeof(d));
        tile_start[k] = tiles;
        tiles += (uint32_t)((q.n + STATS_TILE - 1) / STATS_TILE);
    }
    tile_start[nc] = tiles;
    if (batch_upload(blk, words, wtile_start)) return -1; // the words, the descriptors, the row-tile starts
    RHJ_LAUNCH(k_statsbatch_minmax, dim3(tiles), dim3(256), 0, g.stream, dd, d_tile_start, (uint32_t)nc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(back, d_words, nc * 24, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    for (size_t k = 0; k < nc; ++k) {
        rhj_colstats_desc &q = cols[which[k]];
        q.l = back[3 * k]; q.u = back[3 * k + 1];
        if (q.l > q.u) { fprintf(stderr, "rhj: batched statistics column %zu left no extremes\n", (size_t)which[k]); return -1; }
    }
    const auto bitmap = [&](size_t k) { return stats_bitmap_bytes(stats_flags(cols[which[k]].l, cols[which[k]].u)); };
    // passes 2 and 3 of columns [a, b), whose bitmaps take `bytes` together: one chunk
    const auto chunk = [&](size_t a, size_t b, uint64_t bytes) {
        if (batch_arena(g.stats_arena, (size_t)bytes, STATS_ARENA_BYTES)) return -1;
        size_t at = 0;
        uint32_t tiles = 0, wtiles = 0;                   // of this run: both arrays of tile starts begin at 0
        for (size_t k = a; k < b; ++k) {
            const rhj_colstats_desc &q = cols[which[k]];
            const uint64_t flags = stats_flags(q.l, q.u);
            StatsDesc d;
            memcpy((void *)&d, (const void *)&hd[k], sizeof(d));
            d.bits = (uint32_t *)((char *)g.stats_arena.p + at);
            d.lo = q.l;
            d.fold = q.u - q.l + 1 == flags ? 0 : (uint32_t)STATS_FOLD;
            d.nwords = (uint32_t)((flags + 31) / 32);
            memcpy((void *)&hd[k], (const void *)&d, sizeof(d));
            at += bitmap(k);
            tile_start[k - a] = tiles;
            tiles += (uint32_t)((q.n + STATS_TILE - 1) / STATS_TILE);
            wtile_start[k - a] = wtiles;
            wtiles += (d.nwords + STATS_WORD_TILE - 1) / STATS_WORD_TILE;
        }
        tile_start[b - a] = tiles; wtile_start[b - a] = wtiles;
        // the placement: the descriptors, both arrays of tile starts (the columns' words stay as the device has them)
        if (batch_upload(blk, hd, blk.host_end())) return -1;
        HIP_TRY(hipMemsetAsync(g.stats_arena.p, 0, at, g.stream));
        RHJ_LAUNCH(k_statsbatch_mark, dim3(tiles), dim3(256), 0, g.stream, dd + a, d_tile_start, (uint32_t)(b - a));
        RHJ_LAUNCH(k_statsbatch_count, dim3(wtiles), dim3(256), 0, g.stream, dd + a, d_wtile_start, (uint32_t)(b - a));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(back, d_words, nc * 24, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        for (size_t k = a; k < b; ++k) {
            cols[which[k]].d = (double)back[3 * k + 2];
            cols[which[k]].path = PATH_BATCH_STATS;
        }
        ++g_stats_info.chunks;
        g_stats_info.columns += (uint32_t)(b - a);
        return 0;
    };
    return batch_cut(nc, nc, STATS_ARENA_BYTES, [&](size_t k, uint64_t bytes) { return bytes + bitmap(k); }, chunk);   // (one column's bitmap alone always fits)
}

static int stats_batch(rhj_colstats_desc *cols, uint64_t n)
{
    memset(&g_stats_info, 0, sizeof(g_stats_info));
    if (n == 0) return 0;
    bool timed = false;
    const auto reset = [](rhj_colstats_desc &q) { q.rc = 0; q.path = 0; return q.n <= STATS_MAX_ROWS && (q.n == 0 || q.d_col); };
    if (const int rc = batch_open(cols, n, reset, timed)) return rc;
    std::vector<uint64_t> which;
    uint64_t rows = 0;
    for (uint64_t i = 0; i < n; ++i) {
        rows += cols[i].n;
        if (cols[i].n) which.push_back(i);
        else { cols[i].l = cols[i].u = 0; cols[i].d = 0; }   // an empty column: nothing to launch
    }
    const auto tiles = [&](size_t k, uint64_t t) { return t + (cols[which[k]].n + STATS_TILE - 1) / STATS_TILE; };   // (one column never has more than the limit: the validation)
    if (batch_cut(which.size(), STATS_MAX_COLUMNS, STATS_MAX_TILES, tiles,
                  [&](size_t lo, size_t hi, uint64_t) { return stats_group(cols, which.data() + lo, hi - lo); })) return -1;
    rhj_stats st = {};
    st.n_r = rows; st.units = which.size();
    st.reserved = PATH_BATCH_STATS;
    return batch_close(timed, st);
}

// ---- the table batches: batched final joins and weighted join folds (rhj_join_sum_batch.hip.h, rhj_join_fold_batch.hip.h) --------
// rhj_join_sum_batch_device (path 12), rhj_join_fold_batch_device (path 13), rhj_join_foldk_batch_device (path 14, the folds on
// tuple keys of rhj_join_foldk_batch.hip.h) and rhj_join_foldn_batch_device (path 16, those with a row-id vector per key word,
// rhj_join_foldn_batch.hip.h) are ONE scheme over four descriptors (templates over rhj_join_sum_desc / rhj_join_fold_desc /
// rhj_join_foldk_desc / rhj_join_foldn_desc, as filter_batch is over its two).  Every item with two non-empty sides runs in the
// launches of its chunk; there is no run-alone class.  Every item has a hash table in the arena g.jsum_arena, which both share.
// A chunk holds at most JSUM_MAX_ITEMS items and JSUM_MAX_TILES tiles of both sides together, so that no launch's grid passes the
// limit (conditions, as the apply batch's), and JSUM_ARENA_BYTES of tables, and a batch beyond any of them is cut in call order:
// by the first two into groups, a group by the third into chunks.  A chunk takes its first item whatever its table needs.  A
// chunk is one upload, one memset of exactly its tables, three launches (the folds' first only when some item's R builds), one
// copy of its accumulator words and one stream synchronisation; the uploaded block is
//   [descriptors][items + 1 tile starts of the first launch][of the second][of the third][the indices of the resident items][the
//   item's accumulator words, zero]
// (the resident items: those of the three fold batches that one workgroup folds in LDS with rhj_set_fold_resident, on one key, or
// rhj_set_fold_resident_keys, on tuple keys, on; they have
// no table, no tile in the three launches and a launch of their own, and a chunk of them alone has no memset: tbatch_resident below)
constexpr size_t JSUM_MAX_ITEMS = 4096;
constexpr uint64_t JSUM_MAX_TILES = 1ull << 24;
constexpr uint64_t JSUM_MAX_ROWS = 1ull << 32;            // a side has fewer rows than this: a slot's counts are 32-bit words
constexpr size_t JSUM_ARENA_BYTES = BATCH_ARENA_BUDGET;

static inline uint64_t jsum_tiles(uint64_t rows) { return (rows + JSUM_TILE - 1) / JSUM_TILE; }
template <class D> static inline uint64_t tbatch_slots(const D &q) { return jsum_slots(jsum_build_side(q.nR, q.nS) ? q.nS : q.nR); }
// a non-empty side has a column, and both sides have fewer than JSUM_MAX_ROWS rows
template <class D> static inline bool tbatch_sides_valid(const D &q) { return !(q.nR && !q.d_colR) && !(q.nS && !q.d_colS) && q.nR < JSUM_MAX_ROWS && q.nS < JSUM_MAX_ROWS; }

// What differs between the two: the device descriptor and its accumulator words, the validity rule, the results and how they are
// zeroed and taken, a table's bytes, how a descriptor is filled and what tiles the item adds to the three launches, the three
// kernels, the path id, the noun of the error text, and whether the statistics count matches.
template <class D> struct tbatch_dev;
template <> struct tbatch_dev<rhj_join_sum_desc> { using type = JoinSumDesc; static constexpr size_t words = JSUM_WORDS; static constexpr bool first_adds = true; };
template <> struct tbatch_dev<rhj_join_fold_desc> { using type = JoinFoldDesc; static constexpr size_t words = FOLD_WORDS; static constexpr bool first_adds = false; };
template <> struct tbatch_dev<rhj_join_foldk_desc> { using type = JoinFoldKDesc; static constexpr size_t words = FOLDK_WORDS; static constexpr bool first_adds = false; };
template <> struct tbatch_dev<rhj_join_foldn_desc> { using type = JoinFoldNDesc; static constexpr size_t words = FOLDK_WORDS; static constexpr bool first_adds = false; };
static_assert(JSUM_W_COMBINE + COMBINE_WORDS == JSUM_WORDS && FOLD_W_COMBINE + COMBINE_WORDS == FOLD_WORDS && FOLDK_W_COMBINE + COMBINE_WORDS == FOLDK_WORDS,
              "the combiner's counters are the last words of an item (tbatch_combine_take)");

// The combiner of the add launches (rhj_slot_combine.hip.h).  g_fold_combine goes into every device descriptor
// (tbatch_fill) and sizes the add launches' LDS (tbatch_launch).  g_combine_info sums, over the table batches of one public call
// (the four entry points reset it, and rhj_query_batch_device does for the batches inside it): the add launches' tiles, taken
// from the launch counts, and the two counters every item brings back in its last two words.  All zero with the switch off.
rhj_table_batch_combine_info g_combine_info = {};
static inline size_t combine_lds_bytes(bool sums) { return !g_fold_combine ? 0 : sums ? sizeof(CombineLds<unsigned long long>) : sizeof(CombineLds<uint32_t>); }
// a group of items' launches (t: their tiles in the three launches) and their words as copied back
template <class D>
static void tbatch_combine_take(const uint32_t (&t)[3], const unsigned long long *back, size_t ni)
{
    if (!g_fold_combine) return;
    constexpr size_t WORDS = tbatch_dev<D>::words;
    g_combine_info.tiles += t[1] + (tbatch_dev<D>::first_adds ? t[0] : 0u);
    for (size_t k = 0; k < ni; ++k) {
        g_combine_info.combined_tiles += back[k * WORDS + WORDS - COMBINE_WORDS + COMBINE_W_TILES];
        g_combine_info.slot_adds += back[k * WORDS + WORDS - COMBINE_WORDS + COMBINE_W_ADDS];
    }
}

// The resident form of the folds on one key (rhj_fold_lds.hip.h).  With g_fold_resident on, an item that
// fold_resident_rule names has no table in the arena (tbatch_table_bytes 0), no tile in the three launches (tbatch_fill) and path
// 18; a chunk's such items are ONE k_fold_lds launch over an index array that is uploaded with the chunk.  The descriptors stay
// one array in call order, so fbatch_find passes over a resident item as over any item without a tile in a launch.  The two
// descriptors on tuple keys have the form under a switch of their own (below); the join sums have none.  g_resident_info counts, where g_combine_info counts, the resident items, their
// launches and the table items of the fold batches on one key; all zero with the switch off.
rhj_table_batch_resident_info g_resident_info = {};
template <class D> static inline bool tbatch_resident(const D &) { return false; }
static inline bool tbatch_resident(const rhj_join_fold_desc &q) { return g_fold_resident && fold_resident_rule(q.nR, q.nS, q.nvalues); }
template <class D> static inline size_t tbatch_resident_lds(const D &) { return 0; }
static inline size_t tbatch_resident_lds(const rhj_join_fold_desc &q) { return fold_lds_bytes(q.nR, q.nS, q.nvalues); }
// a group of fold items' resident launch, if it has any: `res` their indices among the descriptors dd, `lds` the largest's bytes
static void tbatch_launch_resident(const JoinFoldDesc *dd, const uint32_t *d_res, uint32_t nres, size_t lds, size_t ni)
{
    if (nres) {
        RHJ_LAUNCH(k_fold_lds, dim3(nres), dim3(256), lds, g.stream, dd, d_res);
        ++g_resident_info.resident_launches;
    }
    if (g_fold_resident) { g_resident_info.resident_items += nres; g_resident_info.table_items += (uint32_t)(ni - nres); }
}
template <class Dev> static void tbatch_launch_resident(const Dev *, const uint32_t *, uint32_t, size_t, size_t) {}
// The same for the folds on tuple keys (rhj_fold_keys_lds.hip.h), under a switch of their own,
// g_fold_resident_keys: an item that fold_keys_resident_rule names has no table in the arena, no tile in the three launches and
// path 19, and a chunk's such items are ONE k_foldk_lds or k_foldn_lds launch.  g_resident_keys_info counts for the two tuple-key
// batches what g_resident_info counts for the batch on one key, and is reset where it is; all zero with the switch off.
rhj_table_batch_resident_info g_resident_keys_info = {};
static inline bool tbatch_resident(const rhj_join_foldk_desc &q) { return g_fold_resident_keys && fold_keys_resident_rule(q.nR, q.nS, q.nvalues); }
static inline bool tbatch_resident(const rhj_join_foldn_desc &q) { return g_fold_resident_keys && fold_keys_resident_rule(q.nR, q.nS, q.nvalues); }
static inline size_t tbatch_resident_lds(const rhj_join_foldk_desc &q) { return fold_keys_lds_bytes(q.nR, q.nS, q.nvalues); }
static inline size_t tbatch_resident_lds(const rhj_join_foldn_desc &q) { return fold_keys_lds_bytes(q.nR, q.nS, q.nvalues); }
static inline void tbatch_resident_keys_count(uint32_t nres, size_t ni)
{
    g_resident_keys_info.resident_launches += nres != 0;
    if (g_fold_resident_keys) { g_resident_keys_info.resident_items += nres; g_resident_keys_info.table_items += (uint32_t)(ni - nres); }
}
static void tbatch_launch_resident(const JoinFoldKDesc *dd, const uint32_t *d_res, uint32_t nres, size_t lds, size_t ni)
{
    if (nres) RHJ_LAUNCH(k_foldk_lds, dim3(nres), dim3(256), lds, g.stream, dd, d_res);
    tbatch_resident_keys_count(nres, ni);
}
static void tbatch_launch_resident(const JoinFoldNDesc *dd, const uint32_t *d_res, uint32_t nres, size_t lds, size_t ni)
{
    if (nres) RHJ_LAUNCH(k_foldn_lds, dim3(nres), dim3(256), lds, g.stream, dd, d_res);
    tbatch_resident_keys_count(nres, ni);
}

static bool tbatch_valid(const rhj_join_sum_desc &q)
{
    if (!tbatch_sides_valid(q) || q.nterms < 0 || q.nterms > RHJ_JOIN_SUM_MAX_TERMS) return false;
    for (int t = 0; t < q.nterms; ++t)
        if (q.terms[t].side < 0 || q.terms[t].side > 1 || !q.terms[t].d_col) return false;
    return true;
}
static bool tbatch_valid(const rhj_join_fold_desc &q)
{
    if (!tbatch_sides_valid(q) || q.nvalues < 0 || q.nvalues > RHJ_FOLD_MAX_VALUES || q.nouts < 0 || q.nouts > RHJ_FOLD_MAX_OUTS) return false;
    for (int o = 0; o < q.nouts; ++o)
        if (q.outs[o].value < 0 || q.outs[o].value >= q.nvalues) return false;
    return true;
}
// the fold batch's rule on tuple keys: 1..RHJ_FOLD_MAX_KEYS key columns, the first nkeys of a side with rows all given (a word's
// row-id vector may always be NULL, so the two tuple-key descriptors have one rule)
template <class D>
static bool tbatch_valid_tuple(const D &q)
{
    if (q.nkeys < 1 || q.nkeys > RHJ_FOLD_MAX_KEYS || q.nR >= JSUM_MAX_ROWS || q.nS >= JSUM_MAX_ROWS) return false;
    for (int t = 0; t < q.nkeys; ++t)
        if ((q.nR && !q.d_colR[t]) || (q.nS && !q.d_colS[t])) return false;
    if (q.nvalues < 0 || q.nvalues > RHJ_FOLD_MAX_VALUES || q.nouts < 0 || q.nouts > RHJ_FOLD_MAX_OUTS) return false;
    for (int o = 0; o < q.nouts; ++o)
        if (q.outs[o].value < 0 || q.outs[o].value >= q.nvalues) return false;
    return true;
}
static bool tbatch_valid(const rhj_join_foldk_desc &q) { return tbatch_valid_tuple(q); }
static bool tbatch_valid(const rhj_join_foldn_desc &q) { return tbatch_valid_tuple(q); }

static void tbatch_zero(rhj_join_sum_desc &q) { q.matches = 0; for (int t = 0; t < q.nterms; ++t) q.terms[t].sum = 0; }
static void tbatch_zero(rhj_join_fold_desc &q) { for (int o = 0; o < q.nouts; ++o) q.outs[o].total = 0; }
static void tbatch_zero(rhj_join_foldk_desc &q) { for (int o = 0; o < q.nouts; ++o) q.outs[o].total = 0; }
static void tbatch_zero(rhj_join_foldn_desc &q) { for (int o = 0; o < q.nouts; ++o) q.outs[o].total = 0; }

static inline uint64_t tbatch_table_bytes(const rhj_join_sum_desc &q) { return tbatch_slots(q) * JSUM_SLOT_BYTES; }
static inline uint64_t tbatch_table_bytes(const rhj_join_fold_desc &q) { return tbatch_resident(q) ? 0 : tbatch_slots(q) * (uint64_t)(1 + q.nvalues) * 8; }    // (a resident item's table is in LDS)
static inline uint64_t tbatch_table_bytes(const rhj_join_foldk_desc &q) { return tbatch_resident(q) ? 0 : tbatch_slots(q) * (uint64_t)(1 + q.nvalues) * 8; }
static inline uint64_t tbatch_table_bytes(const rhj_join_foldn_desc &q) { return tbatch_resident(q) ? 0 : tbatch_slots(q) * (uint64_t)(1 + q.nvalues) * 8; }

// the fields both device descriptors have
template <class D, class Dev>
static void tbatch_common(const D &q, unsigned long long *table, unsigned long long *words, Dev &d)
{
    memset((void *)&d, 0, sizeof(d));
    d.col[0] = q.d_colR; d.sel[0] = q.d_selR; d.n[0] = q.nR;
    d.col[1] = q.d_colS; d.sel[1] = q.d_selS; d.n[1] = q.nS;
    d.build = jsum_build_side(q.nR, q.nS);
    d.log2_slots = jsum_log2_slots(d.n[d.build]);
    d.table = table; d.words = words;
    d.combine = g_fold_combine;
}

// fills d and adds the item's tiles to the three launches' counts: the build side's, the other side's, both sides'
static void tbatch_fill(const rhj_join_sum_desc &q, unsigned long long *table, unsigned long long *words, JoinSumDesc &d, uint32_t (&t)[3])
{
    tbatch_common(q, table, words, d);
    d.tilesR = (uint32_t)jsum_tiles(q.nR);
    d.nterms = q.nterms;
    for (int k = 0; k < q.nterms; ++k) { d.t[k].src = q.terms[k].d_src; d.t[k].col = q.terms[k].d_col; d.t[k].side = q.terms[k].side; }
    t[0] += (uint32_t)jsum_tiles(d.n[d.build]); t[1] += (uint32_t)jsum_tiles(d.n[d.build ^ 1]); t[2] += (uint32_t)(jsum_tiles(q.nR) + jsum_tiles(q.nS));
}
// the values, the outputs and the tiles of a fold, on one key or on a tuple: the claim launch's (R's where R builds), the add
// launch's (S's), the apply launch's (R's)
template <class D, class Dev>
static void tbatch_fill_fold(const D &q, Dev &d, uint32_t (&t)[3])
{
    d.slot_words = (uint32_t)(1 + q.nvalues);
    d.nvalues = q.nvalues; d.nouts = q.nouts;
    for (int c = 0; c < q.nvalues; ++c) d.v[c] = FoldFactor{q.values[c].d_w, q.values[c].d_src, q.values[c].d_col};
    for (int o = 0; o < q.nouts; ++o) {
        d.o[o].p = FoldFactor{q.outs[o].p.d_w, q.outs[o].p.d_src, q.outs[o].p.d_col};
        d.o[o].out = q.outs[o].d_out; d.o[o].value = q.outs[o].value;
    }
    if (d.build == 0) t[0] += (uint32_t)jsum_tiles(q.nR);               // (an item whose S builds has no tile there: fbatch_find passes over it)
    t[1] += (uint32_t)jsum_tiles(q.nS); t[2] += (uint32_t)jsum_tiles(q.nR);
}
static void tbatch_fill(const rhj_join_fold_desc &q, unsigned long long *table, unsigned long long *words, JoinFoldDesc &d, uint32_t (&t)[3])
{
    tbatch_common(q, table, words, d);
    if (tbatch_resident(q)) {                            // no table in the arena and no tile in the three launches: k_fold_lds takes the item
        uint32_t none[3] = {0, 0, 0};
        d.table = nullptr;
        tbatch_fill_fold(q, d, none);
        return;
    }
    tbatch_fill_fold(q, d, t);
}
static void tbatch_fill(const rhj_join_foldk_desc &q, unsigned long long *table, unsigned long long *words, JoinFoldKDesc &d, uint32_t (&t)[3])
{
    memset((void *)&d, 0, sizeof(d));
    for (int k = 0; k < q.nkeys; ++k) { d.col[0][k] = q.d_colR[k]; d.col[1][k] = q.d_colS[k]; }
    d.sel[0] = q.d_selR; d.n[0] = q.nR;
    d.sel[1] = q.d_selS; d.n[1] = q.nS;
    d.build = jsum_build_side(q.nR, q.nS);
    d.log2_slots = jsum_log2_slots(d.n[d.build]);
    d.table = table; d.words = words;
    d.nkeys = q.nkeys;
    d.combine = g_fold_combine;
    if (tbatch_resident(q)) {                            // no table in the arena and no tile in the three launches: the LDS kernel takes the item
        uint32_t none[3] = {0, 0, 0};
        d.table = nullptr;
        tbatch_fill_fold(q, d, none);
        return;
    }
    tbatch_fill_fold(q, d, t);
}
static void tbatch_fill(const rhj_join_foldn_desc &q, unsigned long long *table, unsigned long long *words, JoinFoldNDesc &d, uint32_t (&t)[3])
{
    memset((void *)&d, 0, sizeof(d));
    for (int k = 0; k < q.nkeys; ++k) {                  // (a word beyond nkeys keeps no pointer: the kernels test nkeys first)
        d.col[0][k] = q.d_colR[k]; d.sel[0][k] = q.d_selR[k];
        d.col[1][k] = q.d_colS[k]; d.sel[1][k] = q.d_selS[k];
    }
    d.n[0] = q.nR; d.n[1] = q.nS;
    d.build = jsum_build_side(q.nR, q.nS);
    d.log2_slots = jsum_log2_slots(d.n[d.build]);
    d.table = table; d.words = words;
    d.nkeys = q.nkeys;
    d.combine = g_fold_combine;
    if (tbatch_resident(q)) {                            // no table in the arena and no tile in the three launches: the LDS kernel takes the item
        uint32_t none[3] = {0, 0, 0};
        d.table = nullptr;
        tbatch_fill_fold(q, d, none);
        return;
    }
    tbatch_fill_fold(q, d, t);
}

static void tbatch_launch(const rhj_join_sum_desc &, const JoinSumDesc *dd, uint32_t ni, uint32_t *const (&ts)[3], const uint32_t (&t)[3])
{
    RHJ_LAUNCH(k_jsum_insert, dim3(t[0]), dim3(256), combine_lds_bytes(false), g.stream, dd, ts[0], ni);
    RHJ_LAUNCH(k_jsum_count, dim3(t[1]), dim3(256), combine_lds_bytes(false), g.stream, dd, ts[1], ni);
    RHJ_LAUNCH(k_jsum_sum, dim3(t[2]), dim3(256), 0, g.stream, dd, ts[2], ni);
}
static void tbatch_launch(const rhj_join_fold_desc &, const JoinFoldDesc *dd, uint32_t ni, uint32_t *const (&ts)[3], const uint32_t (&t)[3])
{
    if (t[0]) RHJ_LAUNCH(k_fold_claim, dim3(t[0]), dim3(256), 0, g.stream, dd, ts[0], ni);
    RHJ_LAUNCH(k_fold_add, dim3(t[1]), dim3(256), combine_lds_bytes(true), g.stream, dd, ts[1], ni);
    RHJ_LAUNCH(k_fold_apply, dim3(t[2]), dim3(256), 0, g.stream, dd, ts[2], ni);
}
static void tbatch_launch(const rhj_join_foldk_desc &, const JoinFoldKDesc *dd, uint32_t ni, uint32_t *const (&ts)[3], const uint32_t (&t)[3])
{
    if (t[0]) RHJ_LAUNCH(k_foldk_claim, dim3(t[0]), dim3(256), 0, g.stream, dd, ts[0], ni);
    RHJ_LAUNCH(k_foldk_add, dim3(t[1]), dim3(256), combine_lds_bytes(true), g.stream, dd, ts[1], ni);
    RHJ_LAUNCH(k_foldk_apply, dim3(t[2]), dim3(256), 0, g.stream, dd, ts[2], ni);
}
static void tbatch_launch(const rhj_join_foldn_desc &, const JoinFoldNDesc *dd, uint32_t ni, uint32_t *const (&ts)[3], const uint32_t (&t)[3])
{
    if (t[0]) RHJ_LAUNCH(k_foldn_claim, dim3(t[0]), dim3(256), 0, g.stream, dd, ts[0], ni);
    RHJ_LAUNCH(k_foldn_add, dim3(t[1]), dim3(256), combine_lds_bytes(true), g.stream, dd, ts[1], ni);
    RHJ_LAUNCH(k_foldn_apply, dim3(t[2]), dim3(256), 0, g.stream, dd, ts[2], ni);
}

static void tbatch_take(rhj_join_sum_desc &q, const unsigned long long *h)
{
    q.matches = h[JSUM_W_MATCHES];
    for (int t = 0; t < q.nterms; ++t) q.terms[t].sum = h[JSUM_W_SUM + t];
}
static void tbatch_take(rhj_join_fold_desc &q, const unsigned long long *h) { for (int o = 0; o < q.nouts; ++o) q.outs[o].total = h[FOLD_W_TOTAL + o]; }
static void tbatch_take(rhj_join_foldk_desc &q, const unsigned long long *h) { for (int o = 0; o < q.nouts; ++o) q.outs[o].total = h[o]; }
static void tbatch_take(rhj_join_foldn_desc &q, const unsigned long long *h) { for (int o = 0; o < q.nouts; ++o) q.outs[o].total = h[o]; }

static inline int tbatch_path(const rhj_join_sum_desc &) { return PATH_BATCH_JOIN_SUM; }
static inline int tbatch_path(const rhj_join_fold_desc &) { return PATH_BATCH_JOIN_FOLD; }
static inline int tbatch_path(const rhj_join_foldk_desc &) { return PATH_BATCH_JOIN_FOLDK; }
static inline int tbatch_path(const rhj_join_foldn_desc &) { return PATH_BATCH_JOIN_FOLDN; }
// what an item reports; tbatch_path is what the call does (rhj_last_stats().reserved)
static inline int tbatch_resident_path(const rhj_join_fold_desc &) { return PATH_BATCH_JOIN_FOLD_LDS; }
template <class D> static inline int tbatch_resident_path(const D &) { return PATH_BATCH_JOIN_FOLDK_LDS; }             // (the two on tuple keys; the join sums are never resident)
template <class D> static inline int tbatch_item_path(const D &q) { return tbatch_resident(q) ? tbatch_resident_path(q) : tbatch_path(q); }
static inline const char *tbatch_noun(const rhj_join_sum_desc &) { return "join sums"; }
static inline const char *tbatch_noun(const rhj_join_fold_desc &) { return "join folds"; }
static inline const char *tbatch_noun(const rhj_join_foldk_desc &) { return "join folds on tuple keys"; }
static inline const char *tbatch_noun(const rhj_join_foldn_desc &) { return "join folds on the keys of nodes"; }
static inline uint64_t tbatch_matches(const rhj_join_sum_desc &q) { return q.matches; }
static inline uint64_t tbatch_matches(const rhj_join_fold_desc &) { return 0; }           // (the folds' statistics have no matches)
static inline uint64_t tbatch_matches(const rhj_join_foldk_desc &) { return 0; }
static inline uint64_t tbatch_matches(const rhj_join_foldn_desc &) { return 0; }

// One chunk: items[which[lo, hi)], every one valid and with two non-empty sides; their tables take `bytes` together.
template <class D>
static int tbatch_chunk(D *items, const uint64_t *which, size_t lo, size_t hi, uint64_t bytes)
{
    using Dev = typename tbatch_dev<D>::type;
    constexpr size_t WORDS = tbatch_dev<D>::words;
    static_assert(sizeof(Dev) % 8 == 0, "the tile starts follow the descriptors without padding");
    static_assert(JSUM_EMPTY == 0, "the tables are cleared with a memset of zeros");
    const size_t ni = hi - lo;
    if (batch_arena(g.jsum_arena, (size_t)bytes, JSUM_ARENA_BYTES)) return -1;
    Block blk;
    unsigned long long *back, *words, *d_words; Dev *hd, *dd;
    uint32_t *ts[3], *d_ts[3], *res, *d_res;
    size_t nres = 0, res_lds = 0;                         // the resident items (rhj_set_fold_resident) and the largest's LDS bytes
    for (size_t k = 0; k < ni; ++k) nres += tbatch_resident(items[which[lo + k]]);
    const auto pieces = [&](Block &b) {
        b.back(back, ni * WORDS);
        b.up(hd, dd, ni); b.up(ts[0], d_ts[0], ni + 1); b.up(ts[1], d_ts[1], ni + 1); b.up(ts[2], d_ts[2], ni + 1); b.up(res, d_res, nres); b.up(words, d_words, ni * WORDS);
    };
    if (batch_block(blk, pieces)) return -1;
    memset(words, 0, ni * WORDS * 8);
    uint32_t t[3] = {0, 0, 0};
    size_t at = 0, r = 0;
    for (size_t k = 0; k < ni; ++k) {
        const D &q = items[which[lo + k]];
        ts[0][k] = t[0]; ts[1][k] = t[1]; ts[2][k] = t[2];
        Dev d;
        tbatch_fill(q, (unsigned long long *)((char *)g.jsum_arena.p + at), d_words + k * WORDS, d, t);
        memcpy((void *)&hd[k], (const void *)&d, sizeof(d));
        at += (size_t)tbatch_table_bytes(q);
        if (tbatch_resident(q)) {
            res[r++] = (uint32_t)k;
            res_lds = std::max(res_lds, tbatch_resident_lds(q));
        }
    }
    ts[0][ni] = t[0]; ts[1][ni] = t[1]; ts[2][ni] = t[2];
    if (at != (size_t)bytes || at > g.jsum_arena.cap) { fprintf(stderr, "rhj: the tables of a chunk of %s were placed beyond its arena\n", tbatch_noun(items[which[lo]])); return -1; }
    if (batch_upload(blk, hd, blk.host_end())) return -1;
    if (nres < ni) {                                      // (always, with the resident switch off)
        HIP_TRY(hipMemsetAsync(g.jsum_arena.p, 0, at, g.stream));     // every key word JSUM_EMPTY (0), every count and every A_c 0
        tbatch_launch(items[which[lo]], dd, (uint32_t)ni, d_ts, t);
    }
    tbatch_launch_resident(dd, d_res, (uint32_t)nres, res_lds, ni);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(back, d_words, ni * WORDS * 8, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    for (size_t k = 0; k < ni; ++k) {
        D &q = items[which[lo + k]];
        tbatch_take(q, back + k * WORDS);
        q.path = tbatch_item_path(q);
    }
    tbatch_combine_take<D>(t, back, ni);                 // (a resident item has no tile in t and its two counters are 0)
    return 0;
}

template <class D>
static int table_batch(D *items, uint64_t n)
{
    if (n == 0) return 0;
    bool timed = false;
    const auto reset = [](D &q) { q.rc = 0; q.path = 0; return tbatch_valid(q); };      // (no result is written in a batch that is refused)
    if (const int rc = batch_open(items, n, reset, timed)) return rc;
    std::vector<uint64_t> which;
    rhj_stats st = {};
    for (uint64_t i = 0; i < n; ++i) {
        D &q = items[i];
        tbatch_zero(q);
        st.n_r += q.nR; st.n_s += q.nS;
        if (q.nR && q.nS) which.push_back(i);             // an empty side: no pair, nothing to launch, no d_out touched
    }
    const auto tiles = [&](size_t k, uint64_t t) { return t + jsum_tiles(items[which[k]].nR) + jsum_tiles(items[which[k]].nS); };   // (one item never has more than the limit: tbatch_sides_valid)
    const auto group = [&](size_t lo, size_t hi, uint64_t) {
        return batch_cut(hi - lo, hi - lo, JSUM_ARENA_BYTES, [&](size_t k, uint64_t bytes) { return bytes + tbatch_table_bytes(items[which[lo + k]]); },
                         [&](size_t a, size_t b, uint64_t bytes) { return tbatch_chunk(items, which.data() + lo, a, b, bytes); });
    };
    if (batch_cut(which.size(), JSUM_MAX_ITEMS, JSUM_MAX_TILES, tiles, group)) return -1;
    st.units = which.size();
    for (uint64_t i = 0; i < n; ++i) st.matches += tbatch_matches(items[i]);
    st.reserved = tbatch_path(items[0]);
    return batch_close(timed, st);
}

// ---- batched folds with no child (rhj_fold_self_batch.hip.h) ---------------------------------------------------------------------
// rhj_fold_self_batch_device (path 15): every item with rows runs in the one launch of its chunk; there is no table, no arena and
// no run-alone class.  A chunk holds at most FSELF_MAX_ITEMS items and FSELF_MAX_TILES tiles (conditions, as the apply batch's),
// and a batch beyond either is cut in call order by batch_cut.  A chunk is one upload, one launch, one copy of its accumulator
// words and one stream synchronisation; the uploaded block is
//   [descriptors][items + 1 tile starts][the items' accumulator words, zero]
constexpr size_t FSELF_MAX_ITEMS = 4096;
constexpr uint64_t FSELF_MAX_TILES = 1ull << 24;

static bool fself_valid(const rhj_fold_self_desc &q)
{
    if (q.nterms < 0 || q.nterms > RHJ_FOLD_SELF_MAX_TERMS || q.nouts < 0 || q.nouts > RHJ_FOLD_MAX_OUTS || q.n >= JSUM_MAX_ROWS) return false;
    for (int t = 0; t < q.nterms; ++t)
        if (q.n && (!q.terms[t].d_colA || !q.terms[t].d_colB)) return false;
    return true;
}

// One chunk: items[which[lo, hi)], every one valid and of at least one row.
static int fself_chunk(rhj_fold_self_desc *items, const std::vector<uint64_t> &which, size_t lo, size_t hi)
{
    constexpr size_t WORDS = FOLD_SELF_WORDS;
    static_assert(sizeof(FoldSelfDesc) % 8 == 0, "the words' padding is that of the tile starts alone");
    const size_t ni = hi - lo;
    Block blk;
    unsigned long long *back, *words, *d_words; FoldSelfDesc *hd, *dd; uint32_t *tile_start, *d_tile_start;
    if (batch_block(blk, [&](Block &b) { b.back(back, ni * WORDS); b.up(hd, dd, ni); b.up(tile_start, d_tile_start, ni + 1); b.up(words, d_words, ni * WORDS); })) return -1;
    memset(words, 0, ni * WORDS * 8);
    uint32_t tiles = 0;
    for (size_t k = 0; k < ni; ++k) {
        const rhj_fold_self_desc &q = items[which[lo + k]];
        FoldSelfDesc d;
        memset((void *)&d, 0, sizeof(d));
        d.n = q.n; d.words = d_words + k * WORDS; d.nterms = q.nterms; d.nouts = q.nouts;
        for (int t = 0; t < q.nterms; ++t) {
            d.t[t].col[0] = q.terms[t].d_colA; d.t[t].sel[0] = q.terms[t].d_selA;
            d.t[t].col[1] = q.terms[t].d_colB; d.t[t].sel[1] = q.terms[t].d_selB;
        }
        for (int o = 0; o < q.nouts; ++o) {
            d.o[o].p = FoldFactor{q.outs[o].p.d_w, q.outs[o].p.d_src, q.outs[o].p.d_col};
            d.o[o].out = q.outs[o].d_out;
        }
        memcpy((void *)&hd[k], (const void *)&d, sizeof(d));
        tile_start[k] = tiles;
        tiles += (uint32_t)jsum_tiles(q.n);
    }
    tile_start[ni] = tiles;
    if (batch_upload(blk, hd, blk.host_end())) return -1;
    RHJ_LAUNCH(k_fold_self, dim3(tiles), dim3(256), 0, g.stream, dd, d_tile_start, (uint32_t)ni);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(back, d_words, ni * WORDS * 8, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    for (size_t k = 0; k < ni; ++k) {
        rhj_fold_self_desc &q = items[which[lo + k]];
        for (int o = 0; o < q.nouts; ++o) q.outs[o].total = back[k * WORDS + (size_t)o];
        q.path = PATH_BATCH_FOLD_SELF;
    }
    return 0;
}

static int fold_self_batch(rhj_fold_self_desc *items, uint64_t n)
{
    if (n == 0) return 0;
    bool timed = false;
    const auto reset = [](rhj_fold_self_desc &q) { q.rc = 0; q.path = 0; return fself_valid(q); };      // (no total is written in a batch that is refused)
    if (const int rc = batch_open(items, n, reset, timed)) return rc;
    std::vector<uint64_t> which;
    rhj_stats st = {};
    for (uint64_t i = 0; i < n; ++i) {
        rhj_fold_self_desc &q = items[i];
        for (int o = 0; o < q.nouts; ++o) q.outs[o].total = 0;
        st.n_r += q.n;
        if (q.n) which.push_back(i);                      // an empty item: nothing to launch, no d_out touched
    }
    const auto tiles = [&](size_t k, uint64_t t) { return t + jsum_tiles(items[which[k]].n); };   // (one item never has more than the limit: fself_valid)
    if (batch_cut(which.size(), FSELF_MAX_ITEMS, FSELF_MAX_TILES, tiles,
                  [&](size_t lo, size_t hi, uint64_t) { return fself_chunk(items, which, lo, hi); })) return -1;
    st.units = which.size();
    st.reserved = PATH_BATCH_FOLD_SELF;
    return batch_close(timed, st);
}

// ---- batched folds with no child and constant predicates (rhj_fold_pred_batch.hip.h) ---------------------------------------------
// rhj_fold_pred_batch_device (path 17): fold_self_batch's frame, limits and block over rhj_fold_pred_desc.  fpred_fill is also
// what a fold program (query_one_wait below) fills its pred descriptors with.
static bool fpred_valid(const rhj_fold_pred_desc &q)
{
    if (q.nconst < 0 || q.nconst > RHJ_FILTER_MAX_TERMS || q.neq < 0 || q.neq > RHJ_FOLD_SELF_MAX_TERMS || q.nouts < 0 || q.nouts > RHJ_FOLD_MAX_OUTS || q.n >= JSUM_MAX_ROWS) return false;
    for (int c = 0; c < q.nconst; ++c)
        if (op_code(q.consts[c].op) < 0 || (q.n && !q.consts[c].d_col)) return false;
    for (int t = 0; t < q.neq; ++t)
        if (q.n && (!q.eqs[t].d_colA || !q.eqs[t].d_colB)) return false;
    return true;
}

static void fpred_fill(const rhj_fold_pred_desc &q, unsigned long long *words, FoldPredDesc &d)
{
    memset((void *)&d, 0, sizeof(d));
    d.n = q.n; d.words = words; d.nconst = q.nconst; d.neq = q.neq; d.nouts = q.nouts;
    for (int c = 0; c < q.nconst; ++c) {
        d.c[c].col = q.consts[c].d_col; d.c[c].sel = q.consts[c].d_sel;
        d.c[c].value = q.consts[c].value; d.c[c].op = op_code(q.consts[c].op);
    }
    for (int t = 0; t < q.neq; ++t) {
        d.t[t].col[0] = q.eqs[t].d_colA; d.t[t].sel[0] = q.eqs[t].d_selA;
        d.t[t].col[1] = q.eqs[t].d_colB; d.t[t].sel[1] = q.eqs[t].d_selB;
    }
    for (int o = 0; o < q.nouts; ++o) {
        d.o[o].p = FoldFactor{q.outs[o].p.d_w, q.outs[o].p.d_src, q.outs[o].p.d_col};
        d.o[o].out = q.outs[o].d_out;
    }
}

// One chunk: items[which[lo, hi)], every one valid and of at least one row.
static int fpred_chunk(rhj_fold_pred_desc *items, const std::vector<uint64_t> &which, size_t lo, size_t hi)
{
    constexpr size_t WORDS = FOLD_PRED_WORDS;
    static_assert(sizeof(FoldPredDesc) % 8 == 0, "the words' padding is that of the tile starts alone");
    const size_t ni = hi - lo;
    Block blk;
    unsigned long long *back, *words, *d_words; FoldPredDesc *hd, *dd; uint32_t *tile_start, *d_tile_start;
    if (batch_block(blk, [&](Block &b) { b.back(back, ni * WORDS); b.up(hd, dd, ni); b.up(tile_start, d_tile_start, ni + 1); b.up(words, d_words, ni * WORDS); })) return -1;
    memset(words, 0, ni * WORDS * 8);
    uint32_t tiles = 0;
    for (size_t k = 0; k < ni; ++k) {
        const rhj_fold_pred_desc &q = items[which[lo + k]];
        FoldPredDesc d;
        fpred_fill(q, d_words + k * WORDS, d);
        memcpy((void *)&hd[k], (const void *)&d, sizeof(d));
        tile_start[k] = tiles;
        tiles += (uint32_t)jsum_tiles(q.n);
    }
    tile_start[ni] = tiles;
    if (batch_upload(blk, hd, blk.host_end())) return -1;
    RHJ_LAUNCH(k_fold_pred, dim3(tiles), dim3(256), 0, g.stream, dd, d_tile_start, (uint32_t)ni);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(back, d_words, ni * WORDS * 8, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    for (size_t k = 0; k < ni; ++k) {
        rhj_fold_pred_desc &q = items[which[lo + k]];
        for (int o = 0; o < q.nouts; ++o) q.outs[o].total = back[k * WORDS + (size_t)o];
        q.path = PATH_BATCH_FOLD_PRED;
    }
    return 0;
}

static int fold_pred_batch(rhj_fold_pred_desc *items, uint64_t n)
{
    if (n == 0) return 0;
    bool timed = false;
    const auto reset = [](rhj_fold_pred_desc &q) { q.rc = 0; q.path = 0; return fpred_valid(q); };      // (no total is written in a batch that is refused)
    if (const int rc = batch_open(items, n, reset, timed)) return rc;
    std::vector<uint64_t> which;
    rhj_stats st = {};
    for (uint64_t i = 0; i < n; ++i) {
        rhj_fold_pred_desc &q = items[i];
        for (int o = 0; o < q.nouts; ++o) q.outs[o].total = 0;
        st.n_r += q.n;
        if (q.n) which.push_back(i);                      // an empty item: nothing to launch, no d_out touched
    }
    const auto tiles = [&](size_t k, uint64_t t) { return t + jsum_tiles(items[which[k]].n); };   // (one item never has more than the limit: fpred_valid)
    if (batch_cut(which.size(), FSELF_MAX_ITEMS, FSELF_MAX_TILES, tiles,
                  [&](size_t lo, size_t hi, uint64_t) { return fpred_chunk(items, which, lo, hi); })) return -1;
    st.units = which.size();
    st.reserved = PATH_BATCH_FOLD_PRED;
    return batch_close(timed, st);
}

// ---- a batch of queries, level by level (include/rhj_inter.h) ------------------------------------------------------------------
// rhj_query_batch_device drives the four batches above: one filter batch, then per join level at most one batch of two-column
// equalities, at most two batches of joins on columns (the second for the joins whose fan-out passed max(nR, nS)) and one
// apply batch.  Host code only.  What a level reads and what it writes never share a buffer:
//   g_qb.filt       the filters' hit lists: a binding's vector until a join rebuilds it, possibly levels later
//   g_qb.idx        the level's index lists (equalities' hits, joins' pairs); dead once the level's apply batch has run
//   g_qb.idx2       the pairs of the joins run a second time (the first call's lists of the others are still needed)
//   g_qb.level[l]   the vectors level l rebuilds: read by any later level, so every level has its own
//   g_qb.fold[r]    the weight and view vectors fold round r writes: read by any later round, so every round has its own
//   g_qb.self       the first weight vectors, written by the fold route's one rhj_fold_self_batch_device call: read by any round
//   g_qb.prog       every weight and view vector of one fold program (the one-wait route): a piece each, none reused inside it
// They belong to the library's own context (the entry point runs on no other), grow and stay, and go with rhj_release().
struct QueryWorkspace {
    Buf              filt, idx, idx2, self, prog;
    std::vector<Buf> level, fold;
    hipEvent_t       ev[2] = {};     // the whole call (its inner batches run untimed); created by the first timed call
} g_qb;

static void query_release()
{
    for (Buf *b : {&g_qb.filt, &g_qb.idx, &g_qb.idx2, &g_qb.self, &g_qb.prog}) { if (b->p) (void)hipFree(b->p); *b = Buf{}; }
    for (Buf &b : g_qb.level) if (b.p) (void)hipFree(b.p);
    g_qb.level.clear();
    for (Buf &b : g_qb.fold) if (b.p) (void)hipFree(b.p);
    g_qb.fold.clear();
}

// query_check is the validation of one query but for its last rule (all bindings in one node): njoins or -3, and node[b] the
// node of binding b after the last predicate (two merged nodes are the A side's).
static int query_check(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, int *kinds, int *node)
{
    if (!q || q->nrels < 1 || q->nrels > RHJ_QUERY_MAX_RELS || !q->rels || q->nviews < 1 || q->nviews > RHJ_QUERY_MAX_VIEWS || !q->views) return -3;
    if (q->nfilters < 0 || q->njoins < 0 || (q->nfilters && !q->filters) || (q->njoins && !q->joins)) return -3;
    for (int b = 0; b < q->nrels; ++b) {
        const int r = q->rels[b];
        if (r < 0 || r >= nrel || (rels && rels[r].num_tuples && rels[r].num_columns && !rels[r].d_columns)) return -3;
    }
    const auto col_ok = [&](int b, int c) {
        if (b < 0 || b >= q->nrels || c < 0) return false;
        if (!rels) return true;
        const rhj_device_relation &R = rels[q->rels[b]];
        return (uint64_t)c < R.num_columns && (R.num_tuples == 0 || R.d_columns[c] != nullptr);
    };
    int per_binding[RHJ_QUERY_MAX_RELS] = {};
    for (int f = 0; f < q->nfilters; ++f) {
        const rhj_query_filter &p = q->filters[f];
        if (!col_ok(p.rel, p.col) || op_code(p.op) < 0 || ++per_binding[p.rel] > RHJ_FILTER_MAX_TERMS) return -3;
    }
    for (int b = 0; b < q->nrels; ++b) node[b] = b;
    for (int l = 0; l < q->njoins; ++l) {
        const rhj_query_join &p = q->joins[l];
        if (!col_ok(p.relA, p.colA) || !col_ok(p.relB, p.colB)) return -3;
        const int na = node[p.relA], nb = node[p.relB];
        if (kinds) kinds[l] = na == nb;
        for (int x = 0; x < q->nrels; ++x) if (node[x] == nb) node[x] = na;      // the two nodes merge into A's
    }
    for (int v = 0; v < q->nviews; ++v) if (!col_ok(q->views[v].rel, q->views[v].col)) return -3;
    return q->njoins;
}

static int query_levels(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, int *kinds)
{
    int node[RHJ_QUERY_MAX_RELS];
    const int lv = query_check(q, nrel, rels, kinds, node);
    if (lv < 0) return -3;
    for (int b = 1; b < q->nrels; ++b) if (node[b] != node[0]) return -3;          // a cross product is not executed here (query_products below runs it as its components)
    return lv;
}

// The components of one query (rhj_query_components): query_check's nodes numbered 0, 1, ... in the order of their lowest binding.
static int query_components(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, int *comp)
{
    int node[RHJ_QUERY_MAX_RELS], id[RHJ_QUERY_MAX_RELS], k = 0;
    if (query_check(q, nrel, rels, nullptr, node) < 0) return -3;
    for (int b = 0; b < q->nrels; ++b) id[b] = -1;
    for (int b = 0; b < q->nrels; ++b) {
        if (id[node[b]] < 0) id[node[b]] = k++;
        if (comp) comp[b] = id[node[b]];
    }
    return k;
}

struct QueryState {
    const uint64_t *vec[RHJ_QUERY_MAX_RELS];              // binding -> its row-id vector; nullptr: the whole relation
    int             node[RHJ_QUERY_MAX_RELS];             // binding -> its node (two merged nodes are the A side's)
    uint64_t        rows[RHJ_QUERY_MAX_RELS];             // node -> its rows
    bool            alive;                                // neither finished nor empty
};

struct TwoNodes {                                         // the nodes a level's predicate joins, and a binding's place in them
    int na, nb;
    TwoNodes(const QueryState &s, const rhj_query_join &p) : na(s.node[p.relA]), nb(s.node[p.relB]) {}
    bool has(const QueryState &s, int x) const { return s.node[x] == na || s.node[x] == nb; }
    int side(const QueryState &s, int x) const { return s.node[x] == nb && na != nb; }     // the word of an index row
};

struct QueryBump {                                        // 16-byte aligned pieces of one buffer: who gets each (take), their addresses once it has its size (resolve)
    struct Piece { size_t item; int sub; size_t off; };
    size_t             at = 0;
    std::vector<Piece> pieces;
    void take(size_t item, int sub, uint64_t words) { pieces.push_back({item, sub, at}); at += (size_t)((words + 1) / 2 * 2) * 8; }
    template <class Set> int resolve(Buf &b, Set set) const
    {
        if (ensure(b, at)) return -1;
        for (const Piece &p : pieces) set(p.item, p.sub, (char *)b.p + p.off);
        return 0;
    }
};

struct QueryTimingOff {                                   // the inner batches record and wait for no events of their own
    int was;
    QueryTimingOff() : was(g.timing) { g.timing = 0; }
    ~QueryTimingOff() { g.timing = was; }
};

rhj_query_batch_info g_query_info = {};
rhj_query_batch_sum_info g_query_sum_info = {};
rhj_query_batch_fold_info g_query_fold_info = {};
rhj_query_batch_foldk_info g_query_foldk_info = {};
rhj_query_batch_fold_self_info g_query_fold_self_info = {};
rhj_query_batch_fold_nodes_info g_query_fold_nodes_info = {};
rhj_query_batch_one_wait_info g_query_one_wait_info = {};
rhj_query_batch_products_info g_query_products_info = {};
static void query_infos_clear()
{
    g_query_info = {}; g_query_sum_info = {}; g_query_fold_info = {}; g_query_foldk_info = {};
    g_query_fold_self_info = {}; g_query_fold_nodes_info = {}; g_query_one_wait_info = {}; g_query_products_info = {};
}

struct QueryRun {                                         // what the stages of one call share
    const rhj_device_relation      *rels;
    rhj_query_desc                 *queries;
    uint64_t                        n;
    std::vector<QueryState>         st;
    std::vector<char>               folds;                // a query that takes the fold route (empty: none does): 1, 2 when only rhj_set_query_fold_keys lets it, 3 when only rhj_set_query_fold_self does, 4 when it hands over from levels to folds over its nodes (rhj_set_query_fold_nodes)
    std::vector<char>               one_wait;             // a query that ran in a fold program with one wait (empty: none did): it is finished before the filters, and no stage below sees it
    std::vector<int>                park;                 // of a query with folds 4: the levels it runs before it is parked for the nodes' pass (empty: no such query)
    std::vector<uint64_t>           active, awho;         // of the level at hand: the queries that take part; an apply item's query
    std::vector<int>                kind;                 // of an active query's predicate: 0 a join, 1 an equality, 2 none (level 0 of a query without joins), 3 a last join taken as its sums ...
    std::vector<size_t>             where;                // ... and its descriptor in ed / jd / sd
    std::vector<rhj_eq2_desc>       ed;
    std::vector<rhj_join_cols_desc> jd;
    std::vector<rhj_apply_desc>     ad;
    std::vector<rhj_join_sum_desc>  sd;
    auto column(const rhj_query_desc &q, int b, int c) const { return rels[q.rels[b]].d_columns[c]; }
    bool finishes(uint64_t i, int l) const { return queries[i].njoins == 0 || l == queries[i].njoins - 1; }
    bool parked(uint64_t i, int l) const { return !park.empty() && park[i] && l >= park[i]; }        // its level prefix is over
};

// The filters of all queries: all of one binding are one conjunction, all of them over all queries one call.
static int query_filters(QueryRun &R)
{
    std::vector<rhj_filter_desc> fd;
    std::vector<std::pair<uint64_t, int>> fwho;           // (query, binding) of a descriptor
    QueryBump fb;
    for (uint64_t i = 0; i < R.n; ++i) {
        const rhj_query_desc &q = R.queries[i];
        QueryState &s = R.st[i];
        s.alive = R.one_wait.empty() || !R.one_wait[i];   // (a query of a fold program has its answer already)
        for (int b = 0; b < q.nrels; ++b) {
            s.vec[b] = nullptr; s.node[b] = b; s.rows[b] = R.rels[q.rels[b]].num_tuples;
            if (s.rows[b] == 0) s.alive = false;          // an empty relation: every result it takes part in is empty
        }
        if (!s.alive) continue;
        for (int b = 0; b < q.nrels; ++b) {
            rhj_filter_desc d = {};
            for (int f = 0; f < q.nfilters; ++f) {
                const rhj_query_filter &p = q.filters[f];
                if (p.rel != b) continue;
                rhj_filter_term &t = d.terms[d.nterms++];
                t.d_col = R.column(q, b, p.col); t.value = p.value; t.op = p.op;
            }
            if (d.nterms == 0) continue;                  // no filter: the binding stays its whole relation
            d.n = s.rows[b];
            fb.take(fd.size(), 0, d.n);
            fd.push_back(d); fwho.emplace_back(i, b);
        }
    }
    if (fd.empty()) return 0;
    if (fb.resolve(g_qb.filt, [&](size_t k, int, char *p) { fd[k].d_out = (uint64_t *)p; })) return -1;
    ++g_query_info.filter_calls;
    if (const int rc = filter_batch(fd.data(), fd.size())) return rc;     // (0 or an error)
    for (size_t k = 0; k < fd.size(); ++k) {
        QueryState &s = R.st[fwho[k].first];
        const int b = fwho[k].second;
        s.vec[b] = fd[k].d_out; s.rows[b] = fd[k].hits;
        if (fd[k].hits == 0) s.alive = false;             // a filter without a hit: rows = 0
    }
    return 0;
}

// The joins whose fan-out passed the guess, again: the counts are known now.
static int query_rerun_short(QueryRun &R)
{
    std::vector<rhj_join_cols_desc> jd2;
    std::vector<size_t> short_k;
    QueryBump rb;
    for (size_t k = 0; k < R.jd.size(); ++k) {
        if (R.jd[k].rc != 1) continue;
        rhj_join_cols_desc d = R.jd[k];
        d.out_capacity = d.matches;
        rb.take(jd2.size(), 0, 2 * d.out_capacity);
        short_k.push_back(k); jd2.push_back(d);
    }
    if (rb.resolve(g_qb.idx2, [&](size_t k, int, char *p) { jd2[k].d_out = (rhj_result_tuple *)p; })) return -1;
    ++g_query_info.join_reruns;
    const int rc = join_batch(jd2.data(), jd2.size());
    if (rc < 0) return rc;
    if (rc != 0) { fprintf(stderr, "rhj: a join run again with room for its count was short once more\n"); return -1; }
    for (size_t k = 0; k < jd2.size(); ++k) R.jd[short_k[k]] = jd2[k];
    return 0;
}

// Level l's predicates: at most one batch of two-column equalities (both bindings in one node) and one of joins on columns.
static int query_level_joins(QueryRun &R, int l)
{
    QueryBump ib;
    R.active.clear(); R.kind.clear(); R.where.clear(); R.ed.clear(); R.jd.clear(); R.ad.clear(); R.awho.clear(); R.sd.clear();   // the level before
    for (uint64_t i = 0; i < R.n; ++i) {
        const rhj_query_desc &q = R.queries[i];
        const QueryState &s = R.st[i];
        if (!s.alive || (q.njoins <= l && (l || q.njoins)) || R.parked(i, l)) continue;
        R.active.push_back(i);
        if (q.njoins == 0) { R.kind.push_back(2); R.where.push_back(0); continue; }     // no predicate at all: level 0 sums its views
        const rhj_query_join &p = q.joins[l];
        const TwoNodes two(s, p);
        const bool as_sums = g_query_sum_last && two.na != two.nb && R.finishes(i, l) && s.rows[two.na] < JSUM_MAX_ROWS && s.rows[two.nb] < JSUM_MAX_ROWS;
        R.kind.push_back(as_sums ? 3 : two.na == two.nb);
        if (as_sums) {                                    // the last join: its row count and view sums, no pairs
            rhj_join_sum_desc d = {};
            d.d_colR = R.column(q, p.relA, p.colA); d.d_selR = s.vec[p.relA]; d.nR = s.rows[two.na];
            d.d_colS = R.column(q, p.relB, p.colB); d.d_selS = s.vec[p.relB]; d.nS = s.rows[two.nb];
            for (int v = 0; v < q.nviews; ++v) {
                const int x = q.views[v].rel;
                rhj_join_sum_term &t = d.terms[d.nterms++];
                t.side = two.side(s, x); t.d_src = s.vec[x]; t.d_col = R.column(q, x, q.views[v].col);
            }
            R.where.push_back(R.sd.size()); R.sd.push_back(d);
        } else if (two.na == two.nb) {                           // the two-column equality over the node's rows
            rhj_eq2_desc d = {};
            d.d_colA = R.column(q, p.relA, p.colA); d.d_selA = s.vec[p.relA];
            d.d_colB = R.column(q, p.relB, p.colB); d.d_selB = s.vec[p.relB];
            d.n = s.rows[two.na];
            ib.take(R.ed.size(), 1, d.n);
            R.where.push_back(R.ed.size()); R.ed.push_back(d);
        } else {
            rhj_join_cols_desc d = {};
            d.d_colR = R.column(q, p.relA, p.colA); d.d_selR = s.vec[p.relA]; d.nR = s.rows[two.na];
            d.d_colS = R.column(q, p.relB, p.colB); d.d_selS = s.vec[p.relB]; d.nS = s.rows[two.nb];
            d.out_capacity = d.nR > d.nS ? d.nR : d.nS;
            ib.take(R.jd.size(), 0, 2 * d.out_capacity);
            R.where.push_back(R.jd.size()); R.jd.push_back(d);
        }
    }
    const auto set = [&](size_t k, int eq, char *p) { if (eq) R.ed[k].d_out = (uint64_t *)p; else R.jd[k].d_out = (rhj_result_tuple *)p; };
    if (ib.resolve(g_qb.idx, set)) return -1;
    if (!R.ed.empty()) {
        ++g_query_info.eq2_calls;
        if (const int rc = filter_batch(R.ed.data(), R.ed.size())) return rc;
    }
    if (!R.jd.empty()) {
        ++g_query_info.join_calls;
        const int rc = join_batch(R.jd.data(), R.jd.size());
        if (rc < 0) return rc;
        if (rc == 1) if (const int rc2 = query_rerun_short(R)) return rc2;
    }
    if (!R.sd.empty()) {
        ++g_query_sum_info.sum_calls;
        g_query_sum_info.sum_items += (uint32_t)R.sd.size();
        if (const int rc = table_batch(R.sd.data(), R.sd.size())) return rc;
    }
    return 0;
}

// Level l's apply batch: the queries that go on rebuild the vectors of the two nodes, those that finish sum their views.
static int query_level_apply(QueryRun &R, int l)
{
    QueryBump vb;
    size_t sum_items = 0;
    for (size_t a = 0; a < R.active.size(); ++a) {
        const uint64_t i = R.active[a];
        rhj_query_desc &q = R.queries[i];
        QueryState &s = R.st[i];
        if (R.kind[a] == 3) {                             // finished by the sum batch: no item (matches == 0: rows = 0, as an empty list)
            const rhj_join_sum_desc &d = R.sd[R.where[a]];
            for (int v = 0; v < q.nviews; ++v) q.sums[v] = d.terms[v].sum;
            q.rows = d.matches;
            s.alive = false;
            ++sum_items;
            continue;
        }
        const TwoNodes two(s, q.njoins ? q.joins[l] : rhj_query_join{});       // (no predicate: the one binding, side 0)
        rhj_apply_desc d = {};
        if (R.kind[a] == 2)      { d.n = s.rows[0]; d.idx_stride = 1; }        // the views through the binding's own vector
        else if (R.kind[a] == 1) { d.d_idx = R.ed[R.where[a]].d_out; d.n = R.ed[R.where[a]].hits; d.idx_stride = 1; }
        else                     { d.d_idx = (const uint64_t *)R.jd[R.where[a]].d_out; d.n = R.jd[R.where[a]].matches; d.idx_stride = 2; }
        if (d.n == 0) { s.alive = false; continue; }      // an empty list: rows = 0, no item
        if (R.finishes(i, l)) {
            for (int v = 0; v < q.nviews; ++v) {
                const int x = q.views[v].rel;
                rhj_apply_term &t = d.terms[d.nterms++];
                t.side = two.side(s, x); t.d_src = s.vec[x]; t.d_col = R.column(q, x, q.views[v].col);
            }
        } else {
            for (int x = 0; x < q.nrels; ++x) {
                if (!two.has(s, x)) continue;
                vb.take(R.ad.size(), d.nterms, d.n);      // the rebuilt vector
                rhj_apply_term &t = d.terms[d.nterms++];
                t.side = two.side(s, x); t.d_src = s.vec[x];
            }
        }
        R.ad.push_back(d); R.awho.push_back(i);
    }
    if (R.active.size() == sum_items) return 0;           // nobody alive at this level, or nobody but the sum batch's queries
    if (vb.resolve(g_qb.level[l], [&](size_t a, int t, char *p) { R.ad[a].terms[t].d_dst = (uint64_t *)p; })) return -1;
    ++g_query_info.apply_calls;
    return apply_batch(R.ad.data(), R.ad.size());         // (0 or an error)
}

// What level l's apply batch left: the sums and rows of the queries that finished, the two nodes of the others merged into A's.
static void query_take_back(QueryRun &R, int l)
{
    for (size_t a = 0; a < R.ad.size(); ++a) {
        rhj_query_desc &q = R.queries[R.awho[a]];
        QueryState &s = R.st[R.awho[a]];
        const rhj_apply_desc &d = R.ad[a];
        if (R.finishes(R.awho[a], l)) {
            for (int v = 0; v < q.nviews; ++v) q.sums[v] = d.terms[v].sum;
            q.rows = d.n;
            s.alive = false;                              // finished
            continue;
        }
        const TwoNodes two(s, q.joins[l]);
        int t = 0;
        for (int x = 0; x < q.nrels; ++x) {
            if (!two.has(s, x)) continue;
            s.vec[x] = d.terms[t++].d_dst; s.node[x] = two.na;
        }
        s.rows[two.na] = d.n;
    }
}

// ---- the fold route: a query whose predicates are a tree, summed by weighted folds (include/rhj_inter.h) --------
constexpr int FOLD_MAX_STEPS = RHJ_QUERY_MAX_RELS - 1;

// The schedule of the tree rooted at `root`: steps ascending by round, then by child; returns the rounds.
static int fold_schedule(const rhj_query_desc &q, int root, rhj_fold_step *steps)
{
    const int nb = q.nrels;
    int parent[RHJ_QUERY_MAX_RELS], waits[RHJ_QUERY_MAX_RELS] = {}, order[RHJ_QUERY_MAX_RELS], seen = 1;
    bool folded[RHJ_QUERY_MAX_RELS] = {};
    for (int b = 0; b < nb; ++b) parent[b] = -1;
    order[0] = root; parent[root] = root;
    for (int at = 0; at < seen; ++at)                     // breadth first from the root over the predicates
        for (int l = 0; l < q.njoins; ++l) {
            const rhj_query_join &p = q.joins[l];
            const int other = p.relA == order[at] ? p.relB : p.relB == order[at] ? p.relA : -1;
            if (other < 0 || parent[other] >= 0) continue;
            parent[other] = order[at]; ++waits[order[at]]; order[seen++] = other;
        }
    int nsteps = 0, round = 0;
    for (; nsteps < nb - 1; ++round) {
        bool taken[RHJ_QUERY_MAX_RELS] = {};
        const int first = nsteps;
        for (int c = 0; c < nb; ++c) {                    // the lowest ready child of every parent (ready by the rounds before this one)
            if (c == root || folded[c] || waits[c] || taken[parent[c]]) continue;
            taken[parent[c]] = true;
            steps[nsteps++] = rhj_fold_step{c, parent[c], round};
        }
        for (int k = first; k < nsteps; ++k) { folded[steps[k].child] = true; --waits[steps[k].parent]; }
    }
    return round;
}

// ---- the one planner (include/rhj_inter.h) ----------------------------------------------------------------
// The four plan functions are one rule at four strengths, so one function plans and each of the four decides what it accepts.
// fold_plan_at is the general rule, rhj_query_foldn_plan's for one prefix L of a VALID query (one query_levels accepts): the first
// L predicates merge their nodes as query_levels does and join their (binding, column) terms' classes in a union-find; the others
// go through the same union-find in order.  One that `drop` names is dropped; a kept one inside one node goes to self, counted on
// that node; the others are grouped by unordered node pair, and the groups must be a spanning tree of the nodes.  The schedule is
// fold_schedule's over one edge per group, the root the node that gives the fewest rounds, the lowest on a tie.
enum FoldDrop {
    DROP_REPEATS,                                         // rhj_query_foldk_plan's: the predicate written before, either way round
    DROP_IMPLIED                                          // the others': every predicate whose terms are in one class already (a repeat, 0.1=0.1, an implied one)
};
struct FoldPlan : rhj_foldn_plan {                        // the general plan, and what the weaker rules ask about the predicates from L on:
    bool twice;                                           // one names a binding on both sides
    bool dropped;                                         // one was dropped
};

static bool fold_plan_at(const rhj_query_desc *q, int L, FoldDrop drop, FoldPlan &plan)
{
    struct Term { int b, c; size_t up; };                 // a class member, and the member above it (itself: the class's root)
    std::vector<Term> terms;
    terms.reserve(2 * (size_t)q->njoins);
    const auto term = [&](int b, int c) {
        size_t k = 0;
        while (k < terms.size() && !(terms[k].b == b && terms[k].c == c)) ++k;
        if (k == terms.size()) terms.push_back(Term{b, c, k});
        while (terms[k].up != k) k = terms[k].up;
        return k;
    };
    const auto repeat = [&](int l) {
        const rhj_query_join &p = q->joins[l];
        for (int m = 0; m < l; ++m) {
            const rhj_query_join &e = q->joins[m];
            if ((e.relA == p.relA && e.colA == p.colA && e.relB == p.relB && e.colB == p.colB) ||
                (e.relA == p.relB && e.colA == p.colB && e.relB == p.relA && e.colB == p.colA)) return true;
        }
        return false;
    };
    memset(&plan, 0, sizeof(plan));
    plan.levels = L;
    int *const node = plan.node;
    for (int b = 0; b < q->nrels; ++b) node[b] = b;
    for (int l = 0; l < L; ++l) {
        const rhj_query_join &p = q->joins[l];
        const size_t ca = term(p.relA, p.colA), cb = term(p.relB, p.colB);
        if (ca != cb) terms[cb].up = ca;
        const int na = node[p.relA], nb = node[p.relB];
        for (int x = 0; x < q->nrels; ++x) if (node[x] == nb) node[x] = na;      // the two nodes merge into A's
    }
    struct Group { int a, b, n; int joins[RHJ_FOLD_MAX_KEYS]; };
    Group groups[RHJ_QUERY_MAX_RELS * (RHJ_QUERY_MAX_RELS - 1) / 2];            // (room for every pair of nodes)
    int ngroups = 0, on_node[RHJ_QUERY_MAX_RELS] = {};
    for (int l = L; l < q->njoins; ++l) {
        const rhj_query_join &p = q->joins[l];
        const size_t ca = term(p.relA, p.colA), cb = term(p.relB, p.colB);
        plan.twice |= p.relA == p.relB;
        if (drop == DROP_IMPLIED ? ca == cb : repeat(l)) {                      // said already by the predicates before it
            plan.dropped = true;
            continue;
        }
        if (ca != cb) terms[cb].up = ca;
        const int na = node[p.relA], nb = node[p.relB];
        if (na == nb) {
            if (++on_node[na] > RHJ_FOLD_SELF_MAX_TERMS) return false;          // more terms than an item has
            plan.self[plan.nself++] = l;
            continue;
        }
        const int a = na < nb ? na : nb, b = na < nb ? nb : na;
        int k = 0;
        while (k < ngroups && !(groups[k].a == a && groups[k].b == b)) ++k;
        if (k == ngroups) groups[ngroups++] = Group{a, b, 0, {}};
        if (groups[k].n == RHJ_FOLD_MAX_KEYS) return false;                     // more key words than a tuple has
        groups[k].joins[groups[k].n++] = l;
    }
    int id[RHJ_QUERY_MAX_RELS], of[RHJ_QUERY_MAX_RELS], nodes = 0;              // node -> its rank among the nodes, ascending, and back
    for (int b = 0; b < q->nrels; ++b) {
        bool is_node = false;
        for (int x = 0; x < q->nrels; ++x) is_node |= node[x] == b;
        id[b] = is_node ? nodes : -1;
        if (is_node) of[nodes++] = b;
    }
    // (query_levels saw all bindings connected, and a dropped predicate's are connected by kept ones: nodes - 1 groups are a
    // spanning tree, more are a true cycle)
    if (ngroups != nodes - 1) return false;
    plan.nsteps = ngroups;
    plan.root = of[0];
    if (ngroups == 0) return true;                        // one node: nothing to schedule
    // fold_schedule over the nodes by rank (the ranks ascend with the ids, so "the lowest first" means the same): one edge a group
    rhj_query_join first[FOLD_MAX_STEPS];
    for (int k = 0; k < ngroups; ++k) {
        const rhj_query_join &p = q->joins[groups[k].joins[0]];
        first[k] = rhj_query_join{id[node[p.relA]], p.colA, id[node[p.relB]], p.colB};
    }
    rhj_query_desc tree = *q;
    tree.nrels = nodes; tree.njoins = ngroups; tree.joins = first;
    int best = -1;
    rhj_fold_step mine[FOLD_MAX_STEPS], kept[FOLD_MAX_STEPS];
    for (int r = 0; r < nodes; ++r) {
        const int rounds = fold_schedule(tree, r, mine);
        if (best >= 0 && rounds >= best) continue;
        best = rounds; plan.root = of[r];
        memcpy(kept, mine, sizeof(kept));
    }
    for (int k = 0; k < plan.nsteps; ++k) {
        const int c = of[kept[k].child], p = of[kept[k].parent];
        rhj_foldk_step &st = plan.steps[k];
        st.child = c; st.parent = p; st.round = kept[k].round;
        for (int m = 0; m < ngroups; ++m) {
            const Group &gr = groups[m];
            if (gr.a != (c < p ? c : p) || gr.b != (c < p ? p : c)) continue;
            st.nkeys = gr.n;
            for (int t = 0; t < gr.n; ++t) st.joins[t] = gr.joins[t];
        }
    }
    return true;
}

// The four rules over a valid query; each leaves the plan it accepts in `plan`.
// rhj_query_folds_plan's: the general rule with no level before it.
static bool folds_rule(const rhj_query_desc *q, FoldPlan &plan) { return fold_plan_at(q, 0, DROP_IMPLIED, plan); }
// rhj_query_foldn_plan's: the shortest prefix of levels after which the general rule holds over the nodes.
static bool foldn_rule(const rhj_query_desc *q, FoldPlan &plan)
{
    for (int L = 0; L <= (q->njoins > 0 ? q->njoins - 1 : 0); ++L)
        if (fold_plan_at(q, L, DROP_IMPLIED, plan)) return true;
    return false;                                         // (not reached: with one predicate left the rest is one step, one term or nothing)
}
// rhj_query_foldk_plan's: at least one predicate, none on one binding, and only repeats dropped: an implied predicate stays a key word.
static bool foldk_rule(const rhj_query_desc *q, FoldPlan &plan) { return q->njoins > 0 && fold_plan_at(q, 0, DROP_REPEATS, plan) && !plan.twice; }
// rhj_query_fold_plan's: every predicate joins two distinct nodes, so none is dropped (a repeat lies inside a merged node), none is on
// one binding and none shares its pair of bindings with another.
static bool fold_rule(const rhj_query_desc *q, FoldPlan &plan)
{
    if (q->njoins == 0 || !folds_rule(q, plan) || plan.twice || plan.dropped) return false;
    for (int k = 0; k < plan.nsteps; ++k) if (plan.steps[k].nkeys > 1) return false;
    return true;
}

// The entry points: -3 from query_levels before anything else, 0 where the rule refuses (nothing is written then), else the plan in
// the function's own structure; every output may be NULL.
static int query_fold_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, int *root, rhj_fold_step *steps)
{
    FoldPlan plan;
    if (query_levels(q, nrel, rels, nullptr) < 0) return -3;
    if (!fold_rule(q, plan)) return 0;
    if (root) *root = plan.root;
    for (int k = 0; steps && k < plan.nsteps; ++k) steps[k] = rhj_fold_step{plan.steps[k].child, plan.steps[k].parent, plan.steps[k].round};
    return plan.nsteps;
}

static int query_foldk_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, int *root, rhj_foldk_step *steps)
{
    FoldPlan plan;
    if (query_levels(q, nrel, rels, nullptr) < 0) return -3;
    if (!foldk_rule(q, plan)) return 0;
    if (root) *root = plan.root;
    if (steps) memcpy(steps, plan.steps, (size_t)plan.nsteps * sizeof(rhj_foldk_step));
    return plan.nsteps;
}

static int query_folds_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, rhj_folds_plan *out)
{
    FoldPlan plan;
    if (query_levels(q, nrel, rels, nullptr) < 0) return -3;
    if (!folds_rule(q, plan)) return 0;
    if (!out) return 1;
    memset(out, 0, sizeof(*out));
    out->root = plan.root; out->nsteps = plan.nsteps; out->nself = plan.nself;
    memcpy(out->steps, plan.steps, sizeof(out->steps)); memcpy(out->self, plan.self, sizeof(out->self));
    return 1;
}

static int query_foldn_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, rhj_foldn_plan *out)
{
    FoldPlan plan;
    if (query_levels(q, nrel, rels, nullptr) < 0) return -3;
    if (!foldn_rule(q, plan)) return 0;
    if (out) *out = plan;                                 // (the general plan's first part is this structure)
    return 1;
}

// which rule lets a valid query of lv levels fold under the switches as they stand: 1 rhj_query_fold_plan's, 2 rhj_query_foldk_plan's,
// 3 rhj_query_folds_plan's with its steps within the key switch, 0 none
static int query_fold_how(const rhj_query_desc *q, int lv)
{
    FoldPlan plan;
    if (!(g_query_fold && lv >= 0)) return 0;
    if (fold_rule(q, plan)) return 1;
    if (g_query_fold_keys && foldk_rule(q, plan)) return 2;
    if (!(g_query_fold_self && folds_rule(q, plan))) return 0;
    for (int k = 0; k < plan.nsteps; ++k) if (plan.steps[k].nkeys > 1 && !g_query_fold_keys) return 0;
    return 3;
}

struct FoldQuery {                                        // a query on the fold route
    uint64_t        i;
    int             root, nsteps, next;                   // next: the first step not yet run
    int             nself, self[RHJ_QUERY_MAX_RELS * RHJ_FOLD_SELF_MAX_TERMS];    // the one-binding predicates of a query rhj_set_query_fold_self let in
    rhj_foldk_step  steps[FOLD_MAX_STEPS];                // (nkeys 1 throughout unless rhj_set_query_fold_keys let the query in)
    const uint64_t *w[RHJ_QUERY_MAX_RELS];                // node -> its weight vector; nullptr: ones.  (A node is a binding until levels have merged some: QueryState::node)
    const uint64_t *acc[RHJ_QUERY_MAX_RELS][RHJ_QUERY_MAX_VIEWS];     // node, view -> the view's partial sums per row, when the node carries the view
};

// The plan of a query on the fold route into f: how is QueryRun::folds's code, park the levels of a query with how 4.  The rule
// accepted the query when the batch was validated, so a refusal here is an error, reported under the route's name; counted: the
// query goes into the fold route's infos.
static int fold_query(const rhj_query_desc &q, int how, int park, const char *route, bool counted, FoldQuery &f)
{
    FoldPlan plan;
    if (how == 4) {                                       // parked alive after its level prefix
        if (!foldn_rule(&q, plan) || plan.levels != park) { fprintf(stderr, "rhj: a parked query has no plan over its nodes\n"); return -1; }
    } else if (!(how == 3 ? folds_rule(&q, plan) : foldk_rule(&q, plan))) {       // (3: possibly no step at all; 1: rhj_query_foldk_plan's is rhj_query_fold_plan's)
        fprintf(stderr, "rhj: a query on the %s route has no fold plan\n", route);
        return -1;
    }
    f.root = plan.root; f.nsteps = plan.nsteps; f.nself = plan.nself;
    memcpy(f.steps, plan.steps, sizeof(f.steps)); memcpy(f.self, plan.self, sizeof(f.self));
    if (!counted) return 0;
    if (how == 4) { ++g_query_fold_nodes_info.node_queries; g_query_fold_nodes_info.node_levels += (uint32_t)plan.levels; }
    if (how == 3) ++g_query_fold_self_info.self_queries;
    if (how == 2) ++g_query_foldk_info.foldk_queries;
    return 0;
}

// One step's item before it is a descriptor of its kind: a fold of node `child` into node `parent`, stated over a QueryState (the
// member bindings' vectors, a binding's node, a node's rows).  Key word t is predicate joins[t] of the step, the parent's column
// read through the vector of the member binding the predicate names on that side, the child's likewise.
struct FoldItem {
    int             nkeys, memR[RHJ_FOLD_MAX_KEYS], memS[RHJ_FOLD_MAX_KEYS];      // a word's member binding, parent side and child side
    const uint64_t *colR[RHJ_FOLD_MAX_KEYS], *colS[RHJ_FOLD_MAX_KEYS];
    bool            one_member;                           // every word of a side names the member its word 0 names
    uint64_t        nR, nS;
    int             nvalues, nouts;
    rhj_fold_factor values[RHJ_FOLD_MAX_VALUES];
    rhj_fold_out    outs[RHJ_FOLD_MAX_OUTS];
    std::array<int, RHJ_FOLD_MAX_OUTS> view;              // the view an output belongs to, -1 the weight
};

// Step k of query q as an item.  Unless it is the root's last fold (totals only) every output is a vector of the parent's rows:
// take(o, rows) is asked for output o's, in order, and what it returns is the output's d_out.
template <class Take>
static FoldItem fold_item(const QueryRun &R, const rhj_query_desc &q, const QueryState &s, const FoldQuery &f, int k, Take take)
{
    const rhj_foldk_step &step = f.steps[k];
    const int S = step.child, P = step.parent;
    const bool last = k == f.nsteps - 1;
    FoldItem d = {};
    d.nkeys = step.nkeys;
    d.one_member = true;
    for (int t = 0; t < step.nkeys; ++t) {                // the predicates between the two: word t of both sides
        const rhj_query_join &p = q.joins[step.joins[t]];
        const bool a_is_parent = s.node[p.relA] == P;
        d.memR[t] = a_is_parent ? p.relA : p.relB; d.memS[t] = a_is_parent ? p.relB : p.relA;
        d.colR[t] = R.column(q, d.memR[t], a_is_parent ? p.colA : p.colB);
        d.colS[t] = R.column(q, d.memS[t], a_is_parent ? p.colB : p.colA);
        d.one_member &= d.memR[t] == d.memR[0] && d.memS[t] == d.memS[0];
    }
    d.nR = s.rows[P]; d.nS = s.rows[S];
    int value_of[RHJ_QUERY_MAX_VIEWS];
    d.values[d.nvalues++] = rhj_fold_factor{f.w[S], nullptr, nullptr};             // value 0: the child's weight
    for (int v = 0; v < q.nviews; ++v) {
        const int x = q.views[v].rel;
        value_of[v] = -1;
        if (s.node[x] == S)      d.values[value_of[v] = d.nvalues++] = rhj_fold_factor{f.w[S], s.vec[x], R.column(q, x, q.views[v].col)};
        else if (f.acc[S][v])    d.values[value_of[v] = d.nvalues++] = rhj_fold_factor{f.acc[S][v], nullptr, nullptr};
    }
    const auto out = [&](int value, rhj_fold_factor p, int v) {
        d.view[(size_t)d.nouts] = v;
        rhj_fold_out &o = d.outs[d.nouts];
        o.value = value; o.p = p;
        if (!last) o.d_out = take(d.nouts, d.nR);
        ++d.nouts;
    };
    out(0, rhj_fold_factor{f.w[P], nullptr, nullptr}, -1);                         // the parent's new weight
    for (int v = 0; v < q.nviews; ++v) {
        const int x = q.views[v].rel;
        if (value_of[v] >= 0)                out(value_of[v], rhj_fold_factor{f.w[P], nullptr, nullptr}, v);      // a view coming from the child
        else if (f.acc[P][v])                out(0, rhj_fold_factor{f.acc[P][v], nullptr, nullptr}, v);           // a view the parent carried
        else if (last && s.node[x] == P)     out(0, rhj_fold_factor{f.w[P], s.vec[x], R.column(q, x, q.views[v].col)}, v);   // a view on the root: lazy until now
    }
    return d;
}

// An item as the descriptor of its kind: on one key, on a tuple read through one vector a side (the item's one_member), or on a
// tuple whose every word has its vector.
static void fold_keys(rhj_join_fold_desc &d, const FoldItem &it, const QueryState &s)
{
    d.d_colR = it.colR[0]; d.d_selR = s.vec[it.memR[0]];
    d.d_colS = it.colS[0]; d.d_selS = s.vec[it.memS[0]];
}
static void fold_keys(rhj_join_foldk_desc &d, const FoldItem &it, const QueryState &s)
{
    d.nkeys = it.nkeys;
    for (int w = 0; w < it.nkeys; ++w) { d.d_colR[w] = it.colR[w]; d.d_colS[w] = it.colS[w]; }
    d.d_selR = s.vec[it.memR[0]]; d.d_selS = s.vec[it.memS[0]];
}
static void fold_keys(rhj_join_foldn_desc &d, const FoldItem &it, const QueryState &s)
{
    d.nkeys = it.nkeys;
    for (int w = 0; w < it.nkeys; ++w) {
        d.d_colR[w] = it.colR[w]; d.d_selR[w] = s.vec[it.memR[w]];
        d.d_colS[w] = it.colS[w]; d.d_selS[w] = s.vec[it.memS[w]];
    }
}
template <class D>
static void fold_desc(D &d, const FoldItem &it, const QueryState &s)    // d: all zero
{
    fold_keys(d, it, s);
    d.nR = it.nR; d.nS = it.nS;
    d.nvalues = it.nvalues; d.nouts = it.nouts;
    memcpy(d.values, it.values, sizeof(d.values)); memcpy(d.outs, it.outs, sizeof(d.outs));
}

struct FoldOuts { rhj_fold_out *outs; int nouts; };       // an item's outputs, whatever its kind
template <class D> static FoldOuts fold_outs(D &d) { return FoldOuts{d.outs, d.nouts}; }

// Before round 0, ONE fold_self_batch call over the queries with predicates inside a node (rhj_set_query_fold_self's, whose nodes
// are their bindings, and rhj_set_query_fold_nodes's): a node with such predicates gets its first weight vector (0 / 1 per row),
// each column of a term read through the vector of the member binding it names, and a query of one node is finished.
static int query_fold_self(QueryRun &R, std::vector<FoldQuery> &fq)
{
    std::vector<rhj_fold_self_desc> sd;
    std::vector<std::pair<size_t, int>> who;              // an item's query in fq and its binding
    QueryBump wb;
    for (size_t k = 0; k < fq.size(); ++k) {
        const FoldQuery &f = fq[k];
        const rhj_query_desc &q = R.queries[f.i];
        const QueryState &s = R.st[f.i];
        if (R.folds[f.i] < 3) continue;
        for (int b = 0; b < q.nrels; ++b) {
            if (s.node[b] != b) continue;                 // (a node carries the id of one of its members)
            rhj_fold_self_desc d = {};
            for (int t = 0; t < f.nself; ++t) {
                const rhj_query_join &p = q.joins[f.self[t]];
                if (s.node[p.relA] != b) continue;
                d.terms[d.nterms++] = rhj_fold_eq_term{R.column(q, p.relA, p.colA), s.vec[p.relA], R.column(q, p.relB, p.colB), s.vec[p.relB]};
            }
            if (d.nterms == 0 && f.nsteps > 0) continue;  // no predicate of its own: the node's weight stays ones
            d.n = s.rows[b];
            d.nouts = 1;                                  // output 0: ones, so its total is the rows that pass
            if (f.nsteps == 0) {                          // the whole query is this node: the views' sums, nothing written
                for (int v = 0; v < q.nviews; ++v) d.outs[d.nouts++].p = rhj_fold_factor{nullptr, s.vec[q.views[v].rel], R.column(q, q.views[v].rel, q.views[v].col)};
            } else {
                wb.take(sd.size(), 0, d.n);
            }
            who.emplace_back(k, b); sd.push_back(d);
        }
    }
    if (sd.empty()) return 0;
    if (wb.resolve(g_qb.self, [&](size_t a, int, char *p) { sd[a].outs[0].d_out = (uint64_t *)p; })) return -1;
    ++g_query_fold_self_info.self_calls;
    g_query_fold_self_info.self_items += (uint32_t)sd.size();
    if (const int rc = fold_self_batch(sd.data(), sd.size())) return rc;       // (0 or an error: the items are valid)
    for (size_t a = 0; a < sd.size(); ++a) {
        FoldQuery &f = fq[who[a].first];
        rhj_query_desc &q = R.queries[f.i];
        QueryState &s = R.st[f.i];
        const rhj_fold_self_desc &d = sd[a];
        if (!s.alive) continue;                           // (finished by another item of this call)
        if (d.outs[0].total == 0) { s.alive = false; continue; }               // no row passes: rows = 0, sums 0
        if (f.nsteps == 0) {
            q.rows = d.outs[0].total;
            for (int v = 0; v < q.nviews; ++v) q.sums[v] = d.outs[1 + v].total;
            s.alive = false;                              // finished
            continue;
        }
        f.w[who[a].second] = d.outs[0].d_out;
    }
    return 0;
}

// The folding queries still alive after the filters, round by round: every round is one table_batch call over all their items on
// one key and, with rhj_set_query_fold_keys, one over all their items on tuple keys.  The same over NODES (nodes_pass, after the
// level loop) for the queries that were parked after their level prefix: a step folds a node into a node, a key word, a child's
// view value and a root's lazy view read their column through the vector of the member binding that the predicate or view names
// (QueryState::vec, left by the levels), and a tuple whose words name several members of a side is an item of a third call,
// rhj_join_foldn_batch_device's.  Before the levels every node is its binding, so the first pass issues what it always did.
static int query_folds(QueryRun &R, bool nodes_pass)
{
    std::vector<FoldQuery> fq;
    int rounds = 0;
    for (uint64_t i = 0; i < R.n && !R.folds.empty(); ++i) {
        if (!R.folds[i] || !R.st[i].alive || (R.folds[i] == 4) != nodes_pass) continue;
        FoldQuery f = {};
        f.i = i;
        if (fold_query(R.queries[i], R.folds[i], R.folds[i] == 4 ? R.park[i] : 0, "fold", true, f)) return -1;
        if (f.nsteps && f.steps[f.nsteps - 1].round + 1 > rounds) rounds = f.steps[f.nsteps - 1].round + 1;
        fq.push_back(f);
    }
    g_query_fold_info.fold_queries += (uint32_t)fq.size();
    if (const int rc = query_fold_self(R, fq)) return rc;
    if (g_qb.fold.size() < (size_t)rounds) g_qb.fold.resize((size_t)rounds);
    std::vector<rhj_join_fold_desc> fd;                   // the round's items on one key ...
    std::vector<rhj_join_foldk_desc> kd;                  // ... on tuple keys ...
    std::vector<rhj_join_foldn_desc> nd;                  // ... and on tuple keys whose words name several members of a node
    std::vector<std::pair<int, size_t>> where;            // an item, in the order issued: 0 in fd, 1 in kd, 2 in nd, and its place there
    std::vector<size_t> who;                              // an item's query in fq
    std::vector<int> par;                                 // an item's parent binding
    std::vector<std::array<int, RHJ_FOLD_MAX_OUTS>> view; // an item's outputs: the view each belongs to, -1 the weight
    for (int r = 0; r < rounds; ++r) {
        QueryBump ob;
        fd.clear(); kd.clear(); nd.clear(); where.clear(); who.clear(); par.clear(); view.clear();
        for (size_t k = 0; k < fq.size(); ++k) {
            FoldQuery &f = fq[k];
            const rhj_query_desc &q = R.queries[f.i];
            const QueryState &s = R.st[f.i];
            for (; s.alive && f.next < f.nsteps && f.steps[f.next].round == r; ++f.next) {
                const FoldItem it = fold_item(R, q, s, f, f.next, [&](int o, uint64_t rows) { ob.take(where.size(), o, rows); return (uint64_t *)nullptr; });
                who.push_back(k); par.push_back(f.steps[f.next].parent); view.push_back(it.view);
                if (it.nkeys == 1)       { where.emplace_back(0, fd.size()); fold_desc(fd.emplace_back(), it, s); }
                else if (it.one_member)  { where.emplace_back(1, kd.size()); fold_desc(kd.emplace_back(), it, s); }
                else                     { where.emplace_back(2, nd.size()); fold_desc(nd.emplace_back(), it, s); }
            }
        }
        if (where.empty()) continue;
        const auto outs_of = [&](size_t a) { return where[a].first == 2 ? fold_outs(nd[where[a].second]) : where[a].first ? fold_outs(kd[where[a].second]) : fold_outs(fd[where[a].second]); };
        if (ob.resolve(g_qb.fold[(size_t)r], [&](size_t a, int o, char *p) { outs_of(a).outs[o].d_out = (uint64_t *)p; })) return -1;
        if (!fd.empty()) {
            ++g_query_fold_info.fold_calls;
            g_query_fold_info.fold_items += (uint32_t)fd.size();
            if (const int rc = table_batch(fd.data(), fd.size())) return rc;      // (0 or an error: the items are valid)
        }
        if (!kd.empty()) {
            ++g_query_foldk_info.foldk_calls;
            g_query_foldk_info.foldk_items += (uint32_t)kd.size();
            if (const int rc = table_batch(kd.data(), kd.size())) return rc;
        }
        if (!nd.empty()) {
            ++g_query_fold_nodes_info.foldn_calls;
            g_query_fold_nodes_info.foldn_items += (uint32_t)nd.size();
            if (const int rc = table_batch(nd.data(), nd.size())) return rc;
        }
        for (size_t a = 0; a < where.size(); ++a) {
            FoldQuery &f = fq[who[a]];
            rhj_query_desc &q = R.queries[f.i];
            QueryState &s = R.st[f.i];
            const auto [outs, nouts] = outs_of(a);
            if (!s.alive) continue;                       // (finished by another item of this round)
            if (outs[0].total == 0) { s.alive = false; continue; }           // the subtree's join is empty: rows = 0, sums 0
            const bool last = outs[0].d_out == nullptr;
            if (last) {
                q.rows = outs[0].total;
                for (int o = 1; o < nouts; ++o) q.sums[view[a][(size_t)o]] = outs[o].total;
                s.alive = false;                          // finished
                continue;
            }
            const int P = par[a];                         // the parent's new weight and what it carries now
            f.w[P] = outs[0].d_out;
            for (int o = 1; o < nouts; ++o) f.acc[P][view[a][(size_t)o]] = outs[o].d_out;
        }
    }
    return 0;
}

// ---- the fold program with one wait (include/rhj_inter.h) ----------------------------------------------------------
// A query whose bindings stay whole relations, their filters 0/1 weights (rhj_fold_pred_batch.hip.h), has every size of every round
// known on the host.  The route's queries, in call order, are laid out as programs: ow_build states one query's pred items and
// steps, ow_fits says whether a program still takes them within the batches' chunk limits, ow_run issues a program: one upload,
// k_fold_pred, per round a memset and the fold batches' own launches, one copy back and one wait.  A weight or view vector is a
// piece of ONE buffer a program (g_qb.prog), never reused inside it; until the buffer has its size a descriptor names such a vector
// by its offset (ow_ref), and ow_run turns the offsets into addresses.
static int query_one_wait_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels)
{
    if (!q) return -3;
    const int lv = query_levels(q, nrel, rels, nullptr);
    if (lv < 0) return -3;
    if (!rels || !query_fold_how(q, lv)) return 0;
    for (int b = 0; b < q->nrels; ++b) {
        const uint64_t rows = rels[q->rels[b]].num_tuples;
        if (rows < 1 || rows > g_query_fold_one_wait_rows) return 0;
    }
    return 1;
}

constexpr uintptr_t OW_REF = 16;                          // an offset's bias: no vector is the null pointer
static inline uint64_t *ow_ref(size_t off) { return (uint64_t *)(uintptr_t)(off + OW_REF); }
static inline void ow_fix(const uint64_t *&p, uintptr_t base) { if (p) p = (const uint64_t *)(base + ((uintptr_t)p - OW_REF)); }
static inline void ow_fix(uint64_t *&p, uintptr_t base) { if (p) p = (uint64_t *)(base + ((uintptr_t)p - OW_REF)); }

struct OwStep {                                           // one fold of a program, in the order built
    size_t who;                                           // its query, by its place in the program
    int    round, kind;                                   // kind 0: rounds[round].fd[at], 1: .kd[at]
    size_t at;
    bool   last;                                          // the root's last fold: its totals are rows and sums
    std::array<int, RHJ_FOLD_MAX_OUTS> view;              // the view an output belongs to, -1 the weight
};
struct OwRound {
    std::vector<rhj_join_fold_desc>  fd;
    std::vector<rhj_join_foldk_desc> kd;
    uint64_t tiles[2] = {0, 0}, bytes = 0;                // both sides' tiles by kind; the round's tables
};
struct OwProgram {
    std::vector<uint64_t>           who;                  // the queries
    std::vector<rhj_fold_pred_desc> pd;
    std::vector<size_t>             pwho;                 // a pred item's query, by its place in who
    std::vector<char>               pfinal;               // a pred item that is its whole query: totals are rows and sums
    uint64_t                        ptiles = 0;
    std::vector<OwRound>            rounds;
    std::vector<OwStep>             steps;
    size_t                          vec_at = 0;           // bytes of vectors handed out
};

// Query i alone as a program whose vectors begin at offset vec_at.
static int ow_build(const QueryRun &R, uint64_t i, size_t vec_at, OwProgram &P)
{
    const rhj_query_desc &q = R.queries[i];
    P = OwProgram();
    P.who.push_back(i);
    P.vec_at = vec_at;
    FoldQuery f = {};
    f.i = i;
    if (fold_query(q, R.folds[i], 0, "one-wait", false, f)) return -1;
    QueryState s = {};                                    // every binding its whole relation, its own node
    for (int b = 0; b < q.nrels; ++b) { s.node[b] = b; s.rows[b] = R.rels[q.rels[b]].num_tuples; }
    const auto take = [&](uint64_t n) { uint64_t *p = ow_ref(P.vec_at); P.vec_at += (size_t)((n + 1) / 2 * 2) * 8; return p; };
    // the pred items: a binding's filters and kept one-binding predicates as its first weight vector
    for (int b = 0; b < q.nrels; ++b) {
        rhj_fold_pred_desc d = {};
        for (int k = 0; k < q.nfilters; ++k) {
            const rhj_query_filter &p = q.filters[k];
            if (p.rel != b) continue;
            rhj_fold_const_term &t = d.consts[d.nconst++];
            t.d_col = R.column(q, b, p.col); t.op = p.op; t.value = p.value;
        }
        for (int t = 0; t < f.nself; ++t) {
            const rhj_query_join &p = q.joins[f.self[t]];
            if (p.relA != b) continue;
            d.eqs[d.neq++] = rhj_fold_eq_term{R.column(q, b, p.colA), nullptr, R.column(q, b, p.colB), nullptr};
        }
        if (d.nconst + d.neq == 0 && f.nsteps > 0) continue;       // no predicate of its own: the weight stays ones
        d.n = s.rows[b];
        d.nouts = 1;                                      // output 0: ones, so its total is the rows that pass
        if (f.nsteps == 0) {                              // the whole query is this binding: the views' sums, nothing written
            for (int v = 0; v < q.nviews; ++v) d.outs[d.nouts++].p = rhj_fold_factor{nullptr, nullptr, R.column(q, q.views[v].rel, q.views[v].col)};
        } else {
            d.outs[0].d_out = take(d.n);
            f.w[b] = d.outs[0].d_out;
        }
        P.pd.push_back(d); P.pwho.push_back(0); P.pfinal.push_back(f.nsteps == 0);
        P.ptiles += jsum_tiles(d.n);
    }
    // the steps: query_folds's items.  (Every side is a whole relation, every node one binding: no vector, and no word of a key
    // names another member than word 0's, so no item is rhj_join_foldn_batch_device's.)
    for (int k = 0; k < f.nsteps; ++k) {
        const rhj_foldk_step &step = f.steps[k];
        const bool last = k == f.nsteps - 1;
        if (P.rounds.size() <= (size_t)step.round) P.rounds.resize((size_t)step.round + 1);
        OwRound &rd = P.rounds[(size_t)step.round];
        const FoldItem it = fold_item(R, q, s, f, k, [&](int, uint64_t rows) { return take(rows); });
        if (!last) {                                      // (a round's steps of one query share no node: what a step leaves is read by later rounds only)
            f.w[step.parent] = it.outs[0].d_out;
            for (int o = 1; o < it.nouts; ++o) f.acc[step.parent][it.view[(size_t)o]] = it.outs[o].d_out;
        }
        rd.tiles[it.nkeys > 1] += jsum_tiles(it.nR) + jsum_tiles(it.nS);
        OwStep os = {0, step.round, it.nkeys > 1, 0, last, it.view};
        if (it.nkeys == 1) {
            os.at = rd.fd.size(); fold_desc(rd.fd.emplace_back(), it, s);
            rd.bytes += tbatch_table_bytes(rd.fd.back());
        } else {
            os.at = rd.kd.size(); fold_desc(rd.kd.emplace_back(), it, s);
            rd.bytes += tbatch_table_bytes(rd.kd.back());
        }
        P.steps.push_back(os);
    }
    return 0;
}

// whether program P stays within a chunk's limits once `one` has joined it: items a round and kind, tiles a launch, tables a round
static bool ow_fits(const OwProgram &P, const OwProgram &one)
{
    if (P.pd.size() + one.pd.size() > FSELF_MAX_ITEMS || P.ptiles + one.ptiles > FSELF_MAX_TILES) return false;
    for (size_t r = 0; r < one.rounds.size() && r < P.rounds.size(); ++r) {
        const OwRound &a = P.rounds[r], &b = one.rounds[r];
        if (a.fd.size() + b.fd.size() > JSUM_MAX_ITEMS || a.kd.size() + b.kd.size() > JSUM_MAX_ITEMS) return false;
        if (a.tiles[0] + b.tiles[0] > JSUM_MAX_TILES || a.tiles[1] + b.tiles[1] > JSUM_MAX_TILES || a.bytes + b.bytes > JSUM_ARENA_BYTES) return false;
    }
    return true;
}

static void ow_merge(OwProgram &P, const OwProgram &one)
{
    const size_t me = P.who.size();
    P.who.push_back(one.who[0]);
    P.pd.insert(P.pd.end(), one.pd.begin(), one.pd.end());
    P.pwho.insert(P.pwho.end(), one.pd.size(), me);
    P.pfinal.insert(P.pfinal.end(), one.pfinal.begin(), one.pfinal.end());
    P.ptiles += one.ptiles;
    if (P.rounds.size() < one.rounds.size()) P.rounds.resize(one.rounds.size());
    for (OwStep s : one.steps) {
        s.who = me;
        s.at += s.kind ? P.rounds[(size_t)s.round].kd.size() : P.rounds[(size_t)s.round].fd.size();
        P.steps.push_back(s);
    }
    for (size_t r = 0; r < one.rounds.size(); ++r) {
        OwRound &a = P.rounds[r];
        const OwRound &b = one.rounds[r];
        a.fd.insert(a.fd.end(), b.fd.begin(), b.fd.end());
        a.kd.insert(a.kd.end(), b.kd.begin(), b.kd.end());
        a.tiles[0] += b.tiles[0]; a.tiles[1] += b.tiles[1]; a.bytes += b.bytes;
    }
    P.vec_at = one.vec_at;
}

template <class D>
static void ow_fix_fold(D &d, uintptr_t base)
{
    for (int c = 0; c < d.nvalues; ++c) ow_fix(d.values[c].d_w, base);
    for (int o = 0; o < d.nouts; ++o) { ow_fix(d.outs[o].p.d_w, base); ow_fix(d.outs[o].d_out, base); }
}

// a round's items of one kind into the block: descriptors, tile starts, tables from byte `at` of the arena on, words from `wat` on
// (`res` takes the indices of the resident ones, `res_lds` the largest's LDS bytes: rhj_set_fold_resident)
template <class D, class Dev>
static void ow_fill(const std::vector<D> &items, Dev *hd, uint32_t *const (&ts)[3], uint32_t (&t)[3], size_t &at, unsigned long long *d_words, size_t &wat,
                    uint32_t *res, size_t &res_lds)
{
    constexpr size_t WORDS = tbatch_dev<D>::words;
    t[0] = t[1] = t[2] = 0;
    res_lds = 0;
    for (size_t k = 0, r = 0; k < items.size(); ++k) {
        ts[0][k] = t[0]; ts[1][k] = t[1]; ts[2][k] = t[2];
        Dev d;
        tbatch_fill(items[k], (unsigned long long *)((char *)g.jsum_arena.p + at), d_words + wat, d, t);
        memcpy((void *)&hd[k], (const void *)&d, sizeof(d));
        at += (size_t)tbatch_table_bytes(items[k]);
        wat += WORDS;
        if (tbatch_resident(items[k])) {
            res[r++] = (uint32_t)k;
            res_lds = std::max(res_lds, tbatch_resident_lds(items[k]));
        }
    }
    ts[0][items.size()] = t[0]; ts[1][items.size()] = t[1]; ts[2][items.size()] = t[2];
}

// One program: one upload, the launches of the pred items and of every round, one copy back, one wait; then the answers.
static int ow_run(QueryRun &R, OwProgram &P)
{
    const size_t np = P.pd.size(), nr = P.rounds.size();
    uint64_t arena = 0;
    size_t nwords = np * FOLD_PRED_WORDS;
    for (const OwRound &rd : P.rounds) {
        if (rd.bytes > arena) arena = rd.bytes;
        nwords += rd.fd.size() * FOLD_WORDS + rd.kd.size() * FOLDK_WORDS;
    }
    if (arena && batch_arena(g.jsum_arena, (size_t)arena, JSUM_ARENA_BYTES)) return -1;
    if (ensure(g_qb.prog, P.vec_at)) return -1;
    const uintptr_t base = (uintptr_t)g_qb.prog.p;
    for (rhj_fold_pred_desc &d : P.pd) ow_fix(d.outs[0].d_out, base);
    for (OwRound &rd : P.rounds) {
        for (rhj_join_fold_desc &d : rd.fd) ow_fix_fold(d, base);
        for (rhj_join_foldk_desc &d : rd.kd) ow_fix_fold(d, base);
    }
    struct RoundPieces { JoinFoldDesc *hf, *df; JoinFoldKDesc *hk, *dk; uint32_t *ts[2][3], *d_ts[2][3]; uint32_t t[2][3]; uint32_t *res[2], *d_res[2]; size_t nres[2], res_lds[2]; };
    std::vector<RoundPieces> rp(nr);
    for (size_t r = 0; r < nr; ++r) {
        rp[r].nres[0] = rp[r].nres[1] = 0;               // (by kind: the folds on one key, rhj_set_fold_resident, and on tuples, rhj_set_fold_resident_keys)
        for (const rhj_join_fold_desc &d : P.rounds[r].fd) rp[r].nres[0] += tbatch_resident(d);
        for (const rhj_join_foldk_desc &d : P.rounds[r].kd) rp[r].nres[1] += tbatch_resident(d);
    }
    Block blk;
    unsigned long long *back, *words, *d_words; FoldPredDesc *hp, *dp; uint32_t *ptile, *d_ptile;
    const auto pieces = [&](Block &b) {
        b.back(back, nwords);
        b.up(hp, dp, np); b.up(ptile, d_ptile, np + 1);
        for (size_t r = 0; r < nr; ++r) {
            const size_t nf = P.rounds[r].fd.size(), nk = P.rounds[r].kd.size();
            b.up(rp[r].hf, rp[r].df, nf);
            for (int j = 0; j < 3; ++j) b.up(rp[r].ts[0][j], rp[r].d_ts[0][j], nf + 1);
            b.up(rp[r].res[0], rp[r].d_res[0], rp[r].nres[0]);
            b.up(rp[r].hk, rp[r].dk, nk);
            for (int j = 0; j < 3; ++j) b.up(rp[r].ts[1][j], rp[r].d_ts[1][j], nk + 1);
            b.up(rp[r].res[1], rp[r].d_res[1], rp[r].nres[1]);
        }
        b.up(words, d_words, nwords);
    };
    if (batch_block(blk, pieces)) return -1;
    memset(words, 0, nwords * 8);
    size_t wat = 0;
    uint32_t ptiles = 0;
    for (size_t k = 0; k < np; ++k) {
        FoldPredDesc d;
        fpred_fill(P.pd[k], d_words + wat, d);
        memcpy((void *)&hp[k], (const void *)&d, sizeof(d));
        ptile[k] = ptiles;
        ptiles += (uint32_t)jsum_tiles(P.pd[k].n);
        wat += FOLD_PRED_WORDS;
    }
    ptile[np] = ptiles;
    std::vector<size_t> wfold(nr), wfoldk(nr);           // where a round's words begin, by kind
    for (size_t r = 0; r < nr; ++r) {
        size_t at = 0;
        wfold[r] = wat;
        ow_fill(P.rounds[r].fd, rp[r].hf, rp[r].ts[0], rp[r].t[0], at, d_words, wat, rp[r].res[0], rp[r].res_lds[0]);
        wfoldk[r] = wat;
        ow_fill(P.rounds[r].kd, rp[r].hk, rp[r].ts[1], rp[r].t[1], at, d_words, wat, rp[r].res[1], rp[r].res_lds[1]);
        if (at != (size_t)P.rounds[r].bytes || at > g.jsum_arena.cap) { fprintf(stderr, "rhj: the tables of a round of a fold program were placed beyond its arena\n"); return -1; }
    }
    if (wat != nwords) { fprintf(stderr, "rhj: a fold program's words were miscounted\n"); return -1; }
    rhj_query_batch_one_wait_info &info = g_query_one_wait_info;
    if (batch_upload(blk, hp, blk.host_end())) return -1;
    if (ptiles) {
        RHJ_LAUNCH(k_fold_pred, dim3(ptiles), dim3(256), 0, g.stream, dp, d_ptile, (uint32_t)np);
        ++info.launches;
    }
    for (size_t r = 0; r < nr; ++r) {
        const OwRound &rd = P.rounds[r];
        if (rd.fd.empty() && rd.kd.empty()) continue;
        // the arena's tables of the round before are dead: stream order puts this memset behind their last reader
        // (a round whose items are all resident, rhj_set_fold_resident and rhj_set_fold_resident_keys, has no table: no memset, and
        // one launch a kind)
        if (rd.bytes) {
            HIP_TRY(hipMemsetAsync(g.jsum_arena.p, 0, (size_t)rd.bytes, g.stream));
            ++info.memsets;
        }
        ++info.rounds;
        if (rp[r].nres[0] < rd.fd.size()) {
            tbatch_launch(rd.fd[0], rp[r].df, (uint32_t)rd.fd.size(), rp[r].d_ts[0], rp[r].t[0]);
            info.launches += 2 + (rp[r].t[0][0] != 0);
        }
        if (!rd.fd.empty()) {
            tbatch_launch_resident(rp[r].df, rp[r].d_res[0], (uint32_t)rp[r].nres[0], rp[r].res_lds[0], rd.fd.size());
            info.launches += rp[r].nres[0] != 0;
        }
        if (rp[r].nres[1] < rd.kd.size()) {
            tbatch_launch(rd.kd[0], rp[r].dk, (uint32_t)rd.kd.size(), rp[r].d_ts[1], rp[r].t[1]);
            info.launches += 2 + (rp[r].t[1][0] != 0);
        }
        if (!rd.kd.empty()) {
            tbatch_launch_resident(rp[r].dk, rp[r].d_res[1], (uint32_t)rp[r].nres[1], rp[r].res_lds[1], rd.kd.size());
            info.launches += rp[r].nres[1] != 0;
        }
        info.fold_items += (uint32_t)rd.fd.size(); info.foldk_items += (uint32_t)rd.kd.size();
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(back, d_words, nwords * 8, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    ++info.programs; ++info.waits;
    info.queries += (uint32_t)P.who.size(); info.pred_items += (uint32_t)np;
    // the answers, by the fold route's rule: a weight total of 0 anywhere is the empty result; else the last totals
    std::vector<char> dead(P.who.size(), 0);
    for (size_t k = 0; k < np; ++k)
        if (back[k * FOLD_PRED_WORDS] == 0) dead[P.pwho[k]] = 1;
    for (size_t r = 0; r < nr; ++r) {
        for (size_t k = 0; k < P.rounds[r].fd.size(); ++k) tbatch_take(P.rounds[r].fd[k], back + wfold[r] + k * FOLD_WORDS);
        for (size_t k = 0; k < P.rounds[r].kd.size(); ++k) tbatch_take(P.rounds[r].kd[k], back + wfoldk[r] + k * FOLDK_WORDS);
        tbatch_combine_take<rhj_join_fold_desc>(rp[r].t[0], back + wfold[r], P.rounds[r].fd.size());
        tbatch_combine_take<rhj_join_foldk_desc>(rp[r].t[1], back + wfoldk[r], P.rounds[r].kd.size());
    }
    const auto outs_of = [&](const OwStep &s) { return s.kind ? fold_outs(P.rounds[(size_t)s.round].kd[s.at]) : fold_outs(P.rounds[(size_t)s.round].fd[s.at]); };
    for (const OwStep &s : P.steps)
        if (outs_of(s).outs[0].total == 0) dead[s.who] = 1;
    for (size_t k = 0; k < np; ++k) {
        if (!P.pfinal[k] || dead[P.pwho[k]]) continue;
        rhj_query_desc &q = R.queries[P.who[P.pwho[k]]];
        q.rows = back[k * FOLD_PRED_WORDS];
        for (int v = 0; v < q.nviews; ++v) q.sums[v] = back[k * FOLD_PRED_WORDS + 1 + (size_t)v];
    }
    for (const OwStep &s : P.steps) {
        if (!s.last || dead[s.who]) continue;
        rhj_query_desc &q = R.queries[P.who[s.who]];
        const auto [outs, nouts] = outs_of(s);
        q.rows = outs[0].total;
        for (int o = 1; o < nouts; ++o) q.sums[s.view[(size_t)o]] = outs[o].total;
    }
    return 0;
}

// The one-wait route's queries (R.one_wait), in call order, as programs cut only at the chunk limits.
static int query_one_wait(QueryRun &R)
{
    OwProgram P, one;
    for (uint64_t i = 0; i < R.n; ++i) {
        if (!R.one_wait[i]) continue;
        if (ow_build(R, i, P.vec_at, one)) return -1;
        if (!P.who.empty() && !ow_fits(P, one)) {
            if (const int rc = ow_run(R, P)) return rc;
            P = OwProgram();
            if (ow_build(R, i, 0, one)) return -1;
        }
        if (P.who.empty()) P = one; else ow_merge(P, one);
    }
    return P.who.empty() ? 0 : ow_run(R, P);
}

// whether every binding is small enough for a fold's side: fewer than 2^32 rows
static bool fold_sides_fit(const rhj_query_desc &q, const rhj_device_relation *rels)
{
    for (int b = 0; b < q.nrels; ++b) if (rels[q.rels[b]].num_tuples >= JSUM_MAX_ROWS) return false;
    return true;
}

// whether every merged node (a binding not its node's name lies in one) has few enough rows to be parked for the nodes' pass
static bool fold_nodes_fit(const rhj_query_desc &q, const QueryState &s)
{
    for (int b = 0; b < q.nrels; ++b) if (s.node[b] != b && s.rows[s.node[b]] >= g_query_fold_node_rows) return false;
    return true;
}

static int query_batch(const rhj_device_relation *rels, int nrel, rhj_query_desc *queries, uint64_t n)
{
    if (n == 0) return 0;
    if (!queries || (nrel > 0 && !rels)) return -1;
    query_infos_clear();
    std::vector<char> one_wait;
    const bool hand_over = g_query_fold && g_query_fold_keys && g_query_fold_self && g_query_fold_nodes;
    std::vector<int> park;
    bool invalid = false;                                 // the whole batch is validated before a device is touched
    int maxl = 0;
    std::vector<char> folds;
    if (g_query_fold) folds.assign(n, 0);
    for (uint64_t i = 0; i < n; ++i) {
        const int lv = query_levels(&queries[i], nrel, rels, nullptr);
        queries[i].rc = lv < 0 ? -3 : 0;
        invalid |= lv < 0;
        const int how = query_fold_how(&queries[i], lv);
        int prefix = 0;                                   // of a query none of the three plans takes: the levels before its nodes fold
        if (!how && hand_over && lv >= 0) {
            rhj_foldn_plan plan;
            if (query_foldn_plan(&queries[i], nrel, rels, &plan) == 1) prefix = plan.levels;         // (>= 1: at 0 levels query_folds_plan took it)
        }
        if (how || prefix) {
            const bool fits = fold_sides_fit(queries[i], rels);
            folds[i] = !fits ? 0 : how ? (char)how : 4;
            if (how && g_query_fold_one_wait && query_one_wait_plan(&queries[i], nrel, rels) == 1) {
                if (one_wait.empty()) one_wait.assign(n, 0);
                one_wait[i] = 1;
            }
            if (fits && prefix) {
                if (park.empty()) park.assign(n, 0);
                park[i] = prefix;
                if (prefix > maxl) maxl = prefix;         // (the prefix runs in the level loop)
            }
        }
        if (lv > maxl && !(g_query_fold && folds[i])) maxl = lv;       // (the levels of the queries that run by levels)
    }
    if (invalid) return -3;
    for (uint64_t i = 0; i < n; ++i) { memset(queries[i].sums, 0, sizeof(queries[i].sums)); queries[i].rows = 0; }
    if (ctx_init()) return -1;
    const bool timed = g.timing >= 1;
    if (timed && !g_qb.ev[1]) for (auto &ev : g_qb.ev) HIP_TRY(hipEventCreate(&ev));
    if (timed) HIP_TRY(hipEventRecord(g_qb.ev[0], g.stream));
    g_query_info.levels = (uint32_t)maxl;
    {
        QueryTimingOff inner_untimed;
        QueryRun R = {rels, queries, n, std::vector<QueryState>(n)};
        R.folds.swap(folds); R.park.swap(park); R.one_wait.swap(one_wait);
        if (!R.one_wait.empty())
            if (const int rc = query_one_wait(R)) return rc;       // the fold programs: their queries are finished before the others begin
        if (const int rc = query_filters(R)) return rc;
        if (const int rc = query_folds(R, false)) return rc;       // the fold route's queries: all finished before the levels
        // the levels.  (Level 0 also runs when no query has a join: the queries without one sum their views in its apply call.)
        if (g_qb.level.size() < (size_t)(maxl > 1 ? maxl : 1)) g_qb.level.resize((size_t)(maxl > 1 ? maxl : 1));
        for (int l = 0; l < maxl || l == 0; ++l) {
            if (const int rc = query_level_joins(R, l)) return rc;
            if (const int rc = query_level_apply(R, l)) return rc;
            query_take_back(R, l);
            // the queries whose prefix ends here are parked from the next level on, unless a merged node has too many rows for a
            // fold's side: such a query stays on the levels to its end
            for (uint64_t i = 0; i < n && !R.park.empty(); ++i) {
                if (R.park[i] != l + 1 || !R.st[i].alive) continue;
                if (fold_nodes_fit(queries[i], R.st[i])) continue;
                R.park[i] = 0; R.folds[i] = 0;
                if (queries[i].njoins > maxl) {
                    maxl = queries[i].njoins;
                    g_query_info.levels = (uint32_t)maxl;
                    if (g_qb.level.size() < (size_t)maxl) g_qb.level.resize((size_t)maxl);
                }
            }
        }
        if (const int rc = query_folds(R, true)) return rc;        // the nodes' pass over the parked queries still alive
    }
    uint64_t rows = 0;
    for (uint64_t i = 0; i < n; ++i) rows += queries[i].rows;
    rhj_stats &stt = g.stats;
    memset(&stt, 0, sizeof(stt));
    stt.n_r = n; stt.matches = rows;
    stt.reserved = PATH_QUERY_BATCH;
    if (timed) {
        HIP_TRY(hipEventRecord(g_qb.ev[1], g.stream));
        HIP_TRY(hipEventSynchronize(g_qb.ev[1]));
        stt.ms_total = ev_ms(g_qb.ev[0], g_qb.ev[1]);
    }
    return 0;
}

// rhj_set_query_products: a query whose bindings end in k > 1 nodes is the cross product of its k components, and the batch
// answers in sums and a row count alone, so nothing of the product is ever built: with T_c the rows of
// component c and S_v the sum of view v over its own component c(v),
//     rows = product of the T_c          sums[v] = S_v * product of the T_c, c != c(v)          (mod 2^64)
// Each component is a query of its own that query_batch takes on whatever route the switches give it.  So the caller's batch
// is validated here (query_components; -3 and nothing ran, as always), rewritten into an internal batch in which every such
// query stands as its k components, run by ONE query_batch call, and the answers are multiplied on the host.  A batch without
// such a query goes to query_batch as it came.
struct QueryPart {                                        // what one component's descriptor points to
    int                           rels[RHJ_QUERY_MAX_RELS];
    rhj_query_view                views[RHJ_QUERY_MAX_VIEWS];
    std::vector<rhj_query_filter> filters;
    std::vector<rhj_query_join>   joins;
};
struct QueryProduct {                                     // a caller's query of k > 1 components
    uint64_t query;
    int      k, comp[RHJ_QUERY_MAX_RELS];                 // binding -> component
    int64_t  item[RHJ_QUERY_MAX_RELS];                    // component -> its query of the internal batch; -1: it needed no device work ...
    uint64_t rows[RHJ_QUERY_MAX_RELS];                    // ... and has this many rows
};

// the query of component c of q, its bindings renumbered 0.. in ascending order, everything else in its order; false when the
// component has nothing a device could be asked for: one binding, no filter, no view and no column to stand in for one
static bool query_component(const rhj_query_desc &q, const int *comp, int c, const rhj_device_relation *rels, QueryPart &P,
                            rhj_query_desc &out)
{
    int id[RHJ_QUERY_MAX_RELS], nb = 0, nv = 0;
    for (int b = 0; b < q.nrels; ++b) if (comp[b] == c) { id[b] = nb; P.rels[nb++] = q.rels[b]; }
    for (int f = 0; f < q.nfilters; ++f) {
        const rhj_query_filter &p = q.filters[f];
        if (comp[p.rel] == c) P.filters.push_back({id[p.rel], p.col, p.op, p.value});
    }
    for (int l = 0; l < q.njoins; ++l) {
        const rhj_query_join &p = q.joins[l];
        if (comp[p.relA] == c) P.joins.push_back({id[p.relA], p.colA, id[p.relB], p.colB});      // (relB is in the same component: the predicate made it so)
    }
    for (int v = 0; v < q.nviews; ++v) if (comp[q.views[v].rel] == c) P.views[nv++] = {id[q.views[v].rel], q.views[v].col};
    if (nv == 0) {                                        // a stand-in view, for nviews >= 1: its sum is not read
        if (!P.joins.empty()) P.views[nv++] = {P.joins[0].relA, P.joins[0].colA};
        else if (!P.filters.empty()) P.views[nv++] = {P.filters[0].rel, P.filters[0].col};
        else {                                            // (no predicate: the component is one binding)
            const rhj_device_relation &R = rels[P.rels[0]];
            for (uint64_t col = 0; col < R.num_columns && nv == 0; ++col)
                if (R.num_tuples == 0 || R.d_columns[col]) P.views[nv++] = {0, (int)col};
            if (nv == 0) return false;
        }
    }
    out = rhj_query_desc{};
    out.nrels = nb; out.rels = P.rels;
    out.nfilters = (int)P.filters.size(); out.filters = P.filters.empty() ? nullptr : P.filters.data();
    out.njoins = (int)P.joins.size(); out.joins = P.joins.empty() ? nullptr : P.joins.data();
    out.nviews = nv; out.views = P.views;
    return true;
}

static int query_products(const rhj_device_relation *rels, int nrel, rhj_query_desc *queries, uint64_t n)
{
    if (n == 0 || !queries || (nrel > 0 && !rels)) return query_batch(rels, nrel, queries, n);
    query_infos_clear();
    bool invalid = false;                                 // the caller's batch is validated before anything else
    uint64_t nprod = 0, ncomp = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const int k = query_components(&queries[i], nrel, rels, nullptr);
        queries[i].rc = k < 0 ? -3 : 0;
        invalid |= k < 0;
        if (k > 1) { ++nprod; ncomp += (uint64_t)k; }
    }
    if (invalid) return -3;
    if (nprod == 0) return query_batch(rels, nrel, queries, n);
    // the internal batch, in the caller's order: a query of one component as it is, any other as its components
    std::vector<rhj_query_desc> iq;
    std::vector<uint64_t>       at(n);                    // a one-component query -> its place in iq
    std::vector<QueryPart>      parts(ncomp);             // (sized once: the descriptors point into them)
    std::vector<QueryProduct>   prods(nprod);
    iq.reserve(n - nprod + ncomp);
    uint64_t np = 0, npart = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const rhj_query_desc &q = queries[i];
        int comp[RHJ_QUERY_MAX_RELS];
        const int k = query_components(&q, nrel, rels, comp);
        if (k == 1) { at[i] = iq.size(); iq.push_back(q); continue; }
        QueryProduct &X = prods[np++];
        X.query = i; X.k = k;
        memcpy(X.comp, comp, sizeof(comp));
        for (int c = 0; c < X.k; ++c) {
            rhj_query_desc d;
            if (query_component(q, X.comp, c, rels, parts[npart++], d)) { X.item[c] = (int64_t)iq.size(); iq.push_back(d); continue; }
            X.item[c] = -1;
            for (int b = 0; b < q.nrels; ++b) if (X.comp[b] == c) X.rows[c] = rels[q.rels[b]].num_tuples;
        }
    }
    for (uint64_t i = 0; i < n; ++i) { memset(queries[i].sums, 0, sizeof(queries[i].sums)); queries[i].rows = 0; }
    const int rc = query_batch(rels, nrel, iq.data(), iq.size());       // (iq is not empty: the component of a query's first view has a query)
    g_query_products_info.product_queries = (uint32_t)nprod;
    g_query_products_info.components = (uint32_t)ncomp;
    if (rc) return rc;
    // the answers.  A product of 0 rows, a component's or the wrapped product's, reads as empty: rows 0 and sums 0, the batch's rule.
    uint64_t total = 0;
    np = 0;
    for (uint64_t i = 0; i < n; ++i) {
        rhj_query_desc &q = queries[i];
        if (np == nprod || prods[np].query != i) {
            memcpy(q.sums, iq[at[i]].sums, sizeof(q.sums));
            q.rows = iq[at[i]].rows;
            total += q.rows;
            continue;
        }
        QueryProduct &X = prods[np++];
        uint64_t rows = 1;
        for (int c = 0; c < X.k; ++c) {
            if (X.item[c] >= 0) X.rows[c] = iq[(size_t)X.item[c]].rows;
            rows *= X.rows[c];
        }
        if (rows == 0) continue;
        int seen[RHJ_QUERY_MAX_RELS] = {};                // component -> its views taken so far: view v is its component's next one
        for (int v = 0; v < q.nviews; ++v) {
            const int c = X.comp[q.views[v].rel];
            uint64_t s = iq[(size_t)X.item[c]].sums[seen[c]++];
            for (int o = 0; o < X.k; ++o) if (o != c) s *= X.rows[o];
            q.sums[v] = s;
        }
        q.rows = rows;
        total += rows;
    }
    g.stats.n_r = n; g.stats.matches = total;             // the caller's batch, not the internal one: its queries and their rows
    return 0;
}

// stable selection of the tuples whose bucket lies in [bucket_lo, bucket_hi) (on the calling thread's context, no API lock)
static int select_range(const rhj_tuple *d_in, uint64_t n, uint32_t bucket_lo, uint32_t bucket_hi, rhj_tuple *d_out, uint64_t capacity,
                        uint64_t *count)
{
    if (ctx_init()) return -1;
    *count = 0;
    if (n == 0 || bucket_hi <= bucket_lo) return 0;
    const uint32_t mask = (1u << g.bits) - 1u;
    const uint64_t tiles = (n + SH_TILE - 1) / SH_TILE;
    if (ensure(g.ftile, tiles * 8) || ensure(g.fbase, tiles * 8) || ensure(g.summary, sizeof(PlanSummary))) return -1;
    uint64_t *total = &((PlanSummary *)g.summary.p)->matches;
    RHJ_LAUNCH(k_select_count, dim3((unsigned)tiles), dim3(SH_BLOCK), 0, g.stream, d_in, n, mask, bucket_lo, bucket_hi,
               (uint64_t *)g.ftile.p);
    if (launch_offsets((const uint64_t *)g.ftile.p, (uint64_t *)g.fbase.p, nullptr, tiles, tiles, total)) return -1;
    RHJ_LAUNCH(k_select_write, dim3((unsigned)tiles), dim3(SH_BLOCK), 0, g.stream, d_in, n, mask, bucket_lo, bucket_hi,
               (const uint64_t *)g.fbase.p, d_out, capacity);
    HIP_TRY(hipMemcpyAsync(&g.pin->hits, total, 8, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g.stream));
    *count = g.pin->hits;
    return *count > capacity ? 1 : 0;
}

// (on the calling thread's context, without the API lock: the public entries below, and the per-device workers of a
// multi-device join; q.matches may be null)
static int join_range(JoinReq q, uint32_t bucket_lo, uint32_t bucket_hi, uint64_t first_skip = 0, uint64_t last_end = 0)
{
    uint64_t *const matches = q.matches;
    uint64_t m = 0;
    q.matches = &m;
    if (matches) *matches = 0;
    if (q.ctx_out) *q.ctx_out = nullptr;
    if (g.order_any) { fprintf(stderr, "rhj_join_device_range: bucket numbers belong to the caller's radix; not with RHJ_ORDER=any\n"); return -3; }
    const uint32_t bins = 1u << q.bits;
    if (bucket_hi > bins) bucket_hi = bins;
    if (bucket_lo >= bucket_hi) return 0;                     // an empty range joins nothing
    const bool whole = bucket_lo == 0 && bucket_hi == bins && !first_skip && !last_end;
    q.range_lo = bucket_lo;
    q.range_span = whole ? 0u : bucket_hi - bucket_lo;        // the whole radix is the ordinary join (small path and all)
    q.slice_skip = first_skip; q.slice_end = last_end;
    const int rc = join_device(q);
    if (matches) *matches = m;
    return rc;
}

// ---- several devices behind the C interface (RHJ_DEVICES; 8e: bucket b of R only meets bucket b of S) ------------
// The knobs live in the library's own context; the others take them over at the start of every multi-device call.
static void adopt_knobs(Ctx &d, const Ctx &s)
{
    d.bits = s.bits; d.null_on_empty = s.null_on_empty; d.force_hbm = s.force_hbm; d.order_any = s.order_any;
    d.no_fused = s.no_fused; d.force_fused = s.force_fused; d.no_resident = s.no_resident; d.wide_row_ids = s.wide_row_ids;
    d.timing = s.timing; d.no_count_in_pass1 = s.no_count_in_pass1; d.no_spec = s.no_spec; d.no_exact = s.no_exact;
    d.walk_count = s.walk_count;
    d.lo_override = s.lo_override; d.msd = s.msd; d.no_lowradix = s.no_lowradix; d.no_small = s.no_small; d.small_tiles = s.small_tiles;
    d.node_pairs = s.node_pairs;
}

static int set_devices(int n)
{
    if (n < 1 || n > MAX_DEVICES) return -1;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return -1;
    const int base = g_all[0].device;
    if (!g_same_device && base + n > count) {
        fprintf(stderr, "rhj_set_devices(%d): devices %d..%d asked for, %d visible\n", n, base, base + n - 1, count);
        return -1;
    }
    for (int d = 1; d < n; ++d) {
        const int ordinal = g_same_device ? base : base + d;
        if (g_all[d].ready && g_all[d].device != ordinal) return -1;          // (a context does not move to another device)
        g_all[d].device = ordinal;
    }
    if (!g_same_device)
        for (int a = 0; a < n; ++a)                                           // best effort: peer copies of pair lists go direct over xGMI
            for (int b = 0; b < n; ++b)
                if (a != b && hipSetDevice(base + a) == hipSuccess && hipDeviceEnablePeerAccess(base + b, 0) != hipSuccess) (void)hipGetLastError();
    (void)hipSetDevice(base);
    g_ndev = n;
    return 0;
}

static int devices_ready()
{
    if (g_ndev_env > 1 && g_ndev == 1) { const int want = g_ndev_env; g_ndev_env = 0; return set_devices(want); }
    return 0;
}

// the d-th of n contiguous bucket ranges of equal width (shard.equal_ranges: no histogram, no read-back)
static inline uint32_t range_cut(uint32_t bins, int n, int d) { return (uint32_t)((uint64_t)bins * (uint64_t)d / (uint64_t)n); }

// Runs fn(d) for every device d of the set on a thread of its own whose current context is device d's (d = 0 included: the
// calling thread holds the API lock and only waits).  One device: on the calling thread.
template <class F> static void on_devices(int n, F fn)
{
    if (n == 1) { fn(0); return; }
    std::vector<std::thread> pool;
    pool.reserve((size_t)n);
    for (int d = 0; d < n; ++d)
        pool.emplace_back([d, &fn]() {
            g_cur = &g_all[d];
            if (d) adopt_knobs(g_all[d], g_all[0]);
            try { fn(d); } catch (...) { }             // (nothing may leave a thread; fn records its own result, preset to failure)
        });
    for (auto &t : pool) t.join();
}

}  // namespace

// ------------------------------------------------------------------ C-ABI

extern "C" {

// (rhj_api_lock / rhj_api_unlock: rhj_host.cpp)

int rhj_set_radix_bits(int bits)
{
    RhjApiLock api_lock;
    if (bits < 1 || bits > MAX_BITS) return -1;
    g.bits = bits;
    return 0;
}
int rhj_get_radix_bits(void) { return g.bits; }
void rhj_set_empty_mode(int null_on_empty) { g.null_on_empty = null_on_empty; }
void rhj_set_node_pairs(uint64_t pairs) { g.node_pairs = pairs; }
void rhj_set_force_hbm_table(int on) { g.force_hbm = on; }
void rhj_set_fused(int on) { g.no_fused = !on; g.force_fused = on >= 2; }
void rhj_set_resident(int on) { g.no_resident = !on; }
void rhj_set_small(int on) { g.no_small = !on; }
void rhj_set_lowradix(int on) { g.no_lowradix = !on; }
void rhj_set_spec(int on) { g.no_spec = !on; g.spec_score = 2; g.spec_skipped = 0; }
int rhj_last_spec(void) { return g.last_spec; }
void rhj_set_exact(int on) { g.no_exact = !on; g.exact_score = 2; g.exact_skipped = 0; }
int rhj_last_exact(void) { return g.last_exact; }
void rhj_set_walk_count(int on) { g.walk_count = on != 0; }
int64_t rhj_last_walk_units(void) { return g.last_walk_units; }
void rhj_set_count_in_pass1(int on) { g.no_count_in_pass1 = !on; }
void rhj_set_order(int any) { g.order_any = any != 0; }
int rhj_auto_radix_bits(uint64_t nR, uint64_t nS) { return auto_radix_bits(nR, nS); }
int rhj_sub_bits(int bits, uint64_t nR, uint64_t nS) { return bits < 1 || bits > MAX_BITS ? -1 : lowradix_sub_bits(bits, nR, nS); }
int rhj_get_order(void) { return g.order_any; }
void rhj_set_timing(int level) { g.timing = level < 0 ? 0 : level > 2 ? 2 : level; }
/* diagnostic: copy the per-unit phase stamps of the last fused run (RHJ_STAMPS=1) */
int rhj_debug_stamps(uint64_t *host, uint64_t units)
{
    RhjApiLock api_lock;
    if (!g.dbg.p) return -1;
    return hipMemcpy(host, g.dbg.p, units * 64, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#ifdef RHJ_INSTRUMENT
/* diagnostics build only: per-workgroup start / end stamps of the small path's two partition kernels */
int rhj_debug_small_stamps(uint64_t *host)
{
    RhjApiLock api_lock;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_sm_dbg), sizeof(uint64_t) * 4 * 2048) == hipSuccess ? 0 : -1;
}
/* diagnostics build only: phase stamps of pass 2's workgroups (tools/exp_sr_stamps.py) */
int rhj_debug_sr_stamps(uint64_t *host)
{
    RhjApiLock api_lock;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_sr_dbg), sizeof(uint64_t) * 256 * 16) == hipSuccess ? 0 : -1;
}
/* diagnostics build only: rate of random 16-byte gathers from per-workgroup regions (tools/gather_bench.py) */
int rhj_debug_gather_bench(uint32_t region_elems, uint32_t rounds, uint32_t stream_per_round, uint32_t wgs, float *ms)
{
    RhjApiLock api_lock;
    if (ctx_init()) return -1;
    const size_t reg_bytes = (size_t)wgs * region_elems * 16, str_bytes = (size_t)wgs * rounds * (stream_per_round ? stream_per_round : 1) * FJ_BLOCK * 16;
    void *reg = nullptr, *str = nullptr, *sink = nullptr;
    if (hipMalloc(&reg, reg_bytes) != hipSuccess || hipMalloc(&str, str_bytes) != hipSuccess || hipMalloc(&sink, FJ_BLOCK * 16) != hipSuccess) return -1;
    HIP_TRY(hipMemsetAsync(reg, 1, reg_bytes, g.stream));
    HIP_TRY(hipMemsetAsync(str, 2, str_bytes, g.stream));
    for (int rep = 0; rep < 3; ++rep) {
        RHJ_STAGE(ST_HIST);
        RHJ_LAUNCH(k_gather_bench, dim3(wgs), dim3(FJ_BLOCK), 0, g.stream, (const rhj_tuple *)reg, region_elems, rounds,
                   (const uint4 *)str, stream_per_round, (uint4 *)sink);
        RHJ_STAGE(ST_END);
        HIP_TRY(hipStreamSynchronize(g.stream));
    }
    *ms = stage_ms(ST_HIST, ST_END);
    (void)hipFree(reg); (void)hipFree(str); (void)hipFree(sink);
    return 0;
}
#endif
int rhj_set_device(int ordinal)
{
    RhjApiLock api_lock;
    if (g.ready) return -1;
    g.device = ordinal;
    return 0;
}
int rhj_get_device(void) { return g.device; }
void rhj_set_stream(void *s)
{
    RhjApiLock api_lock;
    // s is a hipStream_t; NULL is HIP's default (null) stream, which is what PyTorch's default
    // stream is: work the caller queued there is ordered before ours.  Until this is called the
    // library launches on a non-blocking stream of its own.
    if (g.own_stream && g.stream) { (void)hipStreamDestroy(g.stream); g.own_stream = false; }
    g.stream = (hipStream_t)s;
    g.stream_set = true;
}
const rhj_stats *rhj_last_stats(void) { return &g.stats; }
const char *rhj_version(void) { return "rhj-mi355x 0.1 (gfx950)"; }

int rhj_join_device(const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS, rhj_result_tuple *d_out,
                    uint64_t out_capacity, uint64_t *matches)
{
    RhjApiLock api_lock;
    uint64_t m = 0;
    const int rc = join_device({d_R, nR, d_S, nS, d_out, out_capacity, false, nullptr, &m, g.bits});
    if (matches) *matches = m;
    return rc;
}

/* Many independent joins in one call (include/rhj.h; join_batch above) */
int rhj_join_batch_device(rhj_join_desc *joins, uint64_t n)
{
    RhjApiLock api_lock;
    return join_batch(joins, n);
}
int rhj_batch_takes(int bits, uint64_t nR, uint64_t nS) { return batch_takes(bits, nR, nS); }

/* The same for joins whose relations are key columns read through optional row-id vectors (include/rhj.h): the batched
 * launches read {col[sel ? sel[i] : i], i} themselves (k_batch_hist_cols, k_batch_scatter_cols), no relation is materialised */
int rhj_join_cols_batch_device(rhj_join_cols_desc *joins, uint64_t n)
{
    RhjApiLock api_lock;
    return join_batch(joins, n);
}

/* The join of two relations given as KEY COLUMNS: tuple i of a relation is {keys[i], i} — what GetRelation makes of a base
 * relation (inter_res.c:199-204, :223-227: row_id = i) — without materialising the 16-byte tuples: on the two-pass partition
 * (9..15 radix bits) pass 1 reads the columns themselves, 8 bytes a tuple instead of 16 (the north_star's "coalesced uint64
 * column loads"); on every other path the tuples are built first (one streaming kernel) and the ordinary join runs.  Same
 * pairs, same order as rhj_join_device on the materialised relations. */
static int keys_two_pass(const JoinReq &q)
{
    return !g.order_any && q.bits > PT_MAX_BITS && !split_bits(q) && !g.wide_row_ids && !g.no_fused && !g.force_hbm && q.nR && q.nS;
}

int rhj_join_keys_device(const uint64_t *d_keysR, uint64_t nR, const uint64_t *d_keysS, uint64_t nS, rhj_result_tuple *d_out,
                         uint64_t out_capacity, uint64_t *matches)
{
    RhjApiLock api_lock;
    uint64_t m = 0;
    if (matches) *matches = 0;
    if (nR >= (1ull << 32) || nS >= (1ull << 32)) return -2;
    JoinReq q = {(const rhj_tuple *)d_keysR, nR, (const rhj_tuple *)d_keysS, nS, d_out, out_capacity, false, nullptr, &m, g.bits};
    q.cols_input = keys_two_pass(q);
    if (!q.cols_input) {
        if (ctx_init() || ensure(g.inR, (nR ? nR : 1) * sizeof(rhj_tuple)) || ensure(g.inS, (nS ? nS : 1) * sizeof(rhj_tuple))) return -1;
        if (rhj_build_relation_device(d_keysR, nullptr, nR, (rhj_tuple *)g.inR.p) || rhj_build_relation_device(d_keysS, nullptr, nS, (rhj_tuple *)g.inS.p)) return -1;
        q.R = (const rhj_tuple *)g.inR.p; q.S = (const rhj_tuple *)g.inS.p;
    }
    const int rc = join_device(q);
    if (matches) *matches = m;
    return rc;
}

/* One join on columns read through optional row-id vectors (include/rhj.h): tuple i of a relation is {col[sel ? sel[i] : i], i}.
 * Where the small path takes the join its partition launches read exactly that (k_small_hist_cols, k_small_scatter_cols);
 * on every other route the relations are materialised first (join_device), except that two whole columns on the two-pass
 * partition are read as rhj_join_keys_device reads them.  Same pairs, same order as rhj_join_device() on the relations
 * rhj_build_relation_device() makes. */
int rhj_join_cols_device(const uint64_t *d_colR, const uint64_t *d_selR, uint64_t nR, const uint64_t *d_colS, const uint64_t *d_selS,
                         uint64_t nS, rhj_result_tuple *d_out, uint64_t out_capacity, uint64_t *matches)
{
    RhjApiLock api_lock;
    uint64_t m = 0;
    if (matches) *matches = 0;
    if ((nR && !d_colR) || (nS && !d_colS)) return -3;
    if (nR >= (1ull << 32) || nS >= (1ull << 32)) return -2;
    JoinReq q = {nullptr, nR, nullptr, nS, d_out, out_capacity, false, nullptr, &m, g.bits};
    if (!d_selR && !d_selS && keys_two_pass(q)) {
        q.R = (const rhj_tuple *)d_colR; q.S = (const rhj_tuple *)d_colS;
        q.cols_input = 1;
    } else {
        q.via_sel = true;
        q.srcR = ColSrc{d_colR, d_selR}; q.srcS = ColSrc{d_colS, d_selS};
    }
    const int rc = join_device(q);
    if (matches) *matches = m;
    return rc;
}

/* One rank's share of a join sharded by bucket range (bucket b of R only meets bucket b of S, rhjoin.c:42-57):
 * the canonical result restricted to the buckets [bucket_lo, bucket_hi) of the current radix.  The first partition pass
 * drops the other buckets' tuples while it reads the relations — one read of each relation, no selection pass and no
 * host round trip in front of the join; the concatenation of the ranks' results in range order is the canonical result. */
int rhj_join_device_range(const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS, uint32_t bucket_lo, uint32_t bucket_hi,
                          rhj_result_tuple *d_out, uint64_t out_capacity, uint64_t *matches)
{
    RhjApiLock api_lock;
    return join_range({d_R, nR, d_S, nS, d_out, out_capacity, false, nullptr, matches, g.bits}, bucket_lo, bucket_hi);
}

/* A share cut INSIDE buckets (a hot bucket joined by several devices): the buckets [bucket_lo, bucket_hi) as above, but of the
 * first one only the probe tuples from first_skip on take part and of the last one (bucket_hi - 1) only those before last_end
 * (0: all of them) — positions among the tuples of the bucket's probe side (R when |R_b| >= |S_b|, rhjoin.c:86) in partition
 * order; the build side of a cut bucket is whole on every device that has a piece of it.  The result is the canonical list's
 * pairs of exactly those probe tuples (rhjoin.c:141-217 walks a bucket's probe tuples in order), so shares that tile the
 * (bucket, probe position) space concatenate to the canonical result. */
int rhj_join_device_slice(const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS, uint32_t bucket_lo, uint32_t bucket_hi,
                          uint64_t first_skip, uint64_t last_end, rhj_result_tuple *d_out, uint64_t out_capacity, uint64_t *matches)
{
    RhjApiLock api_lock;
    return join_range({d_R, nR, d_S, nS, d_out, out_capacity, false, nullptr, matches, g.bits}, bucket_lo, bucket_hi, first_skip, last_end);
}

int rhj_set_devices(int n) { RhjApiLock api_lock; g_ndev_env = 0; return set_devices(n); }
/* Contiguous bucket ranges for n devices balanced by histR + histS (skewed keys): cuts[d] .. cuts[d + 1] is device d's range.
 * shard.bucket_ranges in C: the first bucket at which the running total reaches d / n of all tuples; no device needed. */
int rhj_plan_device_ranges(const uint64_t *histR, const uint64_t *histS, int bits, int n, uint32_t *cuts)
{
    if (bits < 1 || bits > MAX_BITS || n < 1 || n > MAX_DEVICES) return -1;
    const uint32_t bins = 1u << bits;
    double total = 0.0;
    for (uint32_t b = 0; b < bins; ++b) total += (double)histR[b] + (double)histS[b];
    cuts[0] = 0;
    uint32_t at = 0;
    double cum = 0.0;                                  // tuples in front of bucket `at`
    for (int d = 1; d < n; ++d) {
        const double target = total * (double)d / (double)n;
        while (at < bins && cum < target) { cum += (double)histR[at] + (double)histS[at]; ++at; }
        cuts[d] = at;
    }
    cuts[n] = bins;
    return 0;
}
/* The same with cuts INSIDE hot buckets: device d joins from (cut_bucket[d], cut_off[d]) up to (cut_bucket[d + 1], cut_off[d + 1])
 * in (bucket, probe position) order — rhj_cut_to_slice turns two neighbouring cuts into rhj_join_device_slice's arguments.  A cut
 * falls inside a bucket only when that bucket holds at least 1 / (2 n) of all tuples and both relations have tuples in it: the
 * device in front takes the bucket's build side and the probe tuples up to the cut (a multiple of 256; not a sliver: a cut that would
 * leave less than an eighth of the probe side on one side goes to that boundary), so that its tuples reach d / n of the total; every
 * other cut is the range planner's bucket boundary.  shard.bucket_slices in C (integer arithmetic). */
int rhj_plan_device_slices(const uint64_t *histR, const uint64_t *histS, int bits, int n, uint32_t *cut_bucket, uint64_t *cut_off)
{
    if (bits < 1 || bits > MAX_BITS || n < 1 || n > MAX_DEVICES) return -1;
    const uint32_t bins = 1u << bits;
    unsigned __int128 total = 0;
    for (uint32_t b = 0; b < bins; ++b) total += (unsigned __int128)histR[b] + histS[b];
    cut_bucket[0] = 0; cut_off[0] = 0;
    uint32_t at = 0;
    unsigned __int128 cum = 0;                         // tuples in front of bucket `at`
    for (int d = 1; d < n; ++d) {
        const unsigned __int128 target = total * (unsigned)d / (unsigned)n;
        while (at < bins && cum + histR[at] + histS[at] <= target) { cum += (unsigned __int128)histR[at] + histS[at]; ++at; }
        cut_bucket[d] = at; cut_off[d] = 0;            // (all buckets in front of `at` end at or before the target)
        if (at == bins) continue;
        const uint64_t hR = histR[at], hS = histS[at];
        const unsigned __int128 w = (unsigned __int128)hR + hS;
        const bool hot = hR != 0 && hS != 0 && w * 2u * (unsigned)n >= total;
        if (!hot) {
            if (cum < target) { cum += w; ++at; cut_bucket[d] = at; }      // the first boundary at or behind the target
            continue;
        }
        const uint64_t pc = hR >= hS ? hR : hS, bc = hR >= hS ? hS : hR;
        uint64_t off = target > cum + bc ? (uint64_t)(target - cum - bc) : 0u;
        off &= ~(uint64_t)255;
        if (off * 8u < pc) off = 0;                    // (a sliver of a bucket is not worth a second partition of its build side:
        else if ((pc - off) * 8u < pc) off = pc;       //  less than an eighth of the probe side on either side goes to the boundary)
        if (off >= pc) { cum += w; ++at; cut_bucket[d] = at; }
        else cut_off[d] = off;
    }
    cut_bucket[n] = bins; cut_off[n] = 0;
    return 0;
}
/* cuts d and d + 1 of rhj_plan_device_slices -> the arguments of rhj_join_device_slice */
void rhj_cut_to_slice(uint32_t b0, uint64_t o0, uint32_t b1, uint64_t o1, uint32_t *bucket_lo, uint32_t *bucket_hi, uint64_t *first_skip,
                      uint64_t *last_end)
{
    *bucket_lo = b0; *first_skip = o0;
    if (o1) { *bucket_hi = b1 + 1u; *last_end = o1; } else { *bucket_hi = b1; *last_end = 0; }
}
void rhj_set_devices_balance(int mode) { RhjApiLock api_lock; g_balance = mode < 0 ? 0 : mode > 2 ? 2 : mode; }

/* the bucket range device d of n joins at `bits` radix bits (no device needed: the planning half of rhj_join_devices) */
int rhj_device_range(int bits, int n, int d, uint32_t *lo, uint32_t *hi)
{
    if (bits < 1 || bits > MAX_BITS || n < 1 || n > MAX_DEVICES || d < 0 || d >= n) return -1;
    *lo = range_cut(1u << bits, n, d);
    *hi = range_cut(1u << bits, n, d + 1);
    return 0;
}
int rhj_get_devices(void) { RhjApiLock api_lock; (void)devices_ready(); return g_ndev; }

/* One join over the devices of rhj_set_devices(n).  d_R[d] / d_S[d]: the relations ON device d (replicated: a device-resident
 * column store per GPU).  Device d joins the d-th of n equal-width bucket ranges with its own context, stream and workspace,
 * driven by a host thread of its own (rhj_join_device_range's one call per rank, inside one process), and leaves its pairs in
 * out[d] (capacity[d] of them; matches[d] = their number, the call returns 1 when some list did not fit).  The concatenation
 * of the lists in device order is the canonical result. */
int rhj_join_devices(const rhj_tuple *const *d_R, uint64_t nR, const rhj_tuple *const *d_S, uint64_t nS,
                     rhj_result_tuple *const *out, const uint64_t *capacity, uint64_t *matches)
{
    RhjApiLock api_lock;
    if (devices_ready()) return -1;
    const int n = g_ndev;
    const int bits = g_all[0].bits;
    const uint32_t bins = 1u << bits;
    uint32_t cuts[MAX_DEVICES + 1];
    uint64_t offs[MAX_DEVICES + 1] = {0};
    for (int d = 0; d <= n; ++d) cuts[d] = range_cut(bins, n, d);
    if (g_balance && n > 1 && nR && nS) {
        // skewed keys: the library's own device counts both relations' buckets (two launches, one read-back of 2^bits words each)
        if (ctx_init() || ensure(g.passhp, (size_t)2 * bins * 8)) return -1;
        uint64_t *d_h = (uint64_t *)g.passhp.p;
        std::vector<uint64_t> h((size_t)2 * bins);
        if (rhj_bucket_histogram_device(d_R[0], nR, d_h) || rhj_bucket_histogram_device(d_S[0], nS, d_h + bins)) return -1;
        HIP_TRY(hipMemcpyAsync(h.data(), d_h, (size_t)2 * bins * 8, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        if (g_balance == 2 ? rhj_plan_device_slices(h.data(), h.data() + bins, bits, n, cuts, offs)
                           : rhj_plan_device_ranges(h.data(), h.data() + bins, bits, n, cuts)) return -1;
    }
    int rcs[MAX_DEVICES];
    for (int d = 0; d < MAX_DEVICES; ++d) rcs[d] = -1;
    try {
        on_devices(n, [&](int d) {
            uint32_t lo, hi;
            uint64_t skip, end;
            rhj_cut_to_slice(cuts[d], offs[d], cuts[d + 1], offs[d + 1], &lo, &hi, &skip, &end);
            rcs[d] = join_range({d_R[d], nR, d_S[d], nS, out[d], capacity[d], false, nullptr, &matches[d], g.bits}, lo, hi, skip, end);
        });
    } catch (...) { return -1; }
    int rc = 0;
    for (int d = 0; d < n; ++d) { if (rcs[d] < 0) return rcs[d]; if (rcs[d] > rc) rc = rcs[d]; }
    return rc;
}

/* The whole pair list on one device of the set: device d's list (lists[d], matches[d] pairs, as rhj_join_devices left them) is
 * copied to dst + (the pairs of the devices in front of d) — exact sizes, peer to peer (xGMI), on dst_device's stream.  Only a
 * caller whose next operator lives on ONE device needs it (north_star: a match list crosses only when its consumer is elsewhere). */
int rhj_gather_pairs_devices(const rhj_result_tuple *const *lists, const uint64_t *matches, int dst_device, rhj_result_tuple *dst,
                             uint64_t capacity, uint64_t *total)
{
    RhjApiLock api_lock;
    if (devices_ready() || dst_device < 0 || dst_device >= g_ndev) return -1;
    uint64_t sum = 0;
    for (int d = 0; d < g_ndev; ++d) sum += matches[d];
    if (total) *total = sum;
    if (sum > capacity) return 1;
    Ctx *keep = g_cur;
    g_cur = &g_all[dst_device];
    int rc = ctx_init();
    uint64_t at = 0;
    for (int d = 0; d < g_ndev && !rc; ++d) {
        if (matches[d] && (lists[d] != dst + at || d != dst_device))
            if (hipMemcpyPeerAsync(dst + at, g_all[dst_device].device, lists[d], g_all[d].device, matches[d] * sizeof(rhj_result_tuple), g.stream) != hipSuccess) rc = -1;
        at += matches[d];
    }
    if (!rc && hipStreamSynchronize(g.stream) != hipSuccess) rc = -1;
    g_cur = keep;
    (void)hipSetDevice(g.device);
    return rc;
}

int rhj_partition_device(const rhj_tuple *d_in, uint64_t n, rhj_tuple *d_out, uint64_t *h_hist, int64_t *h_psum)
{
    RhjApiLock api_lock;
    if (ctx_init()) return -1;
    const int bits = g.bits;
    const uint32_t bins = 1u << bits;
    if (n >= (1ull << 32)) return -2;
    PartState ps;
    ps.r[0] = RelArgs{d_in, d_out, nullptr, n, 0, 0, nullptr, nullptr};
    ps.tmp[0] = ps.tmp[1] = nullptr;
    if (bits > PT_MAX_BITS) {
        if (ensure(g.tmpR, (n ? n : 1) * sizeof(rhj_tuple))) return -1;
        ps.tmp[0] = (rhj_tuple *)g.tmpR.p;
    }
    uint64_t *hh = (uint64_t *)malloc((size_t)2 * bins * 8);
    if (!hh) return -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (run_partition(ps, bits, 1, attempt == 1 || g.wide_row_ids != 0, false)) { free(hh); return -1; }
        RHJ_STAGE(ST_PLAN);
        PlanSummary *hs = &g.pin->summary;
        HIP_TRY(hipMemcpyAsync(hh, ps.hist, (size_t)bins * 8, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipMemcpyAsync(hh + bins, ps.psum, (size_t)bins * 8, hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipMemcpyAsync(hs, g.summary.p, sizeof(PlanSummary), hipMemcpyDeviceToHost, g.stream));
        HIP_TRY(hipStreamSynchronize(g.stream));
        if (!hs->row_id_overflow) break;                      // else: a row id above 2^32 - 1 met a 12-byte intermediate
        g.seen_wide = 1;
    }
    for (uint32_t b = 0; b < bins; ++b) {
        if (h_hist) h_hist[b] = hh[b];
        if (h_psum) h_psum[b] = hh[b] ? (int64_t)hh[bins + b] : -1;      // preprocess.c:336-347
    }
    free(hh);
    memset(&g.stats, 0, sizeof(g.stats));
    g.stats.n_r = n; g.stats.radix_bits = bits;
    g.stats.ms_hist = stage_ms(ST_HIST, ST_SCAN);
    g.stats.ms_scan = stage_ms(ST_SCAN, ST_SCATTER);
    g.stats.ms_scatter = stage_ms(ST_SCATTER, ST_PLAN);
    g.stats.ms_total = stage_ms(ST_HIST, ST_PLAN);
    return 0;
}

int rhj_filter_device(const uint64_t *d_col, const uint64_t *d_sel, uint64_t n, char op, uint64_t value,
                      uint64_t *d_out, uint64_t *hits)
{
    RhjApiLock api_lock;
    uint64_t h = 0;
    const int rc = filter_device(d_col, d_sel, n, op, value, d_out, false, nullptr, &h);
    if (hits) *hits = h;
    return rc;
}

/* Many independent conjunctive filters in one call (include/rhj.h; filter_batch above) */
int rhj_filter_batch_device(rhj_filter_desc *filters, uint64_t n)
{
    RhjApiLock api_lock;
    return filter_batch(filters, n);
}
int rhj_filter_batch_takes(uint64_t rows) { return filter_batch_takes(rows); }

/* Many row-id rebuilds and view sums in one call (include/rhj_inter.h; apply_batch above) */
int rhj_apply_batch_device(rhj_apply_desc *items, uint64_t n)
{
    RhjApiLock api_lock;
    return apply_batch(items, n);
}

/* Many two-column equalities in one call (include/rhj_inter.h; filter_batch above) */
int rhj_filter_eq2_batch_device(rhj_eq2_desc *items, uint64_t n)
{
    RhjApiLock api_lock;
    return filter_batch(items, n);
}

/* The statistics of many columns in one call (include/rhj_inter.h; stats_batch above) */
int rhj_column_stats_batch_device(rhj_colstats_desc *cols, uint64_t n)
{
    RhjApiLock api_lock;
    return stats_batch(cols, n);
}
uint64_t rhj_column_stats_flags(uint64_t l, uint64_t u) { return stats_flags(l, u); }
const rhj_colstats_batch_info *rhj_column_stats_batch_last_info(void) { return &g_stats_info; }

/* A batch of queries run level by level through the batched entry points (include/rhj_inter.h; query_batch above) */
int rhj_query_batch_device(const rhj_device_relation *rels, int nrel, rhj_query_desc *queries, uint64_t n)
{
    RhjApiLock api_lock;
    g_combine_info = {}; g_resident_info = {}; g_resident_keys_info = {};
    return g_query_products ? query_products(rels, nrel, queries, n) : query_batch(rels, nrel, queries, n);
}
void rhj_set_fold_combine(int on) { RhjApiLock api_lock; g_fold_combine = on != 0; }
int rhj_get_fold_combine(void) { return g_fold_combine; }
const rhj_table_batch_combine_info *rhj_table_batch_last_combine_info(void) { return &g_combine_info; }
void rhj_set_fold_resident(int on) { RhjApiLock api_lock; g_fold_resident = on != 0; }
int rhj_get_fold_resident(void) { return g_fold_resident; }
int rhj_fold_resident_rule(uint64_t nR, uint64_t nS, int nvalues) { return fold_resident_rule(nR, nS, nvalues); }
const rhj_table_batch_resident_info *rhj_table_batch_last_resident_info(void) { return &g_resident_info; }
void rhj_set_fold_resident_keys(int on) { RhjApiLock api_lock; g_fold_resident_keys = on != 0; }
int rhj_get_fold_resident_keys(void) { return g_fold_resident_keys; }
int rhj_fold_resident_keys_rule(uint64_t nR, uint64_t nS, int nvalues) { return fold_keys_resident_rule(nR, nS, nvalues); }
const rhj_table_batch_resident_info *rhj_table_batch_last_resident_keys_info(void) { return &g_resident_keys_info; }
int rhj_query_components(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, int *comp) { return query_components(q, nrel, rels, comp); }
void rhj_set_query_products(int on) { RhjApiLock api_lock; g_query_products = on != 0; }
const rhj_query_batch_products_info *rhj_query_batch_last_products_info(void) { return &g_query_products_info; }
int rhj_query_levels(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, int *kinds) { return query_levels(q, nrel, rels, kinds); }
const rhj_query_batch_info *rhj_query_batch_last_info(void) { return &g_query_info; }
const rhj_query_batch_sum_info *rhj_query_batch_last_sum_info(void) { return &g_query_sum_info; }
void rhj_set_query_sum_last(int on) { RhjApiLock api_lock; g_query_sum_last = on != 0; }
const rhj_query_batch_fold_info *rhj_query_batch_last_fold_info(void) { return &g_query_fold_info; }
void rhj_set_query_fold(int on) { RhjApiLock api_lock; g_query_fold = on != 0; }
const rhj_query_batch_foldk_info *rhj_query_batch_last_foldk_info(void) { return &g_query_foldk_info; }
const rhj_query_batch_fold_self_info *rhj_query_batch_last_fold_self_info(void) { return &g_query_fold_self_info; }
void rhj_set_query_fold_self(int on) { RhjApiLock api_lock; g_query_fold_self = on != 0; }
int rhj_query_folds_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, rhj_folds_plan *plan) { return query_folds_plan(q, nrel, rels, plan); }
int rhj_query_foldn_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, rhj_foldn_plan *plan) { return query_foldn_plan(q, nrel, rels, plan); }
void rhj_set_query_fold_keys(int on) { RhjApiLock api_lock; g_query_fold_keys = on != 0; }
void rhj_set_query_fold_nodes(int on) { RhjApiLock api_lock; g_query_fold_nodes = on != 0; }
void rhj_set_query_fold_node_rows(uint64_t limit) { RhjApiLock api_lock; g_query_fold_node_rows = limit < JSUM_MAX_ROWS ? limit : JSUM_MAX_ROWS; }
const rhj_query_batch_fold_nodes_info *rhj_query_batch_last_fold_nodes_info(void) { return &g_query_fold_nodes_info; }
void rhj_set_query_fold_one_wait(int on) { RhjApiLock api_lock; g_query_fold_one_wait = on != 0; }
void rhj_set_query_fold_one_wait_rows(uint64_t limit) { RhjApiLock api_lock; g_query_fold_one_wait_rows = limit < JSUM_MAX_ROWS ? limit : JSUM_MAX_ROWS - 1; }
int rhj_query_one_wait_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels) { return query_one_wait_plan(q, nrel, rels); }
const rhj_query_batch_one_wait_info *rhj_query_batch_last_one_wait_info(void) { return &g_query_one_wait_info; }
int rhj_query_foldk_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, int *root, rhj_foldk_step *steps) { return query_foldk_plan(q, nrel, rels, root, steps); }
int rhj_query_fold_plan(const rhj_query_desc *q, int nrel, const rhj_device_relation *rels, int *root, rhj_fold_step *steps) { return query_fold_plan(q, nrel, rels, root, steps); }

int rhj_join_sum_batch_device(rhj_join_sum_desc *items, uint64_t n)
{
    RhjApiLock api_lock;
    g_combine_info = {}; g_resident_info = {}; g_resident_keys_info = {};
    return table_batch(items, n);
}

int rhj_join_foldk_batch_device(rhj_join_foldk_desc *items, uint64_t n)
{
    RhjApiLock api_lock;
    g_combine_info = {}; g_resident_info = {}; g_resident_keys_info = {};
    return table_batch(items, n);
}

int rhj_join_foldn_batch_device(rhj_join_foldn_desc *items, uint64_t n)
{
    RhjApiLock api_lock;
    g_combine_info = {}; g_resident_info = {}; g_resident_keys_info = {};
    return table_batch(items, n);
}

int rhj_join_fold_batch_device(rhj_join_fold_desc *items, uint64_t n)
{
    RhjApiLock api_lock;
    g_combine_info = {}; g_resident_info = {}; g_resident_keys_info = {};
    return table_batch(items, n);
}

int rhj_fold_self_batch_device(rhj_fold_self_desc *items, uint64_t n)
{
    RhjApiLock api_lock;
    return fold_self_batch(items, n);
}

int rhj_fold_pred_batch_device(rhj_fold_pred_desc *items, uint64_t n)
{
    RhjApiLock api_lock;
    return fold_pred_batch(items, n);
}

/* ---- bucket-range sharding of one join across GPUs (host side: sigmod-2018_amd/shard.py) ---- */

int rhj_bucket_histogram_device(const rhj_tuple *d_in, uint64_t n, uint64_t *d_hist)
{
    RhjApiLock api_lock;
    if (ctx_init()) return -1;
    const int bits = g.bits;
    HIP_TRY(hipMemsetAsync(d_hist, 0, ((size_t)8) << bits, g.stream));
    if (n) {
        uint64_t blocks = (n + SH_BLOCK * 16 - 1) / (SH_BLOCK * 16);
        if (blocks > (uint64_t)g.cus * 4) blocks = (uint64_t)g.cus * 4;
        RHJ_LAUNCH(k_bucket_hist, dim3((unsigned)blocks), dim3(SH_BLOCK), ((size_t)4) << bits, g.stream, d_in, n, bits,
                   (unsigned long long *)d_hist);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int rhj_select_bucket_range_device(const rhj_tuple *d_in, uint64_t n, uint32_t bucket_lo, uint32_t bucket_hi,
                                   rhj_tuple *d_out, uint64_t capacity, uint64_t *count)
{
    RhjApiLock api_lock;
    return select_range(d_in, n, bucket_lo, bucket_hi, d_out, capacity, count);
}

static void release_current()
{
    if (!g.ready) return;
    (void)hipSetDevice(g.device);
    (void)hipStreamSynchronize(g.stream);
#define RHJ_FREE(name) { if (g.name.p) (void)hipFree(g.name.p); g.name = Buf{}; }
    RHJ_WORKSPACE(RHJ_FREE)
#undef RHJ_FREE
    if (g.batch_pin) { (void)hipHostFree(g.batch_pin); g.batch_pin = nullptr; g.batch_pin_cap = 0; }
    for (auto &kv : g.columns) (void)hipFree(kv.second.dev);
    g.columns.clear();
    for (auto &kv : g.pinned) (void)hipHostUnregister((void *)kv.first);
    g.pinned.clear();
    for (auto &kv : g.free_blocks) (void)hipFree(kv.second);
    g.free_blocks.clear();
    for (auto &kv : g.live_blocks) (void)hipFree(kv.first);
    g.live_blocks.clear();
}

void rhj_release(void)
{
    RhjApiLock api_lock;
    rhj_host_pool_release();
    Ctx *keep = g_cur;
    g_cur = &g_all[0];
    if (g.ready) { (void)hipSetDevice(g.device); (void)hipStreamSynchronize(g.stream); query_release(); }
    for (int d = MAX_DEVICES - 1; d >= 0; --d) { g_cur = &g_all[d]; release_current(); }   // (the library's own device last: it stays current)
    g_cur = keep;
}

// ---- host-side staging used by rhj_abi.c (not part of the public header) ----

// The pairs of the calling thread's context, [d_out, d_out + M), into the caller-visible nodes as elements [base, base + M) of the
// list.  The nodes are plain malloc memory (FreeResult = free(buff); free(node), results.c:144-153): freshly mapped pages, so
// whoever writes them first pays the page faults — a single thread filling them measured 5.8 GB/s (44 ms for 256 MB).  All
// nodes are allocated up front (untouched), the pairs come through a ring of pinned staging blocks (the copy of block i+1..
// runs while block i is moved), and every block is moved into the nodes by several host threads, each faulting in its own pages.
static int pairs_to_nodes(const rhj_result_tuple *d_out, uint64_t base, uint64_t M, uint64_t node_pairs, char *const *nodes, unsigned nthreads)
{
    if (M == 0) return 0;
    constexpr int RING = 4;
    const uint64_t blk = (uint64_t)1 << 20;                               // pairs per staging block (16 MiB)
    if (!g.pin_ring[0]) {
        for (int i = 0; i < RING; ++i) {
            HIP_TRY(hipHostMalloc(&g.pin_ring[i], blk * sizeof(rhj_result_tuple), hipHostMallocDefault));
            HIP_TRY(hipEventCreate(&g.ev_ring[i]));
        }
    }
    HIP_TRY(hipEventRecord(g.ev_x[2], g.stream));
    if (nthreads < 1 || M * sizeof(rhj_result_tuple) < ((size_t)8 << 20)) nthreads = 1;
    // the ring protocol and the mover threads are host-only code (rhj_host.cpp: rhj_move_blocks_at, built and run under the
    // sanitizers on the CPU); this side only starts the copy of a block and waits for it
    struct Copy { const rhj_result_tuple *d_out; uint64_t M, blk; Ctx *c; } cp = {d_out, M, blk, g_cur};
    auto issue = [](void *c, uint64_t b) -> int {
        const Copy *k = (const Copy *)c;
        const uint64_t cnt = k->M - b * k->blk < k->blk ? k->M - b * k->blk : k->blk;
        if (hipMemcpyAsync(k->c->pin_ring[b % RING], k->d_out + b * k->blk, cnt * sizeof(rhj_result_tuple), hipMemcpyDeviceToHost, k->c->stream) != hipSuccess) return -1;
        return hipEventRecord(k->c->ev_ring[b % RING], k->c->stream) == hipSuccess ? 0 : -1;
    };
    auto landed = [](void *c, uint64_t b) -> int { return hipEventSynchronize(((const Copy *)c)->c->ev_ring[b % RING]) == hipSuccess ? 0 : -1; };
    char *staging[RING];
    for (int i = 0; i < RING; ++i) staging[i] = (char *)g.pin_ring[i];
    if (rhj_move_blocks_at(base, M, sizeof(rhj_result_tuple), node_pairs, nodes, blk, RING, staging, nthreads, issue, landed, &cp)) {
        (void)hipGetLastError();
        return -1;
    }
    HIP_TRY(hipEventRecord(g.ev_x[3], g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    g.stats.ms_d2h = ev_ms(g.ev_x[2], g.ev_x[3]);
    return 0;
}

// Upload both relations, join, and copy the pairs back into `node_pairs`-sized
// chunks handed to `sink(ctx, chunk_index, ptr_to_fill, pairs)`-allocated memory.
// With rhj_set_devices(n > 1) / RHJ_DEVICES: every device uploads both relations over its own link, joins the d-th of n
// equal-width bucket ranges (the first partition pass drops the others while it reads), and its pairs go to their place in the
// list — behind the pairs of the devices in front of it — over its own link again: n uploads side by side, 1/n of the kernel
// work and of the read-back each.
int rhj_host_join(const rhj_tuple *R, uint64_t nR, const rhj_tuple *S, uint64_t nS, uint64_t *matches,
                  void *(*alloc_chunk)(void *ctx, uint64_t pairs), void *ctx, uint64_t node_pairs)
{
    RhjApiLock api_lock;
    *matches = 0;
    if (devices_ready()) return -1;
    if (ctx_init()) return -1;
    if (nR == 0 || nS == 0) return 0;
    const int n = g_all[0].order_any ? 1 : g_ndev;             // (bucket ranges belong to the caller's radix: not with RHJ_ORDER=any)
    const uint32_t bins = 1u << g_all[0].bits;
    int rcs[MAX_DEVICES] = {0};
    uint64_t Ms[MAX_DEVICES] = {0};
    rhj_result_tuple *d_outs[MAX_DEVICES] = {nullptr};
    auto upload_and_join = [&](int d) {
        rcs[d] = -1;
        if (ctx_init()) return;
        if (ensure(g.inR, nR * sizeof(rhj_tuple)) || ensure(g.inS, nS * sizeof(rhj_tuple))) return;
        if (hipEventRecord(g.ev_x[0], g.stream) != hipSuccess ||
            hipMemcpyAsync(g.inR.p, R, nR * sizeof(rhj_tuple), hipMemcpyHostToDevice, g.stream) != hipSuccess ||
            hipMemcpyAsync(g.inS.p, S, nS * sizeof(rhj_tuple), hipMemcpyHostToDevice, g.stream) != hipSuccess ||
            hipEventRecord(g.ev_x[1], g.stream) != hipSuccess) return;
        const JoinReq q = {(const rhj_tuple *)g.inR.p, nR, (const rhj_tuple *)g.inS.p, nS, nullptr, 0, true, &d_outs[d], &Ms[d], g.bits};
        rcs[d] = n == 1 ? join_device(q) : join_range(q, range_cut(bins, n, d), range_cut(bins, n, d + 1));
        if (rcs[d] >= 0) g.stats.ms_h2d = ev_ms(g.ev_x[0], g.ev_x[1]);
    };
    try { on_devices(n, upload_and_join); } catch (...) { return -1; }
    uint64_t M = 0, base[MAX_DEVICES] = {0};
    for (int d = 0; d < n; ++d) { if (rcs[d] < 0) return rcs[d]; base[d] = M; M += Ms[d]; }
    *matches = M;
    if (M == 0) return 0;
    if (node_pairs == 0) node_pairs = M;
    const uint64_t nnodes = (M + node_pairs - 1) / node_pairs;
    std::vector<char *> nodes((size_t)nnodes);
    for (uint64_t i = 0; i < nnodes; ++i) {
        const uint64_t cnt = M - i * node_pairs < node_pairs ? M - i * node_pairs : node_pairs;
        nodes[(size_t)i] = (char *)alloc_chunk(ctx, cnt);
        if (!nodes[(size_t)i]) { fprintf(stderr, "rhj: out of host memory for %llu result pairs\n", (unsigned long long)cnt); return -1; }
    }
    unsigned nthreads = std::thread::hardware_concurrency();
    if (nthreads > 8) nthreads = 8;
    nthreads = nthreads / (unsigned)n ? nthreads / (unsigned)n : 1u;      // the devices' movers share the host's cores
    try {
        for (int d = 0; d < n; ++d) rcs[d] = -1;
        on_devices(n, [&](int d) { rcs[d] = pairs_to_nodes(d_outs[d], base[d], Ms[d], node_pairs, nodes.data(), nthreads); });
    } catch (...) { return -1; }
    for (int d = 0; d < n; ++d) if (rcs[d]) return -1;
    return 0;
}

// The device copy of a registered column, or nullptr.
static const uint64_t *registered_column(const uint64_t *host_col, uint64_t rows)
{
    auto it = g.columns.find((const void *)host_col);
    if (it == g.columns.end() || it->second.rows != rows) return nullptr;
    return (const uint64_t *)it->second.dev;
}

// Pin [base, base + bytes) for the H2D copy (relation_map.c:28-50: the columns of a relation are one
// contiguous block of the PROT_READ | MAP_PRIVATE file mapping, hence the read-only flag first).
// Returns whether the range is pinned now; a range that cannot be pinned is copied pageable.
// hipHostRegister of a host range the library copies columns from.  A read-only file mapping (InitRelationMap's
// PROT_READ | MAP_PRIVATE block) takes the read-only flag; memory the caller owns takes either.  Which flag the host
// accepted is traced (RHJ_TRACE=1) and counted: rhj_pinned_ranges(), rhj_pin_refusals().
static bool pin_range(const void *base, size_t bytes)
{
    static const bool trace = getenv("RHJ_TRACE") != nullptr;
    if (bytes < (64u << 10)) return false;                              // registration costs more than it saves
    if (g.pinned.count(base)) return true;
    const char *how = "read-only";
    hipError_t e = hipHostRegister((void *)base, bytes, hipHostRegisterReadOnly);
    if (e != hipSuccess) { (void)hipGetLastError(); how = "default"; e = hipHostRegister((void *)base, bytes, hipHostRegisterDefault); }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ++g.pin_refusals;
        if (trace) fprintf(stderr, "rhj-trace:   hipHostRegister refused %zu bytes at %p (%s): pageable copy\n", bytes, base, hipGetErrorString(e));
        return false;
    }
    if (trace) fprintf(stderr, "rhj-trace:   hipHostRegister(%s) pinned %zu bytes at %p\n", how, bytes, base);
    g.pinned[base] = bytes;
    return true;
}

static void unpin_range(const void *base)
{
    auto it = g.pinned.find(base);
    if (it == g.pinned.end()) return;
    (void)hipHostUnregister((void *)base);
    g.pinned.erase(it);
}

static int register_column(const uint64_t *host_col, uint64_t rows)
{
    auto it = g.columns.find((const void *)host_col);
    if (it != g.columns.end()) {
        if (it->second.rows == rows) return 0;
        (void)hipStreamSynchronize(g.stream);                           // registered again with another length: replace
        (void)hipFree(it->second.dev);
        g.columns.erase(it);
    }
    void *d = nullptr;
    HIP_TRY(hipMalloc(&d, (rows ? rows : 1) * 8));
    if (hipMemcpyAsync(d, host_col, rows * 8, hipMemcpyHostToDevice, g.stream) != hipSuccess) { (void)hipFree(d); return -1; }
    g.columns[(const void *)host_col] = Ctx::Column{d, (size_t)rows};
    return 0;
}

static void unregister_column(const uint64_t *host_col)
{
    auto it = g.columns.find((const void *)host_col);
    if (it == g.columns.end()) return;
    (void)hipFree(it->second.dev);
    g.columns.erase(it);
}

// are the columns of this relation one contiguous block (the layout of relation_map.c:39-50)?
static bool contiguous_columns(const rhj_relation_map *rm)
{
    for (uint64_t c = 1; c < rm->num_columns; ++c)
        if (rm->columns[c] != rm->columns[c - 1] + rm->num_tuples) return false;
    return rm->num_columns > 0;
}

int rhj_register_relation_map(const rhj_relation_map *map, int num_relations)
{
    RhjApiLock api_lock;
    if (ctx_init()) return -1;
    for (int r = 0; r < num_relations; ++r) {
        const rhj_relation_map *rm = &map[r];
        if (contiguous_columns(rm)) pin_range(rm->columns[0], (size_t)rm->num_columns * rm->num_tuples * 8);
        else for (uint64_t c = 0; c < rm->num_columns; ++c) pin_range(rm->columns[c], (size_t)rm->num_tuples * 8);
        for (uint64_t c = 0; c < rm->num_columns; ++c)
            if (register_column(rm->columns[c], rm->num_tuples)) return -1;
    }
    HIP_TRY(hipStreamSynchronize(g.stream));
    return 0;
}

int rhj_unregister_relation_map(const rhj_relation_map *map, int num_relations)
{
    RhjApiLock api_lock;
    if (!g.ready) return 0;
    HIP_TRY(hipSetDevice(g.device));
    HIP_TRY(hipStreamSynchronize(g.stream));                             // queued work may still read the device copies
    for (int r = 0; r < num_relations; ++r)
        for (uint64_t c = 0; c < map[r].num_columns; ++c) {
            unregister_column(map[r].columns[c]);
            unpin_range(map[r].columns[c]);
        }
    return 0;
}

int rhj_registered_columns(void) { return (int)g.columns.size(); }
int rhj_pinned_ranges(void) { return (int)g.pinned.size(); }
int rhj_pin_refusals(void) { return g.pin_refusals; }

// Filter on a host column (its registered device copy, or uploaded for this call) with an optional
// host row-id indirection vector; ids come back in `node_ids`-sized chunks.
int rhj_host_filter(const uint64_t *col, uint64_t col_rows, const uint64_t *sel, uint64_t n, char op, uint64_t value,
                    uint64_t *hits, void *(*alloc_chunk)(void *ctx, uint64_t ids), void *ctx, uint64_t node_ids)
{
    RhjApiLock api_lock;
    *hits = 0;
    if (ctx_init()) return -1;
    if (op_code(op) < 0) return -3;
    if (n == 0) return 0;
    const uint64_t *d_col = registered_column(col, col_rows);
    if (!d_col) {                                      // not registered: upload it for this call only
        if (ensure(g.fcol, (col_rows ? col_rows : 1) * 8)) return -1;
        HIP_TRY(hipMemcpyAsync(g.fcol.p, col, col_rows * 8, hipMemcpyHostToDevice, g.stream));
        d_col = (const uint64_t *)g.fcol.p;
    }
    const uint64_t *d_sel = nullptr;
    if (sel) {
        if (ensure(g.fcol_sel, n * 8)) return -1;
        HIP_TRY(hipMemcpyAsync(g.fcol_sel.p, sel, n * 8, hipMemcpyHostToDevice, g.stream));
        d_sel = (const uint64_t *)g.fcol_sel.p;
    }
    uint64_t *d_out = nullptr, h = 0;
    const int rc = filter_device(d_col, d_sel, n, op, value, nullptr, true, &d_out, &h);
    if (rc) return rc;
    *hits = h;
    for (uint64_t at = 0; at < h; at += node_ids) {
        const uint64_t cnt = h - at < node_ids ? h - at : node_ids;
        void *dst = alloc_chunk(ctx, cnt);
        if (!dst) return -1;
        HIP_TRY(hipMemcpyAsync(dst, d_out + at, cnt * 8, hipMemcpyDeviceToHost, g.stream));
    }
    HIP_TRY(hipStreamSynchronize(g.stream));
    return 0;
}

int rhj_host_null_on_empty(void) { return g.null_on_empty; }
uint64_t rhj_host_node_pairs(void) { return g.node_pairs; }

// ---- device-side services for rhj_inter.hip (device-resident intermediate results) ----

// Device blocks of the intermediate results.  Everything that touches them is queued on the one
// library stream, so a freed block can be handed out again at once: the new user's work is ordered
// behind the old user's by the stream itself.  Blocks are cached by size (never returned to the
// driver before rhj_release()), which keeps hipMalloc/hipFree — both device-wide synchronisations —
// out of the per-operator path.  (hipMallocAsync/hipFreeAsync were tried first: on this stack a
// block freed with work still queued came back with stale contents visible to later kernels.)
void *rhj_dev_alloc(size_t bytes)
{
    RhjApiLock api_lock;
    if (ctx_init()) return nullptr;
    // size classes 2^k and 1.5 * 2^k (a query plan asks for a few dozen different sizes; with 1 MiB granules every one of them
    // was a hipMalloc — a device-wide synchronisation of 50-150 us — the first time: 79 during the `small` run), and a cached
    // block of up to twice the class is taken before the driver is asked
    size_t want = 256;
    const size_t need = bytes < 256 ? 256 : bytes;
    while (want < need) { const size_t mid = want + want / 2; if (want >= ((size_t)1 << 20) && mid >= need) { want = mid; break; } want <<= 1; }
    auto it = g.free_blocks.lower_bound(want);
    if (it != g.free_blocks.end() && it->first <= 2 * want) {
        void *p = it->second;
        g.live_blocks[p] = it->first;
        g.free_blocks.erase(it);
        return p;
    }
    void *p = nullptr;
    static const bool trace = getenv("RHJ_TRACE") != nullptr;
    if (trace) fprintf(stderr, "rhj-trace:   hipMalloc %zu bytes (no cached block of that size)\n", want);
    if (hipMalloc(&p, want) != hipSuccess) {
        // out of device memory: give the cached blocks back and try once more
        (void)hipStreamSynchronize(g.stream);
        for (auto &kv : g.free_blocks) (void)hipFree(kv.second);
        g.free_blocks.clear();
        if (hipMalloc(&p, want) != hipSuccess) {
            fprintf(stderr, "rhj: device allocation of %zu bytes failed\n", bytes);
            return nullptr;
        }
    }
    g.live_blocks[p] = want;
    return p;
}
void rhj_dev_free(void *p)
{
    RhjApiLock api_lock;
    if (!p) return;
    auto it = g.live_blocks.find(p);
    if (it == g.live_blocks.end()) return;
    g.free_blocks.emplace(it->second, p);
    g.live_blocks.erase(it);
}
void *rhj_dev_stream(void) { return ctx_init() ? nullptr : (void *)g.stream; }
// Workspace of joins over relations of up to `rows` tuples a side, allocated now (InitRelationMap knows the base relations'
// sizes: the first joins of a plan then find their buffers in place instead of growing them one by one).
int rhj_dev_reserve(uint64_t rows)
{
    RhjApiLock api_lock;
    if (ctx_init() || rows == 0 || rows >= (1ull << 32)) return -1;
    const uint64_t tiles = (rows + SM_TILE - 1) / SM_TILE + 1, units = 256 + 2 * rows / FJ_BATCH + 16;
    if (ensure(g.partR, rows * sizeof(rhj_tuple)) || ensure(g.partS, rows * sizeof(rhj_tuple)) ||
        ensure(g.cntR, (size_t)tiles * 256 * 4) || ensure(g.cntS, (size_t)tiles * 256 * 4) ||
        ensure(g.stash_cnt, 2 * rows + 64) || ensure(g.stash_row, (2 * rows + 8) * 8) ||
        ensure(g.status, (units + 9) * 8 + 64) || ensure(g.units, units * sizeof(Unit)) ||
        ensure(g.ovf, fj_ovf_bytes((size_t)g.cus)) || ensure(g.ovf_base, (size_t)g.cus * 2 * FJ_GROUPS * 16 * 4))
        return -1;
    return 0;
}
// Device copy of a host column for the resident operators: the registered copy, or — for a column nobody
// registered — a fresh block uploaded now, returned in *temp for the caller to rhj_dev_free() once the
// kernels that read it are queued (blocks are reused in stream order).
const uint64_t *rhj_dev_column(const uint64_t *host_col, uint64_t rows, void **temp)
{
    RhjApiLock api_lock;
    *temp = nullptr;
    if (ctx_init()) return nullptr;
    if (const uint64_t *d = registered_column(host_col, rows)) return d;
    void *blk = rhj_dev_alloc((rows ? rows : 1) * 8);
    if (!blk) return nullptr;
    if (hipMemcpyAsync(blk, host_col, rows * 8, hipMemcpyHostToDevice, g.stream) != hipSuccess) { rhj_dev_free(blk); return nullptr; }
    *temp = blk;
    return (const uint64_t *)blk;
}
int rhj_dev_register_column(const uint64_t *host_col, uint64_t rows, const void *pin_base, uint64_t pin_bytes)
{
    RhjApiLock api_lock;
    if (ctx_init()) return -1;
    if (pin_base) pin_range(pin_base, (size_t)pin_bytes);
    return register_column(host_col, rows);
}
void rhj_dev_unregister_column(const uint64_t *host_col)
{
    RhjApiLock api_lock;
    if (!g.ready) return;
    (void)hipSetDevice(g.device);
    (void)hipStreamSynchronize(g.stream);
    unregister_column(host_col);
    unpin_range(host_col);
}
int rhj_dev_join(const rhj_tuple *d_R, uint64_t nR, const rhj_tuple *d_S, uint64_t nS, rhj_result_tuple **out, uint64_t *matches)
{
    RhjApiLock api_lock;
    *out = nullptr; *matches = 0;
    return join_device({d_R, nR, d_S, nS, nullptr, 0, true, out, matches, g.bits});
}
int rhj_filter_eq2_device(const uint64_t *d_colA, const uint64_t *d_selA, const uint64_t *d_colB, const uint64_t *d_selB,
                          uint64_t n, uint64_t *d_out, uint64_t *hits)
{
    RhjApiLock api_lock;
    uint64_t h = 0;
    const int rc = filter_eq2_device(d_colA, d_selA, d_colB, d_selB, n, d_out, &h);
    if (hits) *hits = h;
    return rc;
}

}  // extern "C"
