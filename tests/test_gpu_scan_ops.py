"""GPU: the filter scan, the two-column equality, the view sums, the gathers and the column statistics at the
sizes where their launches change shape, each through its public entry point against a plain numpy statement
of the same operation (np.nonzero, sum(dtype=np.uint64), fancy indexing), element for element.

Every size is derived from the constants below (each mirrors one line of the C code) and from the device's
compute-unit count, so that the cases stay on their edges if the constants move.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

from helpers import M64, STATS_CAP, STATS_FOLD, column_stats_model

pytestmark = pytest.mark.gpu

u64p = C.POINTER(C.c_uint64)

# ------------------------------------------------------------------ the code's constants
WAVE = 64                                         # rhj_common.hip.h: wavefront width
BLOCK = 256                                       # every kernel below: __launch_bounds__(256)
FILTER_WAVE_ELEMS = 1024                          # rhj_filter.hip.h:11  FILTER_ROUNDS * 2 * WAVE: one mask wave's elements
FILTER_TILE = 4096                                # rhj_filter.hip.h:12  one mask workgroup's elements
FILTER_PAIR = 2 * FILTER_TILE                     # rhj_filter.hip.h:118 one k_filter_write wave's task: a pair of tiles
FILTER_SPARSE = 1024                              # rhj_filter.hip.h:102 most hits of a pair that take the bit-walking form
FILTER_SELF_TILES = 1024                          # rhj_filter.hip.h:107 most tiles of the scan-free (SELF) write pass
FILTER_WRITE_BLOCKS_PER_CU = 32                   # rhj_device.hip:1138  filter_write_grid: cap = cus * 32 workgroups
MAX_TABLES = 16                                   # rhj_inter.hip:26     tables of one k_gather_tables launch
SUM_VIEWS = 8                                     # rhj_inter.hip:72     views of one k_sum_views launch
SUM_VIEWS_BLOCKS = 1024                           # rhj_inter.hip:382    k_sum_views blocks per view at most
REDUCE_BLOCKS = 2048                              # rhj_inter.hip:350, :856 k_sum_gather / k_col_minmax blocks at most
NODE_IDS = 1048576 // 8                           # rhj_abi.c:31,152     RESULT_FINAL_BUFFER / 8: ids per host list node

SELF_EDGE = FILTER_SELF_TILES * FILTER_TILE       # n above this: k_filter_write<false> on the launch_offsets scan
SUM_VIEWS_EDGE = SUM_VIEWS_BLOCKS * BLOCK         # a view longer than this: k_sum_views' grid-stride pass
REDUCE_EDGE = REDUCE_BLOCKS * BLOCK               # n above this: k_sum_gather / k_col_minmax grid-stride pass


def write_stride(cus):
    """elements one grid-stride round of k_filter_write covers: every wave of the capped grid takes one pair"""
    return cus * FILTER_WRITE_BLOCKS_PER_CU * (BLOCK // WAVE) * FILTER_PAIR


SELF_SIZES = [SELF_EDGE - 1, SELF_EDGE, SELF_EDGE + 1, SELF_EDGE + FILTER_PAIR + 77, 3 * SELF_EDGE + 1234]

TOP = 1 << 63
# op -> (constant, column values that satisfy the predicate, values that do not); constants and values around 2^31 and
# 2^63, where a signed or 32-bit compare anywhere in the path would change the answer
OPS = {
    "<": (TOP + 1, [0, 1, (1 << 31) - 1, 1 << 31, TOP - 1, TOP], [TOP + 1, TOP + 2, M64 - 1, M64]),
    ">": (TOP - 1, [TOP, TOP + 1, M64 - 1, M64], [0, 1, 1 << 31, TOP - 1]),
    "=": (TOP + 12345, [TOP + 12345], [TOP + 12344, TOP + 12346, 12345, M64]),
}


def pred(col, op, k):
    k = np.uint64(k)
    return col < k if op == "<" else col > k if op == ">" else col == k


# ------------------------------------------------------------------ plumbing

@pytest.fixture(scope="module")
def rhj():
    mod = importlib.import_module("sigmod-2018_amd")
    r = mod.RHJ()
    L = r.lib
    L.rhj_filter_eq2_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, u64p]
    L.rhj_sum_views_device.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), u64p, u64p]
    L.rhj_sum_gather_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.rhj_build_relation_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.rhj_gather_tables_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_uint64]
    L.rhj_column_stats_device.argtypes = [C.c_void_p, C.c_uint64, u64p, u64p, C.POINTER(C.c_double)]
    return r


@pytest.fixture(scope="module")
def cus(rhj):
    return rhj.torch.cuda.get_device_properties(rhj.dev).multi_processor_count


def dev(rhj, a):
    return rhj.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


def host(t):
    return t.cpu().numpy().view(np.uint64)


def ptr(t):
    return t.data_ptr() if t is not None else None


def new_out(rhj, n):
    """an n-row output, filled with a value no index takes, so that an index the kernel never wrote shows"""
    return rhj.torch.full((max(n, 1),), -1, dtype=rhj.torch.int64, device=rhj.dev)


def filt(rhj, dcol, n, op, k, dsel=None, out=None):
    out = new_out(rhj, n) if out is None else out.fill_(-1)
    hits = C.c_uint64(0)
    assert rhj.lib.rhj_filter_device(ptr(dcol), ptr(dsel), n, op.encode(), k, out.data_ptr(), C.byref(hits)) == 0
    return host(out[:hits.value])


def eq2(rhj, dA, dsA, dB, dsB, n, out):
    out.fill_(-1)
    hits = C.c_uint64(0)
    assert rhj.lib.rhj_filter_eq2_device(ptr(dA), ptr(dsA), ptr(dB), ptr(dsB), n, out.data_ptr(), C.byref(hits)) == 0
    return host(out[:hits.value])


def through(sel, seq):
    """a column c with c[sel[i]] == seq[i] (sel a permutation): scanning c through sel sees seq again"""
    c = np.empty(len(seq), dtype=np.uint64)
    c[sel] = seq
    return c


def hit_masks(n, rng):
    """{name: bool[n]} hit layouts for the filter cases"""
    i = np.arange(n, dtype=np.int64)
    pair = i // FILTER_PAIR
    sparse_step = 2 * FILTER_PAIR // FILTER_SPARSE       # FILTER_SPARSE / 2 hits a pair: the bit-walking form
    dense = i % 4 != 0                                   # 3/4 of a pair: the round-by-round form
    assert FILTER_PAIR // sparse_step <= FILTER_SPARSE < FILTER_PAIR * 3 // 4
    masks = {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool)}
    m = np.zeros(n, dtype=bool)
    m[np.arange(12345 % n, n, 1_000_000)] = True
    m[n - 1] = True
    masks["one in a million"] = m
    kind = pair % 3                                      # none / sparse / dense pairs side by side
    masks["mixed pairs"] = ((kind == 1) & (i % sparse_step == 0)) | ((kind == 2) & dense)
    last_full = n // FILTER_PAIR - 1                     # the last pair of two full tiles
    for k in (FILTER_SPARSE, FILTER_SPARSE + 1):         # the switch, in the last full pair, with hits in front of it
        m = (pair < last_full) & (i % (4 * sparse_step) == 0)
        m[last_full * FILTER_PAIR + np.sort(rng.choice(FILTER_PAIR, k, replace=False))] = True
        assert m[last_full * FILTER_PAIR:(last_full + 1) * FILTER_PAIR].sum() == k
        masks["%d hits in the last full pair" % k] = m
    return masks


def column_for(mask, op):
    k, yes, no = OPS[op]
    i = np.arange(len(mask))
    yes, no = np.array(yes, dtype=np.uint64), np.array(no, dtype=np.uint64)
    return np.where(mask, yes[i % len(yes)], no[i % len(no)]), k


# ------------------------------------------------------------------ filter

@pytest.mark.parametrize("n", SELF_SIZES)
def test_filter_across_the_self_switch(rhj, n):
    """rhj_filter_device on both sides of FILTER_SELF_TILES tiles (the write pass sums the tile counts itself / takes
    the bases of the launch_offsets scan and copies the total back), with every hit layout and all three operators,
    directly and through a row-id vector"""
    rng = np.random.default_rng(n)
    perm = rng.permutation(n).astype(np.uint64)
    dperm = dev(rhj, perm)
    out = new_out(rhj, n)
    for name, mask in hit_masks(n, rng).items():
        for op in OPS:
            col, k = column_for(mask, op)
            want = np.nonzero(pred(col, op, k))[0].astype(np.uint64)
            assert np.array_equal(want, np.nonzero(mask)[0])                      # (the case is what its name says)
            got = filt(rhj, dev(rhj, col), n, op, k, out=out)
            assert np.array_equal(got, want), (n, name, op, "direct")
            got = filt(rhj, dev(rhj, through(perm, col)), n, op, k, dperm, out=out)
            assert np.array_equal(got, want), (n, name, op, "through a row-id vector")


def grid_stride_hits(i):
    """hit layout of the grid-stride case (numpy or torch): pair kinds sparse / dense / none / all in turn"""
    kind = (i // FILTER_PAIR) % 4
    sparse_step = 2 * FILTER_PAIR // FILTER_SPARSE
    return ((kind == 0) & (i % sparse_step == 0)) | ((kind == 1) & (i % 3 != 0)) | (kind == 3)


def test_filter_past_the_grid_stride_edge(rhj, cus):
    """more pairs than the capped write grid has waves: the first waves take a second, partly filled stride
    (three full pairs and a partial one), in which sparse, dense, empty and full pairs follow each other"""
    torch = rhj.torch
    stride = write_stride(cus)
    n = stride + 3 * FILTER_PAIR + 1234
    assert (stride // FILTER_PAIR) % 4 == 0              # the second stride starts on a sparse pair
    chunk = 1 << 24
    col = torch.empty(n, dtype=torch.int64, device=rhj.dev)
    for a in range(0, n, chunk):
        i = torch.arange(a, min(a + chunk, n), dtype=torch.int64, device=rhj.dev)
        col[a:a + len(i)] = torch.where(grid_stride_hits(i), 0, 2)
        del i
    out = torch.empty(n, dtype=torch.int64, device=rhj.dev)
    try:
        out.fill_(-1)
        hits = C.c_uint64(0)
        assert rhj.lib.rhj_filter_device(col.data_ptr(), None, n, b"<", 1, out.data_ptr(), C.byref(hits)) == 0
        pos = 0
        for a in range(0, n, chunk):
            want = a + np.nonzero(grid_stride_hits(np.arange(a, min(a + chunk, n), dtype=np.int64)))[0]
            got = host(out[pos:pos + len(want)])
            assert np.array_equal(got, want.astype(np.uint64)), ("rows from", a)
            pos += len(want)
        assert hits.value == pos
    finally:
        del col, out
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def test_filter_unsigned_compare_at_the_top_of_the_domain(rhj):
    vals = [0, 1, (1 << 31) - 1, 1 << 31, (1 << 63) - 1, 1 << 63, M64 - 1, M64]
    n = 3 * FILTER_TILE + FILTER_WAVE_ELEMS + 37          # full tiles, full waves and a partial wave
    col = np.array(vals, dtype=np.uint64)[(np.arange(n) * 3) % len(vals)]
    dcol = dev(rhj, col)
    for op in OPS:
        for k in vals:
            want = np.nonzero(pred(col, op, k))[0].astype(np.uint64)
            assert np.array_equal(filt(rhj, dcol, n, op, k), want), (op, k)


def test_filter_on_offset_views(rhj):
    """dcol[1:] and dsel[1:] are 8-byte aligned: the mask pass must not take its 16-byte loads on them"""
    rng = np.random.default_rng(77)
    n = 5 * FILTER_TILE + FILTER_WAVE_ELEMS + 333
    col = rng.integers(0, 1000, n + 1, dtype=np.uint64)
    sel = rng.integers(0, n + 1, n + 1, dtype=np.uint64)
    dcol, dsel = dev(rhj, col), dev(rhj, sel)
    assert dcol.data_ptr() % 16 == 0 and dcol[1:].data_ptr() % 16 == 8
    for op, k in (("<", 3), ("<", 500), (">", 10), ("=", 7)):
        want = np.nonzero(pred(col[1:], op, k))[0].astype(np.uint64)
        assert np.array_equal(filt(rhj, dcol[1:], n, op, k), want), (op, k, "col[1:]")
        want = np.nonzero(pred(col[sel[1:]], op, k))[0].astype(np.uint64)
        assert np.array_equal(filt(rhj, dcol, n, op, k, dsel[1:]), want), (op, k, "sel[1:]")
        want = np.nonzero(pred(col[1:][sel[1:] % np.uint64(n)], op, k))[0].astype(np.uint64)
        dsel_in = dev(rhj, np.concatenate([[0], sel[1:] % np.uint64(n)]))
        assert np.array_equal(filt(rhj, dcol[1:], n, op, k, dsel_in[1:]), want), (op, k, "both")


# ------------------------------------------------------------------ two-column equality

@pytest.mark.parametrize("n", SELF_SIZES)
def test_filter_eq2_across_the_self_switch(rhj, n):
    """rhj_filter_eq2_device (SelfJoin / JoinInterNode): every combination of selA / selB, the same vector on both
    sides, and columns equal in a mix of sparse and dense pairs, everywhere, nowhere and only in the last partial wave"""
    rng = np.random.default_rng(n + 1)
    i = np.arange(n, dtype=np.int64)
    kind = (i // FILTER_PAIR) % 3
    last_wave = (n - 1) // FILTER_WAVE_ELEMS * FILTER_WAVE_ELEMS
    layouts = {
        "mixed pairs": ((kind == 1) & (i % 16 == 0)) | ((kind == 2) & (i % 4 != 0)),
        "everywhere": np.ones(n, dtype=bool),
        "nowhere": np.zeros(n, dtype=bool),
        "last partial wave": i >= last_wave,
    }
    pA, pB = rng.permutation(n).astype(np.uint64), rng.permutation(n).astype(np.uint64)
    dpA, dpB = dev(rhj, pA), dev(rhj, pB)
    out = new_out(rhj, n)
    for name, mask in layouts.items():
        a = rng.integers(0, M64, n, dtype=np.uint64, endpoint=True)
        b = np.where(mask, a, a ^ np.uint64(1 << 63))
        combos = [(None, None), (pA, None), (None, pB), (pA, pB), (pA, pA)] if name == "mixed pairs" else [(None, None), (pA, pA)]
        for sA, sB in combos:
            colA = a if sA is None else through(sA, a)
            colB = b if sB is None else through(sB, b)
            seqA = colA if sA is None else colA[sA]
            seqB = colB if sB is None else colB[sB]
            want = np.nonzero(seqA == seqB)[0].astype(np.uint64)
            assert np.array_equal(want, np.nonzero(mask)[0])
            dsA = None if sA is None else (dpA if sA is pA else dpB)
            dsB = None if sB is None else (dpA if sB is pA else dpB)
            got = eq2(rhj, dev(rhj, colA), dsA, dev(rhj, colB), dsB, n, out)
            assert np.array_equal(got, want), (n, name, sA is not None, sB is not None)


# ------------------------------------------------------------------ view sums and gathered sums

def test_sum_views_past_the_block_cap(rhj):
    """rhj_sum_views_device: eight views of very different lengths in one grid, one of them past the block cap,
    values >= 2^62 so that every sum wraps, call after call with other view sets (the device words and the
    last-block ticket must be back at zero every time)"""
    rng = np.random.default_rng(3)
    big_n = 12 * SUM_VIEWS_EDGE + 17
    col = rng.integers(1 << 62, M64, big_n, dtype=np.uint64, endpoint=True)
    sel = rng.integers(0, big_n, big_n, dtype=np.uint64)
    dcol, dsel = dev(rhj, col), dev(rhj, sel)
    lens = [big_n, 0, 1, SUM_VIEWS_EDGE + 1, 1000, 2 * SUM_VIEWS_EDGE + 3, 77, SUM_VIEWS_EDGE]
    views = []
    for k, n in enumerate(lens):
        with_sel = k % 2 == 0
        want = int(col[sel[:n]].sum(dtype=np.uint64)) if with_sel else int(col[:n].sum(dtype=np.uint64))
        views.append((dsel if with_sel else None, n, want))
    views.append((None, big_n, int(col.sum(dtype=np.uint64))))
    views.append((dsel, SUM_VIEWS_EDGE - 1, int(col[sel[:SUM_VIEWS_EDGE - 1]].sum(dtype=np.uint64))))
    assert len(lens) == SUM_VIEWS
    for take in (list(range(SUM_VIEWS)), [9, 3, 0, 8, 1], list(range(SUM_VIEWS))[::-1], [8], [1, 2], [0, 3, 5, 7, 9, 4, 6, 8], [2]):
        k = len(take)
        cols = (C.c_void_p * k)(*[dcol.data_ptr()] * k)
        sels = (C.c_void_p * k)(*[ptr(views[t][0]) for t in take])
        ns = (C.c_uint64 * k)(*[views[t][1] for t in take])
        got = (C.c_uint64 * k)()
        assert rhj.lib.rhj_sum_views_device(k, cols, sels, ns, got) == 0
        assert list(got) == [views[t][2] for t in take], take


def test_sum_gather_past_the_block_cap(rhj):
    rng = np.random.default_rng(4)
    n_max = 6 * REDUCE_EDGE + 5
    col = rng.integers(1 << 62, M64, n_max, dtype=np.uint64, endpoint=True)
    sel = rng.integers(0, n_max, n_max, dtype=np.uint64)
    dcol, dsel = dev(rhj, col), dev(rhj, sel)
    s = C.c_uint64(0)
    for n in (REDUCE_EDGE, REDUCE_EDGE + 1, n_max):
        assert rhj.lib.rhj_sum_gather_device(dcol.data_ptr(), None, n, C.byref(s)) == 0
        assert s.value == int(col[:n].sum(dtype=np.uint64)), (n, "direct")
        assert rhj.lib.rhj_sum_gather_device(dcol.data_ptr(), dsel.data_ptr(), n, C.byref(s)) == 0
        assert s.value == int(col[sel[:n]].sum(dtype=np.uint64)), (n, "sel")


# ------------------------------------------------------------------ gathers

def test_gather_tables_and_build_relation_at_scale(rhj):
    """k_gather_tables with MAX_TABLES tables, some without a source, idx_stride 2 over either side of a pair list;
    k_build_relation at the same n with and without a selection"""
    torch = rhj.torch
    rng = np.random.default_rng(8)
    n, m = (1 << 21) + 5, 1_000_003
    null_src = {3, 9, MAX_TABLES - 1}
    tabs = [None if t in null_src else rng.integers(0, M64, m, dtype=np.uint64, endpoint=True) for t in range(MAX_TABLES)]
    pairs = rng.integers(0, m, (n, 2), dtype=np.uint64)
    d_tabs = [None if t is None else dev(rhj, t) for t in tabs]
    d_pairs = dev(rhj, pairs.reshape(-1))
    outs = [torch.full((n,), -1, dtype=torch.int64, device=rhj.dev) for _ in range(MAX_TABLES)]
    dst = (C.c_void_p * MAX_TABLES)(*[o.data_ptr() for o in outs])
    src = (C.c_void_p * MAX_TABLES)(*[ptr(t) for t in d_tabs])
    for side in (0, 1):
        for o in outs:
            o.fill_(-1)
        assert rhj.lib.rhj_gather_tables_device(dst, src, MAX_TABLES, d_pairs.data_ptr() + 8 * side, 2, n) == 0
        torch.cuda.synchronize()
        for t, (tab, o) in enumerate(zip(tabs, outs)):
            want = pairs[:, side] if tab is None else tab[pairs[:, side]]
            assert np.array_equal(host(o), want), (side, t)
    del outs
    col = rng.integers(0, M64, m, dtype=np.uint64, endpoint=True)
    dcol = dev(rhj, col)
    tup = torch.full((n, 2), -1, dtype=torch.int64, device=rhj.dev)
    sel = pairs[:, 1].copy()
    assert rhj.lib.rhj_build_relation_device(dcol.data_ptr(), dev(rhj, sel).data_ptr(), n, tup.data_ptr()) == 0
    torch.cuda.synchronize()
    t = host(tup.reshape(-1)).reshape(-1, 2)
    assert np.array_equal(t[:, 0], col[sel]) and np.array_equal(t[:, 1], np.arange(n, dtype=np.uint64))
    colN = rng.integers(0, M64, n, dtype=np.uint64, endpoint=True)
    tup.fill_(-1)
    assert rhj.lib.rhj_build_relation_device(dev(rhj, colN).data_ptr(), None, n, tup.data_ptr()) == 0
    torch.cuda.synchronize()
    t = host(tup.reshape(-1)).reshape(-1, 2)
    assert np.array_equal(t[:, 0], colN) and np.array_equal(t[:, 1], np.arange(n, dtype=np.uint64))


# ------------------------------------------------------------------ column statistics

def test_column_stats_at_the_edges(rhj):
    """rhj_column_stats_device past the reduction's block cap, with the extremes on the first and the last row:
    the largest unfolded range (STATS_CAP - 1), the smallest folded one (STATS_CAP), and the full range
    (0, 2^64 - 1), whose u - l + 1 wraps to 0 and which the library folds like any range of STATS_CAP or more"""
    rng = np.random.default_rng(9)
    n = 3 * REDUCE_EDGE + 11
    lo = (1 << 63) - 7
    cols = {}
    for size in (STATS_CAP - 1, STATS_CAP):
        c = rng.integers(lo, lo + size, n, dtype=np.uint64)
        c[0], c[-1] = lo, lo + size - 1
        cols["range %d, min first" % size] = c
        cols["range %d, max first" % size] = c[::-1].copy()
    c = rng.integers(1, M64 - 1, n, dtype=np.uint64)
    c[0], c[-1] = 0, M64
    cols["full range, min first"] = c
    cols["full range, max first"] = c[::-1].copy()
    for name, col in cols.items():
        want = column_stats_model(col)
        if name.startswith("full range"):
            assert want[:2] == (0, M64) and want[2] <= STATS_FOLD          # the folded count
        l, u, d = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
        assert rhj.lib.rhj_column_stats_device(dev(rhj, col).data_ptr(), n, C.byref(l), C.byref(u), C.byref(d)) == 0
        assert (l.value, u.value, d.value) == want, name


# ------------------------------------------------------------------ host ABI: the list Filter() hands back

def test_host_filter_list_shape_on_a_large_column(rhj):
    """Filter() on a host column past the SELF switch: the ids come back in nodes of NODE_IDS, as InsertRowIdResult
    fills them (results.c: RESULT_FINAL_BUFFER bytes a node), and zero hits are NULL (filter.c:94,189)"""
    rng = np.random.default_rng(10)
    n = SELF_EDGE + FILTER_PAIR + 77
    col = rng.permutation(n).astype(np.uint64)                  # col < h: exactly h hits, scattered
    for h in (3 * NODE_IDS + 4321, NODE_IDS, NODE_IDS + 1, n - 5, 0):
        ids, info = rhj.Filter([col], n, 0, "<", h, with_info=True)
        assert np.array_equal(ids, np.nonzero(col < np.uint64(h))[0].astype(np.uint64)), h
        assert info["null"] == (h == 0), h
        want = [NODE_IDS] * (h // NODE_IDS) + ([h % NODE_IDS] if h % NODE_IDS else [])
        assert info["loads"] == want, (h, info["loads"][:4], len(info["loads"]))
