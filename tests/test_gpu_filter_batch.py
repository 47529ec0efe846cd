"""rhj_filter_batch_device (include/rhj.h, csrc/rhj_filter_batch.hip.h): many conjunctive filters in one call — those of at
most 4 194 304 rows in two launches, the larger ones alone — index for index against np.flatnonzero over the AND of the terms,
against rhj_filter_device called alone and against the oracle's Filter chained through row-id vectors.

Every output of a batch lies in ONE buffer whose every other word holds a sentinel, so that a word written at or behind
d_out[hits], or in front of d_out, is found."""
import ctypes as C
import importlib
import threading

import numpy as np
import pytest

from helpers import GUARD_ROWS, M64, SENTINEL, GuardedRows

pytestmark = pytest.mark.gpu

u64p = C.POINTER(C.c_uint64)

BATCHED = 7                                       # rhj_filter_desc::path of a filter that ran in the batched launches
ALONE = 0
WAVE_ELEMS = 1024                                 # rhj_filter.hip.h: one mask wave's elements
TILE = 4096                                       # one mask workgroup's elements
PAIR = 2 * TILE                                   # one write wave's task
SPARSE = 1024                                     # FILTER_SPARSE: most hits of a pair that take the bit-walking form
TOP_ROWS = 1024 * TILE                            # FILTER_SELF_TILES * FILTER_TILE: the largest filter of the batched launches
MAX_FILTERS = 4096                                # filters of one chunk
GAP = 64                                          # sentinel words between two outputs
SENT = np.uint64(SENTINEL & M64)

TOP = 1 << 63
# op -> (constant, column values that satisfy the predicate, values that do not), around 2^31 and 2^63
OPS = {
    "<": (TOP + 1, [0, 1, (1 << 31) - 1, 1 << 31, TOP - 1, TOP], [TOP + 1, TOP + 2, M64 - 1, M64]),
    ">": (TOP - 1, [TOP, TOP + 1, M64 - 1, M64], [0, 1, 1 << 31, TOP - 1]),
    "=": (TOP + 12345, [TOP + 12345], [TOP + 12344, TOP + 12346, 12345, M64]),
}


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def rhj(mod):
    r = mod.RHJ(device=0)
    r.lib.rhj_filter_eq2_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, u64p]
    yield r
    r.lib.rhj_set_timing(2)
    r.set_bits(4)


def dev(rhj, a):
    return rhj.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


def host(t):
    return t.cpu().numpy().view(np.uint64)


def pred(col, op, k):
    k = np.uint64(int(k) & M64)
    return col < k if op == "<" else col > k if op == ">" else col == k


def model(cols, terms, sel=None):
    """np.flatnonzero over the AND of the terms; terms = [(column number, op, value)]"""
    keep = None
    for c, op, k in terms:
        seq = cols[c] if sel is None else cols[c][sel]
        m = pred(seq, op, k)
        keep = m if keep is None else keep & m
    return np.flatnonzero(keep).astype(np.uint64)


class Case:
    """one filter of a batch: device columns and terms, an optional row-id vector, the wanted indices (None: not compared)"""

    def __init__(self, terms, n, want, d_sel=None, count_only=False, nterms=None):
        self.terms, self.n, self.want, self.d_sel, self.count_only = terms, int(n), want, d_sel, count_only
        self.nterms = len(terms) if nterms is None else nterms


def run_guarded(rhj, mod, cases, expect_rc=0):
    """One rhj_filter_batch_device call over `cases`, every output (capacity n) between sentinel words of one buffer.  Asserts
    the return code, every filter's rc 0, exact hits, the wanted indices in d_out[0..hits) and the sentinel in every other word
    of the buffer: nothing at or beyond d_out[hits], nothing in front of d_out.  Returns the descriptors."""
    torch = rhj.torch
    offs, at = [], 0
    for c in cases:
        offs.append(at)
        if not c.count_only:
            at += c.n + GAP
    g = GuardedRows(torch, rhj.dev, (at + 1) // 2)
    flat = g.t.view(-1)
    base = 2 * GUARD_ROWS
    arr = (mod.FilterDesc * max(len(cases), 1))()
    for d, c, o in zip(arr, cases, offs):
        d.d_sel = c.d_sel.data_ptr() if c.d_sel is not None else None
        d.n, d.nterms = c.n, c.nterms
        for t, (d_col, op, value) in zip(d.terms, c.terms):
            t.d_col = d_col.data_ptr() if d_col is not None else None
            t.op, t.value = op.encode(), int(value) & M64
        d.d_out = None if c.count_only else g.ptr + 8 * o
        d.hits, d.rc, d.path = 0xDEAD, -77, -77
    rc = rhj.lib.rhj_filter_batch_device(arr, len(cases))
    torch.cuda.synchronize()
    assert rc == expect_rc, "return code %d" % rc
    got = host(flat)
    want_buf = np.full(len(got), SENT, dtype=np.uint64)
    for k, (d, c, o) in enumerate(zip(arr, cases, offs)):
        if expect_rc == 0:
            assert d.rc == 0, (k, d.rc)
        if c.want is None:
            continue
        assert d.hits == len(c.want), "filter %d (n %d): %d hits, expected %d" % (k, c.n, d.hits, len(c.want))
        if not c.count_only:
            want_buf[base + o:base + o + len(c.want)] = c.want
    if not np.array_equal(got, want_buf):
        w = int(np.flatnonzero(got != want_buf)[0]) - base
        k = int(np.searchsorted(np.array(offs), w, side="right")) - 1
        raise AssertionError("word %d of the buffer (filter %d, its word %d of %d, hits %d) is %d, expected %d"
                             % (w, k, w - offs[max(k, 0)], cases[max(k, 0)].n, arr[max(k, 0)].hits, got[w + base], want_buf[w + base]))
    return arr


def single_filter(rhj, d_col, op, value, d_sel=None):
    return host(rhj.filter_device(d_col, op, int(value) & M64, d_sel))


# ---- 1. the 50 filters of `small` --------------------------------------------------------------------------------------------

def test_small_workload_filters_in_one_batch(rhj, mod, golden, oracle):
    recs = golden.small["filters"]
    assert len(recs) == 50
    rels = {k: dev(rhj, v.astype(np.uint64)) for k, v in golden.small_relations.items()}
    cases, loop = [], []
    for f in recs:
        d_rel = rels["r%d" % f["rel"]]
        assert d_rel.shape[1] == f["rows"]
        d_col = d_rel[f["col"]]
        loop.append(single_filter(rhj, d_col, f["op"], f["value"]))
        cases.append(Case([(d_col, f["op"], f["value"])], f["rows"], loop[-1]))
    arr = run_guarded(rhj, mod, cases)
    for d, f, ids in zip(arr, recs, loop):
        assert d.path == BATCHED, (f["idx"], d.path)
        assert d.hits == f["hits"] and "%016x" % oracle.fnv(ids) == f["fnv"] and int(ids.sum(dtype=np.uint64)) == f["sum"], f
    st = rhj.stats()
    assert st["path"] == "filter_batch" and st["units"] == 50 and st["n_r"] == sum(f["rows"] for f in recs)
    assert st["matches"] == sum(f["hits"] for f in recs)
    # ... and through the Python wrapper: index lists carved from one allocation
    res, paths = rhj.filter_batch_device([(c.terms, None) for c in cases], with_info=True)
    assert set(paths) == {BATCHED}
    for (ids, hits), want in zip(res, loop):
        assert hits == len(want) and np.array_equal(host(ids), want)
    counts = rhj.filter_batch_device([(c.terms, None) for c in cases], count_only=True)
    assert [(a, h) for a, h in counts] == [(None, len(w)) for w in loop]


# ---- 2. sizes and hit layouts ------------------------------------------------------------------------------------------------

SIZES = [1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193]


def hit_layouts(n, rng):
    """{name: bool[n]}: none, all, the first only, the last only, and exactly FILTER_SPARSE / FILTER_SPARSE + 1 hits in the
    first pair of tiles (where it has that many rows)"""
    lay = {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool), "first": np.arange(n) == 0, "last": np.arange(n) == n - 1}
    for h in (SPARSE, SPARSE + 1):
        if min(n, PAIR) >= h:
            m = np.zeros(n, dtype=bool)
            m[rng.choice(min(n, PAIR), h, replace=False)] = True
            lay["%d hits in the pair" % h] = m
    return lay


def column_for(mask, op):
    k, yes, no = OPS[op]
    i = np.arange(len(mask))
    yes, no = np.array(yes, dtype=np.uint64), np.array(no, dtype=np.uint64)
    return np.where(mask, yes[i % len(yes)], no[i % len(no)]), k


@pytest.mark.parametrize("op", sorted(OPS))
def test_sizes_and_hit_layouts_in_one_mixed_batch(rhj, mod, op):
    """every size around a wave's range (1024), a tile (4096) and a task (8192) with every hit layout, direct and through a
    shuffled row-id vector with repeats, as ONE batch per operator"""
    rng = np.random.default_rng(ord(op))
    cases = []
    for n in SIZES:
        for name, mask in hit_layouts(n, rng).items():
            col, k = column_for(mask, op)
            want = np.flatnonzero(mask).astype(np.uint64)
            assert np.array_equal(model([col], [(0, op, k)]), want), (n, name)
            cases.append(Case([(dev(rhj, col), op, k)], n, want))
            # through sel: the column's first half holds, its second half does not; row i goes to a random row of its kind
            m = n + 2
            half = m // 2
            colS, _ = column_for(np.arange(m) < half, op)
            sel = np.where(mask, rng.integers(0, half, n), rng.integers(half, m, n)).astype(np.uint64)
            assert np.array_equal(model([colS], [(0, op, k)], sel), want), (n, name, "sel")
            cases.append(Case([(dev(rhj, colS), op, k)], n, want, d_sel=dev(rhj, sel)))
    arr = run_guarded(rhj, mod, cases)
    assert {d.path for d in arr[:len(cases)]} == {BATCHED}
    # a one-term filter returns what rhj_filter_device returns
    for c in cases[::7]:
        assert np.array_equal(single_filter(rhj, c.terms[0][0], op, c.terms[0][2], c.d_sel), c.want)


# ---- 3. conjunctions -----------------------------------------------------------------------------------------------------

def test_conjunctions_of_one_to_four_terms(rhj, mod, oracle):
    rng = np.random.default_rng(2018)
    n = 2 * PAIR + TILE + WAVE_ELEMS + 37                 # two full tasks and a partial one with a partial wave
    edge = np.array([0, 1, (1 << 31) - 1, 1 << 31, TOP - 1, TOP, TOP + 1, M64 - 1, M64], dtype=np.uint64)
    cols = [rng.integers(0, 1000, n, dtype=np.uint64) for _ in range(4)] + [edge[rng.integers(0, len(edge), n)] for _ in range(2)]
    d_cols = [dev(rhj, c) for c in cols]
    sel = rng.integers(0, n, n + 500, dtype=np.uint64)    # longer than the relation, with repeats
    d_sel = dev(rhj, sel)
    specs = []
    for nt in (1, 2, 3, 4):                               # distinct columns
        for _ in range(3):
            specs.append([(c, "<>="[rng.integers(0, 3)], int(rng.integers(0, 1000))) for c in rng.permutation(4)[:nt]])
    specs += [
        [(0, ">", 200), (0, "<", 700)],                   # the same column twice
        [(1, ">", 10), (1, "<", 12), (1, "=", 11)],
        [(2, ">", 700), (2, "<", 200), (3, ">", 5)],      # the second term empties the mask
        [(0, "<", 0), (1, ">", 5), (2, ">", 5), (3, ">", 5)],          # the first does
        [(0, ">", 100), (1, ">", 100), (2, ">", 100), (3, "=", 1000)],  # the last does
        [(4, "=", M64)], [(4, "<", M64), (5, ">", TOP)],  # (uint64_t)(int)-1 and 2^63
        [(4, ">", TOP - 1), (5, "<", TOP + 1), (0, "<", 900)],
        [(4, "=", TOP), (5, "=", TOP)], [(5, "<", TOP), (4, ">", (1 << 31) - 1), (5, ">", 0), (4, "<", M64)],
    ]
    cases = []
    for spec in specs:
        terms = [(d_cols[c], op, k) for c, op, k in spec]
        cases.append(Case(terms, n, model(cols, spec)))
        cases.append(Case(terms, len(sel), model(cols, spec, sel), d_sel=d_sel))
        cases.append(Case(terms, n, model(cols, spec), count_only=True))
    arr = run_guarded(rhj, mod, cases)
    assert {d.path for d in arr[:len(cases)]} == {BATCHED}
    assert any(len(c.want) == 0 for c in cases) and any(len(c.want) > SPARSE for c in cases)
    # six seeded cases against the reference's way: Filter() after Filter() through the row ids of the one before
    for seed in range(6):
        r = np.random.default_rng(100 + seed)
        nt = 2 + seed % 3
        spec = [(int(c), "<>="[r.integers(0, 3)] if seed % 2 else "<>"[r.integers(0, 2)], int(r.integers(0, 1000))) for c in r.integers(0, 4, nt)]
        if seed == 5:
            spec = [(4, "=", -1), (5, ">", 1 << 30)]     # the oracle converts as the reference does: (uint64_t)(int)value
        through = sel if seed >= 3 else None
        ids = None                                        # positions in [0, n) or in sel that passed so far
        for c, op, k in spec:
            cur = through if ids is None else (ids if through is None else through[ids])
            step = oracle.filter(cols[c], op, k, sel=cur)
            ids = step if ids is None else ids[step]
        terms = [(d_cols[c], op, k) for c, op, k in spec]
        got, hits = rhj.filter_batch_device([(terms, d_sel if through is not None else None)])[0]
        assert hits == len(ids) and np.array_equal(host(got), ids), (seed, spec)
        assert np.array_equal(ids, model(cols, [(c, op, k & M64) for c, op, k in spec], through)), (seed, spec)


# ---- 4. views offset by 8 bytes ------------------------------------------------------------------------------------------

def test_views_offset_by_eight_bytes(rhj, mod):
    """col[1:], sel[1:] and one term only of a two-term filter on an 8-byte-aligned view: no 16-byte loads there, and the
    same indices as on aligned copies of the same data"""
    rng = np.random.default_rng(77)
    n = 5 * TILE + WAVE_ELEMS + 333
    a, b = rng.integers(0, 1000, n + 1, dtype=np.uint64), rng.integers(0, 1000, n + 1, dtype=np.uint64)
    sel = rng.integers(0, n, n + 1, dtype=np.uint64)
    da, db, dsel = dev(rhj, a), dev(rhj, b), dev(rhj, sel)
    a1, b1, sel1 = da[1:], db[1:], dsel[1:]
    assert da.data_ptr() % 16 == 0 and a1.data_ptr() % 16 == 8 and sel1.data_ptr() % 16 == 8
    a1c, sel1c = a1.clone(), sel1.clone()
    assert a1c.data_ptr() % 16 == 0 and sel1c.data_ptr() % 16 == 0
    t2 = lambda x, y: [(x, ">", 300), (y, "<", 800)]
    cols = [a[1:], b[:n], a[:n], b[1:]]
    cases = [
        Case([(a1, "<", 500)], n, model(cols, [(0, "<", 500)])),                          # a column view
        Case([(a1c, "<", 500)], n, model(cols, [(0, "<", 500)])),                         # ... and its aligned copy
        Case([(da, ">", 250)], n, model(cols, [(2, ">", 250)], sel[1:]), d_sel=sel1),     # a row-id view
        Case([(da, ">", 250)], n, model(cols, [(2, ">", 250)], sel[1:]), d_sel=sel1c),
        Case([(a1, ">", 250)], n, model(cols, [(0, ">", 250)], sel[1:]), d_sel=sel1c),    # through an aligned sel the column may sit anywhere
        Case(t2(a1, db[:n]), n, model(cols, [(0, ">", 300), (1, "<", 800)])),             # the first term only
        Case(t2(da[:n], b1), n, model(cols, [(2, ">", 300), (3, "<", 800)])),             # the second term only
        Case(t2(a1c, db[:n]), n, model(cols, [(0, ">", 300), (1, "<", 800)])),
        Case(t2(a1, b1), n, model(cols, [(0, ">", 300), (3, "<", 800)], sel[1:]), d_sel=sel1),      # every vector on a view
    ]
    run_guarded(rhj, mod, cases)
    assert np.array_equal(cases[0].want, cases[1].want) and np.array_equal(cases[2].want, cases[3].want)


# ---- 5. the hand-over at FILTER_SELF_TILES tiles ------------------------------------------------------------------------------

def test_hand_over_at_the_largest_batched_filter(rhj, mod):
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 1000, TOP_ROWS + 1, dtype=np.uint64), rng.integers(0, 1000, TOP_ROWS + 1, dtype=np.uint64)
    da, db = dev(rhj, a), dev(rhj, b)
    small = rng.integers(0, 50, 777, dtype=np.uint64)
    dsmall = dev(rhj, small)
    spec = [(0, "<", 400), (1, ">", 300)]
    terms = lambda n: [(da[:n], "<", 400), (db[:n], ">", 300)]
    cases = [Case([(dsmall, "=", 7)], 777, model([small], [(0, "=", 7)]))]
    for n in (TOP_ROWS, TOP_ROWS + 1):
        cases.append(Case(terms(n), n, model([a[:n], b[:n]], spec)))
    cases.append(Case([(dsmall, ">", 40)], 777, model([small], [(0, ">", 40)])))
    cases.append(Case(terms(TOP_ROWS + 1), TOP_ROWS + 1, cases[2].want, count_only=True))
    arr = run_guarded(rhj, mod, cases)
    assert [d.path for d in arr[:5]] == [BATCHED, BATCHED, ALONE, BATCHED, ALONE]
    assert rhj.lib.rhj_filter_batch_takes(TOP_ROWS) == 1 and rhj.lib.rhj_filter_batch_takes(TOP_ROWS + 1) == 0
    st = rhj.stats()
    assert st["units"] == 3 and st["n_r"] == sum(c.n for c in cases) and st["matches"] == sum(len(c.want) for c in cases)


# ---- 6. chunks -----------------------------------------------------------------------------------------------------------

def test_more_filters_than_one_chunk_holds(rhj, mod):
    rng = np.random.default_rng(6)
    nf, rows = MAX_FILTERS + 1, 100
    table = rng.integers(0, 100, (nf, rows), dtype=np.uint64)
    d_table = dev(rhj, table.reshape(-1)).view(nf, rows)
    cases = [Case([(d_table[k], "<", k % 101)], rows, model([table[k]], [(0, "<", k % 101)])) for k in range(nf)]
    arr = run_guarded(rhj, mod, cases)
    assert {d.path for d in arr[:nf]} == {BATCHED} and rhj.stats()["units"] == nf


def test_count_only_filters_beyond_one_arena(rhj, mod):
    """2100 count-only filters of 4 194 304 rows: 520 KB of masks and tile counts each, more than 1 GiB together — two chunks"""
    torch = rhj.torch
    nf = 2100
    assert nf * (TOP_ROWS // 8 + (TOP_ROWS // TILE) * 8) > 1 << 30 and nf <= MAX_FILTERS
    col = np.sort(np.random.default_rng(66).integers(0, 1 << 40, TOP_ROWS, dtype=np.uint64))
    d_col = dev(rhj, col)
    thresholds = np.unique(np.concatenate([np.array([0, 1, col[0], col[0] + 1, col[-1], col[-1] + 1, 1 << 40], dtype=np.uint64),
                                           np.random.default_rng(67).integers(0, 1 << 40, nf - 7, dtype=np.uint64)]))
    assert len(thresholds) == nf and thresholds.dtype == np.uint64      # distinct
    want = np.searchsorted(col, thresholds, side="left")
    arr = (mod.FilterDesc * nf)()
    for d, t in zip(arr, thresholds):
        d.n, d.nterms = TOP_ROWS, 1
        d.terms[0].d_col, d.terms[0].op, d.terms[0].value = d_col.data_ptr(), b"<", int(t)
    try:
        assert rhj.lib.rhj_filter_batch_device(arr, nf) == 0
        assert [d.hits for d in arr] == want.tolist()
        assert {d.path for d in arr} == {BATCHED} and {d.rc for d in arr} == {0}
        assert rhj.stats()["units"] == nf and rhj.stats()["matches"] == int(want.sum())
    finally:
        rhj.lib.rhj_release()                         # (the 1 GiB arena goes back before the next test)
        torch.cuda.synchronize()


# ---- 7. protocol ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny(rhj):
    """24 tiny filters on the device with the model's lists: one to three terms, every third through a row-id vector"""
    rng = np.random.default_rng(31337)
    out = []
    for k in range(24):
        n = int(rng.integers(1, 3000))
        cols = [rng.integers(0, 50, n, dtype=np.uint64) for _ in range(3)]
        spec = [(c, "<>="[rng.integers(0, 3)], int(rng.integers(0, 50))) for c in range(1 + k % 3)]
        sel = rng.integers(0, n, int(rng.integers(1, 3000)), dtype=np.uint64) if k % 3 == 2 else None
        d_cols = [dev(rhj, c) for c in cols]
        out.append(([(d_cols[c], op, v) for c, op, v in spec], dev(rhj, sel) if sel is not None else None, model(cols, spec, sel)))
    return out


def check_tiny(rhj, tiny, n, offset=0):
    pick = [tiny[(offset + i) % len(tiny)] for i in range(n)]
    res, paths = rhj.filter_batch_device([(terms, d_sel) for terms, d_sel, _ in pick], with_info=True)
    assert len(res) == n
    for i, ((ids, hits), (_, _, want)) in enumerate(zip(res, pick)):
        assert hits == len(want) and np.array_equal(host(ids), want), "filter %d of %d" % (i, n)
    rows = sum((d_sel if d_sel is not None else terms[0][0]).shape[0] for terms, d_sel, _ in pick)
    return paths, rows, sum(len(w) for _, _, w in pick)


def test_empty_filters_and_empty_batches(rhj, mod, tiny):
    assert rhj.lib.rhj_filter_batch_device(None, 0) == 0
    assert rhj.filter_batch_device([]) == []
    terms, d_sel, want = tiny[0]
    n = terms[0][0].shape[0]
    arr = run_guarded(rhj, mod, [Case(terms, n, want)])                  # a batch of one
    assert arr[0].path == BATCHED
    empty = np.zeros(0, dtype=np.uint64)
    cases = [Case(terms, n, want), Case(terms, 0, empty), Case([(None, "<", 5)], 0, empty), Case(terms, n, want, count_only=True),
             Case(terms, 0, empty, d_sel=terms[0][0], count_only=True)]
    arr = run_guarded(rhj, mod, cases)
    assert [d.path for d in arr[:5]] == [BATCHED, ALONE, ALONE, BATCHED, ALONE] and rhj.stats()["units"] == 2
    arr = run_guarded(rhj, mod, [Case(terms, 0, empty)])                 # nothing but an empty filter: nothing is launched
    assert arr[0].hits == 0 and rhj.stats()["units"] == 0 and rhj.stats()["path"] == "filter_batch"


def test_invalid_filters_stop_the_whole_batch(rhj, mod, tiny):
    terms, _, want = tiny[1]
    n = terms[0][0].shape[0]
    good = lambda: Case(terms, n, np.zeros(0, dtype=np.uint64))          # (wanted: nothing written, hits 0)
    bad = [Case([(terms[0][0], "!", 5)], n, None),                       # an unknown operator
           Case(terms + [(terms[0][0], "~", 1)], n, None),               # ... in a later term
           Case(terms, n, None, nterms=0), Case(terms, n, None, nterms=5),
           Case([(None, "<", 5)], n, None),                              # no column, but rows
           Case(terms, 0, None, nterms=0)]                               # (nterms is checked for an empty filter too)
    for b in bad:
        arr = run_guarded(rhj, mod, [good(), b, good()], expect_rc=-3)
        assert [d.rc for d in arr[:3]] == [0, -3, 0] and [d.hits for d in arr[:3]] == [0, 0, 0]
    arr = run_guarded(rhj, mod, [bad[0], good(), bad[3]], expect_rc=-3)
    assert [d.rc for d in arr[:3]] == [-3, 0, -3]
    check_tiny(rhj, tiny, 5)                                             # the library goes on


def test_batches_of_changing_size_back_to_back(rhj, tiny):
    rhj.lib.rhj_set_timing(1)
    for n in (1, 300, 2, 1000):
        paths, rows, hits = check_tiny(rhj, tiny, n, offset=n)
        assert set(paths) == {BATCHED}, n
        st = rhj.stats()
        assert st["path"] == "filter_batch" and st["units"] == n and st["n_r"] == rows and st["matches"] == hits and st["ms_total"] > 0
    rhj.lib.rhj_set_timing(0)
    check_tiny(rhj, tiny, 7)
    assert rhj.stats()["ms_total"] == 0 and rhj.stats()["units"] == 7
    rhj.lib.rhj_set_timing(2)


def test_single_calls_between_batches_find_their_buffers(rhj, oracle, tiny):
    """rhj_filter_device (both write forms), rhj_filter_eq2_device and a join between batches"""
    torch = rhj.torch
    rng = np.random.default_rng(8)
    n = TOP_ROWS + PAIR + 77                                             # beyond the SELF form: the scan's buffers
    col = rng.integers(0, 1000, n, dtype=np.uint64)
    other = np.where(rng.integers(0, 4, n) == 0, col, col + np.uint64(1))
    d_col, d_other = dev(rhj, col), dev(rhj, other)
    R = oracle.generate(30000, 0, 0, 0.0, 81)
    S = oracle.generate(50000, 1, 30000, 0.0, 82)
    want_join = oracle.join(R, S, 4)
    dR, dS = rhj.to_device(R), rhj.to_device(S)
    rhj.set_bits(4)
    out = torch.empty(n, dtype=torch.int64, device=rhj.dev)
    hits = C.c_uint64(0)
    for rep in range(2):
        check_tiny(rhj, tiny, 40, offset=rep)
        assert np.array_equal(single_filter(rhj, d_col, "<", 250), np.flatnonzero(col < 250).astype(np.uint64))
        check_tiny(rhj, tiny, 3, offset=rep)
        assert np.array_equal(single_filter(rhj, d_col[:5000], ">", 990), np.flatnonzero(col[:5000] > 990).astype(np.uint64))
        check_tiny(rhj, tiny, 17, offset=rep)
        assert rhj.lib.rhj_filter_eq2_device(d_col.data_ptr(), None, d_other.data_ptr(), None, n, out.data_ptr(), C.byref(hits)) == 0
        assert np.array_equal(host(out[:hits.value]), np.flatnonzero(col == other).astype(np.uint64))
        check_tiny(rhj, tiny, 9, offset=rep)
        pairs, m = rhj.join_device(dR, dS)
        got = rhj.pairs_to_numpy(pairs)
        assert m == len(want_join) and np.array_equal(got["row_idR"], want_join["row_idR"]) and np.array_equal(got["row_idS"], want_join["row_idS"])
        res = rhj.join_batch_device([(dR, dS)] * 3)                      # the batched joins share the pinned block and the descriptor buffer
        assert all(mm == len(want_join) for _, mm in res)


def test_batches_from_two_host_threads(rhj, tiny):
    errors = []

    def work(offset):
        try:
            for rep in range(4):
                check_tiny(rhj, tiny, 25 + 5 * rep, offset=offset + rep)
        except BaseException as e:                                   # noqa: B036 (reported by the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(o,)) for o in (0, 7)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
