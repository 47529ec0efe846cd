"""rhj_join_cols_batch_device / rhj_join_cols_device (include/rhj.h; csrc/rhj_small.hip.h, csrc/rhj_batch.hip.h): joins whose
relations are key columns read through optional row-id vectors — tuple i = (col[sel[i]], i) — pair for pair against the oracle
on the host-built relations and against rhj_join_batch_device / rhj_join_device on the relations rhj_build_relation_device
makes."""
import ctypes as C
import importlib

import numpy as np
import pytest

import helpers
from helpers import GUARD_ROWS, GuardedRows, make_rel

pytestmark = pytest.mark.gpu

BATCHED = 6                                  # rhj_join_cols_desc::path of a join that ran in the batched launches
TOP = 65536                                  # 8 tiles of 8192 tuples: the largest relation of a batched join
TILE = 8192


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def rhj(mod):
    r = mod.RHJ(device=0)
    yield r
    r.lib.rhj_set_small(1)
    r.lib.rhj_set_order(0)
    r.lib.rhj_set_timing(2)
    r.set_bits(4)


def dev(rhj, a):
    return rhj.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


def same_pairs(rhj, t, want, what):
    got = rhj.pairs_to_numpy(t)
    assert len(got) == len(want), "%s: %d pairs, expected %d" % (what, len(got), len(want))
    assert np.array_equal(got["row_idR"], want["row_idR"]) and np.array_equal(got["row_idS"], want["row_idS"]), what


# ---- a join's two sides on the host and on the device ------------------------------------------------------------------------

def vector(kind, n, rows, rng):
    """a row-id vector of n entries into a column of `rows` rows"""
    if kind == "asc":                        # a filter's output: an ascending subset
        return np.sort(rng.choice(rows, size=n, replace=False)).astype(np.uint64)
    if kind == "perm":
        assert n == rows
        return rng.permutation(rows).astype(np.uint64)
    if kind == "desc":
        return np.arange(rows - 1, rows - 1 - n, -1).astype(np.uint64)
    if kind == "rep":                        # repeated indices
        return rng.integers(0, rows, size=n).astype(np.uint64)
    assert kind == "same"
    return np.full(n, int(rng.integers(0, rows)), dtype=np.uint64)


def side(n, kind, dom, rng):
    """(column, vector or None) of a relation of n tuples with keys below dom"""
    if kind is None:
        return rng.integers(0, max(dom, 1), size=n, dtype=np.uint64), None
    rows = n if kind == "perm" else max(2 * n, 1) if kind == "asc" else n + 3
    return rng.integers(0, max(dom, 1), size=rows, dtype=np.uint64), vector(kind, n, rows, rng)


def rel_of(col, sel):
    """what GetRelation / rhj_build_relation_device make of a column and a vector"""
    return make_rel(col if sel is None else col[sel.astype(np.int64)])


class Devs:
    """device copies by identity of the host array: a column or vector used twice is ONE device buffer"""

    def __init__(self, rhj):
        self.rhj, self.d = rhj, {}

    def __call__(self, a):
        if a is None:
            return None
        if id(a) not in self.d:
            self.d[id(a)] = (a, dev(self.rhj, a))
        return self.d[id(a)][1]

    def join(self, case):
        _, cR, sR, cS, sS = case
        return self(cR), self(sR), self(cS), self(sS)

    def assert_unchanged(self):
        for a, t in self.d.values():
            assert np.array_equal(t.cpu().numpy().view(np.uint64), a), "a column or vector was written"


def build(rhj, col, sel):
    """rhj_build_relation_device: the [n, 2] tuple tensor of a column read through a vector"""
    n = col.shape[0] if sel is None else sel.shape[0]
    t = rhj.torch.empty((max(n, 1), 2), dtype=rhj.torch.int64, device=rhj.dev)
    assert rhj.lib.rhj_build_relation_device(col.data_ptr(), sel.data_ptr() if sel is not None else None, n, t.data_ptr()) == 0
    return t[:n]


def single(rhj, dR, dS):
    pairs, m = rhj.join_device(dR, dS)
    return pairs, m, rhj.lib.rhj_last_stats().contents.reserved & 0xff


def raw_batch(rhj, mod, joins, outs):
    """joins: [(colR, selR, colS, selS)] device tensors; outs: [(pointer or None, capacity)].  Returns (return code, descriptors)."""
    arr = (mod.JoinColsDesc * max(len(joins), 1))()
    for d, (cR, sR, cS, sS), (ptr, cap) in zip(arr, joins, outs):
        d.d_colR, d.d_selR, d.nR = rhj._cols_side(cR, sR)
        d.d_colS, d.d_selS, d.nS = rhj._cols_side(cS, sS)
        d.d_out, d.out_capacity = ptr, cap
        d.matches, d.rc, d.path = 0xDEAD, -77, -77
    return rhj.lib.rhj_join_cols_batch_device(arr, len(joins)), arr


# ---- a seeded mixed batch ------------------------------------------------------------------------------------------------------

def mixed_batch(rng):
    """[(name, colR, selR, colS, selS)]: sizes at the tile, self-histogram and class edges, empty sides, the four source forms
    and the five vector kinds, one column in several joins and on both sides of one, keys with 16 and with more than 16 matches
    (the walk kernel), and a bucket whose build side is beyond the LDS index (that join runs alone, tiled)."""
    out = []

    def add(name, nR, kR, nS, kS):
        dom = max(nR, nS)
        out.append((name,) + side(nR, kR, dom, rng) + side(nS, kS, dom, rng))

    out.append(("1x1", np.array([77], dtype=np.uint64), None, np.array([77], dtype=np.uint64), None))     # (a match for sure)
    add("2x1", 2, "asc", 1, None)
    add("8191x8192", TILE - 1, None, TILE, "perm")
    add("8193x8191", TILE + 1, "desc", TILE - 1, "rep")
    add("16384x16384", 2 * TILE, None, 2 * TILE, None)               # two tiles a side: no histogram launch
    add("16385x100", 2 * TILE + 1, "asc", 100, None)                 # three tiles: the histogram launch
    add("top", TOP, None, TOP, "asc")
    add("top+1 R", TOP + 1, "perm", 300, "same")
    add("top+1 S", 300, None, TOP + 1, None)
    add("empty R", 0, "asc", 50, None)
    add("empty S", 50, None, 0, "rep")
    add("empty both", 0, "asc", 0, "desc")
    shared = rng.integers(0, 15000, size=20000, dtype=np.uint64)
    for k, kind in enumerate(("asc", "rep", "desc")):
        n = 10000 if kind == "asc" else 9000
        out.append(("shared %d" % k, shared, vector(kind, n, len(shared), rng)) + side(5000 + 4000 * k, (None, "perm", "asc")[k], 15000, rng))
    out.append(("shared both", shared, vector("asc", 10000, len(shared), rng), shared, None))
    # every key 16 times on the build side (S, the smaller one in every bucket): the overflow stash holds a probe tuple's
    # 2nd..16th match exactly; 17 and more: beyond the stash, k_join_walk writes those units
    keys = rng.integers(0, 1 << 40, size=400, dtype=np.uint64)
    for name, fR, fS in (("16 matches", 20, 16), ("17 matches", 20, 17), ("40 matches", 50, 40)):
        colS = np.repeat(keys, fS)
        out.append((name, rng.permutation(np.repeat(keys, fR)), None, colS, vector("perm", len(colS), len(colS), rng)))
    # one bucket of 40 000 distinct keys on both sides (the low 8 bits of every key are 0): its build side cannot be indexed
    # in LDS at any width of 1..8 bits
    big = (rng.permutation(1 << 17)[:40000].astype(np.uint64) << np.uint64(8))
    out.append(("beyond LDS", big, None, big, vector("perm", len(big), len(big), rng)))
    return out


def host_rels(case):
    _, cR, sR, cS, sS = case
    return rel_of(cR, sR), rel_of(cS, sS)


@pytest.mark.parametrize("bits", (1, 4, 8))
def test_mixed_batch_equals_the_batch_on_built_relations(rhj, oracle, bits):
    import torch
    cases = mixed_batch(np.random.default_rng(5200 + bits))
    to_dev = Devs(rhj)
    joins = [to_dev.join(c) for c in cases]
    assert joins[12][0].data_ptr() == joins[13][0].data_ptr() == joins[15][2].data_ptr()      # the shared column is ONE device buffer
    forms = {(c[2] is not None, c[4] is not None) for c in cases}
    assert len(forms) == 4                                          # none/none, sel/none, none/sel, sel/sel
    built = [(build(rhj, cR, sR), build(rhj, cS, sS)) for cR, sR, cS, sS in joins]
    rhj.set_bits(bits)
    res, paths = rhj.join_cols_batch_device(joins, with_info=True)
    ref, ref_paths = rhj.join_batch_device(built, with_info=True)
    for c, (dR, dS), (pairs, m), p, (rpairs, rm), rp in zip(cases, built, res, paths, ref, ref_paths):
        name = c[0]
        what = "%s on %d bits" % (name, bits)
        R, S = host_rels(c)
        assert (len(R), len(S)) == (dR.shape[0], dS.shape[0]), what
        assert m == rm == pairs.shape[0], what
        assert torch.equal(pairs, rpairs), what + ": differs from rhj_join_batch_device on the built relations"
        same_pairs(rhj, pairs, oracle.join(R, S, bits), what)
        if len(R) == 0 or len(S) == 0:
            assert p == 0 and m == 0, what
        elif name == "beyond LDS":
            _, _, p1 = single(rhj, dR, dS)
            assert p == 0 and p1 == 0, what                         # alone and tiled, as the single call ends up
        elif rhj.lib.rhj_batch_takes(bits, len(R), len(S)):
            assert p == BATCHED, what
        else:
            _, _, p1 = single(rhj, dR, dS)
            assert p == p1 != BATCHED, what
        assert p == rp, what
    names = [c[0] for c in cases]
    assert paths[names.index("top")] == BATCHED and paths[names.index("16385x100")] == BATCHED
    assert all(paths[i] != BATCHED for i, n in enumerate(names) if n.startswith("top+1"))
    to_dev.assert_unchanged()


# ---- the capacity protocol, per join -----------------------------------------------------------------------------------------

def test_capacity_protocol_per_join(rhj, mod, oracle):
    import torch
    rng = np.random.default_rng(199)
    cases = [c for c in mixed_batch(rng) if c[0] in ("8193x8191", "16385x100", "top+1 R", "empty R", "shared 1", "16 matches", "40 matches",
                                                     "beyond LDS")]
    bits = 5
    rhj.set_bits(bits)
    to_dev = Devs(rhj)
    joins = [to_dev.join(c) for c in cases]
    want = [helpers.pairs_to_device(rhj, oracle.join(*host_rels(c), bits)) for c in cases]
    Ms = [w.shape[0] for w in want]
    assert sum(M > 0 for M in Ms) >= 6

    rc, arr = raw_batch(rhj, mod, joins, [(None, 0)] * len(joins))   # count only
    assert rc == 0
    for d, M, c in zip(arr, Ms, cases):
        assert (d.matches, d.rc) == (M, 0), c[0]

    def caps_of(mode, i):
        M = Ms[i]
        return {"zero": 0, "M-1": max(M - 1, 0), "M": M, "mixed": (0, max(M - 1, 0), M, M + 5)[i % 4]}[mode]

    for mode in ("zero", "M-1", "M", "mixed"):
        caps = [caps_of(mode, i) for i in range(len(joins))]
        guards = [GuardedRows(torch, rhj.dev, max(M, cap)) for M, cap in zip(Ms, caps)]
        rc, arr = raw_batch(rhj, mod, joins, [(g.ptr, cap) for g, cap in zip(guards, caps)])
        torch.cuda.synchronize()
        short = [M > cap for M, cap in zip(Ms, caps)]
        assert rc == (1 if any(short) else 0), mode
        for d, g, M, cap, c, w, s in zip(arr, guards, Ms, caps, cases, want, short):
            what = "%s, capacity %s = %d of %d pairs" % (c[0], mode, cap, M)
            assert d.matches == M and d.rc == (1 if s else 0), what + ": matches %d rc %d" % (d.matches, d.rc)
            g.assert_untouched(-GUARD_ROWS, 0, what + ", in front of the buffer")
            g.assert_untouched(cap, max(M, cap) + GUARD_ROWS, what + ", behind the capacity")
            n = min(cap, M)
            assert torch.equal(g.body(0, n), w[:n]), what
    to_dev.assert_unchanged()


# ---- pointers that are 8-byte but not 16-byte aligned ------------------------------------------------------------------------

@pytest.mark.parametrize("n", (TILE + 1, 20000))
def test_views_offset_by_eight_bytes(rhj, oracle, n):
    import torch
    rng = np.random.default_rng(77 + n)
    bits = 4
    rhj.set_bits(bits)
    cR, cS = (rng.integers(0, n, size=2 * n, dtype=np.uint64) for _ in range(2))
    sR, sS = vector("asc", n, 2 * n, rng), vector("rep", n - 5, 2 * n, rng)

    def odd(a):                              # a[...] behind one spare word: the view starts 8 bytes into an aligned allocation
        t = dev(rhj, np.concatenate([np.zeros(1, dtype=np.uint64), a]))[1:]
        assert t.data_ptr() % 16 == 8
        return t

    dcR, dsR, dcS, dsS = odd(cR), odd(sR), odd(cS), odd(sS)
    want_sel = oracle.join(rel_of(cR, sR), rel_of(cS, sS), bits)
    want_whole = oracle.join(rel_of(cR, None), rel_of(cS, None), bits)
    res, paths = rhj.join_cols_batch_device([(dcR, dsR, dcS, dsS), (dcR, None, dcS, None)], with_info=True)
    assert paths == [BATCHED, BATCHED]
    same_pairs(rhj, res[0][0], want_sel, "vectors and columns 8 bytes off, %d tuples" % n)
    same_pairs(rhj, res[1][0], want_whole, "columns 8 bytes off, %d rows" % (2 * n))
    ref = rhj.join_batch_device([(build(rhj, dcR, dsR), build(rhj, dcS, dsS)), (build(rhj, dcR, None), build(rhj, dcS, None))])
    assert torch.equal(res[0][0], ref[0][0]) and torch.equal(res[1][0], ref[1][0])
    pairs, m = rhj.join_cols_device(dcR, dsR, dcS, dsS)
    assert rhj.stats()["path"] == "small"
    same_pairs(rhj, pairs, want_sel, "single call, vectors and columns 8 bytes off, %d tuples" % n)


# ---- validation: the whole batch before anything is launched -----------------------------------------------------------------

def test_null_column_stops_the_whole_batch(rhj, mod):
    import torch
    rng = np.random.default_rng(5)
    rhj.set_bits(4)
    col = dev(rhj, rng.integers(0, 50, size=500, dtype=np.uint64))
    sel = dev(rhj, vector("asc", 200, 500, rng))
    joins = [(col, sel, col, None), (col, None, col, sel), (col, sel, col, sel)]
    guards = [GuardedRows(torch, rhj.dev, 4000) for _ in joins]
    for bad_side in ("R", "S"):
        arr = (mod.JoinColsDesc * len(joins))()
        for d, (cR, sR, cS, sS), g in zip(arr, joins, guards):
            d.d_colR, d.d_selR, d.nR = rhj._cols_side(cR, sR)
            d.d_colS, d.d_selS, d.nS = rhj._cols_side(cS, sS)
            d.d_out, d.out_capacity = g.ptr, 4000
            d.matches, d.rc, d.path = 0xDEAD, -77, -77
        if bad_side == "R":
            arr[1].d_colR = None
        else:
            arr[1].d_colS = None
        assert rhj.lib.rhj_join_cols_batch_device(arr, len(joins)) == -3
        torch.cuda.synchronize()
        assert [d.rc for d in arr] == [0, -3, 0]
        assert [d.matches for d in arr] == [0, 0, 0] and [d.path for d in arr] == [0, 0, 0]
        for g in guards:
            g.assert_untouched(-GUARD_ROWS, 4000 + GUARD_ROWS, "a batch with an invalid join")
    # a NULL column of an empty side is no error
    rc, arr = raw_batch(rhj, mod, [(col[:0], None, col, sel)], [(None, 0)])
    assert arr[0].d_colR is None and (rc, arr[0].rc, arr[0].matches, arr[0].path) == (0, 0, 0, 0)


# ---- filter -> join with nothing in between ------------------------------------------------------------------------------------

def test_filter_outputs_are_the_joins_vectors(rhj, oracle):
    import torch
    rng = np.random.default_rng(2018)
    rows, nj, bits = 30000, 8, 4
    rhj.set_bits(bits)
    host, filters = [], []
    for j in range(nj):
        for s in range(2):
            key = rng.integers(0, 20000, size=rows, dtype=np.uint64)          # the join's column
            attr = rng.integers(0, 1000, size=rows, dtype=np.uint64)          # the filter's column
            op, k = ("<", 100 + 100 * j) if s == 0 else (">", 900 - 60 * j)
            host.append((key, attr, op, k))
            filters.append(([(dev(rhj, attr), op, k)], None))
    keys = [dev(rhj, h[0]) for h in host]
    hits = rhj.filter_batch_device(filters)                          # [(indices tensor, hits)]: device vectors, counts in the descriptors
    joins = [(keys[2 * j], hits[2 * j][0], keys[2 * j + 1], hits[2 * j + 1][0]) for j in range(nj)]
    for j in range(nj):
        assert joins[j][1].shape[0] == hits[2 * j][1] and joins[j][3].shape[0] == hits[2 * j + 1][1]
    res, paths = rhj.join_cols_batch_device(joins, with_info=True)
    assert paths == [BATCHED] * nj
    ref = rhj.join_batch_device([(build(rhj, cR, sR), build(rhj, cS, sS)) for cR, sR, cS, sS in joins])
    for j in range(nj):
        sides = []
        for key, attr, op, k in host[2 * j:2 * j + 2]:
            keep = np.flatnonzero(attr < np.uint64(k) if op == "<" else attr > np.uint64(k))
            sides.append(make_rel(key[keep]))
        assert len(sides[0]) == hits[2 * j][1] > 0 and len(sides[1]) == hits[2 * j + 1][1] > 0
        same_pairs(rhj, res[j][0], oracle.join(sides[0], sides[1], bits), "filtered join %d" % j)
        assert torch.equal(res[j][0], ref[j][0]), j


# ---- chunks, and state carried between calls ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny(rhj, oracle):
    """16 tiny joins through vectors on the device with the oracle's lists at 4 bits"""
    rng = np.random.default_rng(41337)
    out = []
    for k in range(16):
        nR, nS = int(rng.integers(1, 200)), int(rng.integers(1, 200))
        cR, sR = side(nR, ("asc", "rep", None)[k % 3], 90, rng)
        cS, sS = side(nS, (None, "desc", "asc")[k % 3], 90, rng)
        R, S = rel_of(cR, sR), rel_of(cS, sS)
        d = [None if a is None else dev(rhj, a) for a in (cR, sR, cS, sS)]
        out.append((tuple(d), rhj.to_device(R), rhj.to_device(S), helpers.pairs_to_device(rhj, oracle.join(R, S, 4))))
    return out


def check_tiny(rhj, tiny, n, offset=0):
    import torch
    pick = [tiny[(offset + i) % len(tiny)] for i in range(n)]
    res, paths = rhj.join_cols_batch_device([p[0] for p in pick], with_info=True)
    assert len(res) == n
    for i, ((pairs, m), p) in enumerate(zip(res, pick)):
        assert m == p[3].shape[0] and torch.equal(pairs, p[3]), "join %d of %d" % (i, n)
    return paths


def test_chunks_and_other_calls_in_between(rhj, tiny):
    import torch
    rhj.set_bits(4)
    assert set(check_tiny(rhj, tiny, 400, offset=1)) == {BATCHED}   # about 2.7 MB a join: more than one chunk of the arena
    assert rhj.stats()["path"] == "batch"
    res = rhj.join_batch_device([(p[1], p[2]) for p in tiny])       # the tuple batch shares the arena and the pinned block
    for (pairs, m), p in zip(res, tiny):
        assert torch.equal(pairs, p[3])
    pairs, m = rhj.join_device(tiny[3][1], tiny[3][2])
    assert torch.equal(pairs, tiny[3][3])
    assert set(check_tiny(rhj, tiny, 30, offset=5)) == {BATCHED}
    assert rhj.join_cols_batch_device([]) == []


def test_small_path_off_runs_every_join_alone(rhj, tiny):
    rhj.set_bits(4)
    rhj.lib.rhj_set_small(0)
    try:
        paths = check_tiny(rhj, tiny, 20)
    finally:
        rhj.lib.rhj_set_small(1)
    assert BATCHED not in paths
    assert set(check_tiny(rhj, tiny, 20)) == {BATCHED}


# ---- rhj_join_cols_device: the single call -----------------------------------------------------------------------------------

SINGLE_SIZES = (1, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 1)


@pytest.fixture(scope="module")
def single_cases(rhj):
    """[(name, host sides, device sides, built relations)] for every size and vectors on one side, both sides and neither"""
    rng = np.random.default_rng(777)
    out = []
    for n in SINGLE_SIZES:
        for form, (kR, kS) in (("sel/none", ("asc", None)), ("sel/sel", ("rep", "asc")), ("none/none", (None, None))):
            nS = max(n - 7, 1)
            cR, sR = side(n, kR, n, rng)
            cS, sS = side(nS, kS, n, rng)
            d = tuple(None if a is None else dev(rhj, a) for a in (cR, sR, cS, sS))
            out.append(("%d x %d %s" % (n, nS, form), (cR, sR, cS, sS), d, (build(rhj, d[0], d[1]), build(rhj, d[2], d[3]))))
    return out


@pytest.mark.parametrize("bits", (4, 8, 9))
def test_single_call_at_every_size_and_form(rhj, oracle, single_cases, bits):
    import torch
    rhj.set_bits(bits)
    for name, (cR, sR, cS, sS), d, (bR, bS) in single_cases:
        what = "%s on %d bits" % (name, bits)
        pairs, m = rhj.join_cols_device(*d)
        path = rhj.stats()["path"]
        if bits <= 8:
            assert path == "small", what
        else:
            assert path != "small", what                            # beyond the one-pass partition: the materialising route
        ref, rm = rhj.join_device(bR, bS)
        assert m == rm and torch.equal(pairs, ref), what + ": differs from rhj_join_device on the built relations"
        same_pairs(rhj, pairs, oracle.join(rel_of(cR, sR), rel_of(cS, sS), bits), what)
    for t, (_, h, d, _) in ((t, c) for c in single_cases for t in (0, 1, 2, 3)):
        if h[t] is not None:
            assert np.array_equal(d[t].cpu().numpy().view(np.uint64), h[t]), "a column or vector was written"


def test_single_call_beyond_lds_order_any_and_capacity(rhj, mod, oracle):
    import torch
    rng = np.random.default_rng(4242)
    # one bucket of 40 000 distinct keys on both sides: the small path partitions (reading the columns), the tiled path joins
    big = (rng.permutation(1 << 17)[:40000].astype(np.uint64) << np.uint64(8))
    perm = vector("perm", len(big), len(big), rng)
    dbig, dperm = dev(rhj, big), dev(rhj, perm)
    rhj.set_bits(6)
    pairs, m = rhj.join_cols_device(dbig, None, dbig, dperm)
    assert rhj.stats()["path"] == "tiled"
    same_pairs(rhj, pairs, oracle.join(make_rel(big), make_rel(big[perm.astype(np.int64)]), 6), "beyond LDS: tiled after the small partition")

    # order mode "any": the library's own radix for the sizes
    nR, nS = 24000, 9000
    cR, sR = side(nR, "asc", nR, rng)
    cS, sS = side(nS, "rep", nR, rng)
    d = tuple(dev(rhj, a) for a in (cR, sR, cS, sS))
    R, S = rel_of(cR, sR), rel_of(cS, sS)
    rhj.set_bits(4)
    rhj.lib.rhj_set_order(1)
    try:
        pairs, m = rhj.join_cols_device(*d)
        res = rhj.join_cols_batch_device([d])
    finally:
        rhj.lib.rhj_set_order(0)
    auto = rhj.lib.rhj_auto_radix_bits(nR, nS)
    want = oracle.join(R, S, auto)
    same_pairs(rhj, pairs, want, "order any, %d bits" % auto)
    same_pairs(rhj, res[0][0], want, "order any in a batch, %d bits" % auto)

    # a short buffer and count only, through the raw entry point
    rhj.set_bits(4)
    want = oracle.join(R, S, 4)
    M = len(want)
    assert M > 100
    args = [x for c, s in ((d[0], d[1]), (d[2], d[3])) for x in rhj._cols_side(c, s)]
    m = C.c_uint64(0xDEAD)
    assert rhj.lib.rhj_join_cols_device(*args, None, 0, C.byref(m)) == 0 and m.value == M
    for cap in (0, M - 1, M, M + 5):
        helpers.guarded_join(rhj, lambda ptr, c, mref: rhj.lib.rhj_join_cols_device(*args, ptr, c, mref), d[0], d[2], cap, want)
    for a, t in zip((cR, sR, cS, sS), d):
        assert np.array_equal(t.cpu().numpy().view(np.uint64), a), "a column or vector was written"
