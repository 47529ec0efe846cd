"""The small join's partition (sigmod-2018_amd/csrc/rhj_small.hip.h: small_hist_body, small_selfhist, small_colsum, the plan
workgroup of small_scatter_body, the stable LDS scatter) at its tile, slice, round and self-count edges.

Every case is a shape of tests/small_model.py, which tests/test_small_model.py holds in its regime on the CPU: a large side of T
tiles whose histogram rows differ from one another on purpose (tile_digit, last_tile_only, one_digit_*) or not (uniform),
every tuple of it with exactly one partner among the 4096 distinct keys of the small side.  The device's pair list is compared
with oracle.join on the same host arrays bit for bit, order included — row ids are positions, so a tuple moved inside its
bucket shows — in a buffer of exactly M rows between sentinel rows (helpers.guarded_join), and every single join asserts
stats()["path"], ["units"] and ["max_build"] against the model.

  A  the self-counted path (two launches) and its end at 2 x 8192 tuples       E  A, B and C through rhj_join_cols_device
  B  slice edges: 3, 8, 9, 15, 16, 17 tiles                                    F  row ids beyond 2^32
  C  round edges 128/129, 256/257 and the top at 512 tiles                     G  the cnt buffers reused with changing strides
  D  two large sides, and the hand-over to the tiled path behind them          H  batched: rhj_join_batch_device, ..._cols_...
"""
import importlib

import numpy as np
import pytest

import small_model as sm
from helpers import GUARD_ROWS, GuardedRows, guarded_join, make_rel, pairs_to_device

pytestmark = pytest.mark.gpu

K = sm.constants()
T = K.SM_TILE
BATCHED = 6                                  # rhj_join_desc::path of a join that ran in the batched launches

# rhj_set_* knobs and their defaults; every case restores all of them
DEFAULTS = {"small": 1, "fused": 1, "resident": 1, "lowradix": 1, "order": 0}


def restore(rhj):
    for k, v in DEFAULTS.items():
        getattr(rhj.lib, "rhj_set_" + k)(v)


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def rhj(mod):
    r = mod.RHJ(device=0)
    restore(r)
    yield r
    restore(r)
    r.set_bits(4)


def run(rhj, oracle, bits, R, S, what, path="small", sides=None):
    """One join on the device against the oracle: rhj_join_device on (R, S), or rhj_join_cols_device on sides =
    ((colR, selR), (colS, selS)), host arrays whose tuples are R and S."""
    torch = rhj.torch
    want = oracle.join(R, S, bits)
    rhj.set_bits(bits)
    if sides is None:
        dR, dS = rhj.to_device(R), rhj.to_device(S)

        def call(out, cap, m):
            return rhj.lib.rhj_join_device(dR.data_ptr(), len(R), dS.data_ptr(), len(S), out, cap, m)
    else:
        dev = [[None if a is None else torch.from_numpy(a.view(np.int64)).to(rhj.dev) for a in side] for side in sides]
        args = [x for col, sel in dev for x in rhj._cols_side(col, sel)]
        assert (args[2], args[5]) == (len(R), len(S))
        dR, dS = dev[0][0], dev[1][0]

        def call(out, cap, m):
            return rhj.lib.rhj_join_cols_device(*args, out, cap, m)
    try:
        guarded_join(rhj, call, dR, dS, len(want), want)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from None
    st = rhj.stats()
    e = sm.expected(R["value"], S["value"], bits)
    if path == "small":
        assert e.path == "small"
        assert (st["path"], st["units"], st["max_build"]) == ("small", e.units, e.max_build), (what, st["path"], st["units"], st["max_build"], e)
    else:
        assert e.path is None
        assert st["path"] == path if path else st["path"] != "small", (what, st["path"])
    return len(want)


ORDERS = (True, False)                       # the large side is R, is S


def order_id(large_is_r):
    return "large_R" if large_is_r else "large_S"


def both_orders(rhj, oracle, bits, kL, kO, what, fk=True, orders=ORDERS, **kw):
    """the relation of keys kL as R against kO as S, then as S against kO as R"""
    L, O = make_rel(kL), make_rel(kO)
    for large_is_r in orders:
        n = run(rhj, oracle, bits, *((L, O) if large_is_r else (O, L)), "%s, large side is %s" % (what, "RS"[not large_is_r]), **kw)
        assert not fk or n == len(L)


def cols_sides(R, S, sel_mode, seed):
    """R and S as rhj_join_cols_device reads them: the whole key column, or a longer column through a permutation vector"""
    if sel_mode == "whole column":
        return tuple((np.ascontiguousarray(rel["value"]), None) for rel in (R, S))
    rng = np.random.default_rng(seed)
    out = []
    for rel in (R, S):
        n = len(rel)
        col = rng.integers(0, 1 << 47, size=n + n // 2 + 7, dtype=np.uint64)
        sel = rng.permutation(len(col))[:n].astype(np.uint64)
        col[sel] = rel["value"]
        assert np.array_equal(make_rel(col[sel]), rel)
        out.append((col, sel))
    return tuple(out)


def both_orders_cols(rhj, oracle, bits, kL, kO, what, sel_mode, orders=ORDERS):
    L, O = make_rel(kL), make_rel(kO)
    for large_is_r in orders:
        R, S = (L, O) if large_is_r else (O, L)
        run(rhj, oracle, bits, R, S, "%s, %s, large side is %s" % (what, sel_mode, "RS"[not large_is_r]),
            sides=cols_sides(R, S, sel_mode, 900 + bits))


# ---- A. self-count edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", sm.A_BITS)
@pytest.mark.parametrize("sizes", sm.a_sizes(), ids=lambda s: "%dx%d" % s)
def test_self_count_edges(rhj, oracle, sizes, bits):
    """2 x 8192 tuples is the last size whose scatter workgroups count the digits themselves; one more and k_small_hist is
    launched for a relation whose last tile holds one tuple"""
    n, m = sizes
    for kind in sm.A_KINDS:
        kL, kO = sm.a_keys(kind, bits, n, m)
        both_orders(rhj, oracle, bits, kL, kO, "%s %dx%d on %d bits" % (kind, n, m, bits), fk=m >= 1 << bits)


# ---- B. slice edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", sm.B_BITS)
@pytest.mark.parametrize("ntiles", sm.B_TILES)
def test_slice_edges(rhj, oracle, ntiles, bits):
    """16 slices of ceil(tiles / 16) rows (the plan's workgroup: 8 at 8 bits): empty slices, the last one of one row"""
    for full in (True, False):
        for kind in sm.B_KINDS:
            n = sm.size_of(ntiles, full)
            both_orders(rhj, oracle, bits, sm.large_keys(kind, bits, n), sm.small_keys(bits), "%s, %d tuples on %d bits" % (kind, n, bits))


# ---- C. round edges and the top --------------------------------------------------------------------------------------------------
C_CASES = [(sm.size_of(t, full), bits, kind) for t, (fulls, kinds) in sm.C_ROWS.items() for full in fulls for bits in sm.C_BITS for kind in kinds]


@pytest.mark.parametrize("large_is_r", ORDERS, ids=order_id)
@pytest.mark.parametrize("n,bits,kind", C_CASES)
def test_round_edges(rhj, oracle, n, bits, kind, large_is_r):
    """a slice of SM_ROWS + 1 rows takes a second round of loads that holds one row (the plan's workgroup: 2 * SM_ROWS + 1);
    512 tiles are the most the path takes.  (One join a case: the largest moves 64 MB each way.)"""
    both_orders(rhj, oracle, bits, sm.large_keys(kind, bits, n), sm.small_keys(bits), "%s, %d tuples on %d bits" % (kind, n, bits),
                orders=(large_is_r,))


@pytest.mark.parametrize("large_is_r", ORDERS, ids=order_id)
@pytest.mark.parametrize("bits", sm.C_BITS)
def test_one_tuple_beyond_the_top(rhj, oracle, bits, large_is_r):
    n = K.SM_MAX_TILES * T + 1
    both_orders(rhj, oracle, bits, sm.large_keys("tile_digit", bits, n), sm.small_keys(bits), "%d tuples on %d bits" % (n, bits), path=None,
                orders=(large_is_r,))


# ---- D. two large sides ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", list(sm.D_BITS))
@pytest.mark.parametrize("kind", sm.D_KINDS)
def test_two_large_sides(rhj, oracle, kind, bits):
    """129 x 257 tiles: both relations' histograms in one launch, both halves of the plan's workgroup with rounds of their own.
    At 2 bits (low-radix path off) the build sides are beyond the LDS index: the tiled path takes over this partition."""
    kR, kS = sm.d_keys(kind)
    path = sm.D_BITS[bits]
    try:
        if path == "tiled":
            rhj.lib.rhj_set_lowradix(0)
        n = run(rhj, oracle, bits, make_rel(kR), make_rel(kS), "%s on %d bits" % (kind, bits), path=path)
        assert n == len(kS)
    finally:
        restore(rhj)


# ---- E. through columns ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel_mode", sm.E_SELS)
@pytest.mark.parametrize("bits", sm.A_BITS)
def test_self_count_edges_through_columns(rhj, oracle, bits, sel_mode):
    """small_selfhist<true> at 2 tiles, k_small_hist_cols at 3"""
    for n, m in sm.a_sizes():
        if max(sm.tiles(n), sm.tiles(m)) in sm.E_A_TILES:
            for kind in sm.A_KINDS:
                kL, kO = sm.a_keys(kind, bits, n, m)
                both_orders_cols(rhj, oracle, bits, kL, kO, "%s %dx%d on %d bits" % (kind, n, m, bits), sel_mode)


@pytest.mark.parametrize("sel_mode", sm.E_SELS)
@pytest.mark.parametrize("bits", sm.B_BITS)
@pytest.mark.parametrize("n", [sm.size_of(t, full) for t in sm.E_B_TILES for full in (True, False)])
def test_slice_edges_through_columns(rhj, oracle, n, bits, sel_mode):
    for kind in sm.B_KINDS:
        both_orders_cols(rhj, oracle, bits, sm.large_keys(kind, bits, n), sm.small_keys(bits), "%s, %d tuples on %d bits" % (kind, n, bits), sel_mode)


@pytest.mark.parametrize("large_is_r", ORDERS, ids=order_id)
@pytest.mark.parametrize("sel_mode", sm.E_SELS)
@pytest.mark.parametrize("n,bits,kind", [c for c in C_CASES if sm.tiles(c[0]) in sm.E_C_TILES])
def test_round_edges_through_columns(rhj, oracle, n, bits, kind, sel_mode, large_is_r):
    both_orders_cols(rhj, oracle, bits, sm.large_keys(kind, bits, n), sm.small_keys(bits), "%s, %d tuples on %d bits" % (kind, n, bits), sel_mode,
                     orders=(large_is_r,))


# ---- G. the cnt buffers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("large_is_r", [True, False], ids=["R", "S"])
def test_cnt_buffers_reused_with_changing_strides(rhj, oracle, large_is_r):
    """back to back in one process: the row stride of cnt (bins) changes and the tile count shrinks, nothing is cleared between"""
    for ntiles, bits in sm.G_STEPS:
        L, O = make_rel(sm.large_keys("tile_digit", bits, ntiles * T)), make_rel(sm.small_keys(bits))
        n = run(rhj, oracle, bits, *((L, O) if large_is_r else (O, L)), "%d tiles on %d bits" % (ntiles, bits))
        assert n == len(L)


# ---- H. batched ------------------------------------------------------------------------------------------------------------------
def batch_inputs(bits):
    out = []
    for kind, ntiles, full, large_is_r in sm.h_joins(bits):
        L, O = make_rel(sm.large_keys(kind, bits, sm.size_of(ntiles, full))), make_rel(sm.small_keys(bits))
        out.append(((L, O) if large_is_r else (O, L)) + ("%s, %d tiles, full %d, large side is %s" % (kind, ntiles, full, "RS"[not large_is_r]), len(L)))
    return out


def check_batch(rhj, arr, rc, guards, wants, joins, bits):
    rhj.torch.cuda.synchronize()
    assert rc == 0
    for d, g, w, (R, S, what, large) in zip(arr, guards, wants, joins):
        what = "%s on %d bits" % (what, bits)
        M = w.shape[0]
        assert M == large                                                      # one partner each
        assert (d.matches, d.rc) == (M, 0), what
        assert rhj.lib.rhj_batch_takes(bits, len(R), len(S)) == 1 and d.path == BATCHED, (what, d.path)
        g.assert_untouched(-GUARD_ROWS, 0, what + ", in front of the buffer")
        g.assert_untouched(M, M + GUARD_ROWS, what + ", behind the capacity")
        got = g.body(0, M)
        if not rhj.torch.equal(got, w):
            i = int((got != w).any(dim=1).nonzero()[0].item())
            raise AssertionError("%s: pair %d is %r, expected %r" % (what, i, got[i].tolist(), w[i].tolist()))
    assert rhj.stats()["path"] == "batch"


@pytest.mark.parametrize("bits", sm.H_BITS)
def test_batched_joins(rhj, mod, oracle, bits):
    """one rhj_join_batch_device call: grid (BJ_MAX_TILES + 1, 2, joins), the histogram launch over the joins beyond two tiles only"""
    torch = rhj.torch
    joins = batch_inputs(bits)
    rhj.set_bits(bits)
    wants = [pairs_to_device(rhj, oracle.join(R, S, bits)) for R, S, _, _ in joins]
    dev = [(rhj.to_device(R), rhj.to_device(S)) for R, S, _, _ in joins]
    guards = [GuardedRows(torch, rhj.dev, w.shape[0]) for w in wants]
    arr = (mod.JoinDesc * len(joins))()
    for d, (dR, dS), g, w in zip(arr, dev, guards, wants):
        d.d_R, d.nR, d.d_S, d.nS = dR.data_ptr(), dR.shape[0], dS.data_ptr(), dS.shape[0]
        d.d_out, d.out_capacity = g.ptr, w.shape[0]
        d.matches, d.rc, d.path = 0xDEAD, -77, -77
    rc = rhj.lib.rhj_join_batch_device(arr, len(joins))
    check_batch(rhj, arr, rc, guards, wants, joins, bits)


@pytest.mark.parametrize("bits", sm.H_BITS)
def test_batched_joins_through_columns(rhj, mod, oracle, bits):
    """one rhj_join_cols_batch_device call on the same joins, every other one through row-id vectors"""
    torch = rhj.torch
    joins = batch_inputs(bits)
    rhj.set_bits(bits)
    wants = [pairs_to_device(rhj, oracle.join(R, S, bits)) for R, S, _, _ in joins]
    guards = [GuardedRows(torch, rhj.dev, w.shape[0]) for w in wants]
    arr = (mod.JoinColsDesc * len(joins))()
    keep = []
    for i, (d, (R, S, _, _), g, w) in enumerate(zip(arr, joins, guards, wants)):
        sides = cols_sides(R, S, sm.E_SELS[i % 2], 700 + i)
        dev = [[None if a is None else torch.from_numpy(a.view(np.int64)).to(rhj.dev) for a in side] for side in sides]
        keep.append(dev)
        d.d_colR, d.d_selR, d.nR = rhj._cols_side(*dev[0])
        d.d_colS, d.d_selS, d.nS = rhj._cols_side(*dev[1])
        assert (d.nR, d.nS) == (len(R), len(S))
        d.d_out, d.out_capacity = g.ptr, w.shape[0]
        d.matches, d.rc, d.path = 0xDEAD, -77, -77
    rc = rhj.lib.rhj_join_cols_batch_device(arr, len(joins))
    check_batch(rhj, arr, rc, guards, wants, joins, bits)


# ---- F. wide row ids (last in this module) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", sm.F_BITS)
@pytest.mark.parametrize("ntiles", sm.F_TILES)
def test_wide_row_ids_on_the_large_side(rhj, oracle, ntiles, bits):
    """the one pass keeps 16-byte tuples: row ids beyond 2^32 travel through the stage and the scatter whole"""
    n = sm.size_of(ntiles, False)
    ids = np.arange(n, dtype=np.uint64) | np.uint64(sm.WIDE)
    L, O = make_rel(sm.large_keys("tile_digit", bits, n), ids), make_rel(sm.small_keys(bits))
    for large_is_r in (True, False):
        assert run(rhj, oracle, bits, *((L, O) if large_is_r else (O, L)), "%d tiles on %d bits, large side is %s" % (ntiles, bits, "RS"[not large_is_r])) == n
