"""CPU: the numpy statement of the optimiser's column statistics (helpers.column_stats_model, which the GPU
tests hold rhj_column_stats_device to) against the reference's own InitRelationMap (relation_map.c:13-88,
compiled into oracle/_ref/libref_n4_t1.so), at the ranges where the flag array changes shape and wherever
the reference's code is defined: the full range (0, 2^64 - 1) is not, so it is pinned on the GPU side only."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from helpers import STATS_CAP, column_stats_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libref_n4_t1.so")


class ListNode(C.Structure):                     # structs.h relation_listnode
    pass


ListNode._fields_ = [("filename", C.c_char_p), ("fd", C.c_int), ("next", C.POINTER(ListNode))]


def stats_columns():
    """{name: column}: ranges u - l + 1 of 1, STATS_CAP - 1 (the largest unfolded flag array) and STATS_CAP (the
    smallest folded one), around 2^63, with the extremes on the first and the last row"""
    rng = np.random.default_rng(41)
    n = 100_003
    top = (1 << 63) - 20_000_000
    out = {"range 1": np.full(n, top, dtype=np.uint64)}
    for rng_size in (STATS_CAP - 1, STATS_CAP):
        lo = top
        col = rng.integers(lo, lo + rng_size, n, dtype=np.uint64)
        col[0], col[-1] = lo, lo + rng_size - 1                   # min on the first row, max on the last
        out["range %d" % rng_size] = col
        col = col[::-1].copy()                                     # max first, min last
        out["range %d reversed" % rng_size] = col
    out["wide, across 2^63"] = rng.integers((1 << 63) - (1 << 40), (1 << 63) + (1 << 40), n, dtype=np.uint64)
    out["one row"] = np.array([(1 << 63) + 5], dtype=np.uint64)
    return out


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/libref_n4_t1.so not built (needs the reference at build time)")
def test_column_stats_model_matches_the_reference(tmp_path):
    mod = importlib.import_module("sigmod-2018_amd")
    ref = C.CDLL(REF)
    cols = stats_columns()
    files, want = [], []
    for k, (name, col) in enumerate(cols.items()):
        path = tmp_path / ("r%d" % k)
        with open(path, "wb") as f:
            np.array([len(col), 1], dtype="<u8").tofile(f)        # rows, columns, then the column
            col.astype("<u8").tofile(f)
        files.append(str(path).encode())
        want.append((name, column_stats_model(col)))
    nodes = (ListNode * len(files))()
    for k, fn in enumerate(files):
        nodes[k].filename = fn
        nodes[k].fd = -1
        nodes[k].next = C.pointer(nodes[k + 1]) if k + 1 < len(files) else None
    rm = (mod.RelationMap * len(files))()
    ref.InitRelationMap.argtypes = [C.POINTER(ListNode), C.POINTER(mod.RelationMap)]
    ref.InitRelationMap.restype = None              # relation_map.c:13 falls off its end
    ref.InitRelationMap(nodes, rm)
    for k, (name, (lo, hi, d)) in enumerate(want):
        st = rm[k].col_stats[0]
        assert rm[k].num_tuples == len(cols[name]), name
        assert (st.l, st.u, st.d) == (lo, hi, d), name
        assert st.f == float(len(cols[name])), name
