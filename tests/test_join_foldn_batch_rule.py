"""rhj_join_foldn_batch_device, rhj_query_foldn_plan and the query batch's fold-nodes switch (include/rhj_inter.h) as far as they
go without a device: the symbols, the layouts of the new structures against the ctypes mirrors, the empty batch, and the
validation that comes before any device is touched and writes no total, every invalid form in the middle of a batch."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rhj_join_foldn_batch_device", "rhj_query_foldn_plan", "rhj_set_query_fold_nodes", "rhj_set_query_fold_node_rows",
               "rhj_query_batch_last_fold_nodes_info")

LAYOUTS = {                                              # C type -> (ctypes mirror, fields)
    "rhj_join_foldn_desc": ("JoinFoldNDesc", ("nkeys", "d_colR", "d_selR", "nR", "d_colS", "d_selS", "nS", "nvalues", "nouts", "values", "outs", "rc", "path")),
    "rhj_foldn_plan": ("FoldNPlan", ("levels", "root", "nsteps", "nself", "node", "steps", "self")),
    "rhj_query_batch_fold_nodes_info": ("QueryBatchFoldNodesInfo", ("foldn_calls", "foldn_items", "node_queries", "node_levels")),
}
SENTINEL = 0xDEADBEEFDEADBEEF


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def lib(mod):
    return mod.load_library()


def test_symbols_are_exported(mod, lib):
    for name in NEW_SYMBOLS:
        assert name in mod.INTER_SYMBOLS and hasattr(lib, name), name


def test_layouts_equal_the_ctypes_mirrors(mod, tmp_path):
    """sizeof and every offsetof, as a C compiler sees include/rhj_inter.h, against the structures the Python binding fills"""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler to read include/rhj_inter.h with"
    body = ['    printf("%d %d %d", RHJ_FOLD_MAX_KEYS, RHJ_QUERY_MAX_RELS, RHJ_FOLD_SELF_MAX_TERMS);']
    for ctype, (_, fields) in LAYOUTS.items():
        body.append('    printf(" %%zu", sizeof(%s));' % ctype)
        body += ['    printf(" %%zu", offsetof(%s, %s));' % (ctype, f) for f in fields]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rhj_inter.h"\nint main(void)\n{\n%s\n    printf("\\n");\n    return 0;\n}\n' % "\n".join(body))
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    want = [mod.FOLD_MAX_KEYS, mod.QUERY_MAX_RELS, mod.FOLD_SELF_MAX_TERMS]
    assert want == [4, 8, 4]
    for _, (mirror, fields) in LAYOUTS.items():
        S = getattr(mod, mirror)
        assert [f for f, _ in S._fields_] == list(fields)
        want += [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert got == want


def test_the_statistics_name_path_16(mod):
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        assert "16 a batch of weighted join folds on tuple keys with a row-id vector per key word (rhj_join_foldn_batch_device" in f.read()
    st = mod.Stats()
    st.reserved = 16
    assert st.as_dict()["path"] == "join_foldn_batch"


def test_an_empty_batch_touches_no_device(lib):
    assert lib.rhj_join_foldn_batch_device(None, 0) == 0


def good_items(mod, n=3):
    """items whose pointers are never followed, every output word a sentinel; a word has no vector, the previous word's or its own"""
    arr = (mod.JoinFoldNDesc * n)()
    for k, d in enumerate(arr):
        d.nkeys = 1 + k % 4
        for t in range(d.nkeys):
            d.d_colR[t], d.d_colS[t] = 0x1000 + 0x100 * t, 0x3000 + 0x100 * t
            d.d_selR[t] = (None, 0x2000, 0x2000, 0x2800)[t]
            d.d_selS[t] = (0x9000, None, 0x9800, 0x9800)[t]
        d.nR, d.nS = 10, 20
        d.nvalues, d.nouts = 2, 3
        d.values[0].d_w = 0x4000
        d.values[1].d_w, d.values[1].d_src, d.values[1].d_col = None, 0x5000, 0x6000
        for o, value in zip(d.outs, (0, 1, 1)):
            o.value, o.p.d_w, o.d_out = value, 0x7000, 0x8000 + 0x1000 * value
        d.rc, d.path = -77, -77
        for o in d.outs:
            o.total = SENTINEL
    return arr


def spoil(d, name):
    """(the middle item of good_items has two keys)"""
    if name == "nkeys 0":
        d.nkeys = 0
    elif name == "nkeys -1":
        d.nkeys = -1
    elif name == "nkeys 5":
        d.nkeys = 5
    elif name == "no first column of R":
        d.d_colR[0] = None
    elif name == "no last column of R":
        d.d_colR[d.nkeys - 1] = None
    elif name == "no first column of S":
        d.d_colS[0] = None
    elif name == "no last column of S":
        d.d_colS[d.nkeys - 1] = None
    elif name == "four keys, the third column of S missing":
        d.nkeys = 4
        d.d_colR[2], d.d_colR[3], d.d_colS[3] = 0x1200, 0x1300, 0x3300
    elif name == "nvalues -1":
        d.nvalues, d.nouts = -1, 0
    elif name == "nvalues 10":
        d.nvalues = 10
    elif name == "nouts -1":
        d.nouts = -1
    elif name == "nouts 10":
        d.nouts = 10
    elif name == "a value index of nvalues":
        d.outs[2].value = 2
    elif name == "a value index of -1":
        d.outs[0].value = -1
    elif name == "an output without any value":
        d.nvalues, d.nouts = 0, 1
    elif name == "2^32 rows of R":
        d.nR = 1 << 32
    else:
        assert name == "2^32 rows of S"
        d.nS = 1 << 32


INVALID = ("nkeys 0", "nkeys -1", "nkeys 5", "no first column of R", "no last column of R", "no first column of S", "no last column of S",
           "four keys, the third column of S missing", "nvalues -1", "nvalues 10", "nouts -1", "nouts 10", "a value index of nvalues",
           "a value index of -1", "an output without any value", "2^32 rows of R", "2^32 rows of S")


@pytest.mark.parametrize("name", INVALID)
def test_an_invalid_item_is_refused_before_any_device(mod, lib, name):
    """rc -3 on that item, 0 on its neighbours, -3 returned, and no total written anywhere"""
    arr = good_items(mod)
    assert arr[1].nkeys == 2
    spoil(arr[1], name)
    assert lib.rhj_join_foldn_batch_device(arr, 3) == -3
    assert [d.rc for d in arr] == [0, -3, 0]
    assert all(o.total == SENTINEL for d in arr for o in d.outs)


def test_the_counts_at_their_limits_are_no_error(mod, lib):
    """(the validation alone: four keys, nine values and nine outputs, no value and no output, NULL columns of an empty side,
    NULL columns beyond nkeys and NULL vectors anywhere are valid, so their neighbour's fault is the only one)"""
    arr = good_items(mod, 5)
    arr[0].nvalues, arr[0].nouts = 9, 9
    for o in arr[0].outs:
        o.value = 8
    arr[1].nvalues, arr[1].nouts = 0, 0
    arr[2].nR = 0
    for t in range(4):
        arr[2].d_colR[t] = None
        arr[3].d_selR[t] = arr[3].d_selS[t] = None
    assert arr[3].nkeys == 4 and arr[0].nkeys == 1 and not arr[0].d_colR[1] and not arr[0].d_colS[3]
    spoil(arr[4], "nkeys 5")
    assert lib.rhj_join_foldn_batch_device(arr, 5) == -3
    assert [d.rc for d in arr] == [0, 0, 0, 0, -3]


def test_the_nodes_info_is_zero_before_any_query_batch(lib):
    info = lib.rhj_query_batch_last_fold_nodes_info().contents
    assert (info.foldn_calls, info.foldn_items, info.node_queries, info.node_levels) == (0, 0, 0, 0)
