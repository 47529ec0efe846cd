"""rhj_fold_pred_batch_device (include/rhj_inter.h) as far as it goes without a device: the symbols, the layouts of the new
structures against the ctypes mirrors, the empty batch, and the validation that comes before any device is touched and writes no
total, every invalid form in the middle of a batch."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rhj_fold_pred_batch_device", "rhj_query_one_wait_plan", "rhj_set_query_fold_one_wait", "rhj_set_query_fold_one_wait_rows",
               "rhj_query_batch_last_one_wait_info")

LAYOUTS = {                                              # C type -> (ctypes mirror, fields)
    "rhj_fold_const_term": ("FoldConstTerm", ("d_col", "d_sel", "op", "value")),
    "rhj_fold_pred_desc": ("FoldPredDesc", ("n", "nconst", "neq", "nouts", "consts", "eqs", "outs", "rc", "path")),
    "rhj_query_batch_one_wait_info": ("QueryBatchOneWaitInfo", ("queries", "programs", "pred_items", "fold_items", "foldk_items", "rounds", "launches",
                                                                "memsets", "waits")),
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
    body = ['    printf("%d %d %d", RHJ_FILTER_MAX_TERMS, RHJ_FOLD_SELF_MAX_TERMS, RHJ_FOLD_MAX_OUTS);']
    for ctype, (_, fields) in LAYOUTS.items():
        body.append('    printf(" %%zu", sizeof(%s));' % ctype)
        body += ['    printf(" %%zu", offsetof(%s, %s));' % (ctype, f) for f in fields]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rhj_inter.h"\nint main(void)\n{\n%s\n    printf("\\n");\n    return 0;\n}\n' % "\n".join(body))
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    want = [mod.FILTER_MAX_TERMS, mod.FOLD_SELF_MAX_TERMS, mod.FOLD_MAX_OUTS]
    assert want == [4, 4, 9]
    for _, (mirror, fields) in LAYOUTS.items():
        S = getattr(mod, mirror)
        assert [f for f, _ in S._fields_] == list(fields)
        want += [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert got == want


def test_the_statistics_name_path_17(mod):
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        assert "17 a batch of folds with no child and constant predicates (rhj_fold_pred_batch_device" in f.read()
    st = mod.Stats()
    st.reserved = 17
    assert st.as_dict()["path"] == "fold_pred_batch"


def test_an_empty_batch_touches_no_device(lib):
    assert lib.rhj_fold_pred_batch_device(None, 0) == 0


def good_items(mod, n=3):
    """items whose pointers are never followed, every output word a sentinel"""
    arr = (mod.FoldPredDesc * n)()
    for k, d in enumerate(arr):
        d.n, d.nconst, d.neq, d.nouts = 10 + k, 1 + k % 4, 1 + k % 4, 3
        for t in range(d.nconst):
            d.consts[t].d_col, d.consts[t].d_sel, d.consts[t].op, d.consts[t].value = 0x1000 + 0x100 * t, (0x2000 if t % 2 else None), b"<>="[t % 3:t % 3 + 1], 7 + t
        for t in range(d.neq):
            d.eqs[t].d_colA, d.eqs[t].d_selA = 0x1000 + 0x100 * t, 0x2000
            d.eqs[t].d_colB, d.eqs[t].d_selB = 0x3000 + 0x100 * t, None
        d.outs[0].d_out = 0x8000
        d.outs[1].p.d_w, d.outs[1].d_out = 0x7000, 0x9000
        d.outs[2].p.d_src, d.outs[2].p.d_col = 0x5000, 0x6000
        d.rc, d.path = -77, -77
        for o in d.outs:
            o.total = SENTINEL
    return arr


def spoil(d, name):
    """(the middle item of good_items has two constant terms and two equalities)"""
    if name.startswith("op "):
        d.consts[1].op = {"op !": b"!", "op NUL": b"\0", "op g": b"g", "op l": b"l", "op space": b" "}[name]
    elif name == "nconst -1":
        d.nconst = -1
    elif name == "nconst 5":
        d.nconst = 5
    elif name == "neq -1":
        d.neq = -1
    elif name == "neq 5":
        d.neq = 5
    elif name == "nouts -1":
        d.nouts = -1
    elif name == "nouts 10":
        d.nouts = 10
    elif name == "no column in the first constant term":
        d.consts[0].d_col = None
    elif name == "no column in the last constant term":
        d.consts[d.nconst - 1].d_col = None
    elif name == "no column A in the first equality":
        d.eqs[0].d_colA = None
    elif name == "no column B in the last equality":
        d.eqs[d.neq - 1].d_colB = None
    elif name == "2^32 rows":
        d.n = 1 << 32
    else:
        assert name == "2^63 rows"
        d.n = 1 << 63


INVALID = ("op !", "op NUL", "op g", "op l", "op space", "nconst -1", "nconst 5", "neq -1", "neq 5", "nouts -1", "nouts 10",
           "no column in the first constant term", "no column in the last constant term", "no column A in the first equality",
           "no column B in the last equality", "2^32 rows", "2^63 rows")


@pytest.mark.parametrize("name", INVALID)
def test_an_invalid_item_is_refused_before_any_device(mod, lib, name):
    """rc -3 on that item, 0 on its neighbours, -3 returned, and no total written anywhere"""
    arr = good_items(mod)
    assert arr[1].nconst == 2 and arr[1].neq == 2
    spoil(arr[1], name)
    assert lib.rhj_fold_pred_batch_device(arr, 3) == -3
    assert [d.rc for d in arr] == [0, -3, 0]
    assert all(o.total == SENTINEL for d in arr for o in d.outs)


def test_the_counts_at_their_limits_are_no_error(mod, lib):
    """(the validation alone: four terms of either kind and nine outputs, no term and no output, NULL columns of an item without
    rows, NULL columns and any operator beyond the counts are valid, so their neighbour's fault is the only one)"""
    arr = good_items(mod, 5)
    arr[0].nouts = 9
    arr[0].consts[1].op = b"!"                           # beyond nconst: not read
    arr[1].nconst, arr[1].neq, arr[1].nouts = 0, 0, 0
    arr[2].n = 0
    for t in range(4):
        arr[2].consts[t].d_col = arr[2].eqs[t].d_colA = arr[2].eqs[t].d_colB = None
    assert arr[3].nconst == 4 and arr[3].neq == 4 and arr[0].nconst == 1
    arr[3].n = (1 << 32) - 1
    spoil(arr[4], "nconst 5")
    assert lib.rhj_fold_pred_batch_device(arr, 5) == -3
    assert [d.rc for d in arr] == [0, 0, 0, 0, -3]


def test_the_one_wait_info_is_zero_before_any_query_batch(lib):
    info = lib.rhj_query_batch_last_one_wait_info().contents
    assert all(getattr(info, f) == 0 for f, _ in type(info)._fields_)
