"""rhj_join_sum_batch_device and the query batch's switch (include/rhj_inter.h) as far as they go without a device: the symbols, the
layouts of the new structures against the ctypes mirrors, the empty batch, and the validation that comes before any device is
touched and writes no output word."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rhj_join_sum_batch_device", "rhj_set_query_sum_last", "rhj_query_batch_last_sum_info")

LAYOUTS = {                                              # C type -> (ctypes mirror, fields)
    "rhj_join_sum_term": ("JoinSumTerm", ("d_src", "d_col", "sum", "side")),
    "rhj_join_sum_desc": ("JoinSumDesc", ("d_colR", "d_selR", "nR", "d_colS", "d_selS", "nS", "nterms", "terms", "matches", "rc", "path")),
    "rhj_query_batch_sum_info": ("QueryBatchSumInfo", ("sum_calls", "sum_items")),
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
    body = ['    printf("%d", RHJ_JOIN_SUM_MAX_TERMS);']
    for ctype, (_, fields) in LAYOUTS.items():
        body.append('    printf(" %%zu", sizeof(%s));' % ctype)
        body += ['    printf(" %%zu", offsetof(%s, %s));' % (ctype, f) for f in fields]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rhj_inter.h"\nint main(void)\n{\n%s\n    printf("\\n");\n    return 0;\n}\n' % "\n".join(body))
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    want = [mod.JOIN_SUM_MAX_TERMS]
    for _, (mirror, fields) in LAYOUTS.items():
        S = getattr(mod, mirror)
        assert [f for f, _ in S._fields_] == list(fields)
        want += [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert got == want


def test_an_empty_batch_touches_no_device(lib):
    assert lib.rhj_join_sum_batch_device(None, 0) == 0


def good_items(mod, n=3):
    """items whose pointers are never followed, every output word a sentinel"""
    arr = (mod.JoinSumDesc * n)()
    for d in arr:
        d.d_colR, d.d_selR, d.nR = 0x1000, 0x2000, 10
        d.d_colS, d.d_selS, d.nS = 0x3000, None, 20
        d.nterms = 2
        d.terms[0].d_src, d.terms[0].d_col, d.terms[0].side = None, 0x4000, 0
        d.terms[1].d_src, d.terms[1].d_col, d.terms[1].side = 0x5000, 0x6000, 1
        d.matches, d.rc, d.path = SENTINEL, -77, -77
        for t in d.terms:
            t.sum = SENTINEL
    return arr


def spoil(d, name):
    if name == "no column R":
        d.d_colR = None
    elif name == "no column S":
        d.d_colS = None
    elif name == "nterms -1":
        d.nterms = -1
    elif name == "nterms 9":
        d.nterms = 9
    elif name == "side 2":
        d.terms[1].side = 2
    elif name == "side -1":
        d.terms[0].side = -1
    elif name == "a term without a column":
        d.terms[1].d_col = None
    elif name == "2^32 rows of R":
        d.nR = 1 << 32
    else:
        assert name == "2^32 rows of S"
        d.nS = 1 << 32


INVALID = ("no column R", "no column S", "nterms -1", "nterms 9", "side 2", "side -1", "a term without a column", "2^32 rows of R", "2^32 rows of S")


@pytest.mark.parametrize("name", INVALID)
def test_an_invalid_item_is_refused_before_any_device(mod, lib, name):
    """rc -3 on that item, 0 on its neighbours, -3 returned, and no matches or sum written anywhere"""
    arr = good_items(mod)
    spoil(arr[1], name)
    assert lib.rhj_join_sum_batch_device(arr, 3) == -3
    assert [d.rc for d in arr] == [0, -3, 0]
    assert all(d.matches == SENTINEL and all(t.sum == SENTINEL for t in d.terms) for d in arr)


def test_a_null_column_of_an_empty_side_is_no_error(mod):
    """(the validation alone: the item is valid, so its neighbour's fault is the only one)"""
    lib = mod.load_library()
    arr = good_items(mod)
    arr[0].d_colR, arr[0].nR = None, 0
    spoil(arr[2], "side 2")
    assert lib.rhj_join_sum_batch_device(arr, 3) == -3
    assert [d.rc for d in arr] == [0, 0, -3]


def test_the_sum_info_is_zero_before_any_query_batch(lib):
    info = lib.rhj_query_batch_last_sum_info().contents
    assert (info.sum_calls, info.sum_items) == (0, 0)
