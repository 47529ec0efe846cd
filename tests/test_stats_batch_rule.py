"""rhj_column_stats_batch_device (include/rhj_inter.h) as far as it goes without a device: the symbols, the layouts of its
structures against the ctypes mirrors, rhj_column_stats_flags against the rule of helpers.column_stats_model, the empty batch,
and the validation that comes before any device is touched."""
import ctypes as C
import importlib
import os
import shutil
import struct
import subprocess

import pytest

from helpers import STATS_CAP, STATS_FOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rhj_column_stats_batch_device", "rhj_column_stats_flags", "rhj_column_stats_batch_last_info")
LAYOUTS = {                                              # C type -> (ctypes mirror, fields)
    "rhj_colstats_desc": ("ColStatsDesc", ("d_col", "n", "l", "u", "d", "rc", "path")),
    "rhj_colstats_batch_info": ("ColStatsBatchInfo", ("chunks", "columns")),
}
MAX_ROWS = 1 << 35
L_PAT, U_PAT, D_PAT = 0xDEADBEEFDEADBEEF, 0xFEEDFACEFEEDFACE, struct.unpack("<d", struct.pack("<Q", 0x4242424242424242))[0]


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
    body = []
    for ctype, (_, fields) in LAYOUTS.items():
        body.append('    printf(" %%zu", sizeof(%s));' % ctype)
        body += ['    printf(" %%zu", offsetof(%s, %s));' % (ctype, f) for f in fields]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rhj_inter.h"\nint main(void)\n{\n%s\n    printf("\\n");\n    return 0;\n}\n' % "\n".join(body))
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    want = []
    for _, (mirror, fields) in LAYOUTS.items():
        S = getattr(mod, mirror)
        assert [f for f, _ in S._fields_] == list(fields)
        want += [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert got == want


def model_flags(l, u):
    """the flags helpers.column_stats_model counts over: the range in Python ints, which never wraps"""
    if l > u:
        return 0
    return u - l + 1 if u - l + 1 < STATS_CAP else STATS_FOLD


EXTREMES = (
    [(l, l + r - 1) for r in (1, 2, STATS_CAP - 1, STATS_CAP, STATS_CAP + 1) for l in (0, 7, (1 << 63) - 1, (1 << 64) - r)]
    + [((1 << 63) - 3, (1 << 63) + 3), ((1 << 63) - 1, 1 << 63), ((1 << 63) - STATS_CAP // 2, (1 << 63) + STATS_CAP // 2 - 2),
       ((1 << 63) - STATS_CAP // 2, (1 << 63) + STATS_CAP // 2 - 1), (0, (1 << 64) - 1), (1, (1 << 64) - 1), (0, (1 << 64) - 2),
       (1, 0), ((1 << 64) - 1, 0), ((1 << 63) + 1, (1 << 63) - 1), (STATS_CAP, 0)]
)


@pytest.mark.parametrize("l,u", EXTREMES)
def test_flags_follow_the_models_rule(lib, l, u):
    assert lib.rhj_column_stats_flags(l, u) == model_flags(l, u)


def patterned(mod, count):
    arr = (mod.ColStatsDesc * count)()
    for d in arr:
        d.d_col, d.n, d.l, d.u, d.d, d.rc, d.path = 0x10000, 10, L_PAT, U_PAT, D_PAT, -77, -77
    return arr


def untouched(arr):
    return all(d.l == L_PAT and d.u == U_PAT and struct.pack("<d", d.d) == struct.pack("<d", D_PAT) for d in arr)


@pytest.mark.parametrize("name", ("no column", "too many rows"))
def test_an_invalid_column_is_refused_before_any_device(mod, lib, name):
    """rc -3 on that item, 0 on its neighbours (one of them empty), -3 returned, and no l, u or d written anywhere"""
    arr = patterned(mod, 4)
    arr[0].d_col, arr[0].n = None, 0
    if name == "no column":
        arr[2].d_col = None
    else:
        arr[2].n = MAX_ROWS + 1
    assert lib.rhj_column_stats_batch_device(arr, 4) == -3
    assert [d.rc for d in arr] == [0, 0, -3, 0] and [d.path for d in arr] == [0, 0, 0, 0]
    assert untouched(arr)


def test_the_largest_column_passes_the_validation(mod, lib):
    """n = 2^35 with a column is valid: in a batch whose other items are all invalid (so that nothing launches) it alone keeps rc 0"""
    arr = patterned(mod, 3)
    arr[0].d_col = None
    arr[1].n = MAX_ROWS
    arr[2].n = MAX_ROWS + 1
    assert lib.rhj_column_stats_batch_device(arr, 3) == -3
    assert [d.rc for d in arr] == [-3, 0, -3]
    assert untouched(arr)


def test_an_empty_batch_touches_no_device(lib):
    assert lib.rhj_column_stats_batch_device(None, 0) == 0
    info = lib.rhj_column_stats_batch_last_info().contents
    assert (info.chunks, info.columns) == (0, 0)
