"""rhj_apply_batch_device (include/rhj_inter.h) as far as it goes without a device: the symbol, the layouts of rhj_apply_term
and rhj_apply_desc against their ctypes mirrors, and the empty batch."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TERM_FIELDS = ("d_src", "d_dst", "d_col", "sum", "side")
DESC_FIELDS = ("d_idx", "n", "idx_stride", "nterms", "terms", "rc", "path")


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def lib(mod):
    return mod.load_library()


def test_apply_symbol_is_exported(mod, lib):
    """The declaration sits in include/rhj_inter.h, so the name belongs to that header's list (tests/test_host_abi.py holds
    each list equal to its header); build() checks both lists against the library."""
    name = "rhj_apply_batch_device"
    assert name in mod.ABI_SYMBOLS + mod.INTER_SYMBOLS and name in mod.INTER_SYMBOLS
    assert hasattr(lib, name)


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "rhj_inter.h"
int main(void)
{
    printf("%%d", RHJ_APPLY_MAX_TERMS);
    printf(" %%zu", sizeof(rhj_apply_term));
%s
    printf(" %%zu", sizeof(rhj_apply_desc));
%s
    printf("\n");
    return 0;
}
""" % ("\n".join('    printf(" %%zu", offsetof(rhj_apply_term, %s));' % f for f in TERM_FIELDS),
       "\n".join('    printf(" %%zu", offsetof(rhj_apply_desc, %s));' % f for f in DESC_FIELDS))


def test_apply_layouts_equal_the_ctypes_mirrors(mod, tmp_path):
    """sizeof and every offsetof of rhj_apply_term and rhj_apply_desc, as a C compiler sees include/rhj_inter.h, against the
    structures the Python binding fills"""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler to read include/rhj_inter.h with"
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    T, D = mod.ApplyTerm, mod.ApplyDesc
    assert [f for f, _ in T._fields_] == list(TERM_FIELDS) and [f for f, _ in D._fields_] == list(DESC_FIELDS)
    want = [mod.APPLY_MAX_TERMS, C.sizeof(T)] + [getattr(T, f).offset for f in TERM_FIELDS]
    want += [C.sizeof(D)] + [getattr(D, f).offset for f in DESC_FIELDS]
    assert got == want
    assert D.terms.size == mod.APPLY_MAX_TERMS * C.sizeof(T)


def test_empty_apply_batch_touches_no_device(lib):
    assert lib.rhj_apply_batch_device(None, 0) == 0


INVALID = {
    "stride 0": lambda d: setattr(d, "idx_stride", 0),
    "stride 3": lambda d: setattr(d, "idx_stride", 3),
    "no terms": lambda d: setattr(d, "nterms", 0),
    "nine terms": lambda d: setattr(d, "nterms", 9),
    "side -1": lambda d: setattr(d.terms[1], "side", -1),
    "side 2 of stride 2": lambda d: setattr(d.terms[2], "side", 2),
    "side 1 of stride 1": lambda d: setattr(d, "idx_stride", 1),
    "side 1 without a list": lambda d: setattr(d, "d_idx", None),
    "a term with neither": lambda d: setattr(d.terms[3], "d_dst", None),
    "2^35 + 1 rows": lambda d: setattr(d, "n", (1 << 35) + 1),
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_validation_comes_before_any_device(mod, lib, name):
    """The whole batch is validated before anything is launched, so an invalid item is refused without a device: rc -3 on that
    item, 0 on its neighbours, -3 returned.  (The pointers are never followed.)"""
    arr = (mod.ApplyDesc * 3)()
    for d in arr:
        d.d_idx, d.n, d.idx_stride, d.nterms, d.rc, d.path = 0x1000, 10, 2, 4, -77, -77
        for k, t in enumerate(d.terms):
            t.d_dst, t.side, t.sum = 0x2000, k % 2, 0xDEAD
    INVALID[name](arr[1])
    assert lib.rhj_apply_batch_device(arr, 3) == -3
    assert [d.rc for d in arr] == [0, -3, 0] and [d.path for d in arr] == [0, 0, 0]
