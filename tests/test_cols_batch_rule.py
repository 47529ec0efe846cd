"""rhj_join_cols_batch_device / rhj_join_cols_device (include/rhj.h) as far as they go without a device: the symbols, the layout
of rhj_join_cols_desc against its ctypes mirror, and the empty batch."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("d_colR", "d_selR", "nR", "d_colS", "d_selS", "nS", "d_out", "out_capacity", "matches", "rc", "path")


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def lib(mod):
    return mod.load_library()


def test_cols_symbols_are_exported(mod, lib):
    for name in ("rhj_join_cols_batch_device", "rhj_join_cols_device"):
        assert name in mod.ABI_SYMBOLS and hasattr(lib, name), name


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "rhj.h"
int main(void)
{
    printf("%%zu", sizeof(rhj_join_cols_desc));
%s
    printf("\n");
    return 0;
}
""" % "\n".join('    printf(" %%zu", offsetof(rhj_join_cols_desc, %s));' % f for f in FIELDS)


def test_join_cols_desc_layout_equals_the_ctypes_mirror(mod, tmp_path):
    """sizeof and every offsetof of rhj_join_cols_desc, as a C compiler sees include/rhj.h, against the structure the Python
    binding fills"""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler to read include/rhj.h with"
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    D = mod.JoinColsDesc
    assert [f for f, _ in D._fields_] == list(FIELDS)
    assert got == [C.sizeof(D)] + [getattr(D, f).offset for f in FIELDS]


def test_empty_cols_batch_touches_no_device(lib):
    assert lib.rhj_join_cols_batch_device(None, 0) == 0
