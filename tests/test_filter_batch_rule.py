"""rhj_filter_batch_device / rhj_filter_batch_takes (include/rhj.h) as far as they go without a device: the symbols, the rule
that names the filters of the batched launches, and the layout of rhj_filter_desc against its ctypes mirror."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FILTER_TILE = 4096                                # rhj_filter.hip.h: one mask workgroup's elements
FILTER_SELF_TILES = 1024                          # rhj_filter.hip.h: most tiles of the write pass that sums its tile counts itself


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def lib(mod):
    return mod.load_library()


def test_filter_batch_symbols_are_exported(mod, lib):
    for name in ("rhj_filter_batch_device", "rhj_filter_batch_takes"):
        assert name in mod.ABI_SYMBOLS and hasattr(lib, name), name


def test_filter_batch_takes_follows_the_rule_at_its_edges(lib):
    takes = lib.rhj_filter_batch_takes
    top = FILTER_SELF_TILES * FILTER_TILE
    assert top == 4_194_304
    assert takes(0) == 0
    assert takes(1) == 1
    assert takes(top) == 1
    assert takes(top + 1) == 0
    for n in (63, 64, FILTER_TILE - 1, FILTER_TILE, FILTER_TILE + 1, top - 1):
        assert takes(n) == 1, n
    for n in (2 * top, 1 << 32, (1 << 64) - 1):
        assert takes(n) == 0, n


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "rhj.h"
int main(void)
{
    printf("%d\n", RHJ_FILTER_MAX_TERMS);
    printf("%zu %zu %zu %zu\n", sizeof(rhj_filter_term), offsetof(rhj_filter_term, d_col), offsetof(rhj_filter_term, value),
           offsetof(rhj_filter_term, op));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rhj_filter_desc), offsetof(rhj_filter_desc, d_sel), offsetof(rhj_filter_desc, n),
           offsetof(rhj_filter_desc, nterms), offsetof(rhj_filter_desc, terms), offsetof(rhj_filter_desc, d_out),
           offsetof(rhj_filter_desc, hits), offsetof(rhj_filter_desc, rc), offsetof(rhj_filter_desc, path));
    return 0;
}
"""


def test_filter_desc_layout_equals_the_ctypes_mirror(mod, tmp_path):
    """sizeof and every offsetof of rhj_filter_term / rhj_filter_desc, as a C compiler sees include/rhj.h, against the
    structures the Python binding fills"""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler to read include/rhj.h with"
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split("\n")
    T, D = mod.FilterTerm, mod.FilterDesc
    assert int(lines[0]) == mod.FILTER_MAX_TERMS == 4
    assert [int(x) for x in lines[1].split()] == [C.sizeof(T), T.d_col.offset, T.value.offset, T.op.offset]
    assert [int(x) for x in lines[2].split()] == [C.sizeof(D), D.d_sel.offset, D.n.offset, D.nterms.offset, D.terms.offset,
                                                  D.d_out.offset, D.hits.offset, D.rc.offset, D.path.offset]
