"""rhj_batch_takes (include/rhj.h): which joins of an rhj_join_batch_device call go into the batched launches.  A pure
function of its arguments and the library's path settings: needs no device."""
import importlib

import pytest


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def lib(mod):
    return mod.load_library()


def test_batch_symbols_are_exported(mod, lib):
    for name in ("rhj_join_batch_device", "rhj_batch_takes"):
        assert name in mod.ABI_SYMBOLS and hasattr(lib, name), name


def test_batch_takes_follows_the_rule_at_its_edges(lib):
    takes = lib.rhj_batch_takes
    tile = 8192
    # widths: the one-pass partition's, 1..8 (PT_MAX_BITS)
    for bits in range(1, 9):
        assert takes(bits, 1000, 1000) == 1, bits
    for bits in (0, -1, 9, 12, 15, 16):
        assert takes(bits, 1000, 1000) == 0, bits
    # sizes: at most 8 tiles of 8192 tuples on either side
    top = 8 * tile
    assert top == 65536
    for bits in (1, 4, 8):
        assert takes(bits, top, top) == 1
        assert takes(bits, top + 1, top) == 0 and takes(bits, top, top + 1) == 0 and takes(bits, top + 1, top + 1) == 0
        assert takes(bits, 1, 1) == 1 and takes(bits, 1, top) == 1 and takes(bits, top, 1) == 1
        assert takes(bits, 1 << 20, 5) == 0 and takes(bits, 5, 1 << 32) == 0
        # an empty side launches nothing: not a join of the batched launches
        assert takes(bits, 0, 1000) == 0 and takes(bits, 1000, 0) == 0 and takes(bits, 0, 0) == 0
    # tile edges inside the class change nothing
    for n in (tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1):
        assert takes(4, n, 5) == 1 and takes(4, 5, n) == 1
    # whatever keeps a single join off the small path keeps it out of the batch
    for setter, off, on in ((lib.rhj_set_small, 0, 1), (lib.rhj_set_fused, 0, 1), (lib.rhj_set_force_hbm_table, 1, 0)):
        try:
            setter(off)
            assert takes(4, 1000, 1000) == 0, setter
        finally:
            setter(on)
        assert takes(4, 1000, 1000) == 1, setter
