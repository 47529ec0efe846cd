"""rhj_set_fold_resident_keys and its companions (include/rhj_inter.h) as far as they go without a device: the symbols, the layout
of the info structure against its ctypes mirror, the switch and its environment variable, rhj_fold_resident_keys_rule against the
model of tests/fold_resident_keys_model.py, path 19 in include/rhj.h, and the empty batch."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fold_resident_keys_model as km2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rhj_set_fold_resident_keys", "rhj_get_fold_resident_keys", "rhj_fold_resident_keys_rule", "rhj_table_batch_last_resident_keys_info")
FIELDS = ("resident_items", "resident_launches", "table_items")
ENV = "RHJ_FOLD_RESIDENT_KEYS"


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def lib(mod):
    return mod.load_library()


def test_symbols_are_exported(mod, lib):
    for name in NEW_SYMBOLS:
        assert name in mod.INTER_SYMBOLS and hasattr(lib, name), name


def test_the_info_layout_equals_its_ctypes_mirror(mod, lib, tmp_path):
    """sizeof and every offsetof of what rhj_table_batch_last_resident_keys_info returns, as a C compiler sees include/rhj_inter.h
    (sizeof's operand is not evaluated, so the program needs no library), against the structure the Python binding reads"""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler to read include/rhj_inter.h with"
    body = ['    printf("%zu", sizeof(*rhj_table_batch_last_resident_keys_info()));']
    body += ['    printf(" %%zu", offsetof(rhj_table_batch_resident_info, %s));' % f for f in FIELDS]
    body += ['    printf(" %d", _Generic(rhj_table_batch_last_resident_keys_info(), const rhj_table_batch_resident_info *: 1, default: 0));']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rhj_inter.h"\nint main(void)\n{\n%s\n    printf("\\n");\n    return 0;\n}\n' % "\n".join(body))
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    S = mod.TableBatchResidentInfo
    assert [f for f, _ in S._fields_] == list(FIELDS)
    assert lib.rhj_table_batch_last_resident_keys_info.restype is C.POINTER(S)
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [1] == [12, 0, 4, 8, 1]


def test_the_switch_is_off_by_default_and_follows_the_setter(lib):
    if ENV not in os.environ:
        assert lib.rhj_get_fold_resident_keys() == 0
    was, old = lib.rhj_get_fold_resident_keys(), lib.rhj_get_fold_resident()
    try:
        lib.rhj_set_fold_resident_keys(1)
        assert lib.rhj_get_fold_resident_keys() == 1
        lib.rhj_set_fold_resident_keys(7)                # clamped to 0 or 1
        assert lib.rhj_get_fold_resident_keys() == 1
        lib.rhj_set_fold_resident_keys(-3)
        assert lib.rhj_get_fold_resident_keys() == 1
        assert lib.rhj_get_fold_resident() == old        # the two switches are independent, either way
        lib.rhj_set_fold_resident(1 - old)
        assert lib.rhj_get_fold_resident_keys() == 1
        lib.rhj_set_fold_resident_keys(0)
        assert lib.rhj_get_fold_resident_keys() == 0 and lib.rhj_get_fold_resident() == 1 - old
    finally:
        lib.rhj_set_fold_resident_keys(was)
        lib.rhj_set_fold_resident(old)


@pytest.mark.parametrize("value, want", ((None, 0), ("0", 0), ("1", 1), ("5", 1)))
def test_the_environment_sets_the_default_in_a_fresh_process(value, want):
    env = {k: v for k, v in os.environ.items() if k not in (ENV, "RHJ_FOLD_RESIDENT")}
    if value is not None:
        env[ENV] = value
    code = ("import importlib, sys; sys.path.insert(0, %r); L = importlib.import_module('sigmod-2018_amd').load_library(); "
            "print(L.rhj_get_fold_resident_keys(), L.rhj_get_fold_resident())" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], check=True, stdout=subprocess.PIPE, env=env).stdout.decode().split()
    assert out[-2:] == [str(want), "0"]                  # the variable of the one-key switch is another


def test_the_rule_equals_the_model(lib):
    rng = np.random.default_rng(19)
    cases = list(km2.edges())
    caps = [km2.build_cap(v) for v in range(km2.MAX_VALUES + 1)]
    for _ in range(4000):
        v = int(rng.integers(0, km2.MAX_VALUES + 1))
        pick = lambda: int(rng.choice([rng.integers(0, 20), caps[v] + rng.integers(-3, 4), km2.MAX_ROWS + rng.integers(-3, 4), rng.integers(0, 4 * km2.MAX_ROWS),
                                       rng.integers(0, 2 * caps[v] + 2), (1 << 32) - 1 - rng.integers(0, 3)]))
        cases.append((max(pick(), 0), max(pick(), 0), v))
    cases += [(1 << 40, 5, 1), (5, 1 << 40, 1), ((1 << 64) - 1, (1 << 64) - 1, 0), (5, 5, -1), (5, 5, km2.MAX_VALUES + 1)]
    wrong = [(nR, nS, v) for nR, nS, v in cases if lib.rhj_fold_resident_keys_rule(nR, nS, v) != int(km2.resident(nR, nS, v))]
    assert wrong == []
    assert sum(km2.resident(*c) for c in cases) > 500 and sum(not km2.resident(*c) for c in cases) > 500


def test_the_rule_does_not_depend_on_either_switch(lib):
    was, old = lib.rhj_get_fold_resident_keys(), lib.rhj_get_fold_resident()
    try:
        for new in (0, 1):
            for one_key in (0, 1):
                lib.rhj_set_fold_resident_keys(new)
                lib.rhj_set_fold_resident(one_key)
                assert lib.rhj_fold_resident_keys_rule(1, 1, 1) == 1 and lib.rhj_fold_resident_keys_rule(5000, 5000, 1) == 0
                assert [lib.rhj_fold_resident_keys_rule(*c) for c in km2.edges()] == [int(km2.resident(*c)) for c in km2.edges()]
    finally:
        lib.rhj_set_fold_resident_keys(was)
        lib.rhj_set_fold_resident(old)


def test_the_statistics_name_path_19():
    with open(os.path.join(ROOT, "include", "rhj.h")) as f:
        text = f.read()
    assert "19 an item of a batch of weighted join folds on tuple keys that one workgroup folded in LDS" in text
    assert "18 an item of a batch of weighted join folds that one workgroup folded in LDS" in text
    with open(os.path.join(ROOT, "sigmod-2018_amd", "csrc", "rhj_device.hip")) as f:
        assert "PATH_BATCH_JOIN_FOLDK_LDS = %d" % km2.PATH_RESIDENT in f.read()


def test_an_empty_batch_touches_no_device(lib):
    was = lib.rhj_get_fold_resident_keys()
    try:
        lib.rhj_set_fold_resident_keys(1)
        for entry in (lib.rhj_join_foldk_batch_device, lib.rhj_join_foldn_batch_device):
            assert entry(None, 0) == 0
            info = lib.rhj_table_batch_last_resident_keys_info().contents
            assert (info.resident_items, info.resident_launches, info.table_items) == (0, 0, 0)
    finally:
        lib.rhj_set_fold_resident_keys(was)
