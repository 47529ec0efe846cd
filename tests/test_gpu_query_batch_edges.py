"""rhj_query_batch_device (include/rhj_inter.h) where its driver (csrc/rhj_device.hip: query_filters, query_level_joins,
query_rerun_short, query_level_apply, query_take_back) hands over between the inner batches: the families of
tests/query_shapes.py, each in ONE call.  Every query's (sums, rows) equals the numpy executor's as integers, the call's
rhj_query_batch_last_info() equals call_counts of tests/query_model.py field for field, and rhj_last_stats() names the path, the
queries and the summed rows.  tests/test_query_shapes.py holds every family to its regime without a device."""
import importlib

import numpy as np
import pytest

import query_shapes as qs
from helpers import make_rel
from pyoracle import PAIR
from query_model import INFO_FIELDS, join_takes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def rhj(mod):
    r = mod.RHJ(device=0)
    r.lib.rhj_set_timing(2)
    r.lib.rhj_set_small(1)
    r.lib.rhj_set_order(0)
    r.set_bits(4)
    yield r
    r.lib.rhj_release()                                   # (families b and c grew the workspace by some hundred megabytes)
    r.lib.rhj_set_timing(2)
    r.lib.rhj_set_small(1)
    r.lib.rhj_set_order(0)
    r.set_bits(4)


def dev(rhj, a):
    return rhj.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


def to_device(rhj, rels, prefix=None):
    """cols[r][c] of relations[r][c]; prefix {r: (source, rows)}: relation r is the first rows of the source's tensors"""
    cols = []
    for r, rel in enumerate(rels):
        if prefix and r in prefix:
            src, n = prefix[r]
            assert all(np.shares_memory(a, b) and len(a) == n for a, b in zip(rel, rels[src]))
            cols.append([t[:n] for t in cols[src]])
        else:
            cols.append([dev(rhj, c) for c in rel])
    return cols


def last_info(rhj):
    return rhj.lib.rhj_query_batch_last_info().contents.as_dict()


def run(rhj, cols, queries, want, info, what):
    """one call; the answers, the call counts and the call's statistics against the model"""
    res, got = rhj.query_batch_device(cols, queries, with_info=True)
    st = rhj.stats()
    assert len(res) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(res, want)) if (list(g[0]), g[1]) != (list(w[0]), w[1])]
    assert not bad, "%s: query %d of %d wrong queries gives %r, the executor %r" % (what, bad[0], len(bad), res[bad[0]], want[bad[0]])
    assert got == info, what
    assert set(got) == set(INFO_FIELDS)
    assert st["path"] == "query_batch" and st["n_r"] == len(queries) and st["matches"] == sum(rows for _, rows in want), what
    return res


def run_family(rhj, name, prefix=None):
    rels, queries, want, info, _ = qs.reference(name)
    cols = to_device(rhj, rels, prefix)
    return cols, run(rhj, cols, queries, want, info, name)


def alone(rhj, cols, name, which):
    """a query alone gives what it gives in the batch"""
    _, queries, want, _, _ = qs.reference(name)
    for i in which:
        (sums, rows), = rhj.query_batch_device(cols, [queries[i]])
        assert (sums, rows) == (want[i][0], want[i][1]), "%s: query %d alone" % (name, i)


# ---- a: joins that run alone ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synthetic(rhj):
    """the 24 synthetic queries on the device, and their answers at 4 bits"""
    rels, queries, _, _, _ = qs.reference("synthetic")
    cols = to_device(rhj, rels)
    rhj.set_bits(4)
    return cols, rhj.query_batch_device(cols, queries, with_info=True)


SETTINGS = {"9 bits": dict(bits=9), "11 bits": dict(bits=11), "14 bits": dict(bits=14), "8 bits": dict(bits=8), "small off": dict(bits=4, small=False),
            "any": dict(order_any=True)}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_a1_the_synthetic_queries_at_other_settings(rhj, synthetic, setting):
    cols, (at4, info4) = synthetic
    s = SETTINGS[setting]
    takes = join_takes(**s)
    rels, queries, want, info, detail = qs.reference("synthetic", takes)
    try:
        rhj.set_bits(s.get("bits", 4))
        rhj.lib.rhj_set_small(1 if s.get("small", True) else 0)
        rhj.lib.rhj_set_order(1 if s.get("order_any") else 0)
        for lv in detail["levels"]:                       # the model's rule is the library's at these settings
            for _, nR, nS, _ in lv["joins"]:
                bits = rhj.lib.rhj_auto_radix_bits(nR, nS) if s.get("order_any") else s["bits"]
                assert bool(rhj.lib.rhj_batch_takes(bits, nR, nS)) == takes(nR, nS), (nR, nS)
        res = run(rhj, cols, queries, want, info, setting)
    finally:
        rhj.set_bits(4)
        rhj.lib.rhj_set_small(1)
        rhj.lib.rhj_set_order(0)
    assert res == at4 and info == info4                   # the counts are of calls, not of launches


def test_a2_a_relation_too_large_for_the_batched_joins(rhj):
    run_family(rhj, "join too large")


# ---- b: filters and equalities that run alone ------------------------------------------------------------------------------------------

def test_b1_a_filter_over_the_limit(rhj):
    run_family(rhj, "filter too large", qs.B1_PREFIX)


def test_b2_an_equality_over_the_limit(rhj):
    run_family(rhj, "equality too large")


# ---- c: chunk cuts -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("chunk cuts", "chunk cuts, one short join"))
def test_c_every_inner_batch_is_cut(rhj, name):
    cols, _ = run_family(rhj, name)
    alone(rhj, cols, name, (0, 4095, 4096, 4099) + ((qs.C_SHORT_AT,) if name != "chunk cuts" else ()))


@pytest.mark.parametrize("n", (4096, 4097))
def test_c_the_neighbours_of_the_filter_cut(rhj, n):
    name = "%d filters" % n
    cols, _ = run_family(rhj, name)
    alone(rhj, cols, name, (0, 4095, n - 1))


# ---- d: the rerun's bookkeeping ---------------------------------------------------------------------------------------------------------

def test_d_only_the_short_joins_run_again(rhj):
    for name in ("rerun mixed", "rerun all", "rerun none"):
        run_family(rhj, name)


# ---- e: descriptor limits -------------------------------------------------------------------------------------------------------------

def test_e_the_most_a_descriptor_holds(rhj):
    cols, _ = run_family(rhj, "descriptor limits")
    alone(rhj, cols, "descriptor limits", range(4))


# ---- f: empty relations ---------------------------------------------------------------------------------------------------------------

def test_f_relations_without_a_row(rhj, mod):
    cols, res = run_family(rhj, "empty relations")
    assert all(res[i] == ([0] * len(res[i][0]), 0) for i in qs.EMPTY_ROLES)
    rels, only, want, info, _ = qs.reference("empty only")
    run(rhj, cols, only, want, info, "empty only")
    assert info["filter_calls"] == 0 and info["apply_calls"] == 0
    rels, none, want, info, _ = qs.reference("no survivors")                  # an apply call that no item is left for still counts
    run(rhj, cols, none, want, info, "no survivors")
    assert info["join_calls"] == 1 and info["apply_calls"] == 1
    # relation 3 has no column: nothing can join, filter or sum it, so a query that binds it is refused before a device is touched
    with pytest.raises(ValueError):
        rhj.query_batch_device(cols, [qs.reference("empty relations")[1][0], ([3], [], [], [(0, 0)])])


# ---- g: state -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plain_join(rhj, oracle):
    """a single join of two 10 000-tuple relations and the oracle's pairs"""
    rng = np.random.default_rng(77)
    R, S = (make_rel(rng.integers(0, 8000, size=10000, dtype=np.uint64)) for _ in range(2))
    want = np.ascontiguousarray(oracle.join(R, S, 4), dtype=PAIR)
    return rhj.to_device(R), rhj.to_device(S), np.asarray(want["row_idR"]).copy(), np.asarray(want["row_idS"]).copy()


def join_still_right(rhj, plain_join, level):
    """the single join after a query batch: the oracle's pairs, and the statistics of the timing level set before the batch"""
    dR, dS, wantR, wantS = plain_join
    t, m = rhj.join_device(dR, dS)
    st = rhj.stats()
    got = rhj.pairs_to_numpy(t)
    assert m == len(wantR) and np.array_equal(got["row_idR"], wantR) and np.array_equal(got["row_idS"], wantS)
    assert st["path"] == "small" and (st["ms_total"] > 0) == (level >= 1) and (st["ms_probe"] > 0) == (level >= 2)


def test_g_small_large_and_small_again(rhj, plain_join):
    rhj.lib.rhj_release()
    rhj.torch.cuda.synchronize()
    rhj.set_bits(4)
    first = {}
    for name in ("tiny", "rerun mixed", "tiny", "descriptor limits", "rerun mixed"):
        _, res = run_family(rhj, name)
        assert first.setdefault(name, res) == res
        join_still_right(rhj, plain_join, 2)


def test_g_timing_levels(rhj, plain_join):
    rels, queries, want, info, _ = qs.reference("tiny")
    cols = to_device(rhj, rels)
    rhj.set_bits(4)
    try:
        for level in (0, 1, 2, 0):
            rhj.lib.rhj_set_timing(level)
            run(rhj, cols, queries, want, info, "timing %d" % level)
            assert (rhj.stats()["ms_total"] > 0) == (level >= 1), level
            join_still_right(rhj, plain_join, level)      # the level the call lowered for its inner batches is back
    finally:
        rhj.lib.rhj_set_timing(2)


def test_g_a_refused_batch_leaves_zero_counts_and_the_next_is_right(rhj, plain_join):
    rels, queries, want, info, _ = qs.reference("tiny")
    cols = to_device(rhj, rels)
    run(rhj, cols, queries, want, info, "before")
    assert any(last_info(rhj).values())
    with pytest.raises(ValueError):
        rhj.query_batch_device(cols, [queries[0], ([0, 1], [], [], [(0, 0)]), queries[2]])      # two nodes left: a cross product
    # query_batch clears the counts before it validates, and a refused batch returns before the levels are known: all zero
    assert last_info(rhj) == dict.fromkeys(INFO_FIELDS, 0)
    run(rhj, cols, queries, want, info, "after")
    join_still_right(rhj, plain_join, 2)
