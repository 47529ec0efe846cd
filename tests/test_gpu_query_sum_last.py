"""rhj_query_batch_device with rhj_set_query_sum_last(1) (include/rhj_inter.h): a query's last join is an item of one
rhj_join_sum_batch_device call per level and takes no pair buffer, no second join call and no apply item.  The answers are those
of the switch-off route (the `small` workload's recorded result lines, the numpy executor of query_model.py); the calls are those
query_model.call_counts gives for the switch-off route, moved as the header says."""
import ctypes as C
import importlib

import numpy as np
import pytest

import join_sum_model as jm
from query_model import INFO_FIELDS, call_counts, parse_work, run_query, track_kinds
from query_shapes import B63, CASES, synthetic_relations, tiny

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def rhj(mod):
    r = mod.RHJ(device=0)
    r.lib.rhj_set_timing(2)
    r.set_bits(4)
    yield r
    r.set_query_sum_last(False)
    r.lib.rhj_set_timing(2)
    r.lib.rhj_set_order(0)
    r.set_bits(4)


def dev(rhj, a):
    return rhj.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


def kinds_of(mod, lib, query, nrel):
    arr, keep = mod.query_descs([query])
    kinds = (C.c_int * max(len(query[1]), 1))()
    assert lib.rhj_query_levels(C.byref(arr[0]), nrel, None, kinds) == len(query[1])
    return list(kinds)[:len(query[1])]


def counts_with_the_switch(mod, lib, rels, queries):
    """(info, sum info) the call must report with the switch on, from call_counts' detail of the switch-off route: the first join
    call's items of a level are the joins of the queries alive there; those whose predicate is the query's last are the sum call's."""
    off, detail = call_counts(rels, queries)
    for q in queries:
        assert kinds_of(mod, lib, q, len(rels)) == track_kinds(q)
    on = dict(off, join_calls=0, join_reruns=0, apply_calls=0)
    sums = {"sum_calls": 0, "sum_items": 0}
    for l, lv in enumerate(detail["levels"]):
        last = [k for k, it in enumerate(lv["joins"]) if len(queries[it[0]][1]) - 1 == l]
        pairs = [k for k in range(len(lv["joins"])) if k not in last]
        sums["sum_calls"] += bool(last)
        sums["sum_items"] += len(last)
        on["join_calls"] += bool(pairs)
        on["join_reruns"] += any(k in lv["short"] for k in pairs)
        # who else took part: the equalities, the other joins, and at level 0 the queries without a predicate (alive ones have rows)
        on["apply_calls"] += bool(lv["eq"] or pairs or any(not queries[it[0]][1] for it in lv["apply"]))
    return off, on, sums


def run(rhj, cols, queries, on):
    rhj.set_query_sum_last(on)
    try:
        return rhj.query_batch_device(cols, queries, with_info=True)
    finally:
        rhj.set_query_sum_last(False)


@pytest.mark.parametrize("order", ("4 bits", "any"))
def test_small_workload_with_the_switch_on(rhj, mod, golden, order):
    rels = golden.small_relations
    relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    cols = [[dev(rhj, c) for c in rel] for rel in relations]
    queries = parse_work(golden.small["work_lines"])
    assert len(queries) == 50
    off, on, sums = counts_with_the_switch(mod, rhj.lib, relations, queries)
    rhj.set_bits(4)
    rhj.lib.rhj_set_order(1 if order == "any" else 0)
    try:
        res, info = run(rhj, cols, queries, True)
    finally:
        rhj.lib.rhj_set_order(0)
    lines = [" ".join("NULL" if rows == 0 else str(s) for s in sums_) for sums_, rows in res]
    assert lines == golden.small["result_lines"]
    assert info.sum_info == sums and sums["sum_items"] >= 40 and 1 <= sums["sum_calls"] <= 3
    assert info["join_reruns"] <= off["join_reruns"] and info["apply_calls"] <= off["apply_calls"]
    assert dict(info) == on
    st = rhj.stats()
    assert st["path"] == "query_batch" and st["n_r"] == 50 and st["matches"] == sum(rows for _, rows in res) and st["ms_total"] > 0


def test_synthetic_queries_with_the_switch_on(rhj, mod):
    relations = synthetic_relations()
    cols = [[dev(rhj, c) for c in rel] for rel in relations]
    names = sorted(CASES)
    queries = [CASES[k] for k in names]
    want = {k: run_query(relations, CASES[k]) for k in names}
    off, on, sums = counts_with_the_switch(mod, rhj.lib, relations, queries)
    res, info = run(rhj, cols, queries, True)
    for k, got in zip(names, res):
        assert (list(got[0]), got[1]) == (want[k][0], want[k][1]), k
    assert dict(info) == on and info.sum_info == sums
    # what the cases are here for
    assert want["fan-out on the large relation"][1] > 5000 and want["no match at the last level"] == ([0, 0], 0)
    assert track_kinds(CASES["a self-join last"])[-1] == 1 and not CASES["no join and no filter"][1]
    assert on["join_reruns"] < off["join_reruns"]         # (the fan-out joins that were last need no second call any more)
    # alone, and the switch off again gives the parent's calls
    for k in ("fan-out on the large relation", "no match at the last level", "a self-join last", "no join and no filter", "no filter"):
        (one, info1) = run(rhj, cols, [CASES[k]], True)
        assert (list(one[0][0]), one[0][1]) == (want[k][0], want[k][1]), k
    res0, info0 = run(rhj, cols, queries, False)
    assert res0 == res and dict(info0) == off and info0.sum_info == {"sum_calls": 0, "sum_items": 0}


def test_hand_made_batches_have_exact_counts(rhj, mod):
    relations = synthetic_relations()
    cols = [[dev(rhj, c) for c in rel] for rel in relations]
    single = [CASES[k] for k in ("no filter", "filters on two bindings", "a relation bound twice", "one row joins", "fan-out on the large relation")]
    res, info = run(rhj, cols, single, True)
    assert [(list(s), r) for s, r in res] == [(list(s), r) for s, r in (run_query(relations, q) for q in single)]
    assert dict(info) == dict(zip(INFO_FIELDS, (1, 1, 0, 0, 0, 0))) and info.sum_info == {"sum_calls": 1, "sum_items": 5}
    two = ([1, 2, 1], [(0, 1, 1, 1), (1, 0, 2, 0)], [], [(0, 1), (1, 1), (2, 1), (2, 2)])
    want = [run_query(relations, two), run_query(relations, CASES["no filter"])]
    assert want[0][1] > 0 and want[1][1] > 0
    res, info = run(rhj, cols, [two, CASES["no filter"]], True)
    assert [(list(s), r) for s, r in res] == [(list(s), r) for s, r in want]
    # level 0: the first join of `two` (one pair-list call, one apply call) and the sum call of the other; level 1: one sum call
    assert dict(info) == dict(zip(INFO_FIELDS, (2, 0, 0, 1, 0, 1)))
    assert info.sum_info == {"sum_calls": 2, "sum_items": 2}


def test_a_final_join_whose_pairs_do_not_fit(rhj):
    """200 000 x 200 000 rows with one key on 199 000 of each side: 3.96e10 pairs, which only the switch-on route can answer"""
    rng = np.random.default_rng(31)
    n = 200_000
    keys = [np.full(n, 77, dtype=np.uint64), np.full(n, 77, dtype=np.uint64)]
    keys[0][::200] = np.arange(1000) + 1000
    keys[1][100::200] = np.arange(1000) + 1500
    big = [[k, rng.permutation(n).astype(np.uint64) + np.uint64(B63), rng.integers(0, 1 << 62, size=n).astype(np.uint64)] for k in keys]
    small, small_queries = tiny()
    relations = big + small
    shifted = [([r + 2 for r in q[0]], q[1], q[2], q[3]) for q in small_queries[:2]]
    hot = ([0, 1], [(0, 0, 1, 0)], [], [(0, 1), (0, 2), (0, 0), (1, 1), (1, 2), (1, 0)])
    matches, sums = jm.join_sum(keys[0], keys[1], [(a, relations[a][c]) for a, c in hot[3]])
    assert matches == 199_000 ** 2 + 500
    cols = [[dev(rhj, c) for c in rel] for rel in relations]
    res, info = run(rhj, cols, [shifted[0], hot, shifted[1]], True)
    assert (list(res[1][0]), res[1][1]) == (sums, matches)
    for got, q in ((res[0], shifted[0]), (res[2], shifted[1])):
        w = run_query(relations, q)
        assert w[1] > 0 and (list(got[0]), got[1]) == (w[0], w[1])
    assert info["join_calls"] == 0 and info["join_reruns"] == 0 and info.sum_info == {"sum_calls": 1, "sum_items": 2}


def test_the_switch_off_again_is_the_parent(rhj, golden):
    rels = golden.small_relations
    relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    cols = [[dev(rhj, c) for c in rel] for rel in relations]
    queries = parse_work(golden.small["work_lines"])
    run(rhj, cols, queries[:10], True)
    rhj.set_bits(4)
    res, info = rhj.query_batch_device(cols, queries, with_info=True)
    lines = [" ".join("NULL" if rows == 0 else str(s) for s in sums) for sums, rows in res]
    assert lines == golden.small["result_lines"]
    assert dict(info) == call_counts(relations, queries)[0] and info.sum_info == {"sum_calls": 0, "sum_items": 0}
