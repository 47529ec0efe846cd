"""rhj_query_batch_device with rhj_set_query_fold(1) and rhj_set_query_fold_keys(1) (include/rhj_inter.h): the queries whose
predicates are a tree once parallel predicates are grouped run by rounds of fold items, those on one key through
rhj_join_fold_batch_device and those on tuple keys through rhj_join_foldk_batch_device.  The answers are the `small` workload's
recorded result lines, the numpy executor of query_model.py wherever that can answer, and the model of join_foldk_model.py beyond;
the calls are those join_foldk_model.foldk_counts gives, and with the new switch off those of join_fold_model.fold_counts."""
import importlib

import numpy as np
import pytest

import foldk_shapes as shapes
import join_fold_model as fm
import join_foldk_model as km
from query_model import call_counts, parse_work, run_query

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
NO_FOLDK = {"foldk_calls": 0, "foldk_items": 0, "foldk_queries": 0}
NO_SUMS = {"sum_calls": 0, "sum_items": 0}


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def rhj(mod):
    r = mod.RHJ(device=0)
    r.lib.rhj_set_timing(2)
    r.set_bits(4)
    yield r
    r.set_query_fold(False)
    r.set_query_fold_keys(False)
    r.set_query_sum_last(False)
    r.lib.rhj_set_timing(2)
    r.lib.rhj_set_order(0)
    r.set_bits(4)


def dev(rhj, a):
    return rhj.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


def run(rhj, cols, queries, fold=True, keys=True):
    rhj.set_query_fold(fold)
    rhj.set_query_fold_keys(keys)
    try:
        return rhj.query_batch_device(cols, queries, with_info=True)
    finally:
        rhj.set_query_fold(False)
        rhj.set_query_fold_keys(False)


def answers(res):
    return [(list(s), r) for s, r in res]


@pytest.fixture(scope="module")
def small(rhj, golden):
    rels = golden.small_relations
    relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    queries = parse_work(golden.small["work_lines"])
    assert len(queries) == 50
    return {"relations": relations, "cols": [[dev(rhj, c) for c in rel] for rel in relations], "queries": queries, "lines": golden.small["result_lines"]}


def lines_of(res):
    return [" ".join("NULL" if rows == 0 else str(s) for s in sums_) for sums_, rows in res]


def test_small_workload_with_both_switches_on(rhj, small):
    info_want, fold_want, foldk_want, folded = km.foldk_counts(small["relations"], small["queries"])
    assert all(f is not None for f in folded)            # every query of the workload folds
    res, info = run(rhj, small["cols"], small["queries"])
    assert lines_of(res) == small["lines"]
    assert answers(res) == [(list(s), r) for s, r in folded]
    assert info.fold_info == fold_want and info.foldk_info == foldk_want and dict(info) == info_want and info.sum_info == NO_SUMS
    assert dict(info) == dict(levels=0, filter_calls=1, eq2_calls=0, join_calls=0, join_reruns=0, apply_calls=0)      # nothing runs by levels
    assert foldk_want["foldk_calls"] >= 1 and foldk_want["foldk_items"] >= 2 and 3 <= foldk_want["foldk_queries"] <= 6
    st = rhj.stats()
    assert st["path"] == "query_batch" and st["n_r"] == 50 and st["matches"] == sum(rows for _, rows in res) & M64


def test_small_workload_with_the_new_switch_off(rhj, small):
    """today's answers and today's counts, after a call with both switches on; and with the fold route off the new switch alone does nothing"""
    run(rhj, small["cols"], small["queries"][:30])
    info_want, fold_want, _ = fm.fold_counts(small["relations"], small["queries"])
    res, info = run(rhj, small["cols"], small["queries"], keys=False)
    assert lines_of(res) == small["lines"]
    assert info.fold_info == fold_want and dict(info) == info_want and info.foldk_info == NO_FOLDK
    assert info_want["levels"] == 3                      # the six queries with parallel predicates run by levels
    res, info = run(rhj, small["cols"], small["queries"], fold=False)
    assert lines_of(res) == small["lines"]
    assert dict(info) == call_counts(small["relations"], small["queries"])[0]
    assert info.fold_info == {"fold_calls": 0, "fold_items": 0, "fold_queries": 0} and info.foldk_info == NO_FOLDK


def test_random_trees_with_parallel_predicates(rhj):
    relations, queries = shapes.random_trees()
    cols = [[dev(rhj, c) for c in rel] for rel in relations]
    want = [(list(s), r) for s, r in (run_query(relations, q) for q in queries)]
    info_want, fold_want, foldk_want, folded = km.foldk_counts(relations, queries)
    assert [(list(f[0]), f[1]) for f in folded] == want
    res, info = run(rhj, cols, queries)
    assert answers(res) == want
    assert info.fold_info == fold_want and info.foldk_info == foldk_want and dict(info) == info_want
    assert foldk_want["foldk_queries"] >= 6 and foldk_want["foldk_calls"] >= 2 and fold_want["fold_calls"] >= 2
    # the level route on the same queries
    res, info = run(rhj, cols, queries, fold=False)
    assert answers(res) == want and dict(info) == call_counts(relations, queries)[0]
    # each query that folds only with the new switch alone
    for q, w in zip(queries, want):
        if not fm.folds(q):
            one, info1 = run(rhj, cols, [q])
            assert answers(one) == [w], q
            assert (dict(info1), info1.fold_info, info1.foldk_info) == km.foldk_counts(relations, [q])[:3], q


def test_hand_made_trees(rhj):
    relations = shapes.hand_made()
    cols = [[dev(rhj, c) for c in rel] for rel in relations]
    huge_sums = [int(relations[b][c].sum(dtype=np.uint64)) * 3000 ** 3 & M64 for b, c in shapes.HUGE[3]]
    queries = [shapes.DIES, shapes.HUGE, shapes.CROSSED, shapes.PLAIN, shapes.LIVES]
    info_want, fold_want, foldk_want, folded = km.foldk_counts(relations, queries)
    # the chain of four 3000-row bindings on two constant columns: 8.1e13 rows, exact
    assert folded[1] == (huge_sums, 3000 ** 4) and 3000 ** 4 == 81 * 10 ** 12
    assert km.foldk_route(relations, shapes.HUGE)[2] == {0: [0, 2], 1: [0, 1]}
    for q, f in zip((shapes.DIES, shapes.CROSSED, shapes.PLAIN, shapes.LIVES), (folded[0], folded[2], folded[3], folded[4])):
        w = run_query(relations, q)
        assert (list(f[0]), f[1]) == (list(w[0]), w[1]), q
    assert folded[0] == ([0, 0], 0) and folded[2][1] == 160 and folded[3][1] > 0 and folded[4][1] == 28
    # a zero total at the middle round of a fold on two keys: round 0 has an item on one key and one on two, round 2 is never issued
    assert km.foldk_plan(shapes.DIES) == (1, [(0, 1, 0, [0]), (4, 3, 0, [5, 6]), (3, 2, 1, [3, 4]), (2, 1, 2, [1, 2])])
    assert km.foldk_route(relations, shapes.DIES)[2] == {0: [1, 1], 1: [0, 1]}
    assert km.foldk_route(relations, shapes.LIVES)[2] == {0: [1, 1], 1: [0, 1], 2: [0, 1]}
    res, info = run(rhj, cols, queries)
    assert answers(res) == [(list(f[0]), f[1]) for f in folded]
    assert info.fold_info == fold_want and info.foldk_info == foldk_want
    assert dict(info) == info_want == dict(levels=0, filter_calls=1, eq2_calls=0, join_calls=0, join_reruns=0, apply_calls=0)
    assert rhj.stats()["matches"] == sum(f[1] for f in folded) & M64
    # one round with items on one key and items on tuple keys: two calls counted for it
    res, info = run(rhj, cols, [shapes.DIES])
    assert answers(res) == [([0, 0], 0)]
    assert info.fold_info == {"fold_calls": 1, "fold_items": 1, "fold_queries": 1} and info.foldk_info == {"foldk_calls": 2, "foldk_items": 2, "foldk_queries": 1}
    # the huge query alone, twice, and once after rhj_release()
    for again in range(3):
        if again == 2:
            rhj.lib.rhj_release()
            rhj.torch.cuda.synchronize()
        res, info = run(rhj, cols, [shapes.HUGE])
        assert answers(res) == [(huge_sums, 81 * 10 ** 12)]
        assert info.fold_info == {"fold_calls": 0, "fold_items": 0, "fold_queries": 1} and info.foldk_info == {"foldk_calls": 2, "foldk_items": 3, "foldk_queries": 1}
    # with the new switch off the four queries with parallel predicates run by levels; the huge one cannot, so it stays out
    rest = [shapes.DIES, shapes.CROSSED, shapes.PLAIN, shapes.LIVES]
    res, info = run(rhj, cols, rest, keys=False)
    assert answers(res) == [(list(folded[k][0]), folded[k][1]) for k in (0, 2, 3, 4)]
    assert info.foldk_info == NO_FOLDK and info.fold_info == fm.fold_counts(relations, rest)[1] and info.fold_info["fold_queries"] == 1
