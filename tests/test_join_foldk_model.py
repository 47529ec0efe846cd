"""tests/join_foldk_model.py held to account without a device, and rhj_query_foldk_plan (a pure function) against it: foldk_item
against a double loop and, at one key, against join_fold_model.fold_item; the plan rule on the `small` workload, on the plans and
the refused forms of test_join_fold_model.py and on parallel predicates; the route's model against the numpy executor of
query_model.py and, for trees with parallel predicates, against a brute force by itertools.product."""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import join_fold_model as fm
import join_foldk_model as km
from query_model import parse_work, run_query
from query_shapes import CASES, synthetic_relations
from test_join_fold_model import NO_FOLD, PLANS

M64 = fm.M64
# the six queries of `small` that fold only with parallel predicates grouped: position -> the groups' predicate indices by binding pair
SMALL_GROUPED = {19: {(0, 1): [0], (1, 2): [1]}, 34: {(0, 1): [0], (1, 2): [2]}, 37: {(0, 1): [0], (1, 2): [1]},
                 22: {(0, 1): [0], (1, 2): [1, 2]}, 23: {(0, 1): [0, 2], (0, 2): [1]}, 48: {(0, 1): [0, 1], (1, 2): [2]}}


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def lib(mod):
    return mod.load_library()


def library_plan(mod, lib, query, nrel=None):
    """rhj_query_foldk_plan on one query: (return value, root, [(child, parent, round, [predicate indices])])"""
    arr, keep = mod.query_descs([query])
    root, steps = C.c_int(-1), (mod.FoldKStep * 7)()
    n = lib.rhj_query_foldk_plan(C.byref(arr[0]), nrel if nrel is not None else max(query[0]) + 1, None, C.byref(root), steps)
    return n, root.value, [(s.child, s.parent, s.round, list(s.joins[:s.nkeys])) for s in steps[:max(n, 0)]]


def held(mod, lib, query, nrel=None):
    """the library's plan against the model's; returns the model's"""
    plan = km.foldk_plan(query)
    got = library_plan(mod, lib, query, nrel)
    if plan is None:
        assert got[0] == 0 and got[1] == -1, query
    else:
        assert got == (len(query[0]) - 1, plan[0], plan[1]), query
    return plan


def test_foldk_item_against_a_double_loop():
    rng = np.random.default_rng(20184)
    big = np.array([0, 1, 1 << 63, M64, M64 - 1, 12345, 3], dtype=np.uint64)
    matched = 0
    for case in range(16):
        nk = 1 + case % 4
        nR, nS = int(rng.integers(1, 31)), int(rng.integers(1, 31))
        pool = np.array([0, 1, 2, M64, 1 << 63], dtype=np.uint64)[:2 if nk > 2 else int(rng.integers(2, 6))]
        kR, kS = [rng.choice(pool, size=nR) for _ in range(nk)], [rng.choice(pool, size=nS) for _ in range(nk)]

        def some_factor(n):
            w = rng.choice(big, size=n) if rng.integers(0, 2) else None
            col = rng.choice(big, size=40) if rng.integers(0, 2) else None
            src = rng.integers(0, 40, size=n).astype(np.uint64) if col is not None else None
            return (w, src, col)
        values = [some_factor(nS) for _ in range(1 + case % 9)]
        outs = [(int(rng.integers(0, len(values))), some_factor(nR)) for _ in range(1 + case % 9)]
        want = km.brute_force(kR, kS, values, outs)
        matched += any(t for _, t in want)
        assert km.foldk_item(kR, kS, values, outs) == want, case
        assert [(v.tolist(), t) for v, t in km.foldk_item_np(kR, kS, values, outs)] == want, case
        if nk == 1:
            assert fm.fold_item(kR[0], kS[0], values, outs) == want, case
    assert matched >= 8                                  # (most cases have tuples on both sides)
    ones = (None, None, None)
    u = lambda *x: np.array(x, dtype=np.uint64)
    # (a, b) is not (b, a); a tuple that differs in the last word only, or in the first only, is another tuple
    assert km.foldk_item([u(1, 2, 1), u(2, 1, 3)], [u(2, 1, 1), u(1, 2, 2)], [ones], [(0, ones)]) == [([2, 1, 0], 3)]
    # the all-zero and the all-ones tuples are tuples like any other
    assert km.foldk_item([u(0, M64, 0), u(0, M64, M64)], [u(0, 0, M64), u(0, 0, M64)], [ones], [(0, ones)]) == [([2, 1, 0], 3)]


def test_the_home_slot_of_one_word_is_the_fold_batch_s():
    import join_sum_model as jm
    for key in (0, 1, 12345, M64, 1 << 63):
        for log2 in (1, 7, 33):
            assert km.home([key], log2) == jm.home(key, log2)
    cols = km.tuples_homed_at(5, 6, 20, 3)
    assert len(cols) == 3 and all(km.home([int(c[k]) for c in cols], 6) == 5 for k in range(20))


def test_small_workload_every_query_has_a_plan(golden, mod, lib):
    """44 of the 50 have join_fold_model's plan with one key a step; the six others group their parallel predicates"""
    queries = parse_work(golden.small["work_lines"])
    assert len(queries) == 50
    old = 0
    for i, q in enumerate(queries):
        plan = held(mod, lib, q, len(golden.small_relations))
        assert plan is not None, (i, q)
        before = fm.fold_plan(q)
        if before is not None:
            assert i not in SMALL_GROUPED
            assert (plan[0], [s[:3] for s in plan[1]]) == before and all(len(s[3]) == 1 for s in plan[1])
            old += 1
        else:
            assert {(min(c, p), max(c, p)): idx for c, p, _, idx in plan[1]} == SMALL_GROUPED[i], (i, q)
    assert old == 44


def test_the_six_grouped_queries_pair_the_columns_the_issue_names(golden):
    queries = parse_work(golden.small["work_lines"])
    pairs = lambda i: {(s[1], s[0]): km.key_columns(queries[i], s) for s in km.foldk_plan(queries[i])[1]}
    both = lambda i, a, b: pairs(i).get((a, b)) or [(y, x) for x, y in pairs(i)[(b, a)]]      # as (a's column, b's column)
    assert both(22, 1, 2) == [(0, 1), (0, 2)]            # (1.0, 1.0) = (2.1, 2.2)
    assert both(23, 0, 1) == [(0, 2), (0, 1)]            # (0.0, 0.0) = (1.2, 1.1)
    assert both(48, 0, 1) == [(2, 0), (1, 0)]            # (0.2, 0.1) = (1.0, 1.0)
    assert both(19, 0, 1) == [(2, 0)] and both(19, 1, 2) == [(0, 1)]


@pytest.mark.parametrize("name", sorted(PLANS))
def test_a_plan_of_the_fold_route_is_this_plan_with_one_key(mod, lib, name):
    query, root, steps = PLANS[name]
    plan = held(mod, lib, query)
    by_pair = {(min(a, b), max(a, b)): l for l, (a, _, b, _) in enumerate(query[1])}
    assert plan == (root, [(c, p, r, [by_pair[(min(c, p), max(c, p))]]) for c, p, r in steps])


def test_the_forms_that_did_not_fold(mod, lib):
    assert held(mod, lib, NO_FOLD["two predicates between the same bindings"]) == (0, [(1, 0, 0, [0, 1])])
    for name in ("a self-join", "a self-join after a join", "an equality inside a merged node", "no predicate"):
        assert held(mod, lib, NO_FOLD[name]) is None, name


def parallel(n, cols=None):
    """two bindings joined by n predicates, predicate t on columns (t, t) unless given"""
    return ([0, 1], [(0, a, 1, b) for a, b in (cols or [(t, t) for t in range(n)])], [], [(0, 0)])


def test_parallel_predicates(mod, lib):
    assert held(mod, lib, parallel(4)) == (0, [(1, 0, 0, [0, 1, 2, 3])])
    assert held(mod, lib, parallel(5)) is None
    # a duplicate counts once, written the same way or the other way round: five predicates, four kept
    q = ([0, 1], [(0, 0, 1, 0), (0, 1, 1, 1), (1, 0, 0, 0), (0, 2, 1, 2), (0, 1, 1, 1), (1, 3, 0, 3)], [], [(0, 0)])
    assert held(mod, lib, q) == (0, [(1, 0, 0, [0, 1, 3, 5])])
    # the same two columns the other way round are another predicate: (0.0 = 1.1) and (0.1 = 1.0)
    assert held(mod, lib, parallel(2, [(0, 1), (1, 0)])) == (0, [(1, 0, 0, [0, 1])])
    # mixed directions pair the right columns: the parent's column of a predicate is its column on the parent's binding
    q = ([0, 1, 2], [(0, 0, 1, 1), (1, 2, 0, 3), (2, 5, 1, 4), (1, 6, 2, 7)], [], [(0, 0)])
    plan = held(mod, lib, q)
    assert plan == (0, [(2, 1, 0, [2, 3]), (1, 0, 1, [0, 1])])
    assert km.key_columns(q, plan[1][0]) == [(4, 5), (6, 7)] and km.key_columns(q, plan[1][1]) == [(0, 1), (3, 2)]
    # a cycle over three bindings stays out, with or without parallel predicates
    assert held(mod, lib, ([0, 1, 2], [(0, 0, 1, 0), (1, 0, 2, 0), (2, 0, 0, 0)], [], [(0, 0)])) is None
    assert held(mod, lib, ([0, 1, 2], [(0, 0, 1, 0), (0, 1, 1, 1), (1, 0, 2, 0), (2, 0, 0, 0)], [], [(0, 0)])) is None
    # a self-join next to parallel predicates
    assert held(mod, lib, ([0, 1], [(0, 0, 1, 0), (0, 1, 1, 1), (1, 0, 1, 1)], [], [(0, 0)])) is None


def test_an_invalid_query_has_no_plan(mod, lib):
    assert library_plan(mod, lib, parallel(2), nrel=1)[0] == -3                                  # a relation out of range
    assert library_plan(mod, lib, ([0, 1], [], [], [(0, 0)]))[0] == -3                           # a cross product
    assert library_plan(mod, lib, ([0, 1, 2], [(0, 0, 1, 0), (0, 1, 1, 1)], [], [(0, 0)]))[0] == -3
    assert lib.rhj_query_foldk_plan(None, 1, None, None, None) == -3
    arr, keep = mod.query_descs([parallel(3)])
    assert lib.rhj_query_foldk_plan(C.byref(arr[0]), 2, None, None, None) == 1                   # root and steps may be NULL


def test_the_route_against_the_numpy_executor_on_the_small_workload(golden):
    rels = golden.small_relations
    cols = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    queries = parse_work(golden.small["work_lines"])
    tuples = 0
    for i, q in enumerate(queries):
        sums, rows = run_query(cols, q)
        got = km.foldk_route(cols, q)
        assert (got[0], got[1]) == (list(sums), rows), (i, q)
        tuples += sum(b for _, b in got[2].values())
        if fm.folds(q):
            old = fm.fold_route(cols, q)
            assert (got[0], got[1], {r: a for r, (a, _) in got[2].items()}) == old and not any(b for _, b in got[2].values())
    assert tuples >= 2                                   # (22, 23 and 48 have a step on two keys unless a filter finishes them first)


def test_the_route_against_the_numpy_executor_on_the_synthetic_queries():
    cols = synthetic_relations()
    assert len(CASES) == 24
    folding = [k for k in sorted(CASES) if km.foldk_plan(CASES[k]) is not None]
    assert set(folding) >= {k for k in CASES if fm.folds(CASES[k])} and "two predicates between two bindings" in folding
    for k in folding:
        sums, rows = run_query(cols, CASES[k])
        for item in (km.foldk_item_np, km.foldk_item) if sum(len(cols[r][0]) for r in CASES[k][0]) < 20000 else (km.foldk_item_np,):
            got = km.foldk_route(cols, CASES[k], item=item)
            assert (got[0], got[1]) == (list(sums), rows), k


def product_answer(cols, query):
    """(sums, rows) by trying every combination of rows"""
    rels, joins, filters, views = query
    ops = {"<": lambda x, v: x < v, ">": lambda x, v: x > v, "=": lambda x, v: x == v}
    sums, rows = [0] * len(views), 0
    for combo in itertools.product(*[range(len(cols[r][0])) for r in rels]):
        val = lambda b, c: int(cols[rels[b]][c][combo[b]])
        if all(ops[op](val(a, c), int(v)) for a, c, op, v in filters) and all(val(a, ca) == val(b, cb) for a, ca, b, cb in joins):
            rows += 1
            for v, (b, c) in enumerate(views):
                sums[v] = (sums[v] + val(b, c)) & M64
    return sums, rows


def test_the_route_against_a_brute_force_on_trees_with_parallel_predicates():
    rng = np.random.default_rng(416)
    folded = 0
    for case in range(24):
        nb = int(rng.integers(2, 5))
        cols = [[rng.integers(0, 3, size=n).astype(np.uint64) if c < 4 else rng.integers(0, 1 << 63, size=n).astype(np.uint64) * np.uint64(2) + np.uint64(1)
                 for c in range(5)] for n in rng.integers(1, 13 if nb < 4 else 8, size=3)]
        rels = [int(r) for r in rng.integers(0, 3, size=nb)]
        joins = []
        for b in range(1, nb):
            a = int(rng.integers(0, b))
            for _ in range(int(rng.integers(1, 5)) if rng.integers(0, 2) else 1):
                p = (a, int(rng.integers(0, 4)), b, int(rng.integers(0, 4)))
                joins.append(p if rng.integers(0, 2) else (p[2], p[3], p[0], p[1]))
        joins = [joins[k] for k in rng.permutation(len(joins))]
        filters = [(0, 0, "<", 2)] if case % 3 == 0 else []
        views = [(int(rng.integers(0, nb)), 4) for _ in range(int(rng.integers(1, 4)))]
        q = (rels, joins, filters, views)
        plan = km.foldk_plan(q)
        assert plan is not None, q
        want = product_answer(cols, q)
        for item in (km.foldk_item, km.foldk_item_np):
            got = km.foldk_route(cols, q, item=item)
            assert (got[0], got[1]) == (want[0] if want[1] else [0] * len(views), want[1]), q
        folded += want[1] > 0 and any(len(s[3]) > 1 for s in plan[1])
    assert folded >= 6


def test_the_random_trees_of_the_gpu_test_are_all_within_the_executor_s_reach():
    """tests/foldk_shapes.py: 2..6 bindings, relations of at most 300 rows on key columns of at most 8 distinct values, a share of
    the edges on 2..4 predicates; every one has a plan, a result the executor materialises, and the route's model agrees"""
    import foldk_shapes as shapes
    relations, queries = shapes.random_trees()
    assert len(queries) == shapes.TREES and {len(q[0]) for q in queries} == {2, 3, 4, 5, 6}
    assert max(len(rel[0]) for rel in relations) <= 300 and all(len(np.unique(c)) <= 8 for rel in relations for c in rel[:shapes.KEY_COLUMNS])
    edges = [len(idx) for q in queries for _, idx in km.groups_of(q)]
    assert {2, 3, 4} <= set(edges) and 0.2 <= sum(n > 1 for n in edges) / len(edges) <= 0.45
    most = 0
    for q in queries:
        assert km.foldk_plan(q) is not None, q
        sums, rows = run_query(relations, q)
        got = km.foldk_route(relations, q)
        assert (got[0], got[1]) == (list(sums), rows), q
        most = max(most, rows)
    assert 10_000 < most < 1_000_000 and sum(not fm.folds(q) for q in queries) >= 8
