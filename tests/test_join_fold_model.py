"""tests/join_fold_model.py held to account without a device, and rhj_query_fold_plan (a pure function) against it: fold_item
against a double loop, the whole fold route against the numpy executor of query_model.py on the folding queries of the `small`
workload and of tests/query_shapes.py, and the plan rule on chains, stars, a relation bound twice and a tie between roots."""
import ctypes as C
import importlib

import numpy as np
import pytest

import join_fold_model as fm
from query_model import parse_work, run_query, track_kinds
from query_shapes import CASES, synthetic_relations

M64 = fm.M64


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def lib(mod):
    return mod.load_library()


def library_plan(mod, lib, query, nrel=None):
    """rhj_query_fold_plan on one query: (return value, root, [(child, parent, round)])"""
    arr, keep = mod.query_descs([query])
    root, steps = C.c_int(-1), (mod.FoldStep * 7)()
    n = lib.rhj_query_fold_plan(C.byref(arr[0]), nrel if nrel is not None else max(query[0]) + 1, None, C.byref(root), steps)
    return n, root.value, [(s.child, s.parent, s.round) for s in steps[:max(n, 0)]]


def test_fold_item_against_a_double_loop():
    rng = np.random.default_rng(20182)
    big = np.array([0, 1, 1 << 63, (1 << 64) - 1, (1 << 64) - 2, 12345, 3], dtype=np.uint64)
    for case in range(14):
        nR, nS = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        pool = rng.choice(np.array([0, 1, 2, 3, (1 << 64) - 1, 1 << 63, 77], dtype=np.uint64), size=int(rng.integers(1, 6)), replace=False)
        kR, kS = rng.choice(pool, size=nR), rng.choice(pool, size=nS)

        def some_factor(n):
            w = rng.choice(big, size=n) if rng.integers(0, 2) else None
            col = rng.choice(big, size=50) if rng.integers(0, 2) else None
            src = rng.integers(0, 50, size=n).astype(np.uint64) if col is not None and rng.integers(0, 2) else None
            if col is not None and src is None:
                col = rng.choice(big, size=n)
            return (w, src, col)
        values = [some_factor(nS) for _ in range(1 + case % 9)]
        outs = [(int(rng.integers(0, len(values))), some_factor(nR)) for _ in range(case % 10)]
        want = fm.brute_force(kR, kS, values, outs)
        assert fm.fold_item(kR, kS, values, outs) == want, case
        assert [(v.tolist(), t) for v, t in fm.fold_item_np(kR, kS, values, outs)] == want, case
    ones = (None, None, None)
    # a parent key absent from the child is a 0; a child key absent from the parent adds nothing
    assert fm.fold_item([1, 2, 3], [3, 3, 9], [ones], [(0, ones)]) == [([0, 0, 2], 2)]
    # a product that wraps: three rows of 2^63 are 2^63 modulo 2^64, times a weight of 3 again 2^63
    w63 = np.array([1 << 63] * 3, dtype=np.uint64)
    assert fm.fold_item([5], [5, 5, 5], [(w63, None, None)], [(0, (np.array([3], dtype=np.uint64), None, None))]) == [([1 << 63], 1 << 63)]
    assert fm.fold_item([5], [5, 5], [(np.array([1 << 63] * 2, dtype=np.uint64), None, None)], [(0, ones)]) == [([0], 0)]


def test_the_route_against_the_numpy_executor_on_the_small_workload(golden, mod, lib):
    rels = golden.small_relations
    cols = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    queries = parse_work(golden.small["work_lines"])
    assert len(queries) == 50
    folding = 0
    for q in queries:
        kinds = track_kinds(q)
        plan = fm.fold_plan(q)
        assert (plan is not None) == (bool(kinds) and not any(kinds)), q
        n, root, steps = library_plan(mod, lib, q, len(cols))
        if plan is None:
            assert n == 0, q
            continue
        assert (n, root, steps) == (len(q[1]), plan[0], plan[1]), q
        folding += 1
        sums, rows = run_query(cols, q)
        got = fm.fold_route(cols, q)
        assert (got[0], got[1]) == (list(sums), rows), q
    assert folding >= 40


def test_the_route_against_the_numpy_executor_on_the_synthetic_queries(mod, lib):
    cols = synthetic_relations()
    assert len(CASES) == 24
    folding = [k for k in sorted(CASES) if fm.folds(CASES[k])]
    assert len(folding) >= 12 and "eight bindings in a chain" in folding and "two two-binding nodes merge" in folding
    for k in sorted(CASES):
        n, root, steps = library_plan(mod, lib, CASES[k], len(cols))
        if k not in folding:
            assert n == 0, k
            continue
        assert (n, root, steps) == (len(CASES[k][1]),) + fm.fold_plan(CASES[k]), k
        sums, rows = run_query(cols, CASES[k])
        for item in (fm.fold_item_np, fm.fold_item) if sum(len(cols[r][0]) for r in CASES[k][0]) < 20000 else (fm.fold_item_np,):
            got = fm.fold_route(cols, CASES[k], item=item)
            assert (got[0], got[1]) == (list(sums), rows), k


def chain(n):
    return (list(range(n)), [(k, 0, k + 1, 0) for k in range(n - 1)], [], [(0, 0)])


def star(leaves, centre=0):
    others = [b for b in range(leaves + 1) if b != centre]
    return (list(range(leaves + 1)), [(centre, 0, b, 0) for b in others], [], [(0, 0)])


PLANS = {
    "a chain of two": (chain(2), 0, [(1, 0, 0)]),
    # the middle takes one child a round, so it is no faster than an end: the lower binding
    "a chain of three": (chain(3), 0, [(2, 1, 0), (1, 0, 1)]),
    # rooted in its middle: the arms 0..2 and 4..7 are ready after rounds 1 and 2, the root takes them in rounds 2 and 3
    "a chain of eight": (chain(8), 3, [(0, 1, 0), (7, 6, 0), (1, 2, 1), (6, 5, 1), (2, 3, 2), (5, 4, 2), (4, 3, 3)]),
    # two arms of equal depth: the centre takes one child a round, so one round more than an arm
    "a chain of seven": (chain(7), 2, [(0, 1, 0), (6, 5, 0), (1, 2, 1), (5, 4, 1), (4, 3, 2), (3, 2, 3)]),
    "a star of 1 + 3": (star(3), 0, [(1, 0, 0), (2, 0, 1), (3, 0, 2)]),
    "a star of 1 + 7": (star(7), 0, [(b, 0, b - 1) for b in range(1, 8)]),
    # a leaf as the root costs the centre's two other children and the centre itself: three rounds, as the centre does
    "a star whose centre is binding 2": (star(3, centre=2), 0, [(1, 2, 0), (3, 2, 1), (2, 0, 2)]),
    "a relation bound twice": (([4, 4, 1], [(0, 0, 1, 0), (1, 1, 2, 1)], [], [(2, 0)]), 0, [(2, 1, 0), (1, 0, 1)]),
    # the roots 1 and 2 of a chain of four both give two rounds: the lower binding
    "a tie between roots": (chain(4), 1, [(0, 1, 0), (3, 2, 0), (2, 1, 1)]),
    "the predicates in another order": (([0, 1, 2, 3], [(2, 0, 3, 0), (0, 0, 1, 0), (1, 1, 2, 1)], [], [(0, 0)]), 1, [(0, 1, 0), (3, 2, 0), (2, 1, 1)]),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_the_plan_rule(mod, lib, name):
    query, root, steps = PLANS[name]
    assert fm.fold_plan(query) == (root, steps)
    assert library_plan(mod, lib, query) == (len(steps), root, steps)


def test_the_chain_of_eight_takes_four_rounds():
    rounds = {r: fm.schedule(8, chain(8)[1], r)[0] for r in range(8)}
    assert rounds == {0: 7, 1: 6, 2: 5, 3: 4, 4: 4, 5: 5, 6: 6, 7: 7}
    assert fm.schedule(7, chain(7)[1], 3)[0] == 4 and fm.schedule(7, chain(7)[1], 2)[0] == 4
    assert fm.schedule(8, star(7)[1], 0)[0] == 7 and fm.schedule(8, star(7)[1], 1)[0] == 7


NO_FOLD = {
    "a self-join": ([2], [(0, 2, 0, 0)], [], [(0, 1)]),
    "a self-join after a join": ([1, 2], [(0, 1, 1, 1), (1, 0, 1, 2)], [], [(0, 1)]),
    "two predicates between the same bindings": ([1, 2], [(0, 1, 1, 1), (0, 0, 1, 2)], [], [(0, 2)]),
    "no predicate": ([2], [], [], [(0, 2)]),
    "an equality inside a merged node": ([1, 2, 1], [(0, 1, 1, 1), (1, 0, 2, 0), (0, 2, 2, 2)], [], [(0, 0)]),
}


@pytest.mark.parametrize("name", sorted(NO_FOLD))
def test_forms_that_do_not_fold(mod, lib, name):
    assert fm.fold_plan(NO_FOLD[name]) is None
    n, root, steps = library_plan(mod, lib, NO_FOLD[name])
    assert n == 0 and root == -1


def test_an_invalid_query_has_no_plan(mod, lib):
    assert library_plan(mod, lib, ([0, 1], [(0, 0, 1, 0)], [], [(0, 0)]), nrel=1)[0] == -3       # a relation out of range
    assert library_plan(mod, lib, ([0, 1], [], [], [(0, 0)]))[0] == -3                           # a cross product
    assert lib.rhj_query_fold_plan(None, 1, None, None, None) == -3
    arr, keep = mod.query_descs([chain(3)])
    assert lib.rhj_query_fold_plan(C.byref(arr[0]), 3, None, None, None) == 2                    # root and steps may be NULL
