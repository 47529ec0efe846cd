"""tests/join_folds_model.py held to account without a device, and rhj_query_folds_plan (a pure function) against it: self_item
against a double loop; the plan rule on the `small` workload, on every query of tests/query_shapes.py, on implied and true
triangles and on the limits of an item; the route's model against the numpy executor of query_model.py and, for small random
queries, against a brute force by itertools.product; the four infos of a hand-made batch."""
import importlib
import itertools

import numpy as np
import pytest

import join_fold_model as fm
import join_foldk_model as km
import join_folds_model as sm
import query_shapes as shapes
from query_model import parse_work, run_query, trace_query, track_kinds

M64 = fm.M64
# the queries of tests/query_shapes.py that do NOT fold: (family, position).  Each has a true equality inside a merged node, a
# predicate between two bindings that the tree of the others connects already, on columns the others do not equate.
SHAPES_THAT_DO_NOT_FOLD = {("synthetic", sorted(shapes.CASES).index("two nodes merge, then an equality")),
                           ("descriptor limits", 0), ("descriptor limits", 1), ("descriptor limits", 3), ("tiny", 2)}
TRIANGLE = [(0, 1, 1, 0), (1, 0, 2, 1), (0, 1, 2, 1)]    # the third follows from the first two


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def lib(mod):
    return mod.load_library()


def held(mod, lib, query, nrel=None):
    """the library's plan against the model's; returns the model's"""
    plan = sm.folds_plan(query)
    got = mod.query_folds_plan(lib, query, nrel)
    assert got == plan, query
    return plan


def q(rels, joins, views=((0, 0),), filters=()):
    return (list(rels), list(joins), list(filters), list(views))


def test_self_item_against_a_double_loop():
    rng = np.random.default_rng(20185)
    big = np.array([0, 1, 1 << 63, M64, M64 - 1, 12345, 3], dtype=np.uint64)
    passed = masked = 0
    for case in range(20):
        n = int(rng.integers(1, 40))
        pool = np.array([0, M64, 5], dtype=np.uint64)[:1 + case % 3]

        def some_factor():
            w = rng.choice(big, size=n) if rng.integers(0, 2) else None
            col = rng.choice(big, size=50) if rng.integers(0, 2) else None
            src = rng.integers(0, 50, size=n).astype(np.uint64) if col is not None and rng.integers(0, 2) else None
            return (w, src, col)

        def some_term():
            vec = lambda: rng.integers(0, 60, size=n).astype(np.uint64) if rng.integers(0, 2) else None
            return (rng.choice(pool, size=60), vec(), rng.choice(pool, size=60), vec())
        terms = [some_term() for _ in range(case % 5)]
        outs = [some_factor() for _ in range(case % 10)]
        want = sm.brute_force(n, terms, outs)
        assert sm.self_item(n, terms, outs) == want, case
        assert [(v.tolist(), t) for v, t in sm.self_item_np(n, terms, outs)] == want, case
        m = sm.self_item(n, terms, [(None, None, None)])[0]
        passed += m[1] > 0
        masked += m[1] < n
    assert passed >= 8 and masked >= 8
    u = lambda *x: np.array(x, dtype=np.uint64)
    ones = (None, None, None)
    # A's vector is not B's: the term reads column A through selA and column B through selB
    assert sm.self_item(3, [(u(7, 8, 9), u(2, 1, 0), u(9, 0, 0), None)], [ones]) == [([1, 0, 0], 1)]
    assert sm.self_item(3, [(u(9, 0, 0), None, u(7, 8, 9), u(2, 1, 0))], [ones]) == [([1, 0, 0], 1)]
    assert sm.self_item(3, [(u(7, 8, 9), None, u(9, 0, 0), u(2, 1, 0))], [ones]) == [([0, 0, 1], 1)]      # the vectors swapped: another row
    # no term: the factor itself; no output: nothing
    assert sm.self_item(2, [], [(u(3, 4), None, None)]) == [([3, 4], 7)] and sm.self_item(2, [], []) == []


def test_small_workload_every_plan_is_the_tuple_key_plan(golden, mod, lib):
    queries = parse_work(golden.small["work_lines"])
    assert len(queries) == 50
    for i, query in enumerate(queries):
        plan = held(mod, lib, query, len(golden.small_relations))
        assert plan is not None and plan[2] == [], (i, query)
        assert (plan[0], plan[1]) == km.foldk_plan(query), (i, query)


def test_every_query_of_the_query_shapes(mod, lib):
    seen, refused = set(), set()
    for name in sorted(shapes.FAMILIES):
        _, queries = shapes.FAMILIES[name]()
        for i, query in enumerate(queries):
            shape = (tuple(query[0]), tuple(query[1]))
            if (name, i) not in SHAPES_THAT_DO_NOT_FOLD and shape in seen:
                continue                                 # (thousands of a family's queries differ in a filter's constant alone)
            seen.add(shape)
            plan = held(mod, lib, query)
            kinds = track_kinds(query)
            assert kinds is not None
            if plan is None:
                refused.add((name, i))
                assert any(kinds), (name, i)             # an equality inside a merged node, and a true one
            before = km.foldk_plan(query)
            if before is not None:                       # what folded already keeps its plan (no query here has an implied predicate)
                assert plan == (before[0], before[1], []), (name, i)
    assert refused == SHAPES_THAT_DO_NOT_FOLD
    by_name = lambda n: sm.folds_plan(shapes.CASES[n])
    assert by_name("a self-join first") == (0, [(1, 0, 0, [1])], [0]) and by_name("a self-join last") == (0, [(1, 0, 0, [0])], [1])
    assert by_name("a self-join alone") == (0, [], [0]) and by_name("a self-join without a match") == (0, [], [0])
    assert by_name("no join and no filter") == (0, [], []) and by_name("no join, two filters") == (0, [], [])
    assert by_name("two predicates between two bindings") == (0, [(1, 0, 0, [0, 1])], [])
    # 0.2=0.2 says nothing and is dropped
    assert sm.folds_plan(shapes.rerun_all()[1][2]) == (0, [(1, 0, 0, [0])], [])


def test_the_implied_triangle_folds_in_every_order(mod, lib):
    flip = lambda p: (p[2], p[3], p[0], p[1])
    for order in itertools.permutations(range(3)):
        for flips in itertools.product((False, True), repeat=3):
            joins = [flip(TRIANGLE[k]) if f else TRIANGLE[k] for k, f in zip(order, flips)]
            plan = held(mod, lib, q([0, 1, 2], joins))
            assert plan is not None and len(plan[1]) == 2 and plan[2] == [], joins
            assert sorted(l for s in plan[1] for l in s[3]) == [0, 1] and all(len(s[3]) == 1 for s in plan[1])      # the last one given is the one dropped
            assert km.foldk_plan(q([0, 1, 2], joins)) is None and not fm.folds(q([0, 1, 2], joins))


def test_a_true_triangle_does_not_fold(mod, lib):
    assert held(mod, lib, q([0, 1, 2], [(0, 0, 1, 0), (1, 1, 2, 1), (0, 2, 2, 2)])) is None
    # the triangle's columns with one of them changed: nothing is implied any more
    assert held(mod, lib, q([0, 1, 2], [(0, 1, 1, 0), (1, 0, 2, 1), (0, 2, 2, 1)])) is None
    assert held(mod, lib, q([0, 1, 2], [(0, 1, 1, 0), (1, 1, 2, 1), (0, 1, 2, 1)])) is None


def test_the_limits_of_an_item(mod, lib):
    five = [(0, c, 0, c + 1) for c in range(5)]
    assert held(mod, lib, q([0], five)) is None
    assert held(mod, lib, q([0], five[:4])) == (0, [], [0, 1, 2, 3])
    assert held(mod, lib, q([0, 1], five + [(0, 0, 1, 0)])) is None
    # five written, four kept: 0.0=0.2 follows from 0.0=0.1 and 0.1=0.2
    assert held(mod, lib, q([0, 1], [(1, 0, 0, 0)] + five[:2] + [(0, 0, 0, 2)] + five[2:4])) == (0, [(1, 0, 0, [0])], [1, 2, 4, 5])
    # four on each of two bindings
    assert held(mod, lib, q([0, 1], five[:4] + [(0, 0, 1, 0)] + [(1, c, 1, c + 1) for c in range(1, 5)])) == (0, [(1, 0, 0, [4])], [0, 1, 2, 3, 5, 6, 7, 8])
    # 0.1=0.1 is dropped wherever it stands
    assert held(mod, lib, q([0], [(0, 1, 0, 1)])) == (0, [], [])
    assert held(mod, lib, q([0, 1], [(0, 1, 0, 1), (0, 0, 1, 0), (1, 2, 1, 2)])) == (0, [(1, 0, 0, [1])], [])
    # the same predicate twice, either way round: kept once
    assert held(mod, lib, q([0], [(0, 1, 0, 2), (0, 2, 0, 1), (0, 1, 0, 2)])) == (0, [], [0])
    # a fourth parallel predicate that the first three imply: three key words, where the tuple-key plan keeps four
    par = q([0, 1], [(0, 0, 1, 0), (0, 1, 1, 0), (0, 0, 1, 1), (0, 1, 1, 1)])
    assert held(mod, lib, par) == (0, [(1, 0, 0, [0, 1, 2])], []) and km.foldk_plan(par) == (0, [(1, 0, 0, [0, 1, 2, 3])])
    # five parallel predicates on five column pairs: more key words than a tuple has
    assert held(mod, lib, q([0, 1], [(0, c, 1, c) for c in range(5)])) is None
    # one binding, with and without predicates
    assert held(mod, lib, q([3], [])) == (0, [], [])
    assert held(mod, lib, q([3], [(0, 0, 0, 1)])) == (0, [], [0])


def test_which_switch_lets_a_query_in():
    tri = q([0, 1, 2], TRIANGLE)
    assert sm.how(tri) == 3 and sm.how(tri, keys=False) == 3 and sm.how(tri, self_=False) == 0
    both = q([0, 1], [(0, 0, 1, 0), (0, 1, 1, 1), (1, 2, 1, 1)])          # a two-key step and a one-binding predicate
    assert sm.how(both) == 3 and sm.how(both, keys=False) == 0
    assert sm.how(q([0, 1], [(0, 0, 1, 0)])) == 1 and sm.how(q([0, 1], [(0, 0, 1, 0), (0, 1, 1, 1)])) == 2
    assert sm.how(q([0], [])) == 3 and sm.how(q([0], []), self_=False) == 0


# every family of tests/query_shapes.py whose relations and numpy answers take well under a second here: the others ("join too
# large", "filter too large" with 4 194 305 rows, "equality too large" with 4.41 M pairs, the two "chunk cuts" of 4100 joins) are
# held to run_query by tests/test_gpu_query_fold_self.py, which computes the same model for all sixteen
SHAPE_FAMILIES = ("synthetic", "tiny", "descriptor limits", "no survivors", "empty relations", "empty only", "rerun all", "rerun none", "rerun mixed",
                  "4096 filters", "4097 filters")


@pytest.mark.parametrize("name", SHAPE_FAMILIES)
def test_the_route_against_the_numpy_executor(name):
    rels, queries, want = shapes.reference(name)[:3]
    info, fold, foldk, self_, answers = sm.folds_counts(rels, queries)
    for i, (query, a) in enumerate(zip(queries, answers)):
        assert (a is None) == ((name, i) in SHAPES_THAT_DO_NOT_FOLD), (name, i)
        if a is not None:
            assert (list(a[0]), a[1]) == (list(want[i][0]), want[i][1]), (name, i)
    if name == "4097 filters":                           # 4097 queries of one binding with a predicate on it: one call of 4097 items
        assert self_ == {"self_calls": 1, "self_items": 4097, "self_queries": 4097} and fold == {"fold_calls": 0, "fold_items": 0, "fold_queries": 4097}
        assert info == dict(levels=0, filter_calls=1, eq2_calls=0, join_calls=0, join_reruns=0, apply_calls=0)


def test_the_route_against_a_cross_product():
    rels, queries = sm.random_queries()
    kinds = [sm.how(query) for query in queries]
    assert kinds.count(3) >= 24 and kinds.count(0) >= 1 and sum(len(query[0]) == 1 for query in queries) >= 2
    assert sum(1 for query, k in zip(queries, kinds) if k == 3 and sm.folds_plan(query)[2] and len(query[0]) > 1) >= 6
    for query, k in zip(queries, kinds):
        assert sm.valid(query)
        steps = trace_query(rels, query)[3]
        assert all(s[3] < sm.RANDOM_LIMIT for s in steps), query         # no intermediate result left out for its size
        want = sm.product_answer(rels, query)
        got = run_query(rels, query)
        assert (list(got[0]), got[1]) == (want[0], want[1]), query
        if k:
            sums, rows = sm.folds_route(rels, query, None if k == 3 else km.foldk_plan(query), item=km.foldk_item, first=sm.self_item)[:2]
            assert (list(sums), rows) == (want[0], want[1]), query
            sums, rows = sm.folds_route(rels, query, None if k == 3 else km.foldk_plan(query))[:2]
            assert (list(sums), rows) == (want[0], want[1]), query


def test_the_infos_of_a_hand_made_batch():
    rels = sm.random_relations()
    tree = q([0, 1], [(0, 0, 1, 0)], [(0, 2), (1, 2)])                                   # folds anyway
    grouped = q([1, 2], [(0, 0, 1, 0), (0, 3, 1, 3)], [(0, 2)])                          # the keys switch
    leaf = q([0, 1, 2], [(0, 0, 1, 0), (2, 3, 2, 4), (1, 3, 2, 3)], [(0, 2), (2, 2)])    # a one-binding predicate on a leaf
    alone = q([0], [(0, 0, 0, 1), (0, 3, 0, 4)], [(0, 2), (0, 0)])                       # finished in the pre-round
    plain = q([1], [], [(0, 2)], [(0, 0, "<", 5)])                                       # no join, one filter: one item without a term
    dead = q([1, 2], [(0, 0, 0, 2), (0, 0, 1, 0)], [(0, 2)])                             # c0 = c2 never holds: dies in the pre-round
    cycle = q([1, 2, 3], [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3)], [(0, 2)])           # a true triangle: by levels
    batch = [tree, grouped, leaf, alone, plain, dead, cycle]
    info, fold, foldk, self_, answers = sm.folds_counts(rels, batch)
    assert [sm.how(x) for x in batch] == [1, 2, 3, 3, 3, 3, 0]
    assert self_ == {"self_calls": 1, "self_items": 4, "self_queries": 4}
    assert fold == {"fold_calls": 2, "fold_items": 3, "fold_queries": 6} and foldk == {"foldk_calls": 1, "foldk_items": 1, "foldk_queries": 1}
    assert info["levels"] == 3 and info["filter_calls"] == 1 and info["join_calls"] >= 2 and info["eq2_calls"] == 1
    assert answers[5] == ([0], 0) and answers[6] is None
    for x, a in zip(batch[:6], answers):
        w = run_query(rels, x)
        assert (list(a[0]), a[1]) == (list(w[0]), w[1])
    # with the new switch off the last four run by levels, and nothing else changes
    info0, fold0, foldk0, self0, answers0 = sm.folds_counts(rels, batch, self_=False)
    assert self0 == sm.NO_SELF and fold0["fold_queries"] == 2 and foldk0 == foldk and answers0[2:] == [None] * 5
    assert (info0, fold0, foldk0) == km.foldk_counts(rels, batch)[:3]
    # with the keys switch off the grouped query runs by levels too
    assert sm.folds_counts(rels, batch, keys=False)[1]["fold_queries"] == 5
