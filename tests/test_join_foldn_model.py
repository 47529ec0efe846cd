"""tests/join_foldn_model.py held to account without a device, and rhj_query_foldn_plan (a pure function) against it: foldn_item
against a double loop; the plan rule on the `small` workload, on every query of tests/query_shapes.py, on triangles, cycles,
parallel predicates and predicates on one binding; the route's model (levels by query_model.py's pair executor, then folds over
the merged nodes) against the numpy executor and, for small random queries, against a brute force by itertools.product; the
infos of a hand-made batch."""
import importlib
import itertools

import numpy as np
import pytest

import join_fold_model as fm
import join_foldk_model as km
import join_foldn_model as nm
import join_folds_model as sm
import query_shapes as shapes
from query_model import call_counts, parse_work, run_query, trace_query
from test_join_folds_model import SHAPE_FAMILIES, SHAPES_THAT_DO_NOT_FOLD

M64 = fm.M64
# the levels the five queries of tests/query_shapes.py that do not fold run before they hand over
SHAPE_LEVELS = {("synthetic", sorted(shapes.CASES).index("two nodes merge, then an equality")): 2,
                ("descriptor limits", 0): 6, ("descriptor limits", 1): 6, ("descriptor limits", 3): 11, ("tiny", 2): 1}
TRIANGLE = [(0, 0, 1, 0), (1, 1, 2, 1), (0, 2, 2, 2)]    # a true one: three column pairs
CYCLE4 = [(0, 0, 1, 0), (1, 1, 2, 1), (2, 2, 3, 2), (3, 3, 0, 3)]


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def lib(mod):
    return mod.load_library()


def q(rels, joins, views=((0, 2),), filters=()):
    return (list(rels), list(joins), list(filters), list(views))


def held(mod, lib, query, nrel=None):
    """the library's plan against the model's, and against rhj_query_folds_plan wherever that folds; returns the model's"""
    plan = nm.foldn_plan(query)
    assert mod.query_foldn_plan(lib, query, nrel) == plan, query
    before = sm.folds_plan(query)
    assert (plan[0] == 0) == (before is not None), query
    if before is not None:
        assert plan == (0, list(range(len(query[0]))), before[0], before[1], before[2]), query
        assert mod.query_folds_plan(lib, query, nrel) == before
    L, node, root, steps, selfs = plan
    assert L <= max(len(query[1]) - 1, 0) and root in node and all(node[n] == n for n in set(node))
    assert len(steps) == len(set(node)) - 1 and all(c in node and p in node and 1 <= len(idx) <= nm.MAX_KEYS for c, p, _, idx in steps)
    assert all(l >= L for l in selfs) and all(l >= L for s in steps for l in s[3])
    return plan


def test_foldn_item_against_a_double_loop():
    rng = np.random.default_rng(20186)
    big = np.array([0, 1, 1 << 63, M64, M64 - 1, 12345, 3], dtype=np.uint64)
    matched = own = 0
    for case in range(24):
        nR, nS, nk = int(rng.integers(1, 30)), int(rng.integers(1, 30)), 1 + case % 4
        pool = np.array([0, M64, 5], dtype=np.uint64)[:1 + case % 3]

        def side(n):
            cols = [rng.choice(pool, size=40) for _ in range(nk)]
            sels, last = [], None
            for t in range(nk):
                kind = int(rng.integers(0, 3))           # no vector, the previous word's, one of its own
                last = None if kind == 0 else last if kind == 1 and last is not None else rng.integers(0, 40, size=n).astype(np.uint64)
                sels.append(last)
            return cols, sels, n

        def some_factor(n):
            w = rng.choice(big, size=n) if rng.integers(0, 2) else None
            col = rng.choice(big, size=50) if rng.integers(0, 2) else None
            src = rng.integers(0, 50, size=n).astype(np.uint64) if col is not None and rng.integers(0, 2) else None
            return (w, src, col)
        R, S = side(nR), side(nS)
        values = [some_factor(nS) for _ in range(1 + case % 9)]
        outs = [(int(rng.integers(0, len(values))), some_factor(nR)) for _ in range(case % 10)] + [(0, (None, None, None))]
        want = nm.brute_force(R, S, values, outs)
        assert nm.foldn_item(R, S, values, outs) == want, case
        assert [(v.tolist(), t) for v, t in nm.foldn_item_np(R, S, values, outs)] == want, case
        matched += nm.foldn_item(R, S, [(None, None, None)], [(0, (None, None, None))])[0][1] > 0
        own += len({id(s) for s in R[1] if s is not None}) > 1
    assert matched >= 12 and own >= 6
    u = lambda *x: np.array(x, dtype=np.uint64)
    ones = (None, None, None)
    # word 1 of R has a vector of its own: read through word 0's vector (or through none) it is another row's value
    colsR, colsS = [u(1, 1, 1), u(7, 8, 9)], [u(1), u(9)]
    assert nm.foldn_item((colsR, [None, u(2, 2, 0)], 3), (colsS, [None, None], 1), [ones], [(0, ones)]) == [([1, 1, 0], 2)]
    assert nm.foldn_item((colsR, [None, None], 3), (colsS, [None, None], 1), [ones], [(0, ones)]) == [([0, 0, 1], 1)]
    # the same on the child side: its rows' values are summed under the tuple its own vectors give
    assert nm.foldn_item((colsS, [None, None], 1), (colsR, [u(0, 1, 2), u(2, 2, 2)], 3), [(u(10, 20, 30), None, None)], [(0, ones)]) == [([60], 60)]
    # every word through one vector: the tuple-key item on the gathered columns
    sel = u(2, 0)
    assert nm.foldn_item((colsR, [sel, sel], 2), (colsS, [None, None], 1), [ones], [(0, ones)]) == km.foldk_item([c[[2, 0]] for c in colsR], colsS, [ones], [(0, ones)])


def test_small_workload_every_query_folds_from_the_start(golden, mod, lib):
    queries = parse_work(golden.small["work_lines"])
    assert len(queries) == 50
    for query in queries:
        assert held(mod, lib, query, len(golden.small_relations))[0] == 0


def test_every_query_of_the_query_shapes(mod, lib):
    seen, handed = set(), {}
    for name in sorted(shapes.FAMILIES):
        _, queries = shapes.FAMILIES[name]()
        for i, query in enumerate(queries):
            shape = (tuple(query[0]), tuple(query[1]))
            if (name, i) not in SHAPES_THAT_DO_NOT_FOLD and shape in seen:
                continue                                 # (thousands of a family's queries differ in a filter's constant alone)
            seen.add(shape)
            plan = held(mod, lib, query)
            if plan[0]:
                handed[(name, i)] = plan[0]
    assert handed == SHAPE_LEVELS
    # two merged nodes and a two-word group whose words come through different vectors on both sides
    assert nm.foldn_plan(shapes.CASES["two nodes merge, then an equality"]) == (2, [0, 0, 2, 2], 0, [(2, 0, 0, [2, 3])], [])
    # one node, four inside equalities, no step
    plan = nm.foldn_plan(shapes.FAMILIES["descriptor limits"]()[1][3])
    assert plan[1] == [0] * 8 and plan[3] == [] and len(plan[4]) == 4


def test_triangles_in_all_six_orders_both_ways_round(mod, lib):
    flip = lambda p: (p[2], p[3], p[0], p[1])
    for order in itertools.permutations(range(3)):
        for flips in itertools.product((False, True), repeat=3):
            joins = [flip(TRIANGLE[k]) if f else TRIANGLE[k] for k, f in zip(order, flips)]
            L, node, root, steps, selfs = held(mod, lib, q([0, 1, 2], joins))
            assert L == 1 and selfs == [] and len(steps) == 1 and steps[0][3] == [1, 2], joins
            assert node[joins[0][2]] == node[joins[0][0]] == joins[0][0]          # B's node takes A's id


def test_cycles_chains_and_a_first_predicate_off_the_cycle(mod, lib):
    assert held(mod, lib, q([0, 1, 2, 3], CYCLE4)) == (2, [0, 0, 0, 3], 0, [(3, 0, 0, [2, 3])], [])
    # a triangle with a chain on it: the chain's predicates stay folds
    chain = [(2, 0, 3, 0), (3, 0, 4, 0), (4, 0, 5, 0)]
    L, node, root, steps, selfs = held(mod, lib, q([0, 1, 2, 3, 4, 5], TRIANGLE + chain))
    assert L == 1 and node == [0, 0, 2, 3, 4, 5] and selfs == [] and sorted(len(s[3]) for s in steps) == [1, 1, 1, 2]
    # the first predicate is off the cycle: it is merged anyway, and the triangle's first after it
    L, node, root, steps, selfs = held(mod, lib, q([0, 1, 2, 3], [(2, 0, 3, 0)] + TRIANGLE))
    assert L == 2 and node == [0, 0, 2, 2]
    # a 4-cycle closed by an implied predicate folds from the start
    implied = [(0, 0, 1, 0), (1, 0, 2, 0), (2, 0, 3, 0), (3, 0, 0, 0)]
    assert held(mod, lib, q([0, 1, 2, 3], implied))[0] == 0


def test_parallel_predicates_and_predicates_on_one_binding(mod, lib):
    par = lambda n: q([0, 1], [(0, c, 1, c) for c in range(n)])
    assert held(mod, lib, par(4)) == (0, [0, 1], 0, [(1, 0, 0, [0, 1, 2, 3])], [])
    assert held(mod, lib, par(5)) == (1, [0, 0], 0, [], [1, 2, 3, 4])
    assert held(mod, lib, par(6)) == (2, [0, 0], 0, [], [2, 3, 4, 5])
    one = lambda n: q([0], [(0, c, 0, c + 1) for c in range(n)])
    assert held(mod, lib, one(4))[0] == 0 and held(mod, lib, one(5)) == (1, [0], 0, [], [1, 2, 3, 4])
    assert held(mod, lib, one(9)) == (5, [0], 0, [], [5, 6, 7, 8])
    # no predicate, one binding
    assert held(mod, lib, q([3], [])) == (0, [0], 0, [], [])
    with pytest.raises(ValueError):
        mod.query_foldn_plan(lib, q([0, 1], []))           # a cross product: refused where rhj_query_levels refuses


@pytest.mark.parametrize("name", SHAPE_FAMILIES)
def test_the_route_against_the_numpy_executor(name):
    rels, queries, want = shapes.reference(name)[:3]
    info, fold, foldk, self_, nodes, answers = nm.foldn_counts(rels, queries)
    assert [(list(a[0]), a[1]) for a in answers] == [(list(s), r) for s, r in want]
    mine = {k: v for k, v in SHAPE_LEVELS.items() if k[0] == name}
    if not mine:                                         # nothing hands over: the three switches' counts
        assert nodes == nm.NO_NODES and (info, fold, foldk, self_) == sm.folds_counts(rels, queries)[:4]
    else:
        assert nodes["node_queries"] == len(mine) and nodes["node_levels"] == sum(mine.values())
        assert info["levels"] == max(mine.values())
    if name == "synthetic":                              # both sides' words come through different vectors: one foldn item
        assert nodes == {"foldn_calls": 1, "foldn_items": 1, "node_queries": 1, "node_levels": 2}


def test_the_route_against_a_cross_product():
    rels, queries = nm.random_queries()
    levels = [nm.foldn_plan(query)[0] for query in queries]
    assert len(queries) >= 48 and 2 * sum(1 for L in levels if L >= 1) >= len(queries)
    parked = foldn = lived = 0
    for query, L in zip(queries, levels):
        assert sm.valid(query)
        assert all(s[3] < nm.RANDOM_LIMIT for s in trace_query(rels, query)[3]), query
        want = sm.product_answer(rels, query)
        got = run_query(rels, query)
        assert (list(got[0]), got[1]) == (want[0], want[1]), query
        assert (L >= 1) == (sm.how(query) == 0)
        if L:
            for item, first in ((nm.foldn_item, sm.self_item), (nm.foldn_item_np, sm.self_item_np)):
                run = nm.foldn_route(rels, query, item=item, first=first)
                assert (run["sums"], run["rows"]) == (want[0], want[1]), query
            parked += run["parked"]
            foldn += sum(k[2] for k in run["rounds"].values())
            lived += run["rows"] > 0
            stays = nm.foldn_route(rels, query, node_rows=1)             # every merged node is too large: the levels to the end
            assert (stays["sums"], stays["rows"]) == (want[0], want[1]) and not stays["parked"]
    assert parked >= 16 and foldn >= 4 and lived >= 4


def test_the_infos_of_a_hand_made_batch():
    rels = nm.random_relations()
    tree = q([0, 1], [(0, 0, 1, 0)], [(0, 2), (1, 2)])                                   # folds from the start
    tri = q([1, 2, 3], TRIANGLE[:2] + [(0, 3, 2, 3)], [(0, 2), (2, 2)])                  # L 1; one foldk-shaped or foldn item
    cyc = q([1, 2, 3, 2], [(0, 0, 1, 0), (2, 0, 3, 0), (1, 1, 2, 1), (0, 3, 3, 3)], [(1, 2), (3, 2)])       # L 2: two merged nodes, a foldn item
    one = q([2, 3], [(0, c, 1, c) for c in (0, 1, 3)] + [(0, 0, 1, 1), (0, 1, 1, 3)], [(0, 2)])          # L 1: a single node, finished in the pre-round
    dead = q([1, 2, 3], [(0, 0, 1, 2)] + TRIANGLE[1:], [(0, 2)])                         # c0 = c2 never holds: dies in its prefix
    batch = [tree, tri, cyc, one, dead]
    assert [nm.foldn_plan(x)[0] for x in batch] == [0, 1, 2, 1, 1]
    info, fold, foldk, self_, nodes, answers = nm.foldn_counts(rels, batch)
    for x, a in zip(batch, answers):
        w = run_query(rels, x)
        assert (list(a[0]), a[1]) == (list(w[0]), w[1])
    assert answers[4] == ([0], 0) and answers[2][1] > 0 and answers[1][1] > 0
    assert nodes == {"foldn_calls": 1, "foldn_items": 2, "node_queries": 3, "node_levels": 4}
    assert info == dict(levels=2, filter_calls=0, eq2_calls=0, join_calls=2, join_reruns=info["join_reruns"], apply_calls=2)
    assert fold["fold_queries"] == 4 and self_["self_calls"] == 1 and self_["self_queries"] == 0
    # with every merged node too large all four hand-over queries run by levels to their end
    info1, fold1, foldk1, self1, nodes1, answers1 = nm.foldn_counts(rels, batch, node_rows=1)
    assert nodes1 == nm.NO_NODES and answers1 == answers and info1["levels"] == 5 and fold1["fold_queries"] == 1
    # level_info is query_model.call_counts on queries that run by levels
    others = [tri, cyc, one, dead]
    runs = [(trace_query(rels, x)[3], len(x[1])) for x in others]
    cut = [(s[:[k for k, t in enumerate(s) if t[3] == 0][0] + 1] if any(t[3] == 0 for t in s) else s, n) for s, n in runs]
    assert nm.level_info(cut) == call_counts(rels, others)[0]
