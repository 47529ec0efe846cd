"""tests/fold_exact.py held to account without a device, and the families of tests/fold_families.py held to what they are named
for: exact_tree against itertools.product, against the numpy pair executor of query_model.py and under relabelling; the model
of the fold route (join_fold_model.fold_route) against exact_tree on every query tests/test_gpu_query_fold_edges.py runs; and
the conditions the generated families must meet, so that another seed cannot hollow them out."""
import numpy as np

import fold_exact as fe
import fold_families as ff
import join_fold_model as fm
from query_model import parse_work, run_query
from query_shapes import CASES, synthetic_relations

M64 = fe.M64


def route(relations, query):
    sums, rows, _ = fm.fold_route(relations, query)
    return list(sums), rows


def test_exact_tree_against_the_product_of_all_rows():
    rng = np.random.default_rng(4140)
    relations = fe.random_relations(rng, (1, 2, 3, 5, 8, 13, 20), spread=(0.15, 0.6))
    done, alive, counts = 0, 0, set()
    for k in range(630):
        q = fe.random_tree_query(rng, relations, 2 + k % 7)
        if np.prod([float(len(r)) for r in fe.filtered_rows(relations, q)]) > 200000:
            continue
        want = fe.brute(relations, q)
        assert fe.exact_tree(relations, q) == want, q
        if k % 4 == 0:                                    # and under another numbering, with the sides swapped
            other, order = fe.relabel(q, rng.permutation(len(q[0])).tolist(), rng)
            sums, rows = fe.exact_tree(relations, other)
            assert (fe.views_back(sums, order), rows) == want, (q, other)
        done, alive = done + 1, alive + (want[1] > 0)
        counts.add(len(q[0]))
    assert done >= 300 and alive >= 100 and counts == set(range(2, 9))


def test_exact_tree_against_the_pair_executor_on_the_small_workload(golden):
    rels = golden.small_relations
    relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    folding = [q for q in parse_work(golden.small["work_lines"]) if fm.folds(q)]
    assert len(folding) >= 40
    for q in folding:
        sums, rows = run_query(relations, q)
        assert fe.modulo(fe.exact_tree(relations, q)) == (list(sums), rows), q


def test_exact_tree_against_the_pair_executor_on_the_synthetic_queries():
    relations = synthetic_relations()
    folding = [k for k in sorted(CASES) if fm.folds(CASES[k])]
    assert len(folding) >= 12
    for k in folding:
        sums, rows = run_query(relations, CASES[k])
        assert fe.modulo(fe.exact_tree(relations, CASES[k])) == (list(sums), rows), k


def test_relabel_asks_the_same_question():
    q = ([3, 4, 5], [(0, 1, 1, 0), (2, 0, 1, 1)], [(0, 2, "<", 9), (2, 3, "=", 1)], [(2, 4), (0, 0), (1, 1)])
    assert fe.relabel(q, [2, 0, 1]) == (([4, 5, 3], [(2, 1, 0, 0), (1, 0, 0, 1)], [(2, 2, "<", 9), (1, 3, "=", 1)], [(1, 4), (2, 0), (0, 1)]), [0, 1, 2])
    assert fe.views_back([10, 11, 12], [2, 0, 1]) == [11, 12, 10]
    rng = np.random.default_rng(1)
    other, order = fe.relabel(q, [1, 2, 0], rng)
    assert other[0] == [5, 3, 4] and sorted(order) == [0, 1, 2] and [other[3][k] for k in range(3)] == [([1, 2, 0][q[3][v][0]], q[3][v][1]) for v in order]
    assert sorted((a, ca, b, cb) if a < b else (b, cb, a, ca) for a, ca, b, cb in other[1]) == [(0, 0, 2, 1), (1, 1, 2, 0)]
    assert sorted(other[2]) == [(0, 3, "=", 1), (1, 2, "<", 9)]


# ---- the device families --------------------------------------------------------------------------------------------------------------

def test_the_random_trees_are_what_the_device_tests_need():
    relations, queries = ff.random_trees()
    answers = ff.random_answers()
    assert len(queries) >= 200 and all(fm.folds(q) for q in queries)
    assert {len(q[0]) for q in queries} == set(range(2, 9))
    assert 3 * sum(rows > 0 for _, rows in answers) >= len(queries)
    zero = [(ff.zero_round(relations, q), ff.rounds(q)) for q in queries]
    assert sum(1 for z, r in zero if z is not None and 0 < z < r - 1) >= 10
    assert sum(1 for q in queries if max(ff.depths(q)[b] for b, _ in q[3]) >= 3) >= 20     # a view carried through two or more further folds
    assert sum(1 for q in queries if all(ff.child_first(q))) >= 20
    assert sum(1 for q in queries if any(0 in a and 0 in b for a, b in ff.sides(relations, q))) >= 5
    # what the generator promises: chains and stars, both ways of writing a predicate, relations bound twice, one to eight
    # views on leaves, inner bindings and the root, repeated views, up to four filters on a binding, sides of one row and of
    # the tile edges, keys 0 and 2^64 - 1
    sizes = {len(r) for q in queries for r in fe.filtered_rows(relations, q)}
    assert {1} | set(fe.EDGE_ROWS) <= sizes and max(sizes) == 2100
    degree = lambda q: max(sum(b in (j[0], j[2]) for j in q[1]) for b in range(len(q[0])))
    assert any(degree(q) == 7 for q in queries) and any(degree(q) == 2 and len(q[0]) == 8 for q in queries)
    assert any(not any(ff.child_first(q)) for q in queries if len(q[0]) >= 3) and any(len(set(ff.child_first(q))) == 2 for q in queries)
    assert any(len(set(q[0])) < len(q[0]) for q in queries) and {len(q[3]) for q in queries} == set(range(1, 9))
    assert any(len(set(q[3])) < len(q[3]) for q in queries)
    where = {("root" if d == 0 else "leaf" if b not in ff.parents(q)[1].values() else "inner") for q in queries for b, _ in q[3] for d in [ff.depths(q)[b]]}
    assert where == {"root", "leaf", "inner"}
    assert max(sum(f[0] == b for f in q[2]) for q in queries for b in range(len(q[0]))) == 4
    assert all(0 in c and M64 in c for rel in relations if len(rel[0]) >= 4 for c in (rel[0].tolist(), rel[1].tolist()))
    assert all(int(rel[c].max()) > 1 << 63 and int(rel[c].min()) < 1 << 61 for rel in relations if len(rel[0]) >= 63 for c in (2, 3, 4))


def test_the_random_trees_against_the_pair_executor_and_the_route():
    relations, queries = ff.random_trees()
    dropped = ff.random_dropped()
    assert 10 * len(dropped) <= len(queries)
    for k, (q, want) in enumerate(zip(queries, ff.random_answers())):
        assert route(relations, q) == want, k
        if k not in dropped:
            sums, rows = run_query(relations, q)
            assert (list(sums), rows) == want, k


def test_the_relabelled_trees():
    relations, queries = ff.random_trees()
    answers = ff.random_answers()
    picked = ff.relabelled()
    assert len(picked) == 30 and sum(answers[k][1] > 0 for k, _ in picked) == 20
    for k, others in picked:
        assert len(others) == 3
        for other, order, perm in others:
            assert fm.folds(other)
            sums, rows = fe.modulo(fe.exact_tree(relations, other))
            assert (fe.views_back(sums, order), rows) == answers[k], (k, other)
            sums, rows = route(relations, other)
            assert (fe.views_back(sums, order), rows) == answers[k], (k, other)
    # the numberings differ in what the route does with them: another binding as the root, other ways round a predicate
    assert sum(1 for k, others in picked if len({perm.index(ff.parents(o)[0]) for o, _, perm in others}) > 1) >= 10
    assert sum(1 for k, others in picked if len({tuple(ff.child_first(o)) for o, _, _ in others}) > 1) >= 10


def test_the_aimed_trees():
    ff.check_aimed()
    relations, q = ff.aimed()
    for name, query in q.items():
        assert route(relations, query) == fe.modulo(fe.exact_tree(relations, query)), name


def test_the_trees_beyond_2_64():
    ff.check_beyond()
    relations, q = ff.beyond()
    for name, query in q.items():
        assert route(relations, query) == fe.modulo(fe.exact_tree(relations, query)), name


def test_the_star_whose_weights_total_2_64():
    """the route takes a weight total that is 0 modulo 2^64 for an empty result.  The same question has 2^63 rows
    in both numberings; the route says so where the selective child is folded first and says 0 where it is folded last."""
    ff.check_limit_star()
    relations, first, last, order = ff.limit_star()
    want = fe.modulo(fe.exact_tree(relations, first))
    assert want[1] == 1 << 63 and any(want[0])
    sums, rows = fe.modulo(fe.exact_tree(relations, last))
    assert (fe.views_back(sums, order), rows) == want
    assert route(relations, first) == want
    assert route(relations, last) == ([0] * len(last[3]), 0)                        # the limit: the hub's weights are 2^63 + 2^63 before the last fold
    assert fm.fold_route(relations, last)[2] == {r: 1 for r in range(6)} and fm.fold_route(relations, first)[2] == {r: 1 for r in range(7)}


def test_the_chunked_and_the_grown_family():
    relations, queries = ff.chunked()
    assert len(queries) == ff.CHUNK_ITEMS + 1 and all(fm.folds(q) and len(q[0]) == 2 for q in queries)
    assert all(len(rel[0]) == 8 for rel in relations)
    alive = 0
    for k, q in enumerate(queries):
        assert all(fe.filtered_rows(relations, q)), k     # no filter finishes one: every query is an item of round 0
        want = fe.modulo(fe.exact_tree(relations, q))
        assert route(relations, q) == want, k
        alive += want[1] > 0
    assert alive >= 2000 and alive < len(queries)
    assert {ff.child_first(q)[0] for q in queries} == {False, True}
    relations, query = ff.grown()
    assert [len(relations[r][0]) for r in query[0]] == [50000] * 3 and len(query[3]) == 4
    want = fe.modulo(fe.exact_tree(relations, query))
    assert route(relations, query) == want and want[1] > 50000
    assert sorted(ff.depths(query)[b] for b, _ in query[3]) == [0, 1, 2, 2]        # two carried vectors beside the weights in round 0's buffer
    relations, small, at = ff.small_batch()
    assert {len(q[0]) for q in small} == set(range(2, 9)) and max(ff.rounds(q) for q in small) >= 3
