"""rhj_query_batch_device with rhj_set_query_fold(1), rhj_set_query_fold_keys(1) and rhj_set_query_fold_self(1)
(include/rhj_inter.h): the queries with one-binding predicates, with implied predicates and without a join fold too, after one
rhj_fold_self_batch_device call before round 0.  The answers are the `small` workload's recorded result lines, the numpy executor
of query_model.py, a brute force by itertools.product and a closed form; the calls are those join_folds_model.folds_counts gives.
Every comparison is an integer equality."""
import importlib

import numpy as np
import pytest

import join_folds_model as sm
import query_shapes as shapes
from query_model import call_counts, parse_work, run_query

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
B63 = 1 << 63
NO_FOLD = {"fold_calls": 0, "fold_items": 0, "fold_queries": 0}
NO_FOLDK = {"foldk_calls": 0, "foldk_items": 0, "foldk_queries": 0}
NO_LEVELS = dict(levels=0, filter_calls=0, eq2_calls=0, join_calls=0, join_reruns=0, apply_calls=0)


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
    r.set_query_fold_self(False)
    r.set_query_sum_last(False)
    r.lib.rhj_set_timing(2)
    r.lib.rhj_set_order(0)
    r.set_bits(4)


def dev(rhj, a):
    return rhj.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


def to_device(rhj, rels, prefix=None):
    cols = []
    for r, rel in enumerate(rels):
        if prefix and r in prefix:
            src, n = prefix[r]
            cols.append([t[:n] for t in cols[src]])
        else:
            cols.append([dev(rhj, c) for c in rel])
    return cols


def run(rhj, cols, queries, fold=True, keys=True, self_=True):
    rhj.set_query_fold(fold)
    rhj.set_query_fold_keys(keys)
    rhj.set_query_fold_self(self_)
    try:
        return rhj.query_batch_device(cols, queries, with_info=True)
    finally:
        rhj.set_query_fold(False)
        rhj.set_query_fold_keys(False)
        rhj.set_query_fold_self(False)


def answers(res):
    return [(list(s), r) for s, r in res]


def infos(info):
    return dict(info), info.fold_info, info.foldk_info, info.fold_self_info


def held(rhj, rels, cols, queries, want, keys=True):
    """one batch on the new route: the answers, and the four infos against the model; returns the model's infos"""
    model = sm.folds_counts(rels, queries, keys=keys)
    for a, w in zip(model[4], want):
        assert a is None or (list(a[0]), a[1]) == w
    res, info = run(rhj, cols, queries, keys=keys)
    assert answers(res) == want
    assert infos(info) == model[:4]
    return model[:4]


def q(rels, joins, views=((0, 2),), filters=()):
    return (list(rels), list(joins), list(filters), list(views))


def test_small_workload_with_all_three_switches_on(rhj, golden):
    rels = golden.small_relations
    relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    cols = to_device(rhj, relations)
    queries = parse_work(golden.small["work_lines"])
    lines_of = lambda res: [" ".join("NULL" if rows == 0 else str(s) for s in sums_) for sums_, rows in res]
    rhj.lib.rhj_set_order(1)                             # order mode "any"
    try:
        two, info2 = run(rhj, cols, queries, self_=False)
        three, info3 = run(rhj, cols, queries)
    finally:
        rhj.lib.rhj_set_order(0)
    assert lines_of(three) == golden.small["result_lines"] == lines_of(two)
    assert info3.fold_info == info2.fold_info and info3.foldk_info == info2.foldk_info and dict(info3) == dict(info2)
    assert all(sm.how(x, self_=False) for x in queries)  # all 50 fold without the new switch; 45 of them are alive after the filters
    assert info3.fold_info["fold_queries"] == 45 and info3.fold_self_info == sm.NO_SELF == info2.fold_self_info


@pytest.mark.parametrize("name", sorted(shapes.FAMILIES))
def test_the_queries_of_the_query_shapes(rhj, name):
    rels, queries, want = shapes.reference(name)[:3]
    cols = to_device(rhj, rels, shapes.B1_PREFIX if name == "filter too large" else None)
    info, fold, foldk, self_ = held(rhj, rels, cols, queries, [(list(s), r) for s, r in want])
    before = call_counts(rels, queries)[0]
    assert info["levels"] <= before["levels"] and info["eq2_calls"] <= before["eq2_calls"]
    if name == "synthetic":
        assert self_ == {"self_calls": 1, "self_items": 8, "self_queries": 8} and info["levels"] == 4


@pytest.fixture(scope="module")
def random_batch(rhj):
    rels, queries = sm.random_queries()
    return rels, to_device(rhj, rels), queries, [sm.product_answer(rels, x) for x in queries]


def test_random_queries_on_the_new_route(rhj, random_batch):
    rels, cols, queries, want = random_batch
    want = [(list(s), r) for s, r in want]
    info, fold, foldk, self_ = held(rhj, rels, cols, queries, want)
    assert self_["self_calls"] == 1 and self_["self_items"] >= 20 and self_["self_queries"] >= 24
    # each query alone: its own pre-round and rounds
    for x, w in zip(queries[:12], want):
        held(rhj, rels, cols, [x], [w])


def test_random_queries_on_the_level_route(rhj, random_batch):
    rels, cols, queries, want = random_batch
    res, info = run(rhj, cols, queries, fold=False)
    assert answers(res) == [(list(s), r) for s, r in want]
    assert infos(info) == (call_counts(rels, queries)[0], NO_FOLD, NO_FOLDK, sm.NO_SELF)


def chain_relations():
    """relation 0: 3000 rows, c0 = 5 in every row, c1 = 5 in the first 1500 rows and 6 in the others, c2 unique and near 2^63;
    relations 1..3: small ones with keys of a few values in c0, c1, c3 and unique values in c2"""
    rng = np.random.default_rng(20188)
    n = 3000
    rels = [[np.full(n, 5, dtype=np.uint64), np.where(np.arange(n) < 1500, 5, 6).astype(np.uint64), rng.permutation(n).astype(np.uint64) + np.uint64(B63),
             np.full(n, 5, dtype=np.uint64)]]
    for r, rows in enumerate((60, 45, 30), start=1):
        c0 = rng.integers(0, 4, size=rows).astype(np.uint64)
        c1 = np.where(rng.integers(0, 2, size=rows) == 1, c0, rng.integers(0, 4, size=rows)).astype(np.uint64)
        rels.append([c0, c1, rng.permutation(rows).astype(np.uint64) + np.uint64(B63 + (r << 20)), rng.integers(0, 2, size=rows).astype(np.uint64)])
    return rels


@pytest.fixture(scope="module")
def chains(rhj):
    rels = chain_relations()
    return rels, to_device(rhj, rels)


def test_implied_and_true_triangles(rhj, chains):
    rels, cols = chains
    implied = q([1, 2, 3], [(0, 1, 1, 0), (1, 0, 2, 1), (0, 1, 2, 1)], [(0, 2), (2, 2)])
    true = q([1, 2, 3], [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3)], [(0, 2), (2, 2)])
    want = [(list(s), r) for s, r in (run_query(rels, x) for x in (implied, true))]
    assert want[0][1] > 0 and want[1][1] > 0
    info, fold, foldk, self_ = held(rhj, rels, cols, [implied], want[:1])
    assert info == NO_LEVELS and self_ == {"self_calls": 0, "self_items": 0, "self_queries": 1} and fold == {"fold_calls": 2, "fold_items": 2, "fold_queries": 1}
    info, fold, foldk, self_ = held(rhj, rels, cols, [true], want[1:])
    assert info["levels"] == 3 and self_ == sm.NO_SELF and fold == NO_FOLD
    # with the new switch off the implied triangle runs by levels, as before
    res, info = run(rhj, cols, [implied], self_=False)
    assert answers(res) == want[:1] and dict(info)["levels"] == 3 and info.fold_self_info == sm.NO_SELF and info.fold_info == NO_FOLD


def test_a_one_binding_predicate_anywhere_in_the_tree(rhj, chains):
    rels, cols = chains
    tree = [(0, 0, 1, 0), (1, 1, 2, 1)]                  # a chain of three: the plan's root is binding 0, binding 1 inner, binding 2 a leaf
    views = [(0, 2), (1, 2), (2, 2)]
    assert sm.folds_plan(q([1, 2, 3], tree))[:2] == (0, [(2, 1, 0, [1]), (1, 0, 1, [0])])
    queries = [q([1, 2, 3], tree + [(b, 0, b, 1)], views) for b in (0, 1, 2)]
    queries += [q([1, 2, 3], [(2, 0, 2, 1)] + tree + [(0, 1, 0, 0), (1, 0, 1, 1), (1, 3, 1, 0)], views),      # everywhere, and two on the inner one
                q([1, 1, 1], tree + [(1, 0, 1, 1)], views),                                                  # on a relation bound three times
                q([2, 2], [(0, 0, 1, 0), (1, 0, 1, 1)], views[:2], [(1, 3, "=", 1)])]                          # bound twice, through a filter's hit list
    want = [(list(s), r) for s, r in (run_query(rels, x) for x in queries)]
    assert all(r > 0 for _, r in want)
    info, fold, foldk, self_ = held(rhj, rels, cols, queries, want)
    assert info == dict(NO_LEVELS, filter_calls=1) and self_ == {"self_calls": 1, "self_items": 8, "self_queries": 6}


def test_one_query_dies_in_the_pre_round_beside_one_alive_through_round_2(rhj, chains):
    rels, cols = chains
    star = q([1, 2, 3, 1], [(0, 0, 1, 0), (0, 0, 2, 0), (0, 1, 3, 1), (2, 0, 2, 1)], [(0, 2), (3, 2), (2, 2)])
    dead = q([2, 0], [(0, 0, 1, 0), (1, 2, 1, 1)], [(0, 2), (1, 2)])         # c2 is near 2^63, c1 is 5 or 6: no row passes
    assert max(s[2] for s in sm.folds_plan(star)[1]) == 2
    want = [(list(s), r) for s, r in (run_query(rels, x) for x in (dead, star))]
    assert want[0] == ([0, 0], 0) and want[1][1] > 0
    info, fold, foldk, self_ = held(rhj, rels, cols, [dead, star], want)
    assert self_ == {"self_calls": 1, "self_items": 2, "self_queries": 2} and fold == {"fold_calls": 3, "fold_items": 3, "fold_queries": 2}


def test_a_query_without_a_join_with_eight_views_and_four_filters(rhj, chains):
    rels, cols = chains
    views = [(0, c % 4) for c in range(8)]
    filters = [(0, 2, ">", B63 + 100), (0, 2, "<", B63 + 2900), (0, 0, "=", 5), (0, 1, "<", 7)]
    queries = [q([0], [], views, filters), q([0], [(0, 0, 0, 1)], views, filters), q([0], [(0, 0, 0, 1), (0, 3, 0, 0), (0, 1, 0, 3)], views[:1])]
    want = [(list(s), r) for s, r in (run_query(rels, x) for x in queries)]
    assert want[0][1] == 2799 and 0 < want[1][1] < 2799 and want[2][1] == 1500
    info, fold, foldk, self_ = held(rhj, rels, cols, queries, want)
    assert info == dict(NO_LEVELS, filter_calls=1) and fold == {"fold_calls": 0, "fold_items": 0, "fold_queries": 3}
    assert self_ == {"self_calls": 1, "self_items": 3, "self_queries": 3}


def test_the_chain_of_four_3000_row_bindings_against_the_closed_form(rhj, chains):
    """3000^3 * 1500 rows: c0 = c1 on an inner binding, which its first 1500 rows pass"""
    rels, cols = chains
    c2 = rels[0][2]
    huge = q([0, 0, 0, 0], [(0, 0, 1, 0), (1, 0, 2, 0), (1, 0, 1, 1), (2, 0, 3, 0)], [(0, 2), (1, 2), (3, 2)])
    rows = 3000 ** 3 * 1500
    whole, half = int(c2.sum(dtype=np.uint64)), int(c2[:1500].sum(dtype=np.uint64))
    want = ([whole * 3000 ** 2 * 1500 & M64, half * 3000 ** 3 & M64, whole * 3000 ** 2 * 1500 & M64], rows)
    assert rows == 40500000000000 and sm.folds_route(rels, huge)[:2] == want
    res, info = run(rhj, cols, [huge])
    assert answers(res) == [want]
    assert info.fold_self_info == {"self_calls": 1, "self_items": 1, "self_queries": 1} and dict(info) == NO_LEVELS
    assert rhj.stats()["matches"] == rows


def test_a_one_binding_predicate_with_a_two_key_step(rhj, chains):
    rels, cols = chains
    both = q([1, 2, 3], [(0, 0, 1, 0), (0, 1, 1, 1), (1, 0, 1, 1), (1, 3, 2, 3)], [(0, 2), (2, 2)])
    want = [(list(s), r) for s, r in [run_query(rels, both)]]
    assert want[0][1] > 0
    info, fold, foldk, self_ = held(rhj, rels, cols, [both], want)
    assert info == NO_LEVELS and foldk["foldk_items"] == 1 and foldk["foldk_queries"] == 0 and self_["self_queries"] == 1
    info, fold, foldk, self_ = held(rhj, rels, cols, [both], want, keys=False)
    assert info["levels"] == 4 and fold == NO_FOLD and foldk == NO_FOLDK and self_ == sm.NO_SELF


def test_state(rhj, chains):
    rels, cols = chains
    queries = [q([1, 2], [(0, 0, 1, 0), (1, 0, 1, 1)], [(0, 2), (1, 2)]), q([3], [(0, 0, 0, 1)], [(0, 2)]), q([0], [], [(0, 2)], [(0, 2, "<", B63 + 10)])]
    want = [(list(s), r) for s, r in (run_query(rels, x) for x in queries)]
    # the new switch on with the fold route off: today's counts
    res, info = run(rhj, cols, queries, fold=False)
    assert answers(res) == want and infos(info) == (call_counts(rels, queries)[0], NO_FOLD, NO_FOLDK, sm.NO_SELF)
    on = held(rhj, rels, cols, queries, want)
    assert on[3] == {"self_calls": 1, "self_items": 3, "self_queries": 3}
    # the switch off again
    res, info = run(rhj, cols, queries, self_=False)
    assert answers(res) == want and infos(info) == sm.folds_counts(rels, queries, self_=False)[:4] and info.fold_self_info == sm.NO_SELF
    # rhj_release() between two calls: the weight vectors' buffer goes and comes back
    rhj.lib.rhj_release()
    rhj.torch.cuda.synchronize()
    assert held(rhj, rels, cols, queries, want) == on
