"""The fold route of rhj_query_batch_device (rhj_set_query_fold(1)) against an executor that shares none of
its choices: tests/fold_exact.py's exact_tree, rooted at binding 0, in unbounded Python integers, reduced modulo 2^64 here.
The families are those of tests/fold_families.py, and tests/test_fold_exact.py holds the executor and every family to account
without a device.  Every comparison is integer equality; the calls are those join_fold_model.fold_counts gives."""
import importlib

import numpy as np
import pytest

import fold_exact as fe
import fold_families as ff
import join_fold_model as fm

pytestmark = pytest.mark.gpu

M64 = fe.M64
NO_FOLDS = {"fold_calls": 0, "fold_items": 0, "fold_queries": 0}


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
    r.set_query_sum_last(False)
    r.lib.rhj_set_timing(2)
    r.lib.rhj_set_order(0)
    r.set_bits(4)


def device(rhj, relations):
    return [[rhj.torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint64).view(np.int64)).to(rhj.dev) for c in rel] for rel in relations]


def run(rhj, cols, queries, fold=True, sum_last=False):
    rhj.set_query_fold(fold)
    rhj.set_query_sum_last(sum_last)
    try:
        res, info = rhj.query_batch_device(cols, queries, with_info=True)
    finally:
        rhj.set_query_fold(False)
        rhj.set_query_sum_last(False)
    return [(list(s), r) for s, r in res], info


def folded(rhj, relations, cols, queries):
    """the answers of a batch on the fold route, its calls checked against the model's counts"""
    info_want, fold_want, _ = fm.fold_counts(relations, queries)
    res, info = run(rhj, cols, queries)
    assert info.fold_info == fold_want and dict(info) == info_want and info.sum_info == {"sum_calls": 0, "sum_items": 0}
    return res


@pytest.fixture(scope="module")
def random_cols(rhj):
    return device(rhj, ff.random_trees()[0])


def test_random_trees_on_three_routes(rhj, random_cols):
    relations, queries = ff.random_trees()
    want, dropped = ff.random_answers(), ff.random_dropped()
    assert len(queries) >= 200 and 10 * len(dropped) <= len(queries)
    got = folded(rhj, relations, random_cols, queries)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, queries[k])
    # the level route, and the level route that sums every last join without its pairs, on the queries whose levels stay small
    kept = [k for k in range(len(queries)) if k not in dropped]
    for sum_last in (False, True):
        got, info = run(rhj, random_cols, [queries[k] for k in kept], fold=False, sum_last=sum_last)
        for k, g in zip(kept, got):
            assert g == want[k], (k, sum_last, queries[k])
        assert info.fold_info == NO_FOLDS and (info.sum_info["sum_items"] > 0) == sum_last


def test_relabelled_trees_in_one_batch(rhj, random_cols):
    relations, queries = ff.random_trees()
    want = ff.random_answers()
    picked = ff.relabelled()
    batch = [other for _, others in picked for other, _, _ in others]
    assert len(batch) == 90
    got = iter(folded(rhj, relations, random_cols, batch))
    for k, others in picked:
        mine = [(fe.views_back(sums, order), rows) for (sums, rows), (_, order, _) in zip((next(got) for _ in others), others)]
        assert mine[0] == mine[1] == mine[2] == want[k], (k, queries[k])


def test_aimed_trees(rhj):
    ff.check_aimed()                                      # every tree does what it is named for, by the plan and the model
    relations, q = ff.aimed()
    cols = device(rhj, relations)
    names = list(q)
    want = ff.exact(relations, [q[n] for n in names])
    got = folded(rhj, relations, cols, [q[n] for n in names])
    for n, g, w in zip(names, got, want):
        assert g == w, n
    # one query finished in round 0 beside one that lives through round 2; then the one finished in round 1 beside it
    for n, items in (("finished in the first round", 2), ("finished in the second of three rounds", 3)):
        pair = [q[n], q["alive through three rounds"]]
        info_want, fold_want, _ = fm.fold_counts(relations, pair)
        assert fold_want == {"fold_calls": 3, "fold_items": items + 4, "fold_queries": 2}
        assert folded(rhj, relations, cols, pair) == [want[names.index(n)], want[names.index("alive through three rounds")]]
        assert want[names.index(n)] == ([0, 0, 0, 0], 0)


def test_trees_beyond_2_64(rhj):
    ff.check_beyond()
    relations, q = ff.beyond()
    cols = device(rhj, relations)
    queries = [q["a chain of four"], q["a subtotal in the middle"]]
    true = [fe.exact_tree(relations, query) for query in queries]
    assert true[0][1] == ff.BIG ** 4 >= 1 << 64 and true[0][1] & M64 and true[1][1] == ff.BIG ** 3
    want = [fe.modulo(t) for t in true]
    assert folded(rhj, relations, cols, queries) == want
    assert rhj.stats()["matches"] == sum(rows for _, rows in want) & M64
    for k, query in enumerate(queries):
        assert folded(rhj, relations, cols, [query]) == [want[k]]


def test_a_weight_total_of_2_64_is_taken_for_an_empty_result(rhj):
    """"treats a weight total that is 0 modulo 2^64 as an empty result".  One question, 2^63 rows, in two
    numberings.  Where the selective child is folded first the hub's weights are 1 and 0 and never total 0: the route answers.
    Where it is folded last the six children before it leave 2^63 + 2^63, and the route reports no row.  Lifting the limit
    turns the second assertion into the first."""
    ff.check_limit_star()
    relations, first, last, order = ff.limit_star()
    cols = device(rhj, relations)
    want = fe.modulo(fe.exact_tree(relations, first))
    assert want[1] == 1 << 63 and fe.modulo(fe.exact_tree(relations, last)) == ([want[0][v] for v in order], want[1])
    nothing = ([0] * len(last[3]), 0)
    assert folded(rhj, relations, cols, [first, last]) == [want, nothing]            # section 8's limit: `last` has 2^63 rows
    assert folded(rhj, relations, cols, [first]) == [want]
    assert folded(rhj, relations, cols, [last]) == [nothing]                         # section 8's limit


def test_more_items_in_a_round_than_a_chunk_takes(rhj):
    relations, queries = ff.chunked()
    cols = device(rhj, relations)
    want = ff.exact(relations, queries)
    info_want, fold_want, _ = fm.fold_counts(relations, queries)
    assert fold_want == {"fold_calls": 1, "fold_items": 4097, "fold_queries": 4097}
    got = folded(rhj, relations, cols, queries)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, queries[k])
    for k in (0, 4095, 4096):
        assert folded(rhj, relations, cols, [queries[k]]) == [want[k]], k


def test_round_buffers_grow_and_serve_a_smaller_call(rhj, random_cols):
    relations, small, at = ff.small_batch()
    want = [ff.random_answers()[k] for k in at]
    big_relations, big = ff.grown()
    big_cols = device(rhj, big_relations)
    big_want = fe.modulo(fe.exact_tree(big_relations, big))
    assert folded(rhj, relations, random_cols, small) == want
    assert folded(rhj, big_relations, big_cols, [big]) == [big_want]
    assert folded(rhj, relations, random_cols, small) == want
    rhj.lib.rhj_release()
    rhj.torch.cuda.synchronize()
    assert folded(rhj, relations, random_cols, small) == want
    assert folded(rhj, big_relations, big_cols, [big]) == [big_want]
