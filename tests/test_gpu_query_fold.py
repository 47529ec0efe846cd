"""rhj_query_batch_device with rhj_set_query_fold(1) (include/rhj_inter.h): the queries whose predicates are a tree over their
bindings run by rounds of rhj_join_fold_batch_device items and take no pair buffer at any level.  The answers are those of the
switch-off route (the `small` workload's recorded result lines, the numpy executor of query_model.py) wherever that route can
answer, and the model of join_fold_model.py beyond; the calls are those join_fold_model.fold_counts gives."""
import importlib

import numpy as np
import pytest

import join_fold_model as fm
from query_model import call_counts, parse_work, run_query
from query_shapes import B63, CASES, synthetic_relations

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
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


def dev(rhj, a):
    return rhj.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


def run(rhj, cols, queries, fold=True, sum_last=False):
    rhj.set_query_fold(fold)
    rhj.set_query_sum_last(sum_last)
    try:
        return rhj.query_batch_device(cols, queries, with_info=True)
    finally:
        rhj.set_query_fold(False)
        rhj.set_query_sum_last(False)


def answers(res):
    return [(list(s), r) for s, r in res]


@pytest.fixture(scope="module")
def synthetic(rhj):
    relations = synthetic_relations()
    names = sorted(CASES)
    return {"relations": relations, "cols": [[dev(rhj, c) for c in rel] for rel in relations], "names": names, "queries": [CASES[k] for k in names],
            "want": [(list(s), r) for s, r in (run_query(relations, CASES[k]) for k in names)]}


@pytest.mark.parametrize("order", ("4 bits", "any"))
def test_small_workload_with_the_switch_on(rhj, golden, order):
    rels = golden.small_relations
    relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    cols = [[dev(rhj, c) for c in rel] for rel in relations]
    queries = parse_work(golden.small["work_lines"])
    assert len(queries) == 50
    info_want, fold_want, _ = fm.fold_counts(relations, queries)
    rhj.set_bits(4)
    rhj.lib.rhj_set_order(1 if order == "any" else 0)
    try:
        res, info = run(rhj, cols, queries)
    finally:
        rhj.lib.rhj_set_order(0)
    lines = [" ".join("NULL" if rows == 0 else str(s) for s in sums_) for sums_, rows in res]
    assert lines == golden.small["result_lines"]
    assert info.fold_info == fold_want and fold_want["fold_queries"] >= 25 and fold_want["fold_calls"] <= 4      # (most of the workload folds; an empty filter finishes some before)
    assert dict(info) == info_want and info.sum_info == {"sum_calls": 0, "sum_items": 0}
    st = rhj.stats()
    assert st["path"] == "query_batch" and st["n_r"] == 50 and st["matches"] == sum(rows for _, rows in res) and st["ms_total"] > 0


def test_synthetic_queries_with_the_switch_on(rhj, synthetic):
    info_want, fold_want, folded = fm.fold_counts(synthetic["relations"], synthetic["queries"])
    res, info = run(rhj, synthetic["cols"], synthetic["queries"])
    for k, got, want, f in zip(synthetic["names"], answers(res), synthetic["want"], folded):
        assert got == want and (f is None or (list(f[0]), f[1]) == want), k
    assert info.fold_info == fold_want and dict(info) == info_want
    assert fold_want["fold_queries"] >= 10 and fold_want["fold_calls"] >= 4         # (the chain of eight bindings takes four rounds)
    # a folding query that an empty filter finishes sits next to live ones and issues no item
    k = synthetic["names"].index("a filter without a hit")
    assert fm.folds(synthetic["queries"][k]) and folded[k] == ([0], 0)
    # a fold whose total is 0 in the first of two rounds, and one in the last
    first, last = (synthetic["names"].index("no match at the %s level" % x) for x in ("last", "first"))
    assert fm.fold_route(synthetic["relations"], synthetic["queries"][first])[2] == {0: 1} and len(synthetic["queries"][first][1]) == 2
    assert fm.fold_route(synthetic["relations"], synthetic["queries"][last])[2] == {0: 1, 1: 1} and folded[last] == ([0, 0], 0)
    # each folding query alone
    for k, q in enumerate(synthetic["queries"]):
        if folded[k] is not None:
            one, info1 = run(rhj, synthetic["cols"], [q])
            assert answers(one) == [synthetic["want"][k]], synthetic["names"][k]
            assert info1.fold_info == fm.fold_counts(synthetic["relations"], [q])[1]


def test_the_switch_off_is_the_parent(rhj, synthetic):
    """after calls with the switch on: the answers and the info of the level route, and no fold"""
    run(rhj, synthetic["cols"], synthetic["queries"][:8])
    res, info = run(rhj, synthetic["cols"], synthetic["queries"], fold=False)
    assert answers(res) == synthetic["want"]
    assert dict(info) == call_counts(synthetic["relations"], synthetic["queries"])[0]
    assert info.fold_info == NO_FOLDS and info.sum_info == {"sum_calls": 0, "sum_items": 0}


def test_folding_and_other_queries_mixed(rhj, synthetic):
    relations, cols = synthetic["relations"], synthetic["cols"]
    picked = ["a self-join last", "no filter", "eight bindings in a chain", "no join and no filter", "two predicates between two bindings",
              "five bindings, four levels", "a filter without a hit", "fan-out on the large relation", "a self-join first"]
    queries = [CASES[k] for k in picked]
    want = [(list(s), r) for s, r in (run_query(relations, q) for q in queries)]
    info_want, fold_want, _ = fm.fold_counts(relations, queries)
    assert fold_want["fold_queries"] == 4 and info_want["levels"] == 2
    res, info = run(rhj, cols, queries)
    assert answers(res) == want and info.fold_info == fold_want and dict(info) == info_want
    # the other switch on as well: the folding queries are no sum items, the others' last joins are
    res, info = run(rhj, cols, queries, sum_last=True)
    assert answers(res) == want and info.fold_info == fold_want
    assert info.sum_info == {"sum_calls": 1, "sum_items": 1}                         # "a self-join first" ends in a join; the three others in equalities or nothing
    assert info["filter_calls"] == info_want["filter_calls"] and info["eq2_calls"] == info_want["eq2_calls"]
    # two calls back to back, and one after rhj_release()
    assert answers(run(rhj, cols, queries)[0]) == want
    rhj.lib.rhj_release()
    rhj.torch.cuda.synchronize()
    res, info = run(rhj, cols, queries)
    assert answers(res) == want and info.fold_info == fold_want and dict(info) == info_want


def hand_made():
    """relations 0..3 of 3000 rows with one key in c0 (values in c1, c2); relation 4 of 300 rows with a unique key in c0 and a
    second unique key in c3; relation 5 of 40 rows with keys 0..9"""
    rng = np.random.default_rng(77)
    rels = []
    for r in range(4):
        n = 3000
        rels.append([np.full(n, 7, dtype=np.uint64), rng.permutation(n).astype(np.uint64) + np.uint64(B63), rng.integers(0, 1 << 62, size=n).astype(np.uint64)])
    n = 300
    rels.append([np.arange(n, dtype=np.uint64), rng.permutation(n).astype(np.uint64) + np.uint64(B63), rng.integers(0, 9, size=n).astype(np.uint64),
                 rng.permutation(n).astype(np.uint64)])
    rels.append([(np.arange(40) % 10).astype(np.uint64), rng.integers(0, 1 << 63, size=40).astype(np.uint64), np.arange(40, dtype=np.uint64)])
    return rels


def test_hand_made_trees(rhj):
    relations = hand_made()
    cols = [[dev(rhj, c) for c in rel] for rel in relations]
    # a chain of four 3000-row bindings on one key: 8.1e13 rows, which only this route can answer
    huge = ([0, 1, 2, 3], [(0, 0, 1, 0), (1, 0, 2, 0), (2, 0, 3, 0)], [], [(0, 1), (1, 2), (2, 1), (3, 2)])
    huge_sums = [int(relations[b][c].sum(dtype=np.uint64)) * 3000 ** 3 & M64 for b, c in huge[3]]
    # eight bindings in a chain with eight views; a 1 + 7 star; a root that is not binding 0; a fold that is empty at a middle round
    chain8 = ([4] * 8, [(k, 0, k + 1, 3) for k in range(7)], [(0, 0, "<", 250)], [(k, 1 + k % 2) for k in range(8)])
    star = ([5, 4, 4, 5, 4, 5, 4, 4], [(0, 0, b, 0) for b in range(1, 8)], [(3, 2, "<", 30)], [(0, 1), (1, 1), (3, 1), (5, 2), (7, 2)])
    rooted = ([5, 4, 5, 4], [(0, 0, 1, 0), (1, 0, 2, 0), (2, 0, 3, 0)], [], [(0, 1), (3, 1), (2, 2)])
    dies = ([4, 4, 4, 4, 5], [(0, 0, 1, 0), (1, 0, 2, 0), (2, 0, 3, 0), (3, 0, 4, 0)], [(2, 0, ">", 100), (3, 0, "<", 50)], [(4, 1), (2, 1)])
    queries = [chain8, huge, star, rooted, dies]
    assert fm.fold_plan(rooted)[0] == 1 and fm.fold_plan(chain8)[0] == 3 and fm.fold_plan(star)[0] == 0
    assert fm.fold_plan(dies) == (1, [(0, 1, 0), (4, 3, 0), (3, 2, 1), (2, 1, 2)])
    info_want, fold_want, folded = fm.fold_counts(relations, queries)
    assert folded[1] == (huge_sums, 3000 ** 4) and 3000 ** 4 == 81 * 10 ** 12
    for q, f in zip((chain8, star, rooted, dies), (folded[0], folded[2], folded[3], folded[4])):
        w = run_query(relations, q)
        assert (list(f[0]), f[1]) == (list(w[0]), w[1]), q
    assert folded[0][1] > 0 and folded[2][1] > 0 and folded[3][1] > 0 and folded[4] == ([0, 0], 0)
    assert fm.fold_route(relations, dies)[2] == {0: 2, 1: 1}                          # finished at round 1 of 3: the items of round 2 are never issued
    assert fold_want == {"fold_calls": 7, "fold_items": 3 + 7 + 3 + 7 + 3, "fold_queries": 5}
    res, info = run(rhj, cols, queries)
    assert answers(res) == [(list(f[0]), f[1]) for f in folded]
    assert info.fold_info == fold_want and dict(info) == info_want == dict(levels=0, filter_calls=1, eq2_calls=0, join_calls=0, join_reruns=0, apply_calls=0)
    assert rhj.stats()["matches"] == sum(f[1] for f in folded) & M64
    # the huge query alone, twice
    for _ in range(2):
        res, info = run(rhj, cols, [huge])
        assert answers(res) == [(huge_sums, 81 * 10 ** 12)] and info.fold_info == {"fold_calls": 2, "fold_items": 3, "fold_queries": 1}
