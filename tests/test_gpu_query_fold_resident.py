"""rhj_query_batch_device on the fold route with rhj_set_fold_resident on (include/rhj_inter.h): the switch reaches
the fold batches on one key inside the route, by waits and in the one-wait programs.  With the fold, keys and self switches on,
the `small` workload and the forms of tests/query_shapes.py give the same rows and sums with the resident switch off and on, on
both routes, and the fold, foldk and self infos do not move; a one-wait program whose rounds hold resident items only issues no
memset and one launch a round.  Every comparison is an integer equality."""
import importlib

import numpy as np
import pytest

import fold_exact as fe
import fold_pred_model as pm
import fold_resident_model as rm
import query_shapes as shapes
from query_model import parse_work

pytestmark = pytest.mark.gpu

LIMIT = pm.SMALL_ROWS                                    # 65 536 rows: the limit that admits `small`
NO_RESIDENT = {"resident_items": 0, "resident_launches": 0, "table_items": 0}


def all_off(r):
    r.set_query_fold(False)
    r.set_query_fold_keys(False)
    r.set_query_fold_self(False)
    r.set_query_fold_one_wait(False)
    r.set_query_fold_one_wait_rows(pm.DEFAULT_ROWS)
    r.set_fold_resident(False)


@pytest.fixture(scope="module")
def rhj():
    mod = importlib.import_module("sigmod-2018_amd")
    r = mod.RHJ(device=0)
    r.lib.rhj_set_timing(0)
    r.set_bits(4)
    yield r
    all_off(r)
    r.lib.rhj_set_timing(2)


def to_device(rhj, rels, prefix=None):
    dev = lambda a: rhj.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)
    cols = []
    for r, rel in enumerate(rels):
        if prefix and r in prefix:
            src, n = prefix[r]
            cols.append([t[:n] for t in cols[src]])
        else:
            cols.append([dev(c) for c in rel])
    return cols


def run(rhj, cols, queries, resident, one_wait):
    """(answers, the fold, foldk and self infos, the one-wait info, the resident info) of one batch"""
    rhj.set_query_fold(True)
    rhj.set_query_fold_keys(True)
    rhj.set_query_fold_self(True)
    rhj.set_query_fold_one_wait(one_wait)
    rhj.set_query_fold_one_wait_rows(LIMIT)
    rhj.set_fold_resident(resident)
    try:
        res, info = rhj.query_batch_device(cols, queries, with_info=True)
        resident_info = rhj.table_batch_last_resident_info()
    finally:
        all_off(rhj)
    return [(list(s), r) for s, r in res], (info.fold_info, info.foldk_info, info.fold_self_info), info.one_wait_info, resident_info


def on_and_off(rhj, cols, queries, want=None):
    """both routes with the switch off and on: the same answers and the same three infos; returns the four runs by (route, switch)"""
    runs = {}
    for one_wait in (False, True):
        off = runs[one_wait, False] = run(rhj, cols, queries, False, one_wait)
        on = runs[one_wait, True] = run(rhj, cols, queries, True, one_wait)
        for k, (a, b) in enumerate(zip(on[0], off[0])):
            assert a == b, (one_wait, k, queries[k])
        assert on[1] == off[1] and off[3] == NO_RESIDENT
        # the route's items are the same items: the programs, their items by kind and their rounds do not move either
        same = ("queries", "programs", "pred_items", "fold_items", "foldk_items", "rounds", "waits")
        assert {k: on[2][k] for k in same} == {k: off[2][k] for k in same}
        assert on[2]["memsets"] <= off[2]["memsets"] == off[2]["rounds"] and on[2]["launches"] <= off[2]["launches"] + on[2]["rounds"]
        items = on[2]["fold_items"] if one_wait else on[1][0]["fold_items"]
        if not one_wait:
            assert on[3]["resident_items"] + on[3]["table_items"] == items
    assert runs[False, True][0] == runs[True, True][0]
    if want is not None:
        assert runs[True, True][0] == [(list(s), r) for s, r in want]
    return runs


def test_the_small_workload(rhj, golden):
    rels = golden.small_relations
    relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    cols = to_device(rhj, relations)
    queries = parse_work(golden.small["work_lines"])
    runs = on_and_off(rhj, cols, queries)
    lines = [" ".join("NULL" if rows == 0 else str(s) for s in sums) for sums, rows in runs[True, True][0]]
    assert lines == golden.small["result_lines"]
    for one_wait in (False, True):                       # the workload has items of both forms on either route
        info = runs[one_wait, True][3]
        assert info["resident_items"] > 0 and info["resident_launches"] > 0
    ow = runs[True, True][2]
    assert ow["queries"] == 50 and ow["programs"] == 1 and ow["waits"] == 1
    assert runs[True, True][3]["resident_items"] + runs[True, True][3]["table_items"] == ow["fold_items"]


@pytest.mark.parametrize("name", sorted(shapes.FAMILIES))
def test_the_queries_of_the_query_shapes(rhj, name):
    rels, queries, want = shapes.reference(name)[:3]
    cols = to_device(rhj, rels, shapes.B1_PREFIX if name == "filter too large" else None)
    on_and_off(rhj, cols, queries, want)


def test_chains_of_resident_items_issue_no_memset_and_one_launch_a_round(rhj):
    """three-binding chains on one key over relations of 1000 rows, a filter on one binding each: every item of every round is
    resident, so the program is the pred launch and one k_fold_lds launch a round, with no memset; with the switch off every
    round has its memset and the three launches"""
    rng = np.random.default_rng(422)
    relations = [fe.make_relation(rng, 1000, 400, 300) for _ in range(3)]
    cols = to_device(rhj, relations)
    rank = lambda r, k: int(np.sort(relations[r][fe.RANK_COL])[k])
    queries = []
    for k in range(12):
        a, b, c = k % 3, (k + 1) % 3, (k + 2) % 3
        queries.append(([a, b, c], [(0, 0, 1, 0), (1, 0, 2, 0)], [(k % 3, fe.RANK_COL, "<", rank([a, b, c][k % 3], 500 + 30 * k))], [(k % 3, 2)]))
    assert all(rm.resident(1000, 1000, v) for v in (1, 2, 3))
    want = [fe.modulo(fe.exact_tree(relations, x)) for x in queries]
    assert all(r > 0 for _, r in want)
    on, _, ow_on, res_on = run(rhj, cols, queries, True, True)
    off, _, ow_off, res_off = run(rhj, cols, queries, False, True)
    assert on == off == [(list(s), r) for s, r in want]
    rounds = ow_on["rounds"]
    assert ow_on["queries"] == 12 and ow_on["programs"] == 1 and ow_on["waits"] == 1 and rounds == ow_off["rounds"] == 2
    assert ow_on["fold_items"] == 24 and ow_on["foldk_items"] == 0 and ow_on["pred_items"] == 12
    assert ow_on["memsets"] == 0 and ow_on["launches"] == 1 + rounds
    assert res_on == {"resident_items": 24, "resident_launches": rounds, "table_items": 0}
    assert ow_off["memsets"] == rounds and ow_off["launches"] >= 1 + 2 * rounds and res_off == NO_RESIDENT
