"""rhj_query_batch_device on the fold route with rhj_set_fold_resident_keys on (include/rhj_inter.h): the switch
reaches the fold batches on tuple keys inside the route, by waits and in the one-wait programs.  With the fold, keys and self
switches on, the `small` workload and the forms of tests/query_shapes.py give the same rows and sums with the new switch off and
on and with both resident switches on, on both routes, and the fold, foldk and self infos do not move; a one-wait program whose
rounds hold resident items only issues no memset and one launch a round and kind; with the nodes switch on as well, the items of
rhj_join_foldn_batch_device are reported resident.  Every comparison is an integer equality."""
import importlib

import numpy as np
import pytest

import fold_exact as fe
import fold_pred_model as pm
import fold_resident_keys_model as rk
import fold_resident_model as rm
import query_shapes as shapes
from query_model import parse_work, run_query

pytestmark = pytest.mark.gpu

LIMIT = pm.SMALL_ROWS                                    # 65 536 rows: the limit that admits `small`
NO_RESIDENT = {"resident_items": 0, "resident_launches": 0, "table_items": 0}
OFF, KEYS, BOTH = (False, False), (False, True), (True, True)          # (rhj_set_fold_resident, rhj_set_fold_resident_keys)


def all_off(r):
    r.set_query_fold(False)
    r.set_query_fold_keys(False)
    r.set_query_fold_self(False)
    r.set_query_fold_nodes(False)
    r.set_query_fold_one_wait(False)
    r.set_query_fold_one_wait_rows(pm.DEFAULT_ROWS)
    r.set_fold_resident(False)
    r.set_fold_resident_keys(False)


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


def run(rhj, cols, queries, resident, one_wait, nodes=False):
    """(answers, the fold, foldk, self and nodes infos, the one-wait info, the resident info of the tuple-key batches, that of the
    batch on one key) of one batch; resident = (the switch of the folds on one key, that of the folds on tuple keys)"""
    rhj.set_query_fold(True)
    rhj.set_query_fold_keys(True)
    rhj.set_query_fold_self(True)
    rhj.set_query_fold_nodes(nodes)
    rhj.set_query_fold_one_wait(one_wait)
    rhj.set_query_fold_one_wait_rows(LIMIT)
    rhj.set_fold_resident(resident[0])
    rhj.set_fold_resident_keys(resident[1])
    try:
        res, info = rhj.query_batch_device(cols, queries, with_info=True)
        keys_info, one_key_info = rhj.table_batch_last_resident_keys_info(), rhj.table_batch_last_resident_info()
    finally:
        all_off(rhj)
    return ([(list(s), r) for s, r in res], (info.fold_info, info.foldk_info, info.fold_self_info, info.fold_nodes_info), info.one_wait_info,
            keys_info, one_key_info)


def off_and_on(rhj, cols, queries, want=None, nodes=False):
    """both routes with the resident switches off, the new one on, and both on: the same answers and the same infos; returns the
    runs by (route, switches)"""
    runs = {}
    for one_wait in (False, True):
        off = runs[one_wait, OFF] = run(rhj, cols, queries, OFF, one_wait, nodes)
        assert off[3] == NO_RESIDENT and off[4] == NO_RESIDENT
        for switches in (KEYS, BOTH):
            on = runs[one_wait, switches] = run(rhj, cols, queries, switches, one_wait, nodes)
            for k, (a, b) in enumerate(zip(on[0], off[0])):
                assert a == b, (one_wait, switches, k, queries[k])
            assert on[1] == off[1]
            # the route's items are the same items: the programs, their items by kind and their rounds do not move either
            same = ("queries", "programs", "pred_items", "fold_items", "foldk_items", "rounds", "waits")
            assert {k: on[2][k] for k in same} == {k: off[2][k] for k in same}
            assert on[2]["memsets"] <= off[2]["memsets"] == off[2]["rounds"] and on[2]["launches"] <= off[2]["launches"] + 2 * on[2]["rounds"]
            # every item on tuple keys is counted in one form or the other, wherever it was issued
            tuple_items = on[2]["foldk_items"] + on[1][1]["foldk_items"] + on[1][3]["foldn_items"]
            assert on[3]["resident_items"] + on[3]["table_items"] == tuple_items
            if switches == KEYS:
                assert on[4] == NO_RESIDENT                  # the info of the folds on one key does not move
    assert runs[False, KEYS][0] == runs[True, KEYS][0] == runs[True, BOTH][0]
    if want is not None:
        assert runs[True, KEYS][0] == [(list(s), r) for s, r in want]
    return runs


def test_the_small_workload(rhj, golden):
    rels = golden.small_relations
    relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    cols = to_device(rhj, relations)
    queries = parse_work(golden.small["work_lines"])
    runs = off_and_on(rhj, cols, queries)
    for key in ((True, KEYS), (True, BOTH), (False, KEYS)):
        lines = [" ".join("NULL" if rows == 0 else str(s) for s in sums) for sums, rows in runs[key][0]]
        assert lines == golden.small["result_lines"]
    for one_wait in (False, True):                       # (its items on tuple keys are few; every one is counted in one form)
        info = runs[one_wait, KEYS][3]
        print("small, one wait %s: %s, one-wait info %s" % (one_wait, info, runs[one_wait, KEYS][2]))
        assert (info["resident_launches"] > 0) == (info["resident_items"] > 0)
    ow = runs[True, BOTH][2]
    assert ow["queries"] == 50 and ow["programs"] == 1 and ow["waits"] == 1
    assert ow["memsets"] <= runs[True, KEYS][2]["memsets"] <= runs[True, OFF][2]["memsets"]


@pytest.mark.parametrize("name", sorted(shapes.FAMILIES))
def test_the_queries_of_the_query_shapes(rhj, name):
    rels, queries, want = shapes.reference(name)[:3]
    cols = to_device(rhj, rels, shapes.B1_PREFIX if name == "filter too large" else None)
    off_and_on(rhj, cols, queries, want)


@pytest.fixture(scope="module")
def thousand(rhj):
    """three relations of 1000 rows whose pairs (c0, c1) come from 20 x 15 values: a join on both columns neither dies nor blows up"""
    rng = np.random.default_rng(423)
    relations = [fe.make_relation(rng, 1000, 20, 15) for _ in range(3)]
    return relations, to_device(rhj, relations)


def test_chains_of_resident_items_on_two_columns_issue_no_memset_and_one_launch_a_round(rhj, thousand):
    """three-binding chains joined on two columns over relations of 1000 rows, a filter on one binding each: every item of every
    round is on a tuple key and resident, so the program is the pred launch and one k_foldk_lds launch a round, with no memset;
    with the switch off every round has its memset and its table launches"""
    relations, cols = thousand
    rank = lambda r, k: int(np.sort(relations[r][fe.RANK_COL])[k])
    queries = []
    for k in range(12):
        a, b, c = k % 3, (k + 1) % 3, (k + 2) % 3
        queries.append(([a, b, c], [(0, 0, 1, 0), (0, 1, 1, 1), (1, 0, 2, 0), (1, 1, 2, 1)], [(k % 3, fe.RANK_COL, "<", rank([a, b, c][k % 3], 500 + 30 * k))], [(k % 3, 2)]))
    assert all(rk.resident(1000, 1000, v) for v in (1, 2, 3))
    want = [(list(s), r) for s, r in (run_query(relations, x) for x in queries)]
    assert all(r > 0 for _, r in want)                   # (an empty result short-cuts the rounds and would show nothing)
    on, _, ow_on, res_on, one_key_on = run(rhj, cols, queries, KEYS, True)
    off, _, ow_off, res_off, _ = run(rhj, cols, queries, OFF, True)
    old, _, ow_old, res_old, _ = run(rhj, cols, queries, (True, False), True)
    assert on == off == old == want
    rounds = ow_on["rounds"]
    assert ow_on["queries"] == 12 and ow_on["programs"] == 1 and ow_on["waits"] == 1 and rounds == ow_off["rounds"] == 2
    assert ow_on["fold_items"] == 0 and ow_on["foldk_items"] == 24 and ow_on["pred_items"] == 12
    assert ow_on["memsets"] == 0 and ow_on["launches"] == 1 + rounds
    assert res_on == {"resident_items": 24, "resident_launches": rounds, "table_items": 0} and one_key_on == NO_RESIDENT
    assert ow_off["memsets"] == rounds and ow_off["launches"] >= 1 + 2 * rounds and res_off == NO_RESIDENT
    assert ow_old == ow_off and res_old == NO_RESIDENT   # the switch of the folds on one key alone changes nothing here


def test_a_round_of_both_kinds_all_resident_issues_no_memset_and_two_launches(rhj, thousand):
    """two-binding queries, half joined on one column and half on two: one round that holds items of both kinds; with both
    resident switches on it is one k_fold_lds and one k_foldk_lds launch and no memset, with either switch alone the other
    kind keeps its memset and its table launches"""
    relations, cols = thousand
    queries = []
    for k in range(8):
        a, b = k % 3, (k + 1) % 3
        joins = [(0, 0, 1, 0)] if k % 2 == 0 else [(0, 0, 1, 0), (0, 1, 1, 1)]
        queries.append(([a, b], joins, [], [(k % 2, 2), (1 - k % 2, 3)]))
    assert all(rk.resident(1000, 1000, v) and rm.resident(1000, 1000, v) for v in (1, 2, 3))
    want = [(list(s), r) for s, r in (run_query(relations, x) for x in queries)]
    assert all(r > 0 for _, r in want)
    both, _, ow, res, one_key = run(rhj, cols, queries, BOTH, True)
    assert both == want
    assert ow["queries"] == 8 and ow["programs"] == 1 and ow["rounds"] == 1 and ow["fold_items"] == 4 and ow["foldk_items"] == 4
    assert ow["memsets"] == 0 and ow["launches"] == (ow["pred_items"] > 0) + 2
    assert res == {"resident_items": 4, "resident_launches": 1, "table_items": 0} == one_key
    for switches in (KEYS, (True, False), OFF):
        got, _, ow2, res2, one_key2 = run(rhj, cols, queries, switches, True)
        assert got == want and ow2["memsets"] == 1 and ow2["rounds"] == 1
        # (a kind in the table form: claim, add, apply; the sides are equal in rows, so R builds and the claim launch runs)
        assert ow2["launches"] == (ow["pred_items"] > 0) + (1 if switches[0] else 3) + (1 if switches[1] else 3)
        assert res2 == (res if switches[1] else NO_RESIDENT) and one_key2 == (one_key if switches[0] else NO_RESIDENT)


def test_a_triangle_with_a_chain_over_nodes(rhj):
    """with the nodes switch on as well: the triangle's first level makes a node of a few thousand rows, and the folds over it
    are rhj_join_foldn_batch_device's, reported resident with the new switch on; the same answers under every setting"""
    rng = np.random.default_rng(20191)
    rels = [[rng.integers(0, 100, size=500).astype(np.uint64), rng.integers(0, 4, size=500).astype(np.uint64),
             rng.integers(0, 1 << 64, size=500, dtype=np.uint64), rng.integers(0, 3, size=500).astype(np.uint64)] for _ in range(4)]
    cols = to_device(rhj, rels)
    queries = [([0, 1, 2, 3], [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3), (2, 0, 3, 0)], [], [(0, 2), (3, 2)]),
               ([1, 2, 3, 0], [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3), (2, 0, 3, 0)], [], [(1, 2), (2, 2)])]
    want = [(list(s), r) for s, r in (run_query(rels, x) for x in queries)]
    assert all(r > 0 for _, r in want)
    runs = off_and_on(rhj, cols, queries, want, nodes=True)
    for one_wait in (False, True):
        for switches in (KEYS, BOTH):
            _, infos, ow, keys_info, _ = runs[one_wait, switches]
            assert infos[3]["node_queries"] == 2 and infos[3]["foldn_items"] >= 2
            # a node of about 2500 rows against a relation of 500: every item on tuple keys is resident
            assert keys_info["resident_items"] >= infos[3]["foldn_items"] and keys_info["table_items"] == 0 and keys_info["resident_launches"] >= 1
