"""rhj_query_batch_device with rhj_set_query_fold_one_wait(1) beside the four fold switches (include/rhj_inter.h):
the folding queries over small relations run as fold programs with one wait, their filters 0/1 weights over whole relations.  The
answers are the `small` workload's recorded result lines, tests/fold_exact.py's exact_tree in unbounded Python integers, the numpy
executor of query_model.py, and the same library with the switch off; the info counts programs, items and waits.  Every
comparison is an integer equality."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import fold_exact as fe
import fold_families as ff
import fold_pred_model as pm
import join_folds_model as sm
import query_shapes as shapes
from query_model import parse_work, run_query

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
B63 = 1 << 63
LIMIT = pm.SMALL_ROWS                                    # the row limit these tests run at unless they say otherwise: the one that admits `small`
NO_ONE_WAIT = dict.fromkeys(("queries", "programs", "pred_items", "fold_items", "foldk_items", "rounds", "launches", "memsets", "waits"), 0)
NO_FOLD = {"fold_calls": 0, "fold_items": 0, "fold_queries": 0}
NO_FOLDK = {"foldk_calls": 0, "foldk_items": 0, "foldk_queries": 0}
NO_NODES = {"foldn_calls": 0, "foldn_items": 0, "node_queries": 0, "node_levels": 0}
NO_LEVELS = dict(levels=0, filter_calls=0, eq2_calls=0, join_calls=0, join_reruns=0, apply_calls=0)


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


def all_off(r):
    r.set_query_fold(False)
    r.set_query_fold_keys(False)
    r.set_query_fold_self(False)
    r.set_query_fold_nodes(False)
    r.set_query_fold_one_wait(False)
    r.set_query_fold_one_wait_rows(pm.DEFAULT_ROWS)


@pytest.fixture(scope="module")
def rhj(mod):
    r = mod.RHJ(device=0)
    r.lib.rhj_set_timing(2)
    r.set_bits(4)
    yield r
    all_off(r)
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


def run(rhj, cols, queries, one_wait=True, limit=LIMIT, fold=True):
    """(answers, info) of one batch with the four fold switches on and the one-wait switch as given"""
    rhj.set_query_fold(fold)
    rhj.set_query_fold_keys(True)
    rhj.set_query_fold_self(True)
    rhj.set_query_fold_nodes(True)
    rhj.set_query_fold_one_wait(one_wait)
    rhj.set_query_fold_one_wait_rows(limit)
    try:
        res, info = rhj.query_batch_device(cols, queries, with_info=True)
    finally:
        all_off(rhj)
    return [(list(s), r) for s, r in res], info


def infos(info):
    return dict(info), info.fold_info, info.foldk_info, info.fold_self_info, info.fold_nodes_info


def rows_of(rels):
    return [len(rel[0]) if len(rel) else 0 for rel in rels]


def both(rhj, rels, cols, queries, want=None, limit=LIMIT):
    """the batch with the switch on and off: the same answers (and `want`, when given); on the route exactly the queries the model
    names; with every query on the route no other counter moves.  Returns the one-wait info."""
    on, info_on = run(rhj, cols, queries, limit=limit)
    off, info_off = run(rhj, cols, queries, one_wait=False)
    for k, (a, b) in enumerate(zip(on, off)):
        assert a == b, (k, queries[k])
    if want is not None:
        for k, (a, w) in enumerate(zip(on, want)):
            assert a == (list(w[0]), w[1]), (k, queries[k])
    takes = [pm.one_wait(rows_of(rels), q, limit=limit) for q in queries]
    ow = info_on.one_wait_info
    assert ow["queries"] == sum(takes) and info_off.one_wait_info == NO_ONE_WAIT
    assert ow["waits"] == ow["programs"] and ow["memsets"] == ow["rounds"] and (ow["programs"] > 0) == (sum(takes) > 0)
    if all(takes):
        assert infos(info_on) == (NO_LEVELS, NO_FOLD, NO_FOLDK, sm.NO_SELF, NO_NODES)
    else:                                                # the others alone: what a batch of them alone reports
        others = [q for q, t in zip(queries, takes) if not t]
        rest, info_rest = run(rhj, cols, others, one_wait=False)
        assert infos(info_on) == infos(info_rest) and rest == [a for a, t in zip(on, takes) if not t]
    return ow


def q(rels, joins, views=((0, 2),), filters=()):
    return (list(rels), list(joins), list(filters), list(views))


# ---- correctness ---------------------------------------------------------------------------------------------------------------------

def test_small_workload_is_one_program(rhj, golden):
    rels = golden.small_relations
    relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    cols = to_device(rhj, relations)
    queries = parse_work(golden.small["work_lines"])
    lines_of = lambda res: [" ".join("NULL" if rows == 0 else str(s) for s in sums_) for sums_, rows in res]
    on, info = run(rhj, cols, queries)
    off, info_off = run(rhj, cols, queries, one_wait=False)
    assert lines_of(on) == golden.small["result_lines"] and on == off
    ow = info.one_wait_info
    assert ow["queries"] == 50 and ow["programs"] == 1 and ow["waits"] == 1 and info["filter_calls"] == 0
    assert infos(info) == (NO_LEVELS, NO_FOLD, NO_FOLDK, sm.NO_SELF, NO_NODES)
    assert ow["fold_items"] + ow["foldk_items"] == sum(len(x[0]) - 1 for x in queries) and ow["foldk_items"] > 0
    assert ow["pred_items"] == sum(pm.pred_items(x) for x in queries) >= 40 and ow["rounds"] == ow["memsets"] >= 3
    # with the switch off after being on: the four switches' infos, the parent's
    model = sm.folds_counts(relations, queries)
    assert infos(info_off)[:4] == model[:4] and info_off.one_wait_info == NO_ONE_WAIT and info_off.fold_nodes_info == NO_NODES
    # at a limit of 16 384 rows the larger relations keep their queries on the waits route: a mixed batch, the same answers; at the
    # library's default limit every query has a relation beyond it, and the call is the four switches'
    few, info_few = run(rhj, cols, queries, limit=16384)
    takes = sum(pm.one_wait(rows_of(relations), x, limit=16384) for x in queries)
    assert few == off and 0 < info_few.one_wait_info["queries"] == takes < 50
    none_, info_none = run(rhj, cols, queries, limit=pm.DEFAULT_ROWS)
    assert none_ == off and info_none.one_wait_info == NO_ONE_WAIT and infos(info_none) == infos(info_off)
    # every query alone
    for k in range(0, 50, 7):
        alone, info = run(rhj, cols, [queries[k]])
        assert alone == [off[k]] and info.one_wait_info["programs"] == 1


@pytest.mark.parametrize("name", sorted(shapes.FAMILIES))
def test_the_queries_of_the_query_shapes(rhj, name):
    rels, queries, want = shapes.reference(name)[:3]
    cols = to_device(rhj, rels, shapes.B1_PREFIX if name == "filter too large" else None)
    from test_join_folds_model import SHAPES_THAT_DO_NOT_FOLD
    on, info = run(rhj, cols, queries)
    off, info_off = run(rhj, cols, queries, one_wait=False)
    assert on == off == [(list(s), r) for s, r in want]
    takes = [pm.one_wait(rows_of(rels), x, limit=LIMIT) for x in queries]
    assert info.one_wait_info["queries"] == sum(takes)
    for k in range(len(queries)):
        if (name, k) in SHAPES_THAT_DO_NOT_FOLD:
            assert not takes[k]                          # a true cycle is not on the route, and its answer above is unchanged
    if not any(takes):
        assert infos(info) == infos(info_off) and info.one_wait_info == NO_ONE_WAIT
    elif all(takes):
        assert infos(info) == (NO_LEVELS, NO_FOLD, NO_FOLDK, sm.NO_SELF, NO_NODES)
    else:
        rest, info_rest = run(rhj, cols, [x for x, t in zip(queries, takes) if not t], one_wait=False)
        assert infos(info) == infos(info_rest)


@pytest.fixture(scope="module")
def random_cols(rhj):
    return to_device(rhj, ff.random_trees()[0])


def test_random_trees(rhj, random_cols):
    relations, queries = ff.random_trees()
    ow = both(rhj, relations, random_cols, queries, ff.random_answers())
    assert ow["queries"] == len(queries) >= 200 and ow["programs"] == 1 and ow["rounds"] >= 3
    picked = ff.relabelled()
    batch = [other for _, others in picked for other, _, _ in others]
    got = iter(run(rhj, random_cols, batch)[0])
    for k, others in picked:
        mine = [(fe.views_back(sums, order), rows) for (sums, rows), (_, order, _) in zip((next(got) for _ in others), others)]
        assert mine[0] == mine[1] == mine[2] == ff.random_answers()[k], (k, queries[k])


def test_aimed_trees_dead_children_and_relations_bound_twice(rhj):
    """tests/fold_families.py's aimed trees: a filter on every binding, a relation bound three times under different filters, eight
    views, keys 0 and 2^64 - 1, and chains of five that die in the first and in the second of three rounds, two rounds below the
    root, beside one that lives"""
    ff.check_aimed()
    relations, named = ff.aimed()
    cols = to_device(rhj, relations)
    names = list(named)
    want = ff.exact(relations, [named[n] for n in names])
    ow = both(rhj, relations, cols, [named[n] for n in names], want)
    assert ow["queries"] == len(names) and ow["programs"] == 1
    for n in ("finished in the first round", "finished in the second of three rounds"):
        assert want[names.index(n)] == ([0, 0, 0, 0], 0) and ff.zero_round(relations, named[n]) in (0, 1)
        pair = [named[n], named["alive through three rounds"]]
        ow = both(rhj, relations, cols, pair, [want[names.index(n)], want[names.index("alive through three rounds")]])
        assert ow["rounds"] == 3 and ow["fold_items"] == 8  # no early exit: the dead query's later steps run on zero weights
    # the same relation bound twice under different filters, and once more without one
    rank = lambda k: int(np.sort(relations[2][fe.RANK_COL])[k])
    twice = q([2, 2, 2], ff.chain([2, 2, 2], (0, 1)), [(0, 2), (1, 2), (2, 2)], [(0, fe.RANK_COL, "<", rank(200)), (1, fe.RANK_COL, ">", rank(100))])
    both(rhj, relations, cols, [twice], ff.exact(relations, [twice]))


def test_a_filter_that_passes_no_row_beside_a_live_query(rhj):
    relations, named = ff.aimed()
    cols = to_device(rhj, relations)
    live = named["alive through three rounds"]
    none_ = (live[0], live[1], [(2, 0, "<", 0)], live[3])               # nothing is below 0
    none_root = (live[0], live[1], [(1, 0, ">", M64)], live[3])         # nothing is above 2^64 - 1: the root's own weight is all zero
    want = ff.exact(relations, [none_, live, none_root])
    assert [r for _, r in want] == [0, want[1][1], 0] and want[1][1] > 0
    ow = both(rhj, relations, cols, [none_, live, none_root], want)
    assert ow["queries"] == 3 and ow["pred_items"] == 2


def test_a_join_less_query_with_eight_views_and_four_filters(rhj):
    relations, _ = ff.aimed()
    cols = to_device(rhj, relations)
    rank = lambda k: int(np.sort(relations[0][fe.RANK_COL])[k])
    flt = [(0, fe.RANK_COL, ">", rank(20)), (0, fe.RANK_COL, "<", rank(280)), (0, 0, ">", 0), (0, 1, "<", M64)]
    alone = q([0], [], [(0, c) for c in (0, 1, 2, 3, 4, 2, 3, 1)], flt)
    inside = q([0], [(0, 0, 0, 0), (0, 3, 0, 3)], [(0, 2), (0, 4)], flt[:2])     # predicates that say nothing: dropped
    dead = q([0], [], [(0, 2)], [(0, 0, "<", 0)])
    want = [run_query(relations, x) for x in (alone, inside, dead)]
    assert want[0][1] > 100 and want[2] == ([0], 0)
    ow = both(rhj, relations, cols, [alone, inside, dead], want)
    assert ow == dict(NO_ONE_WAIT, queries=3, programs=1, pred_items=3, launches=1, waits=1)


def test_a_two_key_step_behind_a_one_binding_predicate(rhj):
    rels = sm.random_relations()
    cols = to_device(rhj, rels)
    queries = [q([0, 1], [(0, 0, 0, 1), (0, 0, 1, 0), (0, 3, 1, 3)], [(0, 2), (1, 2)], [(1, 0, "<", 6)]),
               q([1, 0, 2], [(1, 3, 1, 4), (0, 0, 1, 0), (1, 1, 0, 1), (1, 3, 2, 3)], [(2, 2), (0, 2), (1, 2)], [(1, 0, ">", 1), (0, 1, "<", 7)]),
               q([0, 1], [(0, 0, 0, 1), (0, 2, 0, 0), (0, 0, 1, 0), (0, 3, 1, 3)], [(0, 2)])]                      # c2 = c0 never holds: the pred item's total is 0
    want = [sm.product_answer(rels, x) for x in queries]
    assert want[0][1] > 0 and want[1][1] > 0 and want[2][1] == 0 and [sm.how(x) for x in queries] == [3, 3, 3]
    ow = both(rhj, rels, cols, queries, want)
    assert ow["queries"] == 3 and ow["foldk_items"] >= 3 and ow["pred_items"] >= 4


def test_random_queries_with_one_binding_predicates_and_cycles(rhj):
    """join_folds_model's random queries: trees, parallel predicates, one-binding predicates, implied ones and true cycles in one
    batch, against a cross product: a mixed batch of one-wait queries and queries that keep today's path"""
    rels, queries = sm.random_queries()
    cols = to_device(rhj, rels)
    want = [sm.product_answer(rels, x) for x in queries]
    ow = both(rhj, rels, cols, queries, want)
    takes = [pm.one_wait(rows_of(rels), x, limit=LIMIT) for x in queries]
    assert 0 < sum(takes) < len(queries) and ow["foldk_items"] > 0 and ow["pred_items"] > 0


def test_a_weight_total_of_2_64_is_taken_for_an_empty_result(rhj):
    """DESIGN.md 8's limit is the route's too: both numberings give what the waits route gives"""
    ff.check_limit_star()
    relations, first, last, order = ff.limit_star()
    cols = to_device(rhj, relations)
    want = fe.modulo(fe.exact_tree(relations, first))
    nothing = ([0] * len(last[3]), 0)
    assert want[1] == 1 << 63
    ow = both(rhj, relations, cols, [first, last], [want, nothing])     # section 8's limit: `last` has 2^63 rows
    assert ow["queries"] == 2
    both(rhj, relations, cols, [first], [want])
    both(rhj, relations, cols, [last], [nothing])                      # section 8's limit


# ---- routes, cuts and state ----------------------------------------------------------------------------------------------------------

def test_a_relation_at_the_limit_and_one_beyond_it(rhj):
    rng = np.random.default_rng(4190)
    relations = [fe.make_relation(rng, n, 500, 300) for n in (2048, 2049, 300)]
    cols = to_device(rhj, relations)
    at = q([0, 2], [(0, 0, 1, 0)], [(0, 2), (1, 2)], [(0, 1, "<", 200)])
    beyond = q([1, 2], [(0, 0, 1, 0)], [(0, 2), (1, 2)], [(0, 1, "<", 200)])
    want = ff.exact(relations, [at, beyond])
    assert want[0][1] > 0 and want[1][1] > 0
    ow = both(rhj, relations, cols, [at, beyond], want, limit=2048)
    assert ow["queries"] == 1 and ow["fold_items"] == 1 and ow["pred_items"] == 1
    on, info = run(rhj, cols, [beyond], limit=2048)
    assert on == [want[1]] and info.one_wait_info == NO_ONE_WAIT and info.fold_info["fold_queries"] == 1 and info["filter_calls"] == 1
    ow = both(rhj, relations, cols, [at, beyond], want, limit=2049)
    assert ow["queries"] == 2


def test_a_mixed_batch_of_all_routes(rhj):
    """one call: queries on the program, queries that fold over nodes after a level prefix, and queries that run by levels (a
    relation beyond the row limit keeps a tree on the waits route; a square runs by levels when its prefix node is too large)"""
    rels = sm.random_relations()
    cols = to_device(rhj, rels)
    tree = q([1, 2, 3], [(0, 0, 1, 0), (1, 1, 2, 1)], [(0, 2), (2, 2)], [(1, 0, "<", 6)])
    keys = q([1, 2], [(0, 0, 1, 0), (0, 3, 1, 3)], [(1, 2)])
    alone = q([2], [], [(0, 2), (0, 0)], [(0, 0, ">", 2)])
    triangle = q([1, 2, 3], [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3)], [(0, 2), (1, 2), (2, 2)])
    big_tree = q([0, 1], [(0, 0, 1, 0)], [(0, 2)], [(0, 1, "<", 5)])                  # relation 0 has 300 rows: beyond a limit of 64
    queries = [tree, triangle, keys, big_tree, alone, triangle, tree]
    want = [sm.product_answer(rels, x) for x in queries]
    assert all(r > 0 for _, r in want)                   # (so every query is alive wherever it is counted)
    on, info = run(rhj, cols, queries, limit=64)
    off, info_off = run(rhj, cols, queries, one_wait=False)
    assert on == off == [(list(s), r) for s, r in want]
    ow = info.one_wait_info
    assert ow["queries"] == 4 and ow["programs"] == 1 and ow["waits"] == 1
    assert info.fold_nodes_info["node_queries"] == 2 and info.fold_info["fold_queries"] == 3 and info["levels"] == 1 and info["filter_calls"] == 1
    rest, info_rest = run(rhj, cols, [triangle, big_tree, triangle], one_wait=False)
    assert infos(info) == infos(info_rest)
    # with the fold route off the switch has no effect
    plain, info_plain = run(rhj, cols, queries, fold=False)
    assert plain == on and info_plain.one_wait_info == NO_ONE_WAIT and info_plain.fold_info == NO_FOLD


def test_more_items_in_a_round_than_a_program_takes(rhj):
    relations, queries = ff.chunked()
    cols = to_device(rhj, relations)
    want = ff.exact(relations, queries)
    on, info = run(rhj, cols, queries)
    for k, (g, w) in enumerate(zip(on, want)):
        assert g == w, (k, queries[k])
    ow = info.one_wait_info
    assert ow["queries"] == 4097 and ow["programs"] == 2 and ow["waits"] == 2 and ow["fold_items"] == 4097 and ow["rounds"] == 2
    assert ow["pred_items"] == sum(1 for x in queries if x[2])
    for k in (0, 4095, 4096):
        assert run(rhj, cols, [queries[k]])[0] == [want[k]], k


def test_buffers_grow_and_serve_a_smaller_call(rhj, random_cols):
    relations, small, at = ff.small_batch()
    want = [ff.random_answers()[k] for k in at]
    big_relations, big = ff.grown()
    big_cols = to_device(rhj, big_relations)
    big_want = fe.modulo(fe.exact_tree(big_relations, big))
    assert run(rhj, random_cols, small)[0] == want
    got, info = run(rhj, big_cols, [big])
    assert got == [big_want] and info.one_wait_info["queries"] == 1
    assert run(rhj, random_cols, small)[0] == want
    rhj.lib.rhj_release()
    rhj.torch.cuda.synchronize()
    assert run(rhj, random_cols, small)[0] == want
    assert run(rhj, big_cols, [big])[0] == [big_want]
    assert run(rhj, random_cols, small, one_wait=False)[0] == want


CHILD = """
import importlib, sys
import numpy as np
sys.path.insert(0, %r)
import fold_families as ff
mod = importlib.import_module("sigmod-2018_amd")
rhj = mod.RHJ(device=0)
rels, queries = ff.random_trees()
cols = [[rhj.torch.from_numpy(c.view(np.int64)).to(rhj.dev) for c in rel] for rel in rels]
if sys.argv[1] == "setter":
    rhj.set_query_fold(True); rhj.set_query_fold_one_wait(True)
res, info = rhj.query_batch_device(cols, queries[:24], with_info=True)
print(repr(([(list(s), r) for s, r in res], dict(info), info.fold_info, info.one_wait_info)))
"""


def test_the_environment_and_the_setter_agree():
    """two fresh processes: RHJ_QUERY_FOLD_ONE_WAIT=1 beside RHJ_QUERY_FOLD=1, and the two setters"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = ("RHJ_QUERY_FOLD", "RHJ_QUERY_FOLD_ONE_WAIT")
    base = {k: v for k, v in os.environ.items() if k not in names + ("RHJ_QUERY_FOLD_KEYS", "RHJ_QUERY_FOLD_SELF", "RHJ_QUERY_FOLD_NODES")}
    outs = []
    for how, env in (("env", dict(base, **{n: "1" for n in names})), ("setter", base)):
        p = subprocess.run([sys.executable, "-c", CHILD % os.path.join(root, "tests"), how], cwd=root, env=env, stdout=subprocess.PIPE, timeout=120, check=True)
        outs.append(p.stdout.decode().strip().splitlines()[-1])
    assert outs[0] == outs[1]
    want = ff.random_answers()[:24]
    got = eval(outs[0])
    assert got[0] == want and got[3]["queries"] == 24 and got[3]["programs"] == 1 and got[2] == NO_FOLD
