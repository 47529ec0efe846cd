"""rhj_query_batch_device with rhj_set_query_fold(1), rhj_set_query_fold_keys(1), rhj_set_query_fold_self(1) and
rhj_set_query_fold_nodes(1) (include/rhj_inter.h): a query with a true cycle runs by levels only until its merged
nodes and remaining predicates are a tree, and folds over the nodes from there.  The answers are the `small` workload's recorded
result lines, the numpy executor of query_model.py, a brute force by itertools.product and a closed form; the calls are those
join_foldn_model.foldn_counts gives.  Every comparison is an integer equality."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import join_foldn_model as nm
import join_folds_model as sm
import query_shapes as shapes
from query_model import call_counts, parse_work, run_query
from test_join_foldn_model import SHAPE_LEVELS, TRIANGLE

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
B63 = 1 << 63
NO_FOLD = {"fold_calls": 0, "fold_items": 0, "fold_queries": 0}
NO_FOLDK = {"foldk_calls": 0, "foldk_items": 0, "foldk_queries": 0}
NO_LEVELS = dict(levels=0, filter_calls=0, eq2_calls=0, join_calls=0, join_reruns=0, apply_calls=0)


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


def all_off(r):
    r.set_query_fold(False)
    r.set_query_fold_keys(False)
    r.set_query_fold_self(False)
    r.set_query_fold_nodes(False)
    r.set_query_fold_node_rows(1 << 32)


@pytest.fixture(scope="module")
def rhj(mod):
    r = mod.RHJ(device=0)
    r.lib.rhj_set_timing(2)
    r.set_bits(4)
    yield r
    all_off(r)
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


def run(rhj, cols, queries, fold=True, keys=True, self_=True, nodes=True, node_rows=1 << 32):
    rhj.set_query_fold(fold)
    rhj.set_query_fold_keys(keys)
    rhj.set_query_fold_self(self_)
    rhj.set_query_fold_nodes(nodes)
    rhj.set_query_fold_node_rows(node_rows)
    try:
        return rhj.query_batch_device(cols, queries, with_info=True)
    finally:
        all_off(rhj)


def answers(res):
    return [(list(s), r) for s, r in res]


def infos(info):
    return dict(info), info.fold_info, info.foldk_info, info.fold_self_info, info.fold_nodes_info


def held(rhj, rels, cols, queries, want, node_rows=1 << 32):
    """one batch with all four switches on: the answers, and the five infos against the model; returns the model's infos"""
    model = nm.foldn_counts(rels, queries, node_rows)
    assert [(list(a[0]), a[1]) for a in model[5]] == want
    res, info = run(rhj, cols, queries, node_rows=node_rows)
    assert answers(res) == want
    assert infos(info) == model[:5]
    return model[:5]


def q(rels, joins, views=((0, 2),), filters=()):
    return (list(rels), list(joins), list(filters), list(views))


def test_small_workload_nothing_hands_over(rhj, golden):
    rels = golden.small_relations
    relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    cols = to_device(rhj, relations)
    queries = parse_work(golden.small["work_lines"])
    lines_of = lambda res: [" ".join("NULL" if rows == 0 else str(s) for s in sums_) for sums_, rows in res]
    rhj.lib.rhj_set_order(1)                             # order mode "any"
    try:
        three, info3 = run(rhj, cols, queries, nodes=False)
        four, info4 = run(rhj, cols, queries)
    finally:
        rhj.lib.rhj_set_order(0)
    assert lines_of(four) == golden.small["result_lines"] == lines_of(three)
    assert infos(info4) == infos(info3) and info4.fold_nodes_info == nm.NO_NODES and info4.fold_info["fold_queries"] == 45


@pytest.mark.parametrize("name", sorted(shapes.FAMILIES))
def test_the_queries_of_the_query_shapes(rhj, name):
    rels, queries, want = shapes.reference(name)[:3]
    cols = to_device(rhj, rels, shapes.B1_PREFIX if name == "filter too large" else None)
    info, fold, foldk, self_, nodes = held(rhj, rels, cols, queries, [(list(s), r) for s, r in want])
    mine = {k: v for k, v in SHAPE_LEVELS.items() if k[0] == name}
    parked = [k for k in mine if all(len(rels[r][0]) for r in queries[k[1]][0])]
    assert nodes["node_queries"] <= len(mine) and nodes["node_levels"] <= sum(mine.values())
    if name == "synthetic":
        assert nodes == {"foldn_calls": 1, "foldn_items": 1, "node_queries": 1, "node_levels": 2} and info["levels"] == 2
    if name == "tiny":
        assert nodes["node_queries"] == 1 and nodes["node_levels"] == 1 and info["levels"] == 1
    if name == "descriptor limits":
        assert len(parked) == 3 and info["levels"] == 11
    if not mine:                                         # nothing hands over: the three switches' counts
        assert nodes == nm.NO_NODES and (info, fold, foldk, self_) == sm.folds_counts(rels, queries)[:4]


@pytest.fixture(scope="module")
def random_batch(rhj):
    rels, queries = nm.random_queries()
    return rels, to_device(rhj, rels), queries, [sm.product_answer(rels, x) for x in queries]


def test_random_queries_hand_over(rhj, random_batch):
    rels, cols, queries, want = random_batch
    want = [(list(s), r) for s, r in want]
    info, fold, foldk, self_, nodes = held(rhj, rels, cols, queries, want)
    assert nodes["node_queries"] >= 16 and nodes["foldn_items"] >= 4 and self_["self_calls"] == 2
    # each handed-over query alone: its own prefix, pre-round and rounds
    alone = [(x, w) for x, w in zip(queries, want) if nm.foldn_plan(x)[0]]
    for x, w in alone[:12]:
        held(rhj, rels, cols, [x], [w])


def test_random_queries_on_the_level_route(rhj, random_batch):
    rels, cols, queries, want = random_batch
    res, info = run(rhj, cols, queries, fold=False)
    assert answers(res) == [(list(s), r) for s, r in want]
    assert infos(info) == (call_counts(rels, queries)[0], NO_FOLD, NO_FOLDK, sm.NO_SELF, nm.NO_NODES)


def test_triangles_and_four_cycles_against_a_cross_product(rhj, random_batch):
    rels, cols = random_batch[:2]
    flip = lambda p: (p[2], p[3], p[0], p[1])
    tri = [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3)]
    cyc = [(0, 0, 1, 0), (1, 1, 2, 1), (2, 3, 3, 3), (3, 1, 0, 1)]
    queries = [q([1, 2, 3], [tri[k] for k in order], [(0, 2), (1, 2), (2, 2)]) for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0))]
    queries += [q([2, 1, 2], [flip(p) for p in tri], [(2, 2), (0, 2)], [(1, 3, "<", 2)])]
    queries += [q([1, 2, 3, 2], [cyc[k] for k in order], [(0, 2), (3, 2), (2, 2)]) for order in ((0, 1, 2, 3), (0, 2, 1, 3), (3, 1, 0, 2))]
    want = [sm.product_answer(rels, x) for x in queries]
    assert sum(1 for _, r in want if r > 0) >= 5
    assert [nm.foldn_plan(x)[0] for x in queries] == [1, 1, 1, 1, 2, 2, 2]
    info, fold, foldk, self_, nodes = held(rhj, rels, cols, queries, want)
    assert nodes["node_queries"] == 7 and nodes["node_levels"] == 10 and info["levels"] == 2
    assert nodes["foldn_items"] >= 3                     # (a triangle's two words name both members of the merged node)


def test_cycles_over_relations_of_one_size(rhj):
    """three relations of 48 rows each: whichever member's vector a key word is read through, the row exists in every relation"""
    rng = np.random.default_rng(20190)
    rels = [[rng.integers(0, 4, size=48).astype(np.uint64), rng.integers(0, 4, size=48).astype(np.uint64),
             rng.permutation(48).astype(np.uint64) + np.uint64(B63 + (r << 20)), rng.integers(0, 3, size=48).astype(np.uint64)] for r in range(3)]
    cols = to_device(rhj, rels)
    tri = q([0, 1, 2], [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3)], [(0, 2), (1, 2), (2, 2)])
    two = q([0, 1, 2, 0], [(0, 0, 1, 0), (2, 1, 3, 1), (1, 3, 2, 3), (0, 1, 3, 0)], [(1, 2), (3, 2)])         # two merged nodes, then two words
    want = [(list(s), r) for s, r in (run_query(rels, x) for x in (tri, two))]
    assert all(r > 500 for _, r in want) and [nm.foldn_plan(x)[0] for x in (tri, two)] == [1, 2]
    info, fold, foldk, self_, nodes = held(rhj, rels, cols, [tri, two], want)
    assert nodes == {"foldn_calls": 1, "foldn_items": 2, "node_queries": 2, "node_levels": 3}


def test_a_hand_over_to_a_single_node_and_three_ways_to_die(rhj, random_batch):
    rels, cols = random_batch[:2]
    views = [(0, 2), (1, 2)]
    one = q([2, 3], [(0, 0, 1, 0), (0, 1, 1, 1), (0, 3, 1, 3), (0, 0, 1, 1), (0, 1, 1, 3)], views)         # five parallel predicates: one node, two inside it
    in_prefix = q([1, 2, 3], [(0, 0, 1, 2)] + TRIANGLE[1:], views)                                      # c0 = c2 never holds: the first level is empty
    in_pre_round = q([2, 3], [(0, 0, 1, 0), (0, 1, 1, 1), (0, 3, 1, 3), (0, 0, 1, 1), (0, 2, 1, 2)], views)    # the c2 are unique per relation: no row passes
    in_a_round = q([1, 2, 3, 4], [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3), (2, 2, 3, 0)], views)         # the chain's key is a c2: the fold finds no tuple
    lives = q([1, 2, 3, 4], [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3), (2, 0, 3, 0)], views + [(3, 2)])
    queries = [one, in_prefix, in_pre_round, in_a_round, lives]
    assert [nm.foldn_plan(x)[0] for x in queries] == [1, 1, 1, 1, 1]
    want = [(list(s), r) for s, r in (run_query(rels, x) for x in queries)]
    assert want[0][1] > 0 and want[4][1] > 0 and [r for _, r in want[1:4]] == [0, 0, 0]
    routes = [nm.foldn_route(rels, x) for x in queries]
    assert [r["parked"] for r in routes] == [True, False, True, True, True]
    assert routes[0]["pre"] == 1 and not routes[0]["rounds"] and routes[2]["pre"] == 1 and not routes[2]["rounds"] and routes[3]["rounds"]
    info, fold, foldk, self_, nodes = held(rhj, rels, cols, queries, want)
    assert nodes["node_queries"] == 4 and nodes["node_levels"] == 4 and self_ == {"self_calls": 1, "self_items": 2, "self_queries": 0}
    for x, w in zip(queries, want):
        held(rhj, rels, cols, [x], [w])


def closed_form_relations():
    """relation 0: 64 rows, one value per key column, c2 unique and near 2^63; relation 1: 3000 rows likewise, c0 the same value"""
    rng = np.random.default_rng(20189)
    rels = []
    for r, n in enumerate((64, 3000)):
        rels.append([np.full(n, 1, dtype=np.uint64), np.full(n, 2, dtype=np.uint64), rng.permutation(n).astype(np.uint64) + np.uint64(B63 + (r << 20)),
                     np.full(n, 3, dtype=np.uint64)])
    return rels


@pytest.fixture(scope="module")
def closed(rhj):
    rels = closed_form_relations()
    return rels, to_device(rhj, rels)


def test_a_triangle_with_a_chain_that_the_levels_cannot_hold(rhj, closed):
    """64^3 * 3000^3 rows: the triangle's first level makes a node of 4096 rows, everything behind it is folded"""
    rels, cols = closed
    chain = [(2, 0, 3, 0), (3, 0, 4, 0), (4, 0, 5, 0)]
    huge = q([0, 0, 0, 1, 1, 1], [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3)] + chain, [(0, 2), (2, 2), (5, 2)])
    rows = 64 ** 3 * 3000 ** 3
    small, large = int(rels[0][2].sum(dtype=np.uint64)), int(rels[1][2].sum(dtype=np.uint64))
    want = ([small * 64 ** 2 * 3000 ** 3 & M64, small * 64 ** 2 * 3000 ** 3 & M64, large * 64 ** 3 * 3000 ** 2 & M64], rows)
    assert rows == 7077888000000000 and nm.foldn_plan(huge)[:2] == (1, [0, 0, 2, 3, 4, 5])
    route = nm.foldn_route(rels, huge)
    assert (route["sums"], route["rows"]) == want and route["levels"] == [(0, 64, 64, 4096)]
    res, info = run(rhj, cols, [huge])
    assert answers(res) == [want]
    assert info.fold_nodes_info == {"foldn_calls": 1, "foldn_items": 1, "node_queries": 1, "node_levels": 1}
    assert dict(info) == dict(NO_LEVELS, levels=1, join_calls=1, join_reruns=1, apply_calls=1)
    assert rhj.stats()["matches"] == rows


def test_a_merged_node_at_the_row_limit_stays_on_the_levels(rhj, closed):
    rels, cols = closed
    tri = q([0, 0, 0], [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3)], [(0, 2), (2, 2)])
    small = int(rels[0][2].sum(dtype=np.uint64))
    want = [([small * 64 ** 2 & M64] * 2, 64 ** 3)]
    stays = held(rhj, rels, cols, [tri], want, node_rows=4096)          # the node has 4096 rows: not fewer than the limit
    assert stays[4] == nm.NO_NODES and stays[0]["levels"] == 3 and stays[1] == NO_FOLD
    hands = held(rhj, rels, cols, [tri], want, node_rows=4097)
    assert hands[4] == {"foldn_calls": 1, "foldn_items": 1, "node_queries": 1, "node_levels": 1} and hands[0]["levels"] == 1
    # larger limits clamp to 2^32
    res, info = run(rhj, cols, [tri], node_rows=M64)
    assert answers(res) == want and infos(info) == hands


def test_a_large_call_and_then_a_small_one(rhj, closed, random_batch):
    rels, cols = closed
    big = [q([0, 0, 0, 1], [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3), (2, 0, 3, 0)], [(0, 2), (3, 2)]) for _ in range(6)]
    route = nm.foldn_route(rels, big[0])
    want = [(route["sums"], route["rows"])] * 6
    assert want[0][1] == 64 ** 3 * 3000
    held(rhj, rels, cols, big, want)
    rels2, cols2, queries, product = random_batch
    picked = [(x, (list(w[0]), w[1])) for x, w in zip(queries, product) if nm.foldn_plan(x)[0]][:3]
    held(rhj, rels2, cols2, [x for x, _ in picked], [w for _, w in picked])


def test_state(rhj, random_batch):
    rels, cols = random_batch[:2]
    queries = [q([1, 2, 3], [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3)], [(0, 2), (2, 2)]), q([3], [(0, 0, 0, 1)], [(0, 2)]), q([1, 2], [(0, 0, 1, 0)], [(1, 2)])]
    want = [(list(s), r) for s, r in (run_query(rels, x) for x in queries)]
    on = held(rhj, rels, cols, queries, want)
    assert on[4]["node_queries"] == 1
    # any one of the other three off: the new switch has no effect
    for off in ("fold", "keys", "self_"):
        with_, info_with = run(rhj, cols, queries, **{off: False})
        without, info_without = run(rhj, cols, queries, nodes=False, **{off: False})
        assert answers(with_) == want == answers(without)
        assert infos(info_with) == infos(info_without) and info_with.fold_nodes_info == nm.NO_NODES
    # the switch off: the three switches' counts
    res, info = run(rhj, cols, queries, nodes=False)
    assert answers(res) == want and infos(info)[:4] == sm.folds_counts(rels, queries)[:4] and info.fold_nodes_info == nm.NO_NODES
    # rhj_release() between two calls: the buffers go and come back
    rhj.lib.rhj_release()
    rhj.torch.cuda.synchronize()
    assert held(rhj, rels, cols, queries, want) == on


CHILD = """
import importlib, sys
import numpy as np
sys.path.insert(0, %r)
import join_foldn_model as nm
mod = importlib.import_module("sigmod-2018_amd")
rhj = mod.RHJ(device=0)
rels, queries = nm.random_queries()
cols = [[rhj.torch.from_numpy(c.view(np.int64)).to(rhj.dev) for c in rel] for rel in rels]
if sys.argv[1] == "setter":
    rhj.set_query_fold(True); rhj.set_query_fold_keys(True); rhj.set_query_fold_self(True); rhj.set_query_fold_nodes(True)
res, info = rhj.query_batch_device(cols, queries[:24], with_info=True)
print(repr(([(list(s), r) for s, r in res], dict(info), info.fold_info, info.foldk_info, info.fold_self_info, info.fold_nodes_info)))
"""


def test_the_environment_and_the_setter_agree(random_batch):
    """two fresh processes: RHJ_QUERY_FOLD_NODES=1 beside the three other variables, and the four setters"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = ("RHJ_QUERY_FOLD", "RHJ_QUERY_FOLD_KEYS", "RHJ_QUERY_FOLD_SELF", "RHJ_QUERY_FOLD_NODES")
    base = {k: v for k, v in os.environ.items() if k not in names}
    outs = []
    for how, env in (("env", dict(base, **{n: "1" for n in names})), ("setter", base)):
        p = subprocess.run([sys.executable, "-c", CHILD % os.path.join(root, "tests"), how], cwd=root, env=env, stdout=subprocess.PIPE, timeout=120, check=True)
        outs.append(p.stdout.decode().strip().splitlines()[-1])
    assert outs[0] == outs[1]
    rels, _, queries, want = random_batch
    model = nm.foldn_counts(rels, queries[:24])
    assert outs[0] == repr(([(list(a[0]), a[1]) for a in model[5]],) + model[:5]) and model[4]["node_queries"] >= 1
