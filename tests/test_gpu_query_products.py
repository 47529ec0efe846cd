"""rhj_query_batch_device with rhj_set_query_products(1) (include/rhj_inter.h): a query whose bindings end in
several components, a cross product, runs as its components in the same batch, and the batch multiplies their rows and sums.
The answers are tests/query_products_model.py's (held to a brute force over the whole cross product in
tests/test_query_products_model.py), under four switch settings: the levels, the last join as its sums, the four fold switches,
and those with the one-wait programs.  Every comparison is an integer equality."""
import ctypes as C
import importlib

import numpy as np
import pytest

import query_products_model as pm
from query_model import run_query
from test_gpu_inter import Engine, make_map, run_plan

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
B63 = 1 << 63
SETTINGS = ("levels", "sum last", "folds", "one wait")
NO_PRODUCTS = {"product_queries": 0, "components": 0}


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


def all_off(r):
    r.set_query_sum_last(False)
    r.set_query_fold(False)
    r.set_query_fold_keys(False)
    r.set_query_fold_self(False)
    r.set_query_fold_nodes(False)
    r.set_query_fold_one_wait(False)
    r.set_query_products(False)


@pytest.fixture(scope="module")
def rhj(mod):
    r = mod.RHJ(device=0)
    r.set_bits(4)
    all_off(r)
    yield r
    all_off(r)
    r.set_bits(4)


def switches(r, setting, products=True):
    all_off(r)
    r.set_query_sum_last(setting == "sum last")
    for f in (r.set_query_fold, r.set_query_fold_keys, r.set_query_fold_self, r.set_query_fold_nodes):
        f(setting in ("folds", "one wait"))
    r.set_query_fold_one_wait(setting == "one wait")
    r.set_query_products(products)


def run(rhj, cols, queries, setting, products=True):
    """([(sums, rows)], info, stats) of one batch under a setting; every switch is off again afterwards"""
    switches(rhj, setting, products)
    try:
        res, info = rhj.query_batch_device(cols, queries, with_info=True)
        stats = rhj.stats()
    finally:
        all_off(rhj)
    return [(list(s), r) for s, r in res], info, stats


def dev(rhj, a):
    return rhj.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


# ---- the relations and the shapes -----------------------------------------------------------------------------------------------------
# Relation r has ROWS[r] rows and four columns: c0 a key of up to 40 values, c1 a key of up to 12, c2 unique and near 2^63 with a
# range of its own per relation (sums wrap; no c2 of one relation is a c2 of another), c3 equal to c0 in about half of the rows.

ROWS = (300, 100, 17, 1, 2049)


def relations():
    rng = np.random.default_rng(202020)
    out = []
    for r, n in enumerate(ROWS):
        c0 = rng.integers(0, min(40, n), size=n)
        c1 = rng.integers(0, min(12, n), size=n)
        c2 = rng.permutation(n).astype(np.uint64) + np.uint64(B63 + (r << 20))
        c3 = np.where(rng.integers(0, 2, size=n) == 1, c0, rng.integers(0, min(40, n), size=n))
        out.append([np.ascontiguousarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)])
    return out


SHAPES = {
    "two join-less bindings": ([0, 1], [], [], [(0, 2), (1, 2), (1, 0)]),
    "a chain and a lone binding": ([0, 1, 2, 1], [(0, 0, 1, 0), (1, 1, 2, 1)], [(0, 2, "<", B63 + 150)], [(0, 2), (3, 2), (2, 2)]),
    "a lone binding first": ([2, 0, 1], [(2, 0, 1, 0)], [], [(1, 2), (0, 2)]),
    "two chains": ([0, 1, 2, 1, 2], [(0, 0, 1, 0), (3, 1, 4, 1), (1, 1, 2, 1)], [(3, 0, "<", 30)], [(4, 2), (0, 2), (3, 2), (2, 0)]),
    "two chains, interleaved bindings": ([1, 2, 0, 1], [(3, 0, 1, 0), (0, 1, 2, 1)], [], [(0, 2), (1, 2), (2, 2), (3, 2)]),
    "three one-binding components": ([0, 1, 2], [], [(1, 0, "<", 20)], [(0, 2), (2, 2), (1, 2)]),
    "eight one-binding components": ([2, 3, 1, 2, 0, 2, 3, 1], [], [(4, 1, "=", 3), (2, 0, ">", 4)], [(k, 2) for k in range(8)]),
    "a relation bound in two components": ([1, 1], [], [(0, 0, "<", 10)], [(0, 2), (1, 2)]),
    "a relation bound in two chains": ([0, 1, 0, 1], [(0, 0, 1, 0), (2, 1, 3, 1)], [(2, 2, "<", B63 + 40)], [(0, 2), (2, 2), (3, 2), (1, 2)]),
    "all views in one component, stand-ins by a filter and by a predicate": ([0, 1, 2, 1, 2], [(1, 1, 2, 1), (3, 0, 4, 0)], [(0, 0, "<", 5)], [(1, 2), (2, 2)]),
    "all views in one component, a stand-in on column 0": ([2, 1, 0], [(1, 0, 2, 0)], [], [(1, 2), (2, 3)]),
    "a view-less component emptied by its filter": ([0, 1], [], [(1, 0, ">", 10 ** 6)], [(0, 2)]),
    "a viewed component emptied by its filter": ([0, 1], [], [(0, 0, ">", 10 ** 6)], [(0, 2)]),
    "a component emptied by its join": ([0, 1, 2], [(1, 2, 2, 2)], [], [(0, 2), (1, 2)]),
    "a triangle beside a tree": ([1, 2, 1, 0, 2], [(0, 0, 1, 0), (1, 1, 2, 1), (2, 3, 0, 3), (3, 1, 4, 1)], [], [(0, 2), (3, 2), (2, 2), (4, 2)]),
    "a two-column key beside a one-binding predicate": ([0, 1, 0], [(0, 0, 1, 0), (0, 1, 1, 1), (2, 0, 2, 3)], [], [(0, 2), (2, 2), (1, 2)]),
    "2049 rows without a join": ([4, 2], [], [], [(0, 2), (1, 2), (0, 0)]),
    "2049 rows in a chain": ([4, 1, 2], [(0, 0, 1, 0)], [(2, 0, "<", 9)], [(0, 2), (2, 2)]),
    "2049 rows under a one-binding predicate": ([3, 4], [(1, 0, 1, 3)], [], [(1, 2), (0, 2)]),
}
ORDINARY = [
    ([0, 1], [(0, 0, 1, 0)], [(0, 2, "<", B63 + 200)], [(0, 2), (1, 2)]),
    ([1, 2, 1], [(0, 0, 1, 0), (1, 1, 2, 1), (2, 3, 0, 3)], [], [(0, 2), (2, 2)]),                 # a true cycle
    ([4], [], [(0, 1, "=", 2)], [(0, 2), (0, 0)]),
    ([0, 1, 2], [(0, 0, 1, 0), (0, 1, 1, 1), (1, 1, 2, 1)], [], [(2, 2), (0, 2)]),
    ([2, 1], [(0, 2, 1, 2)], [], [(0, 2)]),                                                        # no match
]


class World:
    """the relations on the host and on the device, and the model's answers, computed once"""

    def __init__(self, rhj):
        self.rels = relations()
        self.cols = [[dev(rhj, c) for c in rel] for rel in self.rels]
        self.want = {}

    def answer(self, query):
        key = repr(query)
        if key not in self.want:
            sums, rows = pm.answer(self.rels, query)
            self.want[key] = (list(sums), rows)
        return self.want[key]


@pytest.fixture(scope="module")
def world(rhj):
    return World(rhj)


def test_the_shapes_are_what_their_names_say(world):
    ks = {name: max(pm.components(q)) + 1 for name, q in SHAPES.items()}
    assert all(k >= 2 for k in ks.values()) and ks["eight one-binding components"] == 8 and ks["three one-binding components"] == 3
    assert all(max(pm.components(q)) == 0 for q in ORDINARY)
    empty = [name for name, q in SHAPES.items() if world.answer(q)[1] == 0]
    assert empty == ["a view-less component emptied by its filter", "a viewed component emptied by its filter", "a component emptied by its join"]
    for name, q in SHAPES.items():
        if name not in empty:
            assert all(s > 0 for s in world.answer(q)[0]), name
    # the component that empties the third of them has rows on both sides of its join, and the other component has rows
    parts = pm.expand(SHAPES["a component emptied by its join"])
    assert run_query(world.rels, parts[0][0])[1] == 300 and run_query(world.rels, parts[1][0])[1] == 0


@pytest.mark.parametrize("setting", SETTINGS)
def test_every_shape_alone_and_all_in_one_batch(rhj, world, setting):
    names = sorted(SHAPES)
    for name in names:
        got, info, _ = run(rhj, world.cols, [SHAPES[name]], setting)
        assert got == [world.answer(SHAPES[name])], name
        assert info.products_info == {"product_queries": 1, "components": max(pm.components(SHAPES[name])) + 1}, name
    got, info, stats = run(rhj, world.cols, [SHAPES[n] for n in names], setting)
    for name, g in zip(names, got):
        assert g == world.answer(SHAPES[name]), name
    assert info.products_info == {"product_queries": len(names), "components": sum(max(pm.components(SHAPES[n])) + 1 for n in names)}
    assert stats["n_r"] == len(names) and stats["matches"] == sum(r for _, r in got) & M64 and stats["path"] == "query_batch"


@pytest.mark.parametrize("setting", SETTINGS)
def test_a_mixed_batch_leaves_the_ordinary_queries_their_answers(rhj, world, setting):
    names = sorted(SHAPES)
    queries, ordinary = [], []
    for k, name in enumerate(names):                     # P O P O ... P P P: the ordinary ones, a cyclic one among them, in between
        queries.append(SHAPES[name])
        if k < len(ORDINARY):
            ordinary.append(len(queries))
            queries.append(ORDINARY[k])
    got, info, stats = run(rhj, world.cols, queries, setting)
    alone, info_alone, stats_alone = run(rhj, world.cols, ORDINARY, setting, products=False)
    assert [got[i] for i in ordinary] == alone
    assert alone == [(list(s), r) for s, r in (run_query(world.rels, q) for q in ORDINARY)]
    for q, g in zip(queries, got):
        assert g == world.answer(q), q
    assert info.products_info == {"product_queries": len(names), "components": sum(max(pm.components(SHAPES[n])) + 1 for n in names)}
    assert info_alone.products_info == NO_PRODUCTS
    assert stats["n_r"] == len(queries) and stats["matches"] == sum(r for _, r in got) & M64 and stats["path"] == "query_batch"
    assert stats_alone["n_r"] == len(ORDINARY) and stats_alone["matches"] == sum(r for _, r in alone)
    # the switch on over a batch without a product: the same call as with it off
    on, info_on, stats_on = run(rhj, world.cols, ORDINARY, setting)
    assert on == alone and info_on.products_info == NO_PRODUCTS and dict(info_on) == dict(info_alone)
    assert (stats_on["n_r"], stats_on["matches"]) == (stats_alone["n_r"], stats_alone["matches"])


def test_switch_off_a_cross_product_is_refused(rhj, world):
    all_off(rhj)
    with pytest.raises(ValueError):
        rhj.query_batch_device(world.cols, [ORDINARY[0], SHAPES["two join-less bindings"]])


def test_the_infos_count_the_internal_batch(rhj, world):
    queries = [([0, 1, 2], [], [], [(0, 2), (2, 2)]), ORDINARY[0], ([2, 1], [], [(0, 0, "<", 9)], [(1, 2)])]
    got, info, stats = run(rhj, world.cols, queries, "folds")
    assert got == [world.answer(q) for q in queries]
    assert info.products_info == {"product_queries": 2, "components": 5}
    assert info.fold_info["fold_queries"] == 6           # five components and the ordinary query, all alive after the filters
    assert info.fold_self_info["self_items"] == 5 and info["filter_calls"] == 1
    assert stats["n_r"] == 3 and stats["matches"] == sum(r for _, r in got)
    got, info, _ = run(rhj, world.cols, queries, "one wait")
    assert got == [world.answer(q) for q in queries]
    assert info.one_wait_info["queries"] == 6 and info.one_wait_info["waits"] == 1 and info.fold_info["fold_queries"] == 0
    got, info, _ = run(rhj, world.cols, queries, "levels")
    assert got == [world.answer(q) for q in queries]
    assert info["levels"] == 1 and info["apply_calls"] == 1 and info.fold_info["fold_queries"] == 0


def test_a_component_without_a_column_needs_no_device_work(rhj, mod, world):
    """a relation with rows and no column can only be bound without a predicate, a filter or a view: its component is its rows"""
    cols = [world.cols[1], []]
    rels, keep_rels = rhj.device_relations(cols)
    rels[1].num_tuples = 7
    q = ([0, 1, 1], [], [(0, 0, "<", 10)], [(0, 2), (0, 0)])
    sums, rows = run_query(world.rels[1:2], ([0], [], q[2], q[3]))
    assert rows > 0
    for setting in SETTINGS:
        arr, keep = mod.query_descs([q])
        switches(rhj, setting)
        try:
            assert rhj.lib.rhj_query_batch_device(rels, 2, arr, 1) == 0
            info = rhj.lib.rhj_query_batch_last_products_info().contents.as_dict()
        finally:
            all_off(rhj)
        assert (list(arr[0].sums[:2]), arr[0].rows, arr[0].rc) == ([s * 49 & M64 for s in sums], rows * 49, 0)
        assert info == {"product_queries": 1, "components": 3}


@pytest.mark.parametrize("setting", SETTINGS)
def test_more_components_than_a_chunk_of_the_inner_batches(rhj, setting):
    """600 queries of eight one-binding components, every binding under a filter: 4800 filter items, and 4800 items of the first
    apply call, of the fold-self call or of a program's pred launch, where a chunk holds 4096"""
    rng = np.random.default_rng(303030)
    rels = []
    for r, n in enumerate((16, 11, 5, 1)):
        rels.append([np.ascontiguousarray(c, dtype=np.uint64) for c in (rng.integers(0, 6, size=n), rng.permutation(n).astype(np.uint64) + np.uint64(B63 + (r << 8)))])
    cols = [[dev(rhj, c) for c in rel] for rel in rels]
    queries = []
    for k in range(600):
        bind = [int(x) for x in rng.integers(0, 4, size=8)]
        filters = [(b, 1, ">", B63 - 1) if (k + b) % 3 == 0 else (b, 0, ">", 100) if rng.integers(0, 12) == 0 else (b, 0, "<", int(rng.integers(2, 8))) for b in range(8)]
        queries.append((bind, [], filters, [(int(b), 1) for b in rng.permutation(8)[:1 + k % 8]]))
    want = [pm.answer(rels, q) for q in queries]
    alive = sum(run_query(rels, part)[1] > 0 for q in queries for part, _ in pm.expand(q))
    assert 100 < sum(r > 0 for _, r in want) < 600 and 4096 < alive < 4800
    got, info, stats = run(rhj, cols, queries, setting)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == (list(w[0]), w[1]), k
    assert info.products_info == {"product_queries": 600, "components": 4800}
    assert stats["n_r"] == 600 and stats["matches"] == sum(r for _, r in want) & M64
    if setting == "folds":
        assert info.fold_self_info["self_calls"] == 1 and info.fold_self_info["self_items"] == info.fold_info["fold_queries"] == alive
    if setting == "one wait":
        assert info.one_wait_info["queries"] == info.one_wait_info["pred_items"] == 4800 and info.one_wait_info["programs"] >= 2


@pytest.mark.parametrize("setting", ("levels", "folds"))
def test_a_product_of_two_to_the_64_rows_reads_as_empty(rhj, setting):
    """rows is reported modulo 2^64 and 0 reads as empty: 2^22 * 2^22 * 2^20 rows, no component empty, give rows 0
    and sums 0; the neighbour without the second binding has 2^42 rows and its sums"""
    torch = rhj.torch
    cols = [[torch.full((1 << 22,), 3, dtype=torch.int64, device=rhj.dev)], [torch.full((1 << 22,), 5, dtype=torch.int64, device=rhj.dev)],
            [torch.full((1 << 20,), 7, dtype=torch.int64, device=rhj.dev)]]
    whole = ([0, 1, 2], [], [], [(0, 0), (2, 0)])
    less = ([0, 2], [], [], [(0, 0), (1, 0)])
    more = ([0, 1, 2], [], [(1, 0, "=", 5)], [(1, 0)])
    got, info, stats = run(rhj, cols, [whole, less, more], setting)
    assert got == [([0, 0], 0), ([3 << 42, 7 << 42], 1 << 42), ([0], 0)]
    assert info.products_info == {"product_queries": 3, "components": 8}
    assert stats["n_r"] == 3 and stats["matches"] == 1 << 42


def test_parity_with_the_librarys_own_cartesian_operator(rhj, mod, world):
    """the same sums through the reference-named operators of the library: Filter, the two joins (RadixHashJoin with
    InsertJoinToInterResults, the second one opening a second node), CartesianInterResults, then the view sums over the product's
    row-id tables, driven as tests/test_gpu_inter.py drives them (its `cartesian` plan's form)"""
    lib = rhj.lib
    rels = [world.rels[2], world.rels[1]]
    value = int(rels[0][1][0])
    qrel = [0, 0, 0, 1]
    plan = [("filter", 0, 1, "=", value), ("join", 0, 0, 1, 0), ("join", 2, 1, 3, 1), ("cartesian",)]
    query = (qrel, [(0, 0, 1, 0), (2, 1, 3, 1)], [(0, 1, "=", value)], [(0, 2), (1, 2), (2, 2), (3, 2)])
    want = pm.answer(rels, query)
    assert 0 < want[1] <= 10 ** 4 and pm.components(query) == [0, 0, 1, 1]
    rm, keep = make_map(mod, rels)
    engines = [Engine(mod, lib, rhj), Engine(mod, lib, rhj)]
    rhj.set_bits(4)
    final = run_plan(engines, mod, rm, qrel, plan)
    assert len(final) == 1 and final[0][0] == want[1]
    n, tabs = final[0]
    node = engines[1].head.contents.data.contents
    lib.rhj_sum_gather_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    sums = []
    for j in range(4):
        dcol = dev(rhj, rels[qrel[j]][2])
        s = C.c_uint64(0)
        assert lib.rhj_sum_gather_device(dcol.data_ptr(), node.table[j], n, C.byref(s)) == 0
        assert s.value == int(rels[qrel[j]][2][tabs[j]].sum(dtype=np.uint64))
        sums.append(s.value)
    for e in engines:
        e.L.FreeInterResults(e.head)
    cols = [[dev(rhj, c) for c in rel] for rel in rels]
    for setting in SETTINGS:
        got, _, _ = run(rhj, cols, [query], setting)
        assert got == [(sums, n)] and got == [(list(want[0]), want[1])], setting
