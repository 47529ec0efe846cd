"""rhj_query_components and rhj_set_query_products (include/rhj_inter.h) as far as they go without a device: the
symbols and the info struct's layout, the component plan against a union-find restated in query_products_model.py, and the
validation of a batch that holds a cross product, which comes before any device is touched whatever the switch says."""
import ctypes as C
import importlib

import pytest

import query_products_model as pm
import query_shapes
from query_model import track_kinds
from test_query_batch_rule import GOOD, INVALID, SHAPES, fake_relations, spoiled

NEW_SYMBOLS = ("rhj_query_components", "rhj_set_query_products", "rhj_query_batch_last_products_info")
PRODUCT = ([0, 1, 2, 1], [(0, 1, 2, 3)], [(1, 0, "<", 9)], [(3, 1), (0, 0)])       # components {0, 2}, {1}, {3}


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def lib(mod):
    return mod.load_library()


@pytest.fixture
def products_on(lib):
    lib.rhj_set_query_products(1)
    yield
    lib.rhj_set_query_products(0)


def components(mod, lib, query, shapes=None):
    """(return value, comp) of rhj_query_components on one query"""
    arr, keep = mod.query_descs([query])
    comp = (C.c_int * mod.QUERY_MAX_RELS)(*([-1] * mod.QUERY_MAX_RELS))
    if shapes is None:
        return lib.rhj_query_components(C.byref(arr[0]), max(query[0]) + 1, None, comp), list(comp)[:len(query[0])]
    rels, keep2 = fake_relations(mod, shapes)
    return lib.rhj_query_components(C.byref(arr[0]), len(shapes), rels, comp), list(comp)[:len(query[0])]


def want(query):
    comp = pm.components(query)
    return max(comp) + 1, comp


def test_symbols_and_the_info_struct(mod, lib):
    for name in NEW_SYMBOLS:
        assert name in mod.INTER_SYMBOLS and hasattr(lib, name), name
    S = mod.QueryBatchProductsInfo
    assert [f for f, _ in S._fields_] == ["product_queries", "components"] and C.sizeof(S) == 8
    assert lib.rhj_query_batch_last_products_info().contents.as_dict() == {"product_queries": 0, "components": 0}


def shape_forms():
    """every query of tests/query_shapes.py, one of each form (two queries that differ in a filter's constant alone are one form)"""
    seen, out = set(), []
    for name in sorted(query_shapes.FAMILIES):
        for rels, joins, filters, views in query_shapes.FAMILIES[name]()[1]:
            key = (tuple(rels), tuple(joins), tuple((a, c, op) for a, c, op, _ in filters), tuple(views))
            if key not in seen:
                seen.add(key)
                out.append((list(rels), list(joins), list(filters), list(views)))
    return out


@pytest.fixture(scope="module")
def forms():
    return shape_forms()


def test_every_shape_is_one_component(mod, lib, forms):
    assert len(forms) >= len(query_shapes.CASES)
    for q in forms:
        assert track_kinds(q) is not None
        assert components(mod, lib, q) == (1, [0] * len(q[0])), q
        assert mod.query_components(lib, q) == [0] * len(q[0])


def test_every_shape_with_one_predicate_removed(mod, lib, forms):
    split = 0
    for q in forms:
        for l in range(len(q[1])):
            less = (q[0], q[1][:l] + q[1][l + 1:], q[2], q[3])
            got = components(mod, lib, less)
            assert got == want(less), less
            assert (got[0] > 1) == (track_kinds(less) is None)
            split += got[0] > 1
    assert split >= 20


def test_the_models_random_queries(mod, lib):
    ks = set()
    for rels, q in pm.random_queries():
        shapes = [(len(r[0]), len(r)) for r in rels]
        for sh in (shapes, None):
            assert components(mod, lib, q, sh) == want(q), q
        ks.add(want(q)[0])
    assert ks == {2, 3, 4}


def test_numbering_follows_the_lowest_binding(mod, lib):
    # the predicates name the high bindings first, and merged nodes take the A side's name: the numbering must not follow either
    q = ([0] * 8, [(7, 0, 5, 0), (6, 0, 1, 0), (5, 0, 2, 0)], [], [(0, 0)])
    assert components(mod, lib, q) == (5, [0, 1, 2, 3, 4, 2, 1, 2]) == want(q)
    assert components(mod, lib, ([0] * 8, [], [], [(3, 0)])) == (8, list(range(8)))
    assert components(mod, lib, PRODUCT, SHAPES) == (3, [0, 1, 0, 2])
    arr, keep = mod.query_descs([PRODUCT])
    assert lib.rhj_query_components(C.byref(arr[0]), 3, None, None) == 3              # (comp may be NULL)


@pytest.mark.parametrize("name", INVALID)
def test_the_invalid_forms_are_refused_as_by_the_levels(mod, lib, name):
    """-3 for every query rhj_query_levels refuses but the one it refuses for its nodes alone"""
    rels, keep = fake_relations(mod, SHAPES)
    bad = spoiled(name)
    negative = bad[2] is None
    if negative:
        bad = (bad[0], bad[1], [], bad[3])
    arr, keep2 = mod.query_descs([bad])
    if negative:
        arr[0].nfilters = -1
    assert lib.rhj_query_levels(C.byref(arr[0]), len(SHAPES), rels, None) == -3
    got = lib.rhj_query_components(C.byref(arr[0]), len(SHAPES), rels, None)
    assert got == (2 if name == "two nodes left" else -3)


def batch(mod, lib, queries, negative=()):
    """(return value, rcs, whether any sums or rows were written) of rhj_query_batch_device over fake relations"""
    rels, keep = fake_relations(mod, SHAPES)
    arr, keep2 = mod.query_descs(queries)
    for i in negative:
        arr[i].nfilters = -1
    for d in arr:
        d.rc, d.rows = -77, 0xDEAD
        for k in range(mod.QUERY_MAX_VIEWS):
            d.sums[k] = 0xBEEF
    rc = lib.rhj_query_batch_device(rels, len(SHAPES), arr, len(queries))
    written = any(d.rows != 0xDEAD or list(d.sums) != [0xBEEF] * mod.QUERY_MAX_VIEWS for d in arr[:len(queries)])
    return rc, [d.rc for d in arr[:len(queries)]], written


def test_switch_off_a_cross_product_is_refused_before_any_device(mod, lib):
    lib.rhj_set_query_products(0)
    assert batch(mod, lib, [GOOD, PRODUCT, GOOD]) == (-3, [0, -3, 0], False)
    assert batch(mod, lib, [PRODUCT]) == (-3, [-3], False)
    assert lib.rhj_query_batch_last_products_info().contents.as_dict() == {"product_queries": 0, "components": 0}


@pytest.mark.parametrize("name", [n for n in INVALID if n != "two nodes left"])
def test_switch_on_an_invalid_query_still_refuses_the_batch(mod, lib, products_on, name):
    bad = spoiled(name)
    negative = bad[2] is None
    if negative:
        bad = (bad[0], bad[1], [], bad[3])
    assert batch(mod, lib, [PRODUCT, GOOD, bad, PRODUCT], negative=(2,) if negative else ()) == (-3, [0, 0, -3, 0], False)
    assert lib.rhj_query_batch_last_products_info().contents.as_dict() == {"product_queries": 0, "components": 0}


def test_switch_on_the_levels_and_the_plans_keep_refusing_a_cross_product(mod, lib, products_on):
    rels, keep = fake_relations(mod, SHAPES)
    for q, r, nrel in ((PRODUCT, rels, len(SHAPES)), (PRODUCT, None, 3), (spoiled("two nodes left"), rels, len(SHAPES))):
        arr, keep2 = mod.query_descs([q])
        d = C.byref(arr[0])
        assert lib.rhj_query_levels(d, nrel, r, None) == -3
        assert lib.rhj_query_fold_plan(d, nrel, r, None, None) == -3
        assert lib.rhj_query_foldk_plan(d, nrel, r, None, None) == -3
        assert lib.rhj_query_folds_plan(d, nrel, r, None) == -3
        assert lib.rhj_query_foldn_plan(d, nrel, r, None) == -3
        assert lib.rhj_query_one_wait_plan(d, nrel, r) == -3
        assert lib.rhj_query_components(d, nrel, r, None) > 1
    with pytest.raises(ValueError):
        mod.query_folds_plan(lib, PRODUCT)
    assert mod.query_components(lib, PRODUCT) == [0, 1, 0, 2]


def test_the_binding_refuses_what_the_library_refuses(mod, lib):
    with pytest.raises(ValueError):
        mod.query_components(lib, ([0, 1], [(0, 0, 2, 0)], [], [(0, 0)]))
