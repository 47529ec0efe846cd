"""tests/query_products_model.py, the restatement of rhj_set_query_products' expansion and combination, held to a
brute force that walks the whole cross product and to fold_exact.py run per component.  CPU only: nothing here loads the library."""
import numpy as np
import pytest

import fold_exact
import join_folds_model as sm
import query_products_model as pm

M64 = pm.M64


@pytest.fixture(scope="module")
def drawn():
    return pm.random_queries()


@pytest.fixture(scope="module")
def forests():
    return pm.random_forests()


def test_enough_random_queries_of_two_to_four_components(drawn):
    assert len(drawn) >= 150
    ks = [max(pm.components(q)) + 1 for _, q in drawn]
    assert set(ks) == {2, 3, 4}
    # every kind of component is among them: join-less, a chain, one with a predicate on one binding, one without a view
    parts = [p for _, q in drawn for p in pm.expand(q)]
    assert any(len(p[0][0]) == 1 and not p[0][1] for p in parts)
    assert any(len(p[0][0]) >= 3 for p in parts)
    assert any(any(a == b for a, _, b, _ in p[0][1]) for p in parts)
    assert any(not own for _, own in parts) and any(len(own) >= 2 for _, own in parts)
    assert any(pm.answer(rels, q)[1] == 0 for rels, q in drawn) and sum(pm.answer(rels, q)[1] > 0 for rels, q in drawn) >= 100


def test_model_equals_the_brute_force_over_the_whole_cross_product(drawn):
    for rels, q in drawn:
        sums, rows = sm.product_answer(rels, q)
        assert pm.answer(rels, q) == (sums if rows else [0] * len(sums), rows), q


def test_expansion_keeps_every_predicate_filter_and_view_once(drawn):
    for _, q in drawn:
        rels, joins, filters, views = q
        comp = pm.components(q)
        parts = pm.expand(q)
        assert len(parts) == max(comp) + 1
        assert sum(len(p[0][1]) for p in parts) == len(joins) and sum(len(p[0][2]) for p in parts) == len(filters)
        assert sorted(v for _, own in parts for v in own) == list(range(len(views)))
        for c, ((r, j, f, v), own) in enumerate(parts):
            mine = [b for b in range(len(rels)) if comp[b] == c]
            assert r == [rels[b] for b in mine] and len(v) == max(len(own), 1)
            assert [(mine[a], ca, mine[b], cb) for a, ca, b, cb in j] == [p for p in joins if comp[p[0]] == c]
            assert [(mine[a], col, op, x) for a, col, op, x in f] == [p for p in filters if comp[p[0]] == c]
            if own:
                assert [(mine[a], col) for a, col in v] == [views[k] for k in own]
            else:
                assert v == ([j[0][:2]] if j else [f[0][:2]] if f else [(0, 0)])
            assert max(pm.components((r, j, f, v))) == 0


def test_forests_equal_fold_exact_per_component_and_the_brute_force(forests):
    assert len(forests) >= 40
    for rels, q in forests:
        want = fold_exact.modulo(fold_exact.brute(rels, q))
        want = (want[0] if want[1] else [0] * len(want[0]), want[1])
        assert pm.exact_forest(rels, q) == want, q
        assert pm.answer(rels, q) == want, q


def test_a_component_without_a_column_contributes_its_rows():
    none = [[], [np.arange(5, dtype=np.uint64)]]
    q = ([0, 1], [], [], [(1, 0)])
    assert [p[0] for p in pm.expand(q, [0, 1])] == [None, ([1], [], [], [(0, 0)])]
    assert pm.answer(none, q) == ([0], 0)                  # (a relation without a column has no row)


def test_combination_in_unbounded_integers_reduced_at_the_end():
    # three components of 2^22, 2^22 and 2^20 rows: 2^64 rows read as empty
    parts = [(([7 << 22], 1 << 22), [0]), (([0], 1 << 22), []), (([9 << 20], 1 << 20), [1])]
    assert pm.combine(2, parts) == ([0, 0], 0)
    # one row fewer in a component: nothing is empty, and the sums wrap
    parts = [(([7 << 22], 1 << 22), [0]), (([0], 1 << 22), []), (([9 * ((1 << 20) - 1)], (1 << 20) - 1), [1])]
    rows = (1 << 44) * ((1 << 20) - 1)
    assert pm.combine(2, parts) == ([7 * rows & M64, 9 * rows & M64], rows & M64)
    # an empty component empties the query
    assert pm.combine(1, [(([5], 3), [0]), (([0], 0), [])]) == ([0], 0)
