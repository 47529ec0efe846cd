"""rhj_query_batch_device (include/rhj_inter.h): a batch of queries run level by level through the filter, equality, join and
apply batches.  The `small` workload against the reference's recorded result lines; synthetic queries against the plain numpy
executor of query_model.py (itself held to those result lines by test_query_batch_rule.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from query_model import call_counts, parse_work, run_query, track_kinds
from query_shapes import CASES, ROWS, synthetic_relations

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def rhj(mod):
    r = mod.RHJ(device=0)
    r.lib.rhj_set_timing(2)
    r.set_bits(4)
    yield r
    r.lib.rhj_set_timing(2)
    r.lib.rhj_set_order(0)
    r.set_bits(4)


def dev(rhj, a):
    return rhj.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


# ---- the `small` workload ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_counts(golden):
    """what rhj_query_batch_last_info() must say after the `small` workload, at any radix width and order mode: the counts are of
    calls, not of launches"""
    rels = golden.small_relations
    return call_counts([rels["r%d" % r] for r in range(len(rels))], parse_work(golden.small["work_lines"]))[0]


@pytest.mark.parametrize("order", ("4 bits", "any"))
def test_small_workload_in_one_call(rhj, golden, small_counts, order):
    rels = golden.small_relations
    cols = [[dev(rhj, c) for c in rels["r%d" % r]] for r in range(len(rels))]
    queries = parse_work(golden.small["work_lines"])
    assert len(queries) == 50
    rhj.set_bits(4)
    rhj.lib.rhj_set_order(1 if order == "any" else 0)
    try:
        res, info = rhj.query_batch_device(cols, queries, with_info=True)
    finally:
        rhj.lib.rhj_set_order(0)
    lines = [" ".join("NULL" if rows == 0 else str(s) for s in sums) for sums, rows in res]
    assert lines == golden.small["result_lines"]
    assert all((rows == 0) == ("NULL" in line) for (_, rows), line in zip(res, golden.small["result_lines"]))
    assert info["levels"] == 3 and info["filter_calls"] == 1 and info["apply_calls"] == 3
    assert info == small_counts         # every count, from the numpy executor alone
    assert info["eq2_calls"] >= 1                        # (six of its predicates are equalities inside a node)
    st = rhj.stats()
    assert st["path"] == "query_batch" and st["n_r"] == 50 and st["matches"] == sum(rows for _, rows in res) and st["ms_total"] > 0


# ---- synthetic queries ---------------------------------------------------------------------------------------------------------------
# The relations (1, 100 and 5000 rows) and the 24 CASES live in query_shapes.py: test_gpu_query_batch_edges.py runs them again at
# other settings.

@pytest.fixture(scope="module")
def relations():
    return synthetic_relations()


def test_synthetic_queries_against_the_numpy_executor(rhj, relations):
    cols = [[dev(rhj, c) for c in rel] for rel in relations]
    names = sorted(CASES)
    queries = [CASES[k] for k in names]
    want = {k: run_query(relations, CASES[k]) for k in names}
    # the cases are what their names say
    assert {len(q[1]) for q in queries} >= {0, 1, 2, 3, 4, 7}
    for k in ("a filter without a hit", "a filter without a hit, no join", "no match at the first level", "no match at the last level", "a self-join without a match"):
        assert want[k][1] == 0, k
    for k in names:
        if k not in ("a filter without a hit", "a filter without a hit, no join", "no match at the first level", "no match at the last level",
                     "a self-join without a match"):
            assert want[k][1] > 0, k
    assert want["a relation bound twice, no filter"][1] > ROWS[1] and want["fan-out on the large relation"][1] > ROWS[2]      # (the second join call)
    assert track_kinds(CASES["two predicates between two bindings"]) == [0, 1] and track_kinds(CASES["two nodes merge, then an equality"]) == [0, 0, 0, 1]
    assert any(s < (1 << 62) for s in want["no join and no filter"][0])                                                        # (a sum that wrapped)
    rhj.set_bits(4)
    res, info = rhj.query_batch_device(cols, queries, with_info=True)
    for k, got in zip(names, res):
        assert (list(got[0]), got[1]) == (want[k][0], want[k][1]), k
    assert info["levels"] == 7 and info["filter_calls"] == 1 and info["apply_calls"] == 7
    assert info == call_counts(relations, queries)[0]    # every count, from the numpy executor alone
    assert info["eq2_calls"] >= 2 and info["join_calls"] == 7 and 1 <= info["join_reruns"] <= 7
    assert rhj.stats()["matches"] == sum(want[k][1] for k in names)

    # every query alone gives what it gives in the batch
    for k in ("a self-join alone", "no join and no filter, one row", "a filter without a hit", "two two-binding nodes merge"):
        (sums, rows), = rhj.query_batch_device(cols, [CASES[k]])
        assert (sums, rows) == (want[k][0], want[k][1]), k

    # state: the same batch again, and once more after the workspace was dropped
    again = rhj.query_batch_device(cols, queries)
    rhj.lib.rhj_release()
    rhj.torch.cuda.synchronize()
    fresh, info2 = rhj.query_batch_device(cols, queries, with_info=True)
    assert again == res and fresh == res and info2 == info


def test_an_invalid_query_in_the_middle_leaves_every_sum_untouched(rhj, mod, relations):
    cols = [[dev(rhj, c) for c in rel] for rel in relations]
    rels, keep = rhj.device_relations(cols)
    for bad in (([1, 2], [], [], [(0, 0)]),                               # two nodes left: a cross product
                ([1, 2], [(0, 1, 1, 3)], [], [(0, 0)]),                   # column 3 of 3
                ([1, 3], [(0, 1, 1, 1)], [], [(0, 0)])):                  # relation 3 of 3
        arr, keep2 = mod.query_descs([CASES["no filter"], bad, CASES["a self-join alone"]])
        for d in arr:
            d.rc, d.rows = -77, 0xDEAD
            for k in range(mod.QUERY_MAX_VIEWS):
                d.sums[k] = 0xBEEF
        assert rhj.lib.rhj_query_batch_device(rels, len(cols), arr, 3) == -3
        assert [d.rc for d in arr] == [0, -3, 0]
        assert all(d.rows == 0xDEAD and list(d.sums) == [0xBEEF] * mod.QUERY_MAX_VIEWS for d in arr)
    with pytest.raises(ValueError):
        rhj.query_batch_device(cols, [CASES["no filter"], ([1, 2], [], [], [(0, 0)])])
    (sums, rows), = rhj.query_batch_device(cols, [CASES["no filter"]])
    assert (sums, rows) == run_query(relations, CASES["no filter"])
