"""The families of tests/query_shapes.py held to their regimes by the model alone (tests/query_model.py: the numpy executor and
call_counts), without a device: a shape that drifts out of the code path it was built for fails here.  And call_counts itself
against the counts recorded for the `small` workload and the synthetic queries."""
import numpy as np
import pytest

import query_shapes as qs
from query_model import INFO_FIELDS, LIMITS, call_counts, count_chunks, filter_takes, join_chunks_at_least, join_in_size, join_takes, parse_work, \
    run_query, trace_query, track_kinds

B63 = 1 << 63


def test_the_limits_are_what_the_documents_say():
    assert LIMITS.JOIN_MAX_TUPLES == 65536 and LIMITS.FILTER_MAX_ROWS == 4194304 and LIMITS.FILTER_MAX_ITEMS == 4096 and LIMITS.APPLY_MAX_ITEMS == 4096
    assert LIMITS.PT_MAX_BITS == 8 and LIMITS.APPLY_MAX_TERMS == 8 and LIMITS.QUERY_MAX_RELS == 8 and LIMITS.FILTER_MAX_TERMS == 4
    assert LIMITS.ARENA_BUDGET == 1 << 30 and LIMITS.JOIN_ARENA_FLOOR == 2 << 20      # (batch_place: "2.7 MB + 25 bytes a tuple"; the floor is below it)


def test_call_counts_on_the_small_workload(golden):
    rels = golden.small_relations
    cols = [rels["r%d" % r] for r in range(len(rels))]
    queries = parse_work(golden.small["work_lines"])
    info, detail = call_counts(cols, queries)
    assert set(info) == set(INFO_FIELDS)
    assert info["levels"] == 3 and info["filter_calls"] == 1 and info["apply_calls"] == 3
    assert info == {"levels": 3, "filter_calls": 1, "eq2_calls": 2, "join_calls": 3, "join_reruns": 2, "apply_calls": 3}
    assert sum(len(lv["eq"]) for lv in detail["levels"]) <= 6                           # (six of its predicates are equalities; a query may end before its own)
    assert info == call_counts(cols, queries, join_takes(order_any=True))[0]            # calls, not launches


def test_call_counts_on_the_synthetic_queries():
    rels, queries, want, info, detail = qs.reference("synthetic")
    assert info == {"levels": 7, "filter_calls": 1, "eq2_calls": 3, "join_calls": 7, "join_reruns": 1, "apply_calls": 7}
    assert len(detail["filters"]["items"]) == 13 and not detail["filters"]["alone"]
    for i, q in enumerate(queries):                       # the trace is the executor
        sums, rows, _, steps = trace_query(rels, q)
        assert (sums, rows) == want[i] and [s[0] for s in steps] == track_kinds(q)
    # a query that died adds nothing further: "no match at the first level" has one join item and no apply item
    i = sorted(qs.CASES).index("no match at the first level")
    assert [i in [j[0] for j in lv["joins"]] for lv in detail["levels"][:2]] == [True, False]
    assert all(i not in [a[0] for a in lv["apply"]] for lv in detail["levels"])


# ---- a: joins that run alone ----------------------------------------------------------------------------------------------------------

SETTINGS = {"9 bits": dict(bits=9), "11 bits": dict(bits=11), "14 bits": dict(bits=14), "8 bits": dict(bits=8), "small off": dict(bits=4, small=False),
            "any": dict(order_any=True)}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_a1_the_synthetic_queries_at_other_settings(setting):
    _, _, _, at4, d4 = qs.reference("synthetic")
    _, _, _, info, detail = qs.reference("synthetic", join_takes(**SETTINGS[setting]))
    assert info == at4                                    # the counts are of calls, not of launches
    joins = sum(len(lv["joins"]) for lv in detail["levels"])
    alone = sum(len(lv["join_alone"]) for lv in detail["levels"])
    assert joins == 30 and not any(lv["join_alone"] for lv in d4["levels"])
    if setting in ("9 bits", "11 bits", "14 bits", "small off"):
        assert alone == joins                             # nothing is batched
    if setting == "8 bits":
        assert alone == 0                                 # the last batched width


def test_a2_exactly_the_intended_joins_are_too_large():
    rels, queries, want, info, detail = qs.reference("join too large")
    assert len(rels[0][0]) == LIMITS.JOIN_MAX_TUPLES + 1 and 600 < len(np.unique(rels[0][0])) <= 700
    l0, l1 = detail["levels"]
    assert [(j[1], j[2]) for j in l0["joins"]] == [(65537, 100), (100, 65537), (65536, 100), (65537, 100)]      # the big side is R, S, and one tuple less
    assert [not join_in_size(j[1], j[2]) for j in l0["joins"]] == [True, True, False, True] and l0["join_alone"] == [0, 1, 3]
    assert detail["filters"]["items"] == [(2, 0, 65537, 65536)]
    # the alone-run join's pairs feed a rebuild (two terms), its vectors a batched join
    assert l0["apply"][3] == (3, l0["joins"][3][3], 2) and [j[0] for j in l1["joins"]] == [3] and l1["join_alone"] == []
    assert l1["joins"][0][1] == l0["joins"][3][3] > 0 and all(rows > 0 for _, rows in want)
    assert not l0["short"]


# ---- b: filters and equalities that run alone ------------------------------------------------------------------------------------------

def test_b1_a_filter_one_row_over_the_limit():
    rels, queries, want, info, detail = qs.reference("filter too large")
    assert len(rels[0][0]) == LIMITS.FILTER_MAX_ROWS + 1 and len(rels[1][0]) == LIMITS.FILTER_MAX_ROWS and len(rels[0]) == 3
    assert all(np.shares_memory(a, b) for a, b in zip(rels[0], rels[1])) and qs.B1_PREFIX == {1: (0, LIMITS.FILTER_MAX_ROWS)}
    f = detail["filters"]
    assert [(it[0], it[2]) for it in f["items"]] == [(0, 4194305), (1, 4194305), (2, 4194304)] and f["alone"] == [0, 1]
    assert [filter_takes(it[2]) for it in f["items"]] == [False, False, True]
    assert all(1 <= it[3] <= 20 for it in f["items"])                                   # a handful of rows
    assert len(queries[1][2]) == 2 and f["items"][0][3] == f["items"][2][3] + 1         # two terms; the prefix lacks the last row's hit
    assert all(rows > 0 for _, rows in want) and want[0] != want[2]
    assert len(np.unique(rels[0][1])) == len(rels[0][1])


def test_b2_an_equality_over_the_limit():
    rels, queries, want, info, detail = qs.reference("equality too large")
    assert len(rels[0][0]) == 2100 and len(np.unique(rels[0][0])) == 1 and sorted(np.unique(rels[0][2])) == [0, 1, 2]
    l0, l1, l2 = detail["levels"]
    assert [j[1:] for j in l0["joins"]] == [(2100, 2100, 4410000)] * 2 and l0["short"] == [0, 1] and l0["join_alone"] == []     # capacity 2100, the rerun's count 4 410 000
    assert [e[1:] for e in l1["eq"]] == [(4410000, 1471442)] * 2 and l1["eq_alone"] == [0, 1] and 4410000 > LIMITS.FILTER_MAX_ROWS
    assert [e[1:] for e in l2["eq"]] == [(1471442, 2100)] and l2["eq_alone"] == []
    assert [rows for _, rows in want] == [2100, 1471442]
    assert {a for a, _ in queries[0][3]} == {0, 1}                                        # views on both bindings
    assert info == {"levels": 3, "filter_calls": 0, "eq2_calls": 2, "join_calls": 1, "join_reruns": 1, "apply_calls": 3}


# ---- c: chunk cuts -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("chunk cuts", "chunk cuts, one short join"))
def test_c_every_inner_batch_is_cut(name):
    rels, queries, want, info, detail = qs.reference(name)
    n = len(queries)
    assert n == 4100 and len(rels[0][0]) == 40 and len(np.unique(rels[0][0])) == 6
    l0, l1 = detail["levels"]
    f = detail["filters"]["items"]
    assert len(f) == n > LIMITS.FILTER_MAX_ITEMS and len({q[2][0][3] for q in queries}) == n                  # a different constant each
    assert len(l0["joins"]) == n and len(l1["eq"]) == n > LIMITS.FILTER_MAX_ITEMS
    assert len(l0["apply"]) == n > LIMITS.APPLY_MAX_ITEMS and len(l1["apply"]) == n
    assert count_chunks(len(f), LIMITS.FILTER_MAX_ITEMS) == 2 and count_chunks(n, LIMITS.APPLY_MAX_ITEMS) == 2
    assert not l0["join_alone"] and join_chunks_at_least([(j[1], j[2]) for j in l0["joins"]]) >= 2
    assert all(rows > 0 for _, rows in want)                                                                  # no query empty
    assert [a[2] for a in l0["apply"]] == [2] * n                                                             # rebuilt vectors on both sides of every cut
    if name == "chunk cuts":
        assert l0["short"] == [] and max(j[3] for j in l0["joins"]) <= 40 and info["join_reruns"] == 0
    else:
        at = qs.C_SHORT_AT
        assert l0["short"] == [at] and l0["joins"][at][3] > 40 and info["join_reruns"] == 1
        assert at >= LIMITS.ARENA_BUDGET // LIMITS.JOIN_ARENA_FLOOR                                           # (the first chunk cannot hold that many joins)
        assert 0 < at < n - 1                                                                                 # neighbours on both sides keep their lists
    assert info == {"levels": 2, "filter_calls": 1, "eq2_calls": 1, "join_calls": 1, "join_reruns": int(name != "chunk cuts"), "apply_calls": 2}


@pytest.mark.parametrize("n", (4096, 4097))
def test_c_the_neighbours_of_the_filter_cut(n):
    rels, queries, want, info, detail = qs.reference("%d filters" % n)
    lv, = detail["levels"]
    assert len(queries) == n and len(detail["filters"]["items"]) == n and len(lv["eq"]) == n and len(lv["apply"]) == n and not lv["joins"]
    assert count_chunks(n, LIMITS.FILTER_MAX_ITEMS) == count_chunks(n, LIMITS.APPLY_MAX_ITEMS) == (1 if n == 4096 else 2)
    assert all(rows > 0 for _, rows in want)
    assert info == {"levels": 1, "filter_calls": 1, "eq2_calls": 1, "join_calls": 0, "join_reruns": 0, "apply_calls": 1}


# ---- d: the rerun ---------------------------------------------------------------------------------------------------------------------

def test_d_which_joins_run_again():
    rels, queries, want, info, detail = qs.reference("rerun mixed")
    l0, l1 = detail["levels"]
    assert len(l0["joins"]) == 5 and l0["short"] == [1, 3] and l0["join_alone"] == [3] and l0["rerun_alone"] == [1]
    nR, nS, m = l0["joins"][3][1:]
    assert nR == LIMITS.JOIN_MAX_TUPLES + 1 and m == nR + 2 > max(nR, nS)                 # short by two pairs
    assert len(l0["apply"]) == 5 and len(l1["apply"]) == 5 and all(len(q[1]) == 2 for q in queries)            # all five go on and end non-empty
    assert {a[0] for a in l1["apply"]} == set(range(5)) and all(rows > 0 for _, rows in want)
    assert l1["joins"] and l1["eq"] and not l1["short"]
    assert info["join_reruns"] == 1 and info["join_calls"] == 2
    # lists swapped between queries cannot give equal sums: the summed columns of different relations never meet
    spans = [(int(min(c.min() for c in r[1:])), int(max(c.max() for c in r[1:]))) for r in rels]
    low = sorted((lo & (B63 - 1), hi & (B63 - 1)) for lo, hi in spans)                    # (c1 is c2's range above 2^63)
    assert all(low[k][1] < low[k + 1][0] for k in range(len(low) - 1))
    assert len({tuple(s) for s, _ in want}) == 5

    _, q_all, want_all, info_all, d_all = qs.reference("rerun all")
    assert d_all["levels"][0]["short"] == list(range(len(q_all))) and d_all["levels"][0]["rerun_alone"] == [1] and info_all["join_reruns"] == 1
    assert all(rows > 0 for _, rows in want_all)
    _, q_none, want_none, info_none, d_none = qs.reference("rerun none")
    assert not any(lv["short"] for lv in d_none["levels"]) and info_none["join_reruns"] == 0 and info_none["join_calls"] == 2
    assert all(rows > 0 for _, rows in want_none)


# ---- e: descriptor limits -------------------------------------------------------------------------------------------------------------

def test_e_the_most_a_descriptor_holds():
    rels, queries, want, info, detail = qs.reference("descriptor limits")
    assert len(rels[0][0]) == 300 and len(np.unique(rels[0][0])) == 300
    chain, filters32, pairwise, twenty = queries
    assert all(len(q[0]) == LIMITS.QUERY_MAX_RELS and len(q[3]) == LIMITS.QUERY_MAX_VIEWS for q in queries)
    assert track_kinds(chain) == [0] * 7 + [1, 1] and len(chain[2]) == 16
    assert len(filters32[2]) == LIMITS.FILTER_MAX_TERMS * LIMITS.QUERY_MAX_RELS == 32 and all(sum(f[0] == b for f in filters32[2]) == 4 for b in range(8))
    assert track_kinds(pairwise) == [0] * 7 and track_kinds(twenty) == [0] * 7 + [1] * 13 and len(twenty[1]) == 20
    assert [rows for i, (_, rows) in enumerate(want) if i != 2] == [286] * 3 and 100 < want[2][1] < 286
    assert all(c == 0 for q in (chain, filters32, twenty) for _, c, _, cb in q[1][:7] for c in (c, cb)) and all((c, cb) == (0, 3) for _, c, _, cb in pairwise[1])
    assert len(rels[0]) == 4 and np.count_nonzero(rels[0][0] == rels[0][3]) < 10               # c0 = c3 joins a row with another one
    terms = {(a[0], l): a[2] for l, lv in enumerate(detail["levels"]) for a in lv["apply"]}
    assert terms[(0, 7)] == LIMITS.APPLY_MAX_TERMS == 8 and terms[(0, 8)] == 8              # level 7 rebuilds eight vectors, level 8 sums eight views
    assert [terms[(2, l)] for l in range(7)] == [2, 2, 2, 2, 4, 4, 8]                       # pairwise: the last join's two nodes have four bindings each
    assert all(terms[(3, l)] == 8 for l in range(6, 20))
    assert info == {"levels": 20, "filter_calls": 1, "eq2_calls": 13, "join_calls": 7, "join_reruns": 0, "apply_calls": 20}
    assert all(a[1] == 286 for lv in detail["levels"] for a in lv["apply"] if a[0] != 2)   # nothing changes after the filters
    sizes = [j[1:3] for lv in detail["levels"] for j in lv["joins"] if j[0] == 2]
    assert len(sizes) == 7 and sizes[0] == (286, 286) and max(sizes[-1]) < 286               # pairwise: rows are lost on the way, the bindings differ


# ---- f: empty relations ---------------------------------------------------------------------------------------------------------------

def test_f_relations_without_a_row():
    rels, queries, want, info, detail = qs.reference("empty relations")
    assert len(rels[2]) == 3 and all(len(c) == 0 for c in rels[2]) and rels[3] == []
    for i, q in enumerate(queries):
        assert (2 in q[0]) == (i in qs.EMPTY_ROLES) and 3 not in q[0]
        assert (want[i][1] == 0 and not any(want[i][0])) == (i in qs.EMPTY_ROLES)           # and the neighbours are alive
    roles = [queries[i] for i in qs.EMPTY_ROLES]
    assert roles[0][0] == [2] and not roles[0][1]                                            # the only binding of a no-join query
    assert roles[1][0][roles[1][1][0][0]] == 2 and roles[2][0][roles[2][1][0][2]] == 2       # the A side, the B side
    assert any(roles[3][0][f[0]] == 2 for f in roles[3][2])                                   # under a filter
    assert roles[4][0][2] == 2 and len(roles[4][1]) == 2                                      # the third binding
    busy = {a[0] for lv in detail["levels"] for k in ("eq", "joins", "apply") for a in lv[k]} | {it[0] for it in detail["filters"]["items"]}
    assert not busy & set(qs.EMPTY_ROLES)                                                     # such a query adds no item anywhere
    _, only, want_only, info_only, _ = qs.reference("empty only")
    assert info_only == {"levels": 2, "filter_calls": 0, "eq2_calls": 0, "join_calls": 0, "join_reruns": 0, "apply_calls": 0}
    assert want_only == [([0] * len(q[3]), 0) for q in only]


def test_f_a_level_that_nobody_survives():
    rels, queries, want, info, detail = qs.reference("no survivors")
    assert all(len(r[0]) > 0 for r in rels[:2]) and want == [([0], 0), ([0, 0], 0)]
    l0, l1 = detail["levels"]
    assert len(l0["joins"]) == 2 and all(j[1] and j[2] and j[3] == 0 for j in l0["joins"]) and l0["apply"] == []      # both took part, no item
    assert not (l1["joins"] or l1["eq"] or l1["apply"])
    assert info == {"levels": 2, "filter_calls": 1, "eq2_calls": 0, "join_calls": 1, "join_reruns": 0, "apply_calls": 1}


# ---- g: the tiny batch ----------------------------------------------------------------------------------------------------------------

def test_g_the_tiny_batch_uses_every_stage():
    rels, queries, want, info, detail = qs.reference("tiny")
    assert len(queries) == 3 and all(rows > 0 for _, rows in want)
    assert info["filter_calls"] == 1 and info["eq2_calls"] >= 1 and info["join_calls"] >= 1 and info["join_reruns"] >= 1 and info["apply_calls"] == info["levels"] == 3
    big = qs.reference("rerun mixed")[4]
    assert max(a[1] for lv in big["levels"] for a in lv["apply"]) > 100 * max(a[1] for lv in detail["levels"] for a in lv["apply"])   # every buffer grows


def test_sums_wrap_in_every_family():
    for name in qs.FAMILIES:
        rels, queries, want, _, _ = qs.reference(name)
        assert any(len(r) > 1 and len(r[1]) and int(r[1].min()) >= B63 for r in rels), name
        if name not in ("empty only", "no survivors"):
            assert any(0 < s < B63 for sums, rows in want if rows > 1 for s in sums), name       # (two values near 2^63 or more: a sum that wrapped)
