"""The query families tests/test_gpu_query_fold_edges.py runs on the fold route of rhj_query_batch_device,
built from fixed seeds with the generators of tests/fold_exact.py, and the readers of a fold plan that say what a query does
there: how deep a view sits, which way a predicate is written, how many rounds lie between a vector's write and its read, at
which round a query finishes.  tests/test_fold_exact.py holds every family to what it is named for, without a device.  Every
family function returns the same objects on every call; nobody changes them."""
import functools

import numpy as np

import fold_exact as fe
import join_fold_model as fm
from query_model import trace_query

M64 = fe.M64
PAIR_CAP = 200000                                         # a level of the pair route with more pairs: the query runs on the fold route only


# ---- what a query does on the route, read from its plan ---------------------------------------------------------------------------

def parents(query):
    """(root, {child: parent}, steps) of the plan"""
    root, steps = fm.fold_plan(query)
    return root, {c: p for c, p, _ in steps}, steps


def depths(query):
    """binding -> the folds between it and the root.  A view on a binding of depth d enters as a value of the binding's own
    fold and is then carried, as a vector of its own, through d - 1 further folds; a view on the root is lazy."""
    root, up, _ = parents(query)
    out = {}
    for b in range(len(query[0])):
        d, x = 0, b
        while x != root:
            d, x = d + 1, up[x]
        out[b] = d
    return out


def child_first(query):
    """per step whether its predicate is written child first (relA is the side that is folded away)"""
    _, up, steps = parents(query)
    written = {(a, b) for a, _, b, _ in query[1]}
    return [(c, p) in written for c, p, _ in steps]


def read_gaps(query):
    """per step that folds a binding with children of its own: its round minus the round that last wrote the binding's vectors"""
    _, _, steps = parents(query)
    out = []
    for c, p, r in steps:
        wrote = [r2 for _, p2, r2 in steps if p2 == c]
        if wrote:
            out.append(r - max(wrote))
    return out


def rounds(query):
    return parents(query)[2][-1][2] + 1


def zero_round(relations, query):
    """the round at which a weight total of 0 finishes the query on the route, None when none does (an empty filter is none)"""
    _, rows, issued = fm.fold_route(relations, query)
    return max(issued) if issued and rows == 0 else None


def sides(relations, query):
    """per predicate the two filtered key lists, as sets"""
    col = fe._Columns(relations, query[0])
    rows = fe.filtered_rows(relations, query, col)
    return [({col(a, ca)[i] for i in rows[a]}, {col(b, cb)[i] for i in rows[b]}) for a, ca, b, cb in query[1]]


def level_pairs(relations, query):
    """the pairs of every level of the pair route, as the numpy executor reports them"""
    return [s[3] for s in trace_query(relations, query)[3]]


def exact(relations, queries):
    """[(sums, rows)] modulo 2^64"""
    return [fe.modulo(fe.exact_tree(relations, q)) for q in queries]


# ---- family 1 and 2: random trees ---------------------------------------------------------------------------------------------------

RANDOM_SIZES = (1, 7, 63, 64, 65, 300, 500, 700, 900, 1200, 1500, 2047, 2048, 2049, 2100)
RANDOM_QUERIES = 203                                      # 29 of every node count 2..8


@functools.lru_cache(maxsize=None)
def random_trees():
    """(relations, queries): relations of 1..2100 rows, queries of 2..8 bindings in turn"""
    rng = np.random.default_rng(4150)
    relations = fe.random_relations(rng, RANDOM_SIZES)
    return relations, [fe.random_tree_query(rng, relations, 2 + k % 7) for k in range(RANDOM_QUERIES)]


@functools.lru_cache(maxsize=None)
def random_answers():
    return exact(*random_trees())


@functools.lru_cache(maxsize=None)
def random_dropped():
    """the positions whose pair route has a level beyond PAIR_CAP pairs"""
    relations, queries = random_trees()
    return frozenset(k for k, q in enumerate(queries) if max(level_pairs(relations, q)) > PAIR_CAP)


@functools.lru_cache(maxsize=None)
def relabelled():
    """[(position in random_trees, [(query, order, perm)] of three relabellings)] of thirty queries with three bindings or more, twenty of them with rows,
    sides swapped and predicates, filters and views shuffled"""
    rng = np.random.default_rng(4151)
    relations, queries = random_trees()
    wide = [k for k, q in enumerate(queries) if len(q[0]) >= 3]
    picked = sorted([k for k in wide if random_answers()[k][1]][::2][:20] + [k for k in wide if not random_answers()[k][1]][::4][:10])
    out = []
    for k in picked:
        perms = [rng.permutation(len(queries[k][0])).tolist() for _ in range(3)]
        out.append((k, [fe.relabel(queries[k], perm, rng) + (perm,) for perm in perms]))
    return out


# ---- family 3: aimed trees ----------------------------------------------------------------------------------------------------------

def chain(rels, cols=(0, 0)):
    return [(k, cols[0], k + 1, cols[1]) for k in range(len(rels) - 1)]


def written_child_first(query):
    """the query with every predicate turned so that the side the plan folds away comes first"""
    _, up, _ = parents(query)
    rels, joins, filters, views = query
    return rels, [(a, ca, b, cb) if up.get(a) == b else (b, cb, a, ca) for a, ca, b, cb in joins], filters, views


@functools.lru_cache(maxsize=None)
def aimed():
    """(relations, {name: query}).  Relations 0..3: 300 rows, 150 and 100 keys; relation 4 the same with c1 from keys of its own
    (behind `c1 > 0` and `c1 < 2^64 - 1` it matches nobody's); relation 5: 40 rows whose keys are 0 and 2^64 - 1 alone."""
    rng = np.random.default_rng(4152)
    relations = [fe.make_relation(rng, 300, 150, 100) for _ in range(4)]
    relations.append(fe.make_relation(rng, 300, 150, 100, base1=10 ** 6))
    relations.append(fe.make_relation(rng, 40, 2, 2))
    rank = lambda r, k: int(np.sort(relations[r][fe.RANK_COL])[k])
    own_keys = lambda b: [(b, 1, ">", 0), (b, 1, "<", M64)]
    five = lambda rels, third, last, flt: (rels, [(0, 0, 1, 0), (1, 0, 2, 0), third, last], flt, [(0, 2), (4, 3), (2, 4), (1, 1)])
    q = {
        "every predicate child first": written_child_first(([0, 1, 2, 3, 1], [(0, 0, 1, 0), (1, 1, 2, 1), (1, 0, 3, 1), (3, 0, 4, 0)], [(2, 4, "<", rank(2, 65))],
                                                           [(0, 2), (2, 3), (4, 2), (3, 4), (1, 0)])),
        "eight views on one leaf": ([0, 1, 2], chain([0, 1, 2]), [(2, 4, "<", rank(2, 200))], [(2, c) for c in (0, 1, 2, 3, 4, 2, 3, 1)]),
        "eight views on the root": ([0, 1, 2], chain([0, 1, 2]), [(0, 4, ">", rank(0, 40))], [(0, c) for c in (4, 3, 2, 1, 0, 3, 2, 2)]),
        "eight views of one column": ([3, 1, 2], chain([3, 1, 2], (1, 1)), [], [(1, 2)] * 8),
        "a view three folds below the root": ([0, 1, 2, 3, 0], chain(range(5)), [(4, 4, "<", rank(0, 64))], [(4, 2), (0, 3), (4, 4), (3, 2)]),
        "a vector read two rounds after its write": ([0, 1, 2, 3, 1], [(0, 0, 1, 0), (0, 1, 2, 1), (0, 0, 3, 0), (3, 1, 4, 1)], [], [(4, 2), (3, 3), (1, 2), (0, 2), (2, 3)]),
        "a relation bound three times": ([2, 2, 2], chain([2, 2, 2], (0, 1)), [(0, 4, "<", rank(2, 63)), (1, 3, ">", 1 << 62), (2, 0, "<", M64)], [(0, 2), (1, 2), (2, 2), (1, 4)]),
        "a filter on every binding": ([0, 1, 2, 3], [(1, 0, 0, 0), (1, 1, 2, 1), (3, 0, 1, 0)], [(0, 4, "<", rank(0, 250)), (1, 2, "<", M64 - (1 << 61)), (2, 0, ">", 0), (3, 4, ">", rank(3, 30)), (3, 3, ">", 1 << 60)],
                                      [(0, 2), (1, 3), (2, 2), (3, 3)]),
        "keys 0 and 2^64 - 1 across a predicate": ([5, 5, 0], [(0, 0, 1, 1), (2, 0, 1, 0)], [], [(0, 2), (1, 3), (2, 2)]),
        # chains of five, rooted at binding 1: round 0 folds 0 and 4, round 1 folds 3 into 2, round 2 folds 2 into the root
        "finished in the first round": five([0, 1, 2, 3, 4], (2, 0, 3, 0), (3, 1, 4, 1), own_keys(4)),
        "finished in the second of three rounds": five([0, 1, 2, 4, 3], (2, 1, 3, 1), (3, 0, 4, 0), own_keys(3)),
        "alive through three rounds": five([0, 1, 2, 3, 1], (2, 0, 3, 0), (3, 1, 4, 1), []),
    }
    return relations, q


# ---- family 4: beyond 2^64 ----------------------------------------------------------------------------------------------------------

BIG = 65537


@functools.lru_cache(maxsize=None)
def beyond():
    """(relations, {name: query}).  Relations 0..3: 65 537 rows, c0 the key 7 in every row, c1 the numbers 0..65 536 shuffled, c2
    anywhere in u64; relation 4: one row whose c0 is 5.  The chain has 65 537^4 rows.  In the tree, binding 0 (the one row)
    meets one row of binding 1 through c1, and binding 1's three children make that binding's weights total 65 537^4 while
    the query has 65 537^3 rows."""
    rng = np.random.default_rng(4153)
    relations = [[np.full(BIG, 7, dtype=np.uint64), rng.permutation(BIG).astype(np.uint64), rng.integers(0, 1 << 64, size=BIG, dtype=np.uint64)] for _ in range(4)]
    relations.append([np.array([5], dtype=np.uint64), np.array([11], dtype=np.uint64), rng.integers(0, 1 << 64, size=1, dtype=np.uint64)])
    q = {"a chain of four": ([0, 1, 2, 3], chain(range(4)), [], [(0, 2), (1, 2), (2, 2), (3, 2)]),
         "a subtotal in the middle": ([4, 0, 1, 2, 3], [(0, 0, 1, 1), (1, 0, 2, 0), (3, 0, 1, 0), (1, 0, 4, 0)], [], [(0, 2), (1, 2), (2, 2), (4, 2), (3, 1)])}
    return relations, q


def subtree(query, keep):
    """the query of the bindings `keep` alone (a connected part), renumbered in their order, with one view"""
    rels, joins, filters, _ = query
    at = {b: k for k, b in enumerate(keep)}
    return ([rels[b] for b in keep], [(at[a], ca, at[b], cb) for a, ca, b, cb in joins if a in at and b in at],
            [(at[a], c, op, v) for a, c, op, v in filters if a in at], [(0, 0)])


# ---- family 5: a weight total that is 0 modulo 2^64 --------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def limit_star():
    """(relations, first, last, order).  The hub, relation 0, has two rows with one c0 and two c1; relations 1 and 2 have 2048 and
    1024 rows of that c0; relation 3 has one row that meets the hub's row 0 through c1 (and two that meet nothing).  Six
    children on c0 (2048^3 * 1024^3 = 2^63 rows a hub row, 2^64 over the two) and relation 3 on c1.  `first` folds
    relation 3 first, `last` folds it last; the new view k of `last` is the view order[k] of `first`."""
    rng = np.random.default_rng(4154)
    values = lambda n: rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    relations = [[np.array([5, 5], dtype=np.uint64), np.array([1, 2], dtype=np.uint64), values(2)]]
    relations += [[np.full(n, 5, dtype=np.uint64), values(n), values(n)] for n in (2048, 1024)]
    relations.append([np.array([9, 1, 3], dtype=np.uint64), values(3), values(3)])
    first = ([0, 3, 1, 1, 1, 2, 2, 2], [(0, 1, 1, 0)] + [(0, 0, b, 0) for b in range(2, 8)], [], [(0, 2), (1, 1), (2, 1), (4, 2), (5, 1), (7, 2), (0, 1)])
    last, order = fe.relabel(first, [0, 7, 1, 2, 3, 4, 5, 6])
    return relations, first, last, order


# ---- family 6: more items in a round than a chunk takes ------------------------------------------------------------------------------

CHUNK_ITEMS = 4096


@functools.lru_cache(maxsize=None)
def chunked():
    """(relations, queries): twelve 8-row relations and 4097 two-binding queries over them, none finished by a filter"""
    rng = np.random.default_rng(4155)
    relations = [fe.make_relation(rng, 8, 4, 3) for _ in range(12)]
    queries = []
    for k in range(CHUNK_ITEMS + 1):
        rels = [k % 12, (k // 12 + k) % 12]
        join = (0, int(rng.integers(0, 2)), 1, int(rng.integers(0, 2)))
        flt = []
        if k % 3 == 0:
            b = int(rng.integers(0, 2))
            flt.append((b, fe.RANK_COL, "<", int(np.sort(relations[rels[b]][fe.RANK_COL])[int(rng.integers(1, 8))])))
        views = [(int(rng.integers(0, 2)), int(rng.integers(0, 5))) for _ in range(1 + k % 3)]
        queries.append((rels, [join if k % 2 else join[2:] + join[:2]], flt, views))
    return relations, queries


# ---- family 7: round buffers that grow and are used again for less -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grown():
    """(relations, query): a chain of three 50 000-row bindings with four views, two of them carried"""
    rng = np.random.default_rng(4156)
    relations = [fe.make_relation(rng, 50000, 50000, 40000) for _ in range(3)]
    return relations, ([0, 1, 2], [(0, 0, 1, 0), (2, 1, 1, 1)], [], [(2, 2), (0, 3), (2, 4), (1, 2)])


def small_batch():
    """(relations, queries, positions): every eighth of the random trees (every node count among them)"""
    relations, queries = random_trees()
    at = list(range(0, len(queries), 8))
    return relations, [queries[k] for k in at], at


# ---- what the aimed families are named for, asserted from the plan and the model alone ----------------------------------------------

def check_aimed():
    relations, q = aimed()
    views_at = lambda name, b: sum(1 for x, _ in q[name][3] if x == b)
    leaves = lambda query: set(range(len(query[0]))) - set(parents(query)[1].values())
    assert all(fm.folds(query) for query in q.values())
    assert all(child_first(q["every predicate child first"])) and len(q["every predicate child first"][1]) == 4
    assert views_at("eight views on one leaf", 2) == 8 and 2 in leaves(q["eight views on one leaf"]) and depths(q["eight views on one leaf"])[2] == 2
    assert views_at("eight views on the root", 0) == 8 and parents(q["eight views on the root"])[0] == 0
    assert q["eight views of one column"][3] == [(1, 2)] * 8 and depths(q["eight views of one column"])[1] == 1
    deep = q["a view three folds below the root"]
    assert depths(deep)[4] == 3 and views_at("a view three folds below the root", 4) == 2
    late = q["a vector read two rounds after its write"]
    assert parents(late) == (0, {1: 0, 2: 0, 3: 0, 4: 3}, [(1, 0, 0), (4, 3, 0), (2, 0, 1), (3, 0, 2)]) and read_gaps(late) == [2]
    thrice = q["a relation bound three times"]
    assert len(set(thrice[0])) == 1 and len({tuple(r) for r in fe.filtered_rows(relations, thrice)}) == 3
    assert {f[0] for f in q["a filter on every binding"][2]} == {0, 1, 2, 3}
    assert all({0, M64} <= a and {0, M64} <= b for a, b in sides(relations, q["keys 0 and 2^64 - 1 across a predicate"]))
    first, second, alive = q["finished in the first round"], q["finished in the second of three rounds"], q["alive through three rounds"]
    assert rounds(first) == rounds(second) == rounds(alive) == 3
    assert fm.fold_route(relations, first)[1:] == (0, {0: 2}) and fm.fold_route(relations, second)[1:] == (0, {0: 2, 1: 1})
    assert fm.fold_route(relations, alive)[1] > 0 and fm.fold_route(relations, alive)[2] == {0: 2, 1: 1, 2: 1}
    # none is finished by a filter, and all but the two above have rows
    for name, query in q.items():
        assert all(fe.filtered_rows(relations, query)), name
        assert (fe.exact_tree(relations, query)[1] > 0) == (name not in ("finished in the first round", "finished in the second of three rounds")), name


def check_beyond():
    relations, q = beyond()
    four, mid = q["a chain of four"], q["a subtotal in the middle"]
    assert fe.exact_tree(relations, four)[1] == BIG ** 4 > 1 << 64 and BIG ** 4 & M64
    root, up, steps = parents(mid)
    assert root == 0 and up == {1: 0, 2: 1, 3: 1, 4: 1} and steps[-1] == (1, 0, 3)
    below = fe.exact_tree(relations, subtree(mid, [1, 2, 3, 4]))[1]            # binding 1's weight total before the root's fold
    assert below == BIG ** 4 and below & M64 and fe.exact_tree(relations, mid)[1] == BIG ** 3 < 1 << 64


def check_limit_star():
    """the hub is the root in both numberings; relation 3 is folded first in the one and last in the other; six children leave
    the hub's two weights at 2^63 each"""
    relations, first, last, order = limit_star()
    assert parents(first)[0] == parents(last)[0] == 0
    assert parents(first)[2] == parents(last)[2] == [(b, 0, b - 1) for b in range(1, 8)]
    assert first[0][1] == 3 and last[0][7] == 3 and sorted(order) == list(range(len(first[3])))
    assert fe.exact_tree(relations, first)[1] == fe.exact_tree(relations, last)[1] == 1 << 63
    assert fe.exact_tree(relations, subtree(last, [0, 1, 2, 3, 4, 5, 6]))[1] == 1 << 64
