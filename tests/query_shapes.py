"""The query batches tests/test_gpu_query_batch_edges.py runs, each built for one place where the driver of
rhj_query_batch_device (csrc/rhj_device.hip: query_filters, query_level_joins, query_rerun_short, query_level_apply,
query_take_back) hands over between its inner batches: items that run alone, chunk cuts inside a level, the second join call,
the limits of the descriptors, empty relations.  Every family is a function that returns (relations, queries) from a fixed
seed: relations[r][c] u64 numpy columns, queries as tests/query_model.py takes them.  tests/test_query_shapes.py holds every
family to its regime with the model alone.

A relation has three columns unless said otherwise: c0 the join key, c1 unique within the relation and near 2^63 (sums wrap),
c2 a small number.  Where lists swapped between queries must not give equal sums, every relation's c1 and c2 have a value range
of their own."""
import numpy as np

B63 = 1 << 63


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _rel(rng, n, keys, base=0, c2_mod=8):
    """n rows: c0 in 0..keys, c1 = 2^63 + base + a permutation of 0..n, c2 = base + (0..c2_mod)"""
    return [_u64(rng.integers(0, keys, size=n)), _u64(rng.permutation(n)) + np.uint64(B63 + base),
            _u64(rng.integers(0, c2_mod, size=n)) + np.uint64(base)]


# ---- the synthetic queries of tests/test_gpu_query_batch.py (family a1 runs them at other settings) -----------------------------------
# Relation r has ROWS[r] rows and three columns: c0 a key with many duplicates (a join on it fans out beyond max(nR, nS)), c1
# unique and near 2^63 (sums wrap), c2 equal to c0 in about half of the rows (the self-join) and a small number otherwise.

ROWS = (1, 100, 5000)


def synthetic_relations():
    rng = np.random.default_rng(10001)
    out = []
    for n in ROWS:
        c0 = rng.integers(0, max(n // 100, 1) * 5 if n > 1 else 1, size=n, dtype=np.uint64)
        c1 = rng.permutation(n).astype(np.uint64) + np.uint64(B63)
        c2 = np.where(rng.integers(0, 2, size=n) == 1, c0, rng.integers(0, 8, size=n, dtype=np.uint64)).astype(np.uint64)
        out.append([c0, c1, c2])
    return out


CASES = {
    "no filter": ([1, 2], [(0, 1, 1, 1)], [], [(0, 2), (1, 0)]),
    "four filters on one binding": ([2, 1], [(0, 1, 1, 1)], [(0, 0, ">", 5), (0, 0, "<", 200), (0, 2, ">", 1), (0, 1, "<", B63 + 4000)], [(0, 2), (1, 2)]),
    "filters on two bindings": ([1, 2], [(0, 0, 1, 0)], [(0, 1, "<", B63 + 50), (1, 1, "<", B63 + 2500)], [(0, 1), (1, 1), (1, 2)]),
    "no join, views through a filter": ([2], [], [(0, 0, "=", 7)], [(0, 1), (0, 2)]),
    "no join, two filters": ([1], [], [(0, 0, "<", 3), (0, 1, ">", B63 + 10)], [(0, 1)]),
    "no join and no filter": ([2], [], [], [(0, 2), (0, 0), (0, 1)]),
    "no join and no filter, one row": ([0], [], [], [(0, 1)]),
    "a filter without a hit": ([1, 2], [(0, 1, 1, 1)], [(1, 0, ">", 100000)], [(0, 0)]),
    "a filter without a hit, no join": ([1], [], [(0, 0, "=", 99)], [(0, 0), (0, 1)]),
    "no match at the first level": ([1, 2, 2], [(0, 1, 1, 0), (1, 1, 2, 1)], [], [(0, 0), (2, 2)]),
    "no match at the last level": ([1, 2, 2], [(0, 1, 1, 1), (1, 1, 2, 0)], [], [(0, 0), (2, 2)]),
    "a self-join first": ([2, 1], [(0, 0, 0, 2), (0, 1, 1, 1)], [], [(0, 2), (1, 2), (0, 1)]),
    "a self-join last": ([1, 2], [(0, 1, 1, 1), (1, 0, 1, 2)], [], [(0, 1), (1, 1)]),
    "a self-join alone": ([2], [(0, 2, 0, 0)], [(0, 1, "<", B63 + 3000)], [(0, 1)]),
    "a self-join without a match": ([2], [(0, 1, 0, 0)], [], [(0, 1)]),
    "a relation bound twice": ([2, 2], [(0, 0, 1, 0)], [(0, 1, "<", B63 + 100), (1, 1, "<", B63 + 200)], [(0, 1), (1, 1)]),
    "a relation bound twice, no filter": ([1, 1], [(0, 0, 1, 0)], [], [(0, 1), (1, 1), (1, 2)]),
    "two predicates between two bindings": ([1, 2], [(0, 1, 1, 1), (0, 0, 1, 2)], [], [(0, 2), (1, 0)]),
    "two two-binding nodes merge": ([1, 2, 1, 2], [(0, 1, 1, 1), (2, 1, 3, 1), (1, 0, 2, 0)], [], [(0, 1), (1, 1), (2, 1), (3, 1)]),
    "two nodes merge, then an equality": ([1, 2, 1, 2], [(0, 1, 1, 1), (2, 1, 3, 1), (1, 0, 2, 0), (0, 2, 3, 2)], [], [(3, 1), (0, 0)]),
    "eight bindings in a chain": ([1, 2, 1, 2, 1, 2, 1, 2], [(k, 1, k + 1, 1) for k in range(7)], [(7, 0, "<", 40)], [(k, (k + 1) % 3) for k in range(8)]),
    "one row joins": ([0, 1], [(0, 0, 1, 0)], [], [(0, 1), (1, 1)]),
    "fan-out on the large relation": ([2, 2], [(0, 0, 1, 0)], [(0, 1, "<", B63 + 300)], [(0, 1), (1, 1), (1, 2)]),
    "five bindings, four levels": ([1, 2, 2, 1, 2], [(0, 1, 1, 1), (1, 1, 2, 1), (3, 1, 2, 1), (2, 0, 4, 2)], [(4, 1, "<", B63 + 500)], [(4, 1), (0, 2)]),
}


def synthetic():
    """a1: the 24 cases in the order of their names, as one batch"""
    return synthetic_relations(), [CASES[k] for k in sorted(CASES)]


# ---- a2: a relation one tuple too large for the batched joins --------------------------------------------------------------------------

A2_BIG = 65537


def join_too_large():
    """relation 0 has 65 537 rows and about 700 keys, 1 and 2 have 100.  Queries 0 and 1 join it unfiltered, as the A and as the
    B side: both run alone.  Query 2 joins it through a filter that keeps 65 536 rows: batched.  Query 3 joins it unfiltered and
    then a third binding: the alone-run join's pairs feed a rebuild, and the rebuilt vectors a batched join."""
    rng = np.random.default_rng(20002)
    rels = [_rel(rng, A2_BIG, 700, base=0), _rel(rng, 100, 700, base=1 << 20), _rel(rng, 100, 700, base=1 << 21)]
    queries = [([0, 1], [(0, 0, 1, 0)], [], [(0, 1), (1, 1), (0, 2)]),
               ([1, 0], [(0, 0, 1, 0)], [], [(0, 1), (1, 1), (1, 2)]),
               ([0, 1], [(0, 0, 1, 0)], [(0, 1, "<", B63 + A2_BIG - 1)], [(0, 1), (1, 1), (0, 2)]),
               ([0, 1, 2], [(0, 0, 1, 0), (1, 0, 2, 0)], [], [(0, 1), (1, 1), (2, 1), (2, 2)])]
    return rels, queries


# ---- b1: a filter one row over the batched filters' limit ------------------------------------------------------------------------------

B1_BIG = 4194305


def filter_too_large():
    """relation 0 has 4 194 305 rows; relation 1 is its first 4 194 304 rows (the same arrays, sliced); relation 2 has 100 rows.
    Query 0 filters relation 0 down to a handful of rows with < on the unique column and joins; query 1 has two terms on it;
    query 2 does what query 0 does on the prefix, the batched neighbour, and lacks the last row's hit.  c1 = 2^63 +
    ((n - 1 - i) * 2654435761 mod 2^32) is unique."""
    rng = np.random.default_rng(30003)
    i = np.arange(B1_BIG, dtype=np.uint64)
    j = np.uint64(B1_BIG - 1) - i                         # (the last row has the smallest c1: every filter on relation 0 keeps it)
    big = [_u64(i % np.uint64(97)), (j * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)) + np.uint64(B63), _u64((i + np.uint64(3)) & np.uint64(7))]
    small = _rel(rng, 100, 97, base=1 << 40)
    rels = [big, [c[:B1_BIG - 1] for c in big], small]
    queries = [([0, 2], [(0, 0, 1, 0)], [(0, 1, "<", B63 + 9000)], [(0, 1), (1, 1), (0, 2)]),
               ([0, 2], [(0, 0, 1, 0)], [(0, 1, "<", B63 + 30000), (0, 2, "=", 3)], [(0, 1), (1, 1)]),
               ([1, 2], [(0, 0, 1, 0)], [(0, 1, "<", B63 + 9000)], [(0, 1), (1, 1), (0, 2)])]
    return rels, queries


B1_PREFIX = {1: (0, B1_BIG - 1)}                         # relation 1 is relation 0's first rows: one copy on the device


# ---- b2: an equality over a node one class too large ------------------------------------------------------------------------------------

B2_ROWS = 2100
B2_C2_COUNTS = (684, 685, 731)                           # 684^2 + 685^2 + 731^2 = 1 471 442 rows after c2 = c2


def equality_too_large():
    """one relation of 2100 rows with one key in c0, bound twice and joined on c0: 4 410 000 pairs, so the first join call is
    short and the second has room for 4.41 M pairs; then c2 = c2 over the 4.41 M-row node runs alone and leaves 1 471 442; then
    c1 = c1 leaves 2100.  Query 1 is the same and stops after the equality: a sum over 1.47 M rows."""
    rng = np.random.default_rng(40004)
    c2 = rng.permutation(np.repeat(np.arange(3), B2_C2_COUNTS))
    rels = [[_u64(np.full(B2_ROWS, 5)), _u64(rng.permutation(B2_ROWS)) + np.uint64(B63), _u64(c2)]]
    views = [(0, 1), (1, 1), (0, 2), (1, 2)]
    return rels, [([0, 0], [(0, 0, 1, 0), (0, 2, 1, 2), (0, 1, 1, 1)], [], views), ([0, 0], [(0, 0, 1, 0), (0, 2, 1, 2)], [], views)]


# ---- c: more items than a chunk of any inner batch holds ---------------------------------------------------------------------------------

C_ROWS, C_KEYS, C_STEP = 40, 6, 2000


def _chunk_relation():
    """40 rows, every key of 6 six or seven times, c1 = 2^63 + 2000 * (a permutation), c2 = c0 where the permutation is below 8
    (so a filter that keeps its first rows keeps a self-equality's hit) and 0..2 elsewhere"""
    rng = np.random.default_rng(50005)
    perm = rng.permutation(C_ROWS)
    c0 = rng.permutation(np.arange(C_ROWS) % C_KEYS)
    c2 = np.where(perm < 8, c0, rng.integers(0, 3, size=C_ROWS))
    return [[_u64(c0), _u64(perm * C_STEP) + np.uint64(B63), _u64(c2)]]


def _chunk_filter(k, keep=None):
    """query k's filter: c1 < a constant no other query has, which keeps `keep` rows (1 + k % 5 unless given)"""
    keep = 1 + k % 5 if keep is None else keep
    assert k // 5 + 1 < C_STEP
    return (0, 1, "<", B63 + C_STEP * (keep - 1) + 1 + k // 5)


def chunk_cuts(n=4100, short_at=None):
    """n queries over the relation bound twice: a filter, a join on c0, then c2 = c2 inside the node, two views.  A filter keeps at
    most five rows and a key has at most seven, so no join has more than 35 pairs for its 40: none is short — but query short_at,
    when given, whose filter keeps seven rows (42 pairs or more)."""
    queries = [([0, 0], [(0, 0, 1, 0), (0, 2, 1, 2)], [_chunk_filter(k, 7 if k == short_at else None)], [(0, 1), (1, 2)]) for k in range(n)]
    return _chunk_relation(), queries


def chunk_neighbours(n):
    """n queries with the join removed: a filter, then c0 = c2 on the one binding, two views"""
    return _chunk_relation(), [([0], [(0, 0, 0, 2)], [_chunk_filter(k)], [(0, 1), (0, 2)]) for k in range(n)]


# ---- d: which joins run a second time -------------------------------------------------------------------------------------------------

def _rerun_relations():
    rng = np.random.default_rng(60006)
    big = A2_BIG
    half = (big + 1) // 2                                # keys 0..32768: every key twice, the last once
    rels = [_rel(rng, 100, 100000, base=1 << 24),        # 0, 1: keys that hardly meet twice ...
            _rel(rng, 120, 100000, base=2 << 24),
            _rel(rng, 90, 5, base=3 << 24),              # 2, 3: ... and five keys, every pair a fan-out
            _rel(rng, 110, 5, base=4 << 24),
            [_u64(rng.permutation(np.arange(big) // 2)), _u64(rng.permutation(big)) + np.uint64(B63 + (5 << 24)),
             _u64(rng.integers(0, 8, size=big)) + np.uint64(5 << 24)],
            [_u64(rng.permutation(np.concatenate([np.arange(half), [0]]))), _u64(rng.permutation(half + 1)) + np.uint64(B63 + (6 << 24)),
             _u64(rng.integers(0, 8, size=half + 1)) + np.uint64(6 << 24)],
            _rel(rng, 50, 100000, base=7 << 24)]         # 6: the third binding of the second level
    rels[0][0][:60] = rels[1][0][:60]                    # (so the joins of 0 and 1 are not empty)
    rels[6][0][:] = np.concatenate([rels[0][0][:25], rels[4][0][:25]])
    return rels


def _rerun_query(which):
    """0: not short (relations 0, 1); 1: short and batched (2, 3); 2: short and alone (4 of 65 537 rows with every key twice, 5
    with every key once but key 0 twice: 65 539 pairs for 65 537).  All go on to a second level that reads the rebuilt vectors:
    a join with a third binding, or an equality inside the node."""
    if which == 0:
        return ([0, 1, 6], [(0, 0, 1, 0), (1, 0, 2, 0)], [], [(0, 1), (1, 1), (2, 1), (0, 2), (1, 2)])
    if which == 1:
        return ([2, 3], [(0, 0, 1, 0), (0, 0, 1, 0)], [], [(0, 1), (1, 1), (0, 2), (1, 2)])
    return ([4, 5, 6], [(0, 0, 1, 0), (0, 0, 2, 0)], [], [(0, 1), (1, 1), (2, 1), (0, 2), (1, 2)])


def rerun_mixed():
    """five joins at level 0, in this order: not short, short and batched, not short, short and alone, not short"""
    q0 = _rerun_query(0)
    return _rerun_relations(), [q0, _rerun_query(1), ([1, 0, 6], [(0, 0, 1, 0), (1, 0, 2, 0)], [], q0[3]), _rerun_query(2),
                                ([0, 1], [(0, 0, 1, 0), (0, 0, 1, 0)], [(0, 1, "<", B63 + (1 << 24) + 70)], [(0, 1), (1, 1)])]


def rerun_all():
    """every join of level 0 short"""
    return _rerun_relations(), [_rerun_query(1), _rerun_query(2), ([3, 2], [(0, 0, 1, 0), (0, 2, 0, 2)], [], [(0, 1), (1, 1), (1, 2)])]


def rerun_none():
    """no join short at any level"""
    rels, queries = rerun_mixed()
    return rels, [queries[0], queries[2], queries[4]]


# ---- e: the most a descriptor holds ---------------------------------------------------------------------------------------------------

E_ROWS = 300


def _limit_relation():
    """four columns: c3 is a second unique key, so that c0 = c3 joins a row with another one"""
    rng = np.random.default_rng(70007)
    return [[_u64(rng.permutation(E_ROWS)), _u64(rng.permutation(E_ROWS)) + np.uint64(B63), _u64(rng.integers(0, 8, size=E_ROWS)),
             _u64(rng.permutation(E_ROWS))]]


_CHAIN = [(k, 0, k + 1, 0) for k in range(7)]
_TWO_FILTERS = [f for b in range(8) for f in ((b, 0, ">", 3), (b, 0, "<", 290))]
_EIGHT_VIEWS = [(k, 1 + k % 2) for k in range(8)]


def descriptor_limits():
    """eight bindings of one 300-row relation with a unique key.  Query 0: seven joins in a chain, then two equalities (nine
    levels; level 7 rebuilds eight vectors), two filters on every binding, eight views: 286 rows.  Query 1: four filters on every
    binding, 32 in all.  Query 2: four two-binding nodes that merge pairwise and then once more, so the last join's B side has
    four bindings; it joins c0 with c3, so every binding of a row is another row of the relation (in the chains all eight are the
    same row, and a vector gathered through the wrong side would go unnoticed).  Query 3: 20 predicates, the chain and 13
    equalities that are all true."""
    four = [f for b in range(8) for f in ((b, 0, ">", 3), (b, 0, "<", 290), (b, 1, ">", B63 - 1), (b, 2, "<", 8))]
    pairwise = [(0, 0, 1, 3), (2, 0, 3, 3), (4, 0, 5, 3), (6, 0, 7, 3), (1, 0, 2, 3), (5, 0, 6, 3), (3, 0, 4, 3)]
    true = [(k % 8, 1 + k % 2, (k + 3) % 8, 1 + k % 2) for k in range(13)]
    return _limit_relation(), [([0] * 8, _CHAIN + [(0, 2, 7, 2), (1, 1, 6, 1)], _TWO_FILTERS, _EIGHT_VIEWS),
                               ([0] * 8, _CHAIN + [(0, 2, 7, 2), (1, 1, 6, 1)], four, _EIGHT_VIEWS),
                               ([0] * 8, pairwise, _TWO_FILTERS, _EIGHT_VIEWS),
                               ([0] * 8, _CHAIN + true, _TWO_FILTERS, _EIGHT_VIEWS)]


# ---- f: relations without a row -------------------------------------------------------------------------------------------------------

def empty_relations():
    """relations 0 and 1 have rows, 2 has three columns and no row, 3 has neither.  EMPTY_ROLES names the queries that bind
    relation 2; the others are their live neighbours.  No valid query can bind relation 3 (it has no column to join, filter or
    sum): it only sits in the relation array."""
    rng = np.random.default_rng(80008)
    none = np.zeros(0, dtype=np.uint64)
    rels = [_rel(rng, 50, 10, base=1 << 24), _rel(rng, 60, 10, base=2 << 24), [none, none.copy(), none.copy()], []]
    live = ([0, 1], [(0, 0, 1, 0)], [(0, 1, "<", B63 + (1 << 24) + 30)], [(0, 1), (1, 1), (1, 2)])
    queries = [live,
               ([2], [], [], [(0, 1), (0, 2)]),                                          # the only binding of a no-join query
               ([2, 0], [(0, 0, 1, 0)], [], [(0, 1), (1, 1)]),                           # the A side of a join
               ([1], [], [(0, 0, "<", 5)], [(0, 1)]),
               ([0, 2], [(0, 0, 1, 0)], [], [(0, 1), (1, 1)]),                           # the B side of a join
               ([2, 1], [(0, 0, 1, 0)], [(0, 1, ">", 5), (1, 0, "<", 5)], [(1, 1)]),     # under a filter
               ([0, 1, 2], [(0, 0, 1, 0), (1, 0, 2, 0)], [], [(0, 1), (2, 1)]),          # the third binding of a three-way join
               ([1, 0, 1], [(0, 0, 1, 0), (1, 0, 2, 0)], [], [(0, 1), (2, 1), (1, 2)])]
    return rels, queries


EMPTY_ROLES = (1, 2, 4, 5, 6)


def empty_only():
    rels, queries = empty_relations()
    return rels, [queries[i] for i in EMPTY_ROLES]


def no_survivors():
    """two queries with rows everywhere whose first join has no match (c0 is small, c1 near 2^63): level 0 has a join call and,
    because both took part, an apply call without an item; level 1 has nobody"""
    rels, _ = empty_relations()
    return rels, [([0, 1], [(0, 0, 1, 1), (0, 0, 1, 0)], [], [(0, 1)]), ([1, 0, 1], [(0, 1, 1, 0), (1, 0, 2, 0)], [(0, 0, "<", 5)], [(2, 1), (0, 2)])]


# ---- g: three tiny queries (the state tests run them between larger batches) ----------------------------------------------------------

def tiny():
    rng = np.random.default_rng(90009)
    rels = [_rel(rng, 30, 6, base=1 << 24), _rel(rng, 20, 6, base=2 << 24)]
    return rels, [([0, 1], [(0, 0, 1, 0)], [(0, 1, "<", B63 + (1 << 24) + 4)], [(0, 1), (1, 1)]),
                  ([1], [], [(0, 0, "<", 3)], [(0, 1), (0, 2)]),
                  ([0, 1, 0], [(0, 0, 1, 0), (1, 0, 2, 0), (0, 2, 2, 2)], [(0, 1, "<", B63 + (1 << 24) + 3)], [(0, 1), (2, 1), (1, 2)])]


# ---- every family by name, and its answers by the model (computed once a process) ----------------------------------------------------

FAMILIES = {
    "synthetic": synthetic,
    "join too large": join_too_large,
    "filter too large": filter_too_large,
    "equality too large": equality_too_large,
    "chunk cuts": chunk_cuts,
    "chunk cuts, one short join": lambda: chunk_cuts(short_at=C_SHORT_AT),
    "4096 filters": lambda: chunk_neighbours(4096),
    "4097 filters": lambda: chunk_neighbours(4097),
    "rerun mixed": rerun_mixed,
    "rerun all": rerun_all,
    "rerun none": rerun_none,
    "descriptor limits": descriptor_limits,
    "empty relations": empty_relations,
    "empty only": empty_only,
    "no survivors": no_survivors,
    "tiny": tiny,
}
C_SHORT_AT = 2503                                        # far from the first chunk of joins (a chunk has a few hundred)

_REFERENCE = {}


def reference(name, takes=None):
    """(relations, queries, [(sums, rows)], info, detail) of a family: the numpy executor and call_counts of tests/query_model.py
    (takes: batch_takes at other settings than 4 bits, query_model.join_takes())"""
    from query_model import call_counts, run_query
    if name not in _REFERENCE:
        rels, queries = FAMILIES[name]()
        _REFERENCE[name] = (rels, queries, [run_query(rels, q) for q in queries]) + call_counts(rels, queries)
    if takes is None:
        return _REFERENCE[name]
    rels, queries, want = _REFERENCE[name][:3]
    return (rels, queries, want) + call_counts(rels, queries, takes)
