"""The queries tests/test_gpu_query_foldk.py runs beyond the `small` workload, from fixed seeds: random trees in which a third of
the edges carry 2..4 predicates, and hand-made trees on relations built for one property each.  relations[r][c] are u64 numpy
columns, queries as tests/query_model.py takes them.  tests/test_join_foldk_model.py holds every random tree to the numpy
executor without a device, none left out."""
import numpy as np

B63 = 1 << 63
TREES = 24
KEY_COLUMNS = 4                                          # c0..c3 keys of at most 8 distinct values, c4 unique near 2^63, c5 a small number
MOST_ROWS = {2: 300, 3: 200, 4: 100, 5: 50, 6: 30}       # a relation's rows by the bindings of the tree: the executor's pair lists stay small


def random_trees():
    """(relations, queries): per tree three relations of its own and one query over them"""
    rng = np.random.default_rng(4160)
    relations, queries = [], []
    for k in range(TREES):
        nb = 2 + k % 5
        base = len(relations)
        for _ in range(3):
            n = int(rng.integers(1, MOST_ROWS[nb] + 1))
            relations.append([rng.integers(0, int(rng.integers(2, 9)), size=n).astype(np.uint64) for _ in range(KEY_COLUMNS)] +
                             [rng.permutation(n).astype(np.uint64) + np.uint64(B63 + 1000 * len(relations)), rng.integers(0, 9, size=n).astype(np.uint64)])
        rels = [base + int(r) for r in rng.integers(0, 3, size=nb)]
        joins = []
        for b in range(1, nb):
            a = int(rng.integers(0, b))
            for _ in range(int(rng.integers(2, 5)) if rng.integers(0, 3) == 0 else 1):
                p = (a, int(rng.integers(0, KEY_COLUMNS)), b, int(rng.integers(0, KEY_COLUMNS)))
                joins.append(p if rng.integers(0, 2) else (p[2], p[3], p[0], p[1]))
        joins = [joins[j] for j in rng.permutation(len(joins))]
        filters = [(int(rng.integers(0, nb)), 5, "<", 7)] if k % 3 == 0 else []
        views = [(int(rng.integers(0, nb)), 4 + int(rng.integers(0, 2))) for _ in range(int(rng.integers(1, 5)))]
        queries.append((rels, joins, filters, views))
    return relations, queries


def hand_made():
    """relations 0..3 of 3000 rows with the constants 7 in c0 and 9 in c3 (values in c1, c2); relation 4 of 300 rows with a unique
    key in c0, copied to c4, and a second unique key in c3; relation 5 of 40 rows with the keys 0..9 in c0, copied to c3"""
    rng = np.random.default_rng(78)
    rels = []
    for r in range(4):
        n = 3000
        rels.append([np.full(n, 7, dtype=np.uint64), rng.permutation(n).astype(np.uint64) + np.uint64(B63), rng.integers(0, 1 << 62, size=n).astype(np.uint64),
                     np.full(n, 9, dtype=np.uint64)])
    n = 300
    key = np.arange(n, dtype=np.uint64)
    rels.append([key, rng.permutation(n).astype(np.uint64) + np.uint64(B63), rng.integers(0, 9, size=n).astype(np.uint64), rng.permutation(n).astype(np.uint64), key.copy()])
    k10 = (np.arange(40) % 10).astype(np.uint64)
    rels.append([k10, rng.integers(0, 1 << 63, size=40).astype(np.uint64), np.arange(40, dtype=np.uint64), k10.copy()])
    return rels


# a chain of four 3000-row bindings joined on two constant columns, every edge written in both directions: 8.1e13 rows
HUGE = ([0, 1, 2, 3], [(0, 0, 1, 0), (1, 3, 0, 3), (1, 0, 2, 0), (1, 3, 2, 3), (2, 0, 3, 0), (3, 3, 2, 3)], [], [(0, 1), (1, 2), (2, 1), (3, 2)])
# a chain of five rooted at binding 1: round 0 folds 0 into 1 on one key and 4 into 3 on two; round 1 folds 3 into 2 on two keys, and
# the filters leave those two no common key, so the total is 0 there and round 2 is never issued
DIES = ([4, 4, 4, 4, 5], [(0, 0, 1, 0), (1, 0, 2, 0), (1, 4, 2, 4), (2, 0, 3, 0), (3, 4, 2, 4), (3, 0, 4, 0), (4, 3, 3, 4)],
        [(2, 0, ">", 100), (3, 0, "<", 50)], [(4, 1), (2, 1)])
# the same tree alive: every round of it has an answer
LIVES = (DIES[0], DIES[1], [(2, 0, "<", 50), (3, 0, ">", 2)], DIES[3])
# the 40-row relation bound twice and joined on its key and the key's copy, the second predicate written the other way round; then
# one key into the 300-row relation
CROSSED = ([5, 5, 4], [(0, 0, 1, 0), (1, 3, 0, 3), (1, 2, 2, 0)], [], [(0, 1), (1, 1), (2, 2)])
# one key a step: a plan the fold route had already
PLAIN = ([5, 4, 5, 4], [(0, 0, 1, 0), (1, 0, 2, 0), (2, 0, 3, 0)], [], [(0, 1), (3, 1), (2, 2)])
