"""An exact executor for the queries whose predicates are a tree over their bindings, and generators of such queries: what the
fold route of rhj_query_batch_device (include/rhj_inter.h) must answer, worked out with none of its choices.
exact_tree is always rooted at binding 0 and walks the tree depth first; it keeps Python integers per row in dicts, reduces
modulo nothing, has no rounds and no early exit, and takes a view's values at the binding the view is on.  brute is the same
answer by itertools.product.  The caller reduces modulo 2^64.  A query is query_model's (relations, joins [(a, ca, b, cb)],
filters [(a, c, op, value)], views [(a, c)]); relations[r][c] are u64 numpy columns.

The relations the generators make have five columns: c0 and c1 keys from small domains that hold 0 and 2^64 - 1, c2 and c3
values spread over the whole of u64, c4 distinct values spread over the whole of u64 (a filter `c4 < its k-th smallest` keeps
exactly k rows)."""
import itertools

import numpy as np

M64 = (1 << 64) - 1
KEY_COLS, VALUE_COLS, RANK_COL = (0, 1), (2, 3), 4
EDGE_ROWS = (63, 64, 65, 2047, 2048, 2049)


class _Columns:
    """relations[r][c] as lists of Python integers, made once a call"""

    def __init__(self, relations, rels):
        self.relations, self.rels, self.made = relations, rels, {}

    def __call__(self, b, c):
        r = self.rels[b]
        if (r, c) not in self.made:
            self.made[(r, c)] = np.asarray(self.relations[r][c], dtype=np.uint64).tolist()
        return self.made[(r, c)]


def filtered_rows(relations, query, col=None):
    """per binding the ascending rows of its relation that all of its filters keep"""
    rels, _, filters, _ = query
    col = col or _Columns(relations, rels)
    out = []
    for b, r in enumerate(rels):
        rows = range(len(relations[r][0]) if len(relations[r]) else 0)
        for a, c, op, v in filters:
            if a != b:
                continue
            x, v = col(b, c), int(v) & M64
            rows = [i for i in rows if (x[i] < v if op == "<" else x[i] > v if op == ">" else x[i] == v)]
        out.append(list(rows))
    return out


def exact_tree(relations, query):
    """(sums, rows) in unbounded Python integers.  For the subtree below a binding, W[i] is the number of the subtree's join
    rows that row i is in and S[v][i] the sum of view v over them; a row that is in none is dropped (its integers are 0)."""
    rels, joins, _, views = query
    assert len(joins) == len(rels) - 1, "the predicates are no tree"
    col = _Columns(relations, rels)
    rows = filtered_rows(relations, query, col)
    next_to = {b: [] for b in range(len(rels))}
    for a, ca, b, cb in joins:
        next_to[a].append((b, ca, cb))
        next_to[b].append((a, cb, ca))
    seen = set()

    def below(b):
        seen.add(b)
        W = dict.fromkeys(rows[b], 1)
        S = {}
        for v, (x, c) in enumerate(views):
            if x == b:
                values = col(b, c)
                S[v] = {i: values[i] for i in rows[b]}
        for child, mine, theirs in next_to[b]:
            if child in seen:
                continue
            Wc, Sc = below(child)
            keys = col(child, theirs)
            count, total = {}, {v: {} for v in Sc}
            for j, w in Wc.items():
                k = keys[j]
                count[k] = count.get(k, 0) + w
                for v, part in Sc.items():
                    total[v][k] = total[v].get(k, 0) + part[j]
            keys = col(b, mine)
            kept = {i: w for i, w in W.items() if keys[i] in count}
            S = {v: {i: part[i] * count[keys[i]] for i in kept} for v, part in S.items()}
            for v in Sc:
                S[v] = {i: w * total[v][keys[i]] for i, w in kept.items()}
            W = {i: w * count[keys[i]] for i, w in kept.items()}
        return W, S

    W, S = below(0)
    assert len(seen) == len(rels), "the predicates are no tree"
    return [sum(S[v].values()) for v in range(len(views))], sum(W.values())


def brute(relations, query):
    """(sums, rows) over every combination of the bindings' filtered rows"""
    rels, joins, _, views = query
    col = _Columns(relations, rels)
    rows = filtered_rows(relations, query, col)
    preds = [(a, col(a, ca), b, col(b, cb)) for a, ca, b, cb in joins]
    seen = [(a, col(a, c)) for a, c in views]
    sums, n = [0] * len(views), 0
    for t in itertools.product(*rows):
        if all(ka[t[a]] == kb[t[b]] for a, ka, b, kb in preds):
            n += 1
            for v, (a, values) in enumerate(seen):
                sums[v] += values[t[a]]
    return sums, n


def modulo(answer):
    """(sums, rows) modulo 2^64, as the library reports them: every sum 0 when rows is"""
    sums, rows = answer
    return [s & M64 for s in sums], rows & M64


# ---- generators -------------------------------------------------------------------------------------------------------------------

def key_domain(d, base=0):
    """d >= 2 keys: 0, 2^64 - 1 and base + 1 .. base + d - 2"""
    return np.array([0, M64] + [base + k for k in range(1, d - 1)], dtype=np.uint64)


def make_relation(rng, n, d0, d1, base1=0):
    """n rows: c0 and c1 from key_domain(d0) and key_domain(d1, base1) with 0 and 2^64 - 1 among them, c2 and c3 anywhere in u64, c4 distinct and anywhere"""
    rank = rng.choice(np.unique(rng.integers(0, 1 << 64, size=2 * n + 8, dtype=np.uint64)), size=n, replace=False)
    keys = [rng.choice(key_domain(d0), size=n), rng.choice(key_domain(d1, base1), size=n)]
    for k in keys if n >= 4 else ():                      # both ends of u64 are in every key column of four rows or more
        k[rng.choice(n, size=2, replace=False)] = (0, M64)
    return keys + [rng.integers(0, 1 << 64, size=n, dtype=np.uint64), rng.integers(0, 1 << 64, size=n, dtype=np.uint64), rank]


def random_relations(rng, sizes, spread=(0.2, 0.6)):
    """a relation per size; a key column of n rows has about n * spread keys, so that a join neither dies out nor blows up"""
    return [make_relation(rng, n, *(max(2, int(round(n * rng.uniform(*spread)))) for _ in KEY_COLS)) for n in sizes]


def random_tree_query(rng, relations, nb, shape=None):
    """A query over nb bindings whose predicates are a random spanning tree: shape 0 a chain, 1 a star, between them a mix
    (None: drawn).  The tree's labels are shuffled, every predicate is written parent first or child first, and the
    predicates come in a random order; a relation may be bound more than once; 1..8 views sit on any binding,
    all on one binding in some queries, repeats allowed; a binding has 0..4 filters, some of which leave one row or a row count
    of EDGE_ROWS."""
    shape = rng.choice([0.0, 1.0, rng.random()]) if shape is None else shape
    label = rng.permutation(nb).tolist()
    pick = list(range(len(relations)))
    rels = [int(rng.choice(pick)) for _ in range(nb)]
    joins = []
    for k in range(1, nb):
        u = rng.random()
        p = 0 if u < shape * shape else k - 1 if u > 1 - (1 - shape) ** 2 else int(rng.integers(0, k))
        a, b = (label[p], label[k]) if rng.integers(0, 2) else (label[k], label[p])
        joins.append((a, int(rng.choice(KEY_COLS)), b, int(rng.choice(KEY_COLS))))
    joins = [joins[k] for k in rng.permutation(len(joins))]
    nviews = int(rng.integers(1, 9))
    one = int(rng.integers(0, nb)) if rng.random() < 0.2 else None
    views = [(one if one is not None else int(rng.integers(0, nb)), int(rng.integers(0, 5))) for _ in range(nviews)]
    flt = []
    for b in range(nb):
        cols = relations[rels[b]]
        n = len(cols[0])
        ranks = np.sort(cols[RANK_COL])
        for _ in range(int(rng.choice([0, 0, 0, 0, 0, 1, 1, 1, 2, 3, 4]))):
            u = rng.random()
            if u < 0.35 and n > 1:                         # exactly m rows of this filter alone
                edges = [m for m in EDGE_ROWS if m < n]
                m = int(rng.choice(edges)) if edges and rng.random() < 0.5 else int(rng.integers(max(1, n // 2), n))
                flt.append((b, RANK_COL, "<", int(ranks[m])))
            elif u < 0.45:                                # the rows above a rank
                flt.append((b, RANK_COL, ">", int(ranks[int(rng.integers(0, max(1, n // 3)))])))
            elif u < 0.52:                                # one row
                flt.append((b, RANK_COL, "=", int(ranks[int(rng.integers(0, n))])))
            elif u < 0.60:                                # the rows of one key
                c = int(rng.choice(KEY_COLS))
                flt.append((b, c, "=", int(cols[c][int(rng.integers(0, n))])))
            elif u < 0.70:                                # a key below 2^64 - 1, or above 0
                flt.append((b, int(rng.choice(KEY_COLS))) + (("<", M64) if rng.integers(0, 2) else (">", 0)))
            else:                                         # most of a value column
                cut = int(rng.integers(1 << 60, 1 << 62))
                flt.append((b, int(rng.choice(VALUE_COLS))) + (("<", M64 - cut) if rng.integers(0, 2) else (">", cut)))
    return rels, joins, flt, views


def relabel(query, perm, rng=None):
    """(the query with binding b renamed perm[b], order): the same question, so the same rows and, view for view, the same
    sums.  With rng each predicate's sides are swapped at random and the predicates, the filters and the views are shuffled;
    the new view k is the old view order[k] (views_back puts the sums back)."""
    rels, joins, filters, views = query
    new_rels = [None] * len(rels)
    for b, r in enumerate(rels):
        new_rels[perm[b]] = r
    new_joins = [(perm[a], ca, perm[b], cb) for a, ca, b, cb in joins]
    new_filters = [(perm[a], c, op, v) for a, c, op, v in filters]
    order = list(range(len(views)))
    if rng is not None:
        new_joins = [(b, cb, a, ca) if rng.integers(0, 2) else (a, ca, b, cb) for a, ca, b, cb in new_joins]
        new_joins = [new_joins[k] for k in rng.permutation(len(new_joins))]
        new_filters = [new_filters[k] for k in rng.permutation(len(new_filters))]
        order = rng.permutation(len(views)).tolist()
    return (new_rels, new_joins, new_filters, [(perm[views[k][0]], views[k][1]) for k in order]), order


def views_back(sums, order):
    out = [None] * len(sums)
    for k, v in enumerate(order):
        out[v] = sums[k]
    return out
