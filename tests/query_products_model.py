"""What rhj_query_batch_device answers for a cross product with rhj_set_query_products on (include/rhj_inter.h),
restated without the library: components, a union-find over the bindings; expand, the component queries that stand in a batch
for such a query; combine, their answers multiplied in unbounded Python integers and reduced modulo 2^64 at the end; answer, the
three together over any executor of one-component queries; random_queries, small random cross products that itertools.product
can answer, made of the random queries of join_folds_model and join_foldn_model with predicates removed.  A query is
query_model's (relations, joins [(a, ca, b, cb)], filters [(a, c, op, value)], views [(a, c)])."""
import numpy as np

import fold_exact
import join_foldn_model as nm
import join_folds_model as sm
from query_model import run_query

M64 = (1 << 64) - 1


def components(query):
    """[component of every binding]: two bindings are in one component when predicates connect them; the components are numbered
    0, 1, ... in the order of their lowest binding"""
    rels, joins, _, _ = query
    up = list(range(len(rels)))

    def find(b):
        while up[b] != b:
            b = up[b]
        return b

    for a, _, b, _ in joins:
        x, y = find(a), find(b)
        if x != y:
            up[max(x, y)] = min(x, y)
    names = {}
    return [names.setdefault(find(b), len(names)) for b in range(len(rels))]


def expand(query, columns=None):
    """per component (its query, [the caller's view of each of its views]); the query is None for a component that has nothing to
    ask: one binding, no filter, no view, and a relation without a column (columns[r], the number of relation r's columns; None:
    every relation has some).  The bindings are renumbered 0.. in ascending order; filters, predicates and views keep their order;
    a component without a view gets one stand-in view, on the first column its first predicate names, else its first filter's,
    else column 0, and an empty list of the caller's views."""
    rels, joins, filters, views = query
    comp = components(query)
    out = []
    for c in range(max(comp) + 1):
        mine = [b for b in range(len(rels)) if comp[b] == c]
        new = {b: k for k, b in enumerate(mine)}
        j = [(new[a], ca, new[b], cb) for a, ca, b, cb in joins if comp[a] == c]
        f = [(new[a], col, op, v) for a, col, op, v in filters if comp[a] == c]
        own = [v for v, (a, _) in enumerate(views) if comp[a] == c]
        v = [(new[views[k][0]], views[k][1]) for k in own]
        if not v:
            if j:
                v = [(j[0][0], j[0][1])]
            elif f:
                v = [(f[0][0], f[0][1])]
            elif columns is None or columns[rels[mine[0]]] > 0:
                v = [(0, 0)]
            else:
                out.append((None, []))
                continue
        out.append((([rels[b] for b in mine], j, f, v), own))
    return out


def combine(nviews, parts):
    """(sums, rows) of the product from parts = [((sums, rows) of a component, [the caller's view of each of its sums])], in
    unbounded integers: rows the product of the components' rows, a view's sum its component's sum times the rows of every
    other component; reduced modulo 2^64 at the end.  rows 0 reads as empty, whether a component is empty or the product is a
    multiple of 2^64: every sum is 0 then, as everywhere in the batch."""
    rows = 1
    for (_, n), _ in parts:
        rows *= n
    sums = [0] * nviews
    for (s, n), own in parts:
        others = rows // n if n else 0
        for k, v in enumerate(own):
            sums[v] = s[k] * others
    if rows & M64 == 0:
        return [0] * nviews, 0
    return [s & M64 for s in sums], rows & M64


def answer(cols, query, run=run_query):
    """(sums, rows) below 2^64 of a query of any number of components; run(cols, query) answers a one-component query (sums and
    rows in integers of any size: a sum modulo 2^64 times a row count is the same modulo 2^64)"""
    parts = []
    for q, own in expand(query, [len(c) for c in cols]):
        if q is None:
            r = query[0][components(query).index(len(parts))]
            parts.append((([], len(cols[r][0]) if len(cols[r]) else 0), own))
        else:
            s, n = run(cols, q)
            parts.append(((list(s) if n else [0] * len(q[3]), n), own))
    return combine(len(query[3]), parts)


def exact_forest(cols, query):
    """answer() with fold_exact.exact_tree for every component, for a query whose predicates are a forest"""
    return answer(cols, query, fold_exact.exact_tree)


# ---- random cross products that itertools.product can answer --------------------------------------------------------------------------

def cut(rng, query, want):
    """the query with predicates removed at random until it has `want` components, or None when it cannot have that many (fewer
    bindings); a predicate is removed only with every other predicate between the same two components-to-be, so what is removed
    is drawn as a random split of the bindings"""
    rels, joins, filters, views = query
    if len(rels) < want:
        return None
    side = [int(x) for x in rng.integers(0, want, size=len(rels))]
    kept = [p for p in joins if side[p[0]] == side[p[2]]]
    out = (rels, kept, filters, views)
    return out if max(components(out)) + 1 == want else None


def random_queries(count=160, seed=515151):
    """[(relations, query)]: half from join_folds_model.random_queries' generator and half from join_foldn_model's (cyclic
    components among them), each cut into 2..4 components.  Their RANDOM_PRODUCT cap holds for the whole cross product, which the
    brute force walks; a draw that cannot be cut as wanted is drawn again, none is left out for any other reason."""
    rng = np.random.default_rng(seed)
    out = []
    for model, n, s in ((sm, count // 2, seed + 1), (nm, count - count // 2, seed + 2)):
        rels, pool = None, []
        round_ = 0
        have = 0
        while have < n:
            if not pool:
                rels, pool = model.random_queries(count=64, seed=s + round_)
                round_ += 1
            q = cut(rng, pool.pop(), int(rng.integers(2, 5)))
            if q is None:
                continue
            assert np.prod([len(rels[r][0]) for r in q[0]]) <= model.RANDOM_PRODUCT
            out.append((rels, q))
            have += 1
    return out


def random_forests(count=40, seed=525252):
    """[(relations, query)]: fold_exact's random tree queries over 2..5 bindings of small relations, cut into 2..4 components: every
    component's predicates are a tree, which fold_exact.exact_tree answers"""
    rng = np.random.default_rng(seed)
    rels = fold_exact.random_relations(rng, (40, 17, 9, 5, 1))
    out = []
    while len(out) < count:
        nb = int(rng.integers(2, 6))
        q = cut(rng, fold_exact.random_tree_query(rng, rels, nb), int(rng.integers(2, 5)))
        if q is None or np.prod([len(rels[r][0]) for r in q[0]]) > sm.RANDOM_PRODUCT:
            continue
        out.append((rels, q))
    return out
