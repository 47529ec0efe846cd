"""What rhj_fold_self_batch_device, rhj_query_folds_plan and the fold route with rhj_set_query_fold_self (include/rhj_inter.h)
compute, restated without the library: self_item, a Python-integer model of one item with no child (self_item_np the same in
numpy's wrapping u64 arithmetic); folds_plan, the plan rule over a union-find of (binding, column) terms; folds_route, a query run
by the pre-round and that plan's rounds; folds_counts, the four info structs a batch must report; random_queries, small random
queries that itertools.product can answer.  Factors and queries are join_fold_model's; a term is (colA, selA, colB, selB)."""
import itertools

import numpy as np

import join_fold_model as fm
import join_foldk_model as km
from query_model import INFO_FIELDS, call_counts, track_kinds

M64 = fm.M64
MAX_TERMS = 4
MAX_KEYS = km.MAX_KEYS


def _side(col, sel, n):
    col = np.asarray(col, dtype=np.uint64)
    return col[:n] if sel is None else col[np.asarray(sel[:n], dtype=np.uint64).astype(np.int64)]


def self_item(n, terms, outs):
    """[(vector, total)] of one item in Python integers: m(i) = every term's colA[selA ? selA[i] : i] == colB[selB ? selB[i] : i],
    vector[i] = m(i) * P(i) for the factors P in outs"""
    m = [1] * n
    for colA, selA, colB, selB in terms:
        a, b = _side(colA, selA, n).tolist(), _side(colB, selB, n).tolist()
        m = [m[i] if a[i] == b[i] else 0 for i in range(n)]
    res = []
    for f in outs:
        P = fm.factor(f, n).tolist()
        vec = [(m[i] * P[i]) & M64 for i in range(n)]
        res.append((vec, sum(vec) & M64))
    return res


def self_item_np(n, terms, outs):
    """self_item with numpy's wrapping u64 arithmetic: [(u64 vector, total)]"""
    m = np.ones(n, dtype=bool)
    for colA, selA, colB, selB in terms:
        m &= _side(colA, selA, n) == _side(colB, selB, n)
    res = []
    for f in outs:
        vec = np.where(m, fm.factor(f, n), np.uint64(0)).astype(np.uint64)
        res.append((vec, int(vec.sum(dtype=np.uint64))))
    return res


def brute_force(n, terms, outs):
    """the same by a double loop, over the rows and over the terms, one element at a time"""
    res = []
    for w, src, col in outs:
        vec = []
        for i in range(n):
            x = 1 if w is None else int(w[i])
            if col is not None:
                x = x * int(col[int(src[i]) if src is not None else i]) & M64
            for colA, selA, colB, selB in terms:
                a = int(colA[int(selA[i]) if selA is not None else i])
                b = int(colB[int(selB[i]) if selB is not None else i])
                if a != b:
                    x = 0
            vec.append(x)
        res.append((vec, sum(vec) & M64))
    return res


# ---- the plan ---------------------------------------------------------------------------------------------------------------------

def folds_plan(query):
    """(root, [(child, parent, round, [predicate indices])], [kept one-binding predicates]) of a query that folds once its
    predicates are taken in order over a union-find of their (binding, column) terms, None of any other.  (The caller has a valid
    query: all bindings in one node at the end.)"""
    rels, joins, _, _ = query
    up = {}

    def find(t):
        up.setdefault(t, t)
        while up[t] != t:
            t = up[t]
        return t

    selfs, groups, per = [], {}, {}
    for l, (a, ca, b, cb) in enumerate(joins):
        x, y = find((a, ca)), find((b, cb))
        if x == y:
            continue                                     # a repeat, 0.1=0.1, or implied by the predicates before it
        up[y] = x
        if a == b:
            per[a] = per.get(a, 0) + 1
            if per[a] > MAX_TERMS:
                return None
            selfs.append(l)
        else:
            g = groups.setdefault((min(a, b), max(a, b)), [])
            if len(g) == MAX_KEYS:
                return None
            g.append(l)
    if len(groups) != len(rels) - 1:
        return None                                      # a true cycle
    if not groups:
        return 0, [], selfs
    edges = [joins[idx[0]] for idx in groups.values()]
    best = None
    for r in range(len(rels)):
        rounds, steps = fm.schedule(len(rels), edges, r)
        if best is None or rounds < best[0]:
            best = (rounds, r, steps)
    return best[1], [(c, p, rnd, groups[(min(c, p), max(c, p))]) for c, p, rnd in best[2]], selfs


def how(query, keys=True, self_=True):
    """the reason a valid query takes the fold route: 1 its predicates are a tree, 2 they are once parallel ones are grouped (the
    keys switch), 3 rhj_set_query_fold_self alone lets it in; 0 it runs by levels"""
    if fm.folds(query):
        return 1
    if keys and km.foldk_plan(query) is not None:
        return 2
    plan = folds_plan(query) if self_ else None
    if plan is not None and (keys or all(len(idx) == 1 for _, _, _, idx in plan[1])):
        return 3
    return 0


# ---- the route --------------------------------------------------------------------------------------------------------------------

def folds_route(cols, query, plan=None, item=km.foldk_item_np, first=self_item_np):
    """(sums, rows, items per round, pre-round items, alive after the filters) of a query run as the fold route runs it.  plan None:
    the query is rhj_set_query_fold_self's, with folds_plan's plan and the pre-round; else (root, steps) of one of the other two
    plans and no pre-round.  items per round is a dict round -> [items on one key, items on tuple keys]."""
    rels, joins, filters, views = query
    pre = plan is None
    root, steps, selfs = folds_plan(query) if pre else (plan[0], plan[1], [])
    sel, issued = {}, {}
    for b, r in enumerate(rels):
        n = len(cols[r][0]) if len(cols[r]) else 0
        keep = np.ones(n, dtype=bool)
        mine = [f for f in filters if f[0] == b]
        for a, c, op, v in mine:
            x, v = cols[r][c], np.uint64(int(v) & M64)
            keep &= (x < v) if op == "<" else (x > v) if op == ">" else (x == v)
        sel[b] = np.flatnonzero(keep).astype(np.uint64) if mine else None
    rows = {b: (len(sel[b]) if sel[b] is not None else (len(cols[r][0]) if len(cols[r]) else 0)) for b, r in enumerate(rels)}
    zeros = [0] * len(views)
    if any(len(cols[r][0]) == 0 if len(cols[r]) else True for r in rels) or not all(rows.values()):
        return zeros, 0, issued, 0, False
    w = {b: None for b in range(len(rels))}
    acc = {b: {} for b in range(len(rels))}
    col = lambda b, c: cols[rels[b]][c]
    key = lambda b, c: col(b, c)[sel[b].astype(np.int64)] if sel[b] is not None else col(b, c)
    firsts = []
    for b in range(len(rels)) if pre else ():
        terms = [(col(b, joins[l][1]), sel[b], col(b, joins[l][3]), sel[b]) for l in selfs if joins[l][0] == b]
        if not terms and len(rels) > 1:
            continue
        outs = [(None, None, None)] + ([(None, sel[0], col(0, c)) for _, c in views] if len(rels) == 1 else [])
        firsts.append((b, first(rows[b], terms, outs)))
    for b, res in firsts:
        if res[0][1] == 0:
            return zeros, 0, issued, len(firsts), True
        if len(rels) == 1:
            return [t for _, t in res[1:]], res[0][1], issued, len(firsts), True
        w[b] = np.asarray(res[0][0], dtype=np.uint64)
    steps = list(steps)
    rnd = 0
    while steps:
        now = [s for s in steps if s[2] == rnd]
        steps = [s for s in steps if s[2] != rnd]
        results = []
        for step in now:
            S, P = step[0], step[1]
            last = not steps and step == now[-1]
            kc = km.key_columns(query, step)
            values, value_of = [(w[S], None, None)], {}
            for v, (x, c) in enumerate(views):
                if x == S:
                    value_of[v] = len(values)
                    values.append((w[S], sel[S], col(S, c)))
                elif v in acc[S]:
                    value_of[v] = len(values)
                    values.append((acc[S][v], None, None))
            outs, ov = [(0, (w[P], None, None))], [-1]
            for v, (x, c) in enumerate(views):
                if v in value_of:
                    outs.append((value_of[v], (w[P], None, None)))
                elif v in acc[P]:
                    outs.append((0, (acc[P][v], None, None)))
                elif last and x == P:
                    outs.append((0, (w[P], sel[P], col(P, c))))
                else:
                    continue
                ov.append(v)
            assert len(values) <= fm.MAX_VALUES and len(outs) <= fm.MAX_OUTS
            results.append((P, last, ov, item([key(P, cp) for cp, _ in kc], [key(S, cs) for _, cs in kc], values, outs)))
            issued.setdefault(rnd, [0, 0])[len(kc) > 1] += 1
        for P, last, ov, res in results:
            if res[0][1] == 0:
                return zeros, 0, issued, len(firsts), True
            if last:
                sums = [0] * len(views)
                for (vec, total), v in zip(res[1:], ov[1:]):
                    sums[v] = total
                return sums, res[0][1], issued, len(firsts), True
            w[P] = np.asarray(res[0][0], dtype=np.uint64)
            for (vec, total), v in zip(res[1:], ov[1:]):
                acc[P][v] = np.asarray(vec, dtype=np.uint64)
        rnd += 1
    raise AssertionError("a plan without a last fold")


NO_SELF = {"self_calls": 0, "self_items": 0, "self_queries": 0}


def folds_counts(cols, queries, keys=True, self_=True):
    """(info, fold info, foldk info, self info, [(sums, rows)] of the folding queries by position, None for the others) a batch must
    report with the fold route on and the two other switches as given.  A query folds by how() when every binding has fewer than
    2^32 rows.  The pre-round is one call over the items of all queries of kind 3 alive after the filters; a round issues one
    call for its items on one key and one for its items on tuple keys.  fold_queries counts every folding query alive after the
    filters, foldk_queries those of kind 2, self_queries those of kind 3; info counts the calls and levels of the other queries,
    and the one filter call serves all."""
    nrows = lambda r: len(cols[r][0]) if len(cols[r]) else 0
    kinds = [how(q, keys, self_) if all(nrows(r) < fm.MAX_ROWS for r in q[0]) else 0 for q in queries]
    others = [q for q, k in zip(queries, kinds) if not k]
    info = call_counts(cols, others)[0] if others else dict.fromkeys(INFO_FIELDS, 0)
    info["filter_calls"] = int(any(q[2] and all(nrows(r) for r in q[0]) for q in queries))
    answers, per_round, entered, firsts = [None] * len(queries), {}, {1: 0, 2: 0, 3: 0}, 0
    for i, k in enumerate(kinds):
        if not k:
            continue
        sums, rows, issued, pre, alive = folds_route(cols, queries[i], None if k == 3 else km.foldk_plan(queries[i]))
        answers[i] = (sums, rows)
        entered[k] += alive
        firsts += pre
        for r, (one_key, tuples) in issued.items():
            mine = per_round.setdefault(r, [0, 0])
            mine[0] += one_key
            mine[1] += tuples
    fold = {"fold_calls": sum(1 for a, _ in per_round.values() if a), "fold_items": sum(a for a, _ in per_round.values()), "fold_queries": sum(entered.values())}
    foldk = {"foldk_calls": sum(1 for _, b in per_round.values() if b), "foldk_items": sum(b for _, b in per_round.values()), "foldk_queries": entered[2]}
    return info, fold, foldk, {"self_calls": int(firsts > 0), "self_items": firsts, "self_queries": entered[3]}, answers


# ---- random queries that a cross product can answer -----------------------------------------------------------------------------------

B63 = 1 << 63
RANDOM_SIZES = (300, 40, 12, 7, 5, 1)
RANDOM_PRODUCT = 150000                                  # the most rows of a query's cross product
RANDOM_LIMIT = 2 * 10 ** 5                               # every intermediate result stays below this (asserted by the tests)


def random_relations(seed=424242):
    """relation r has RANDOM_SIZES[r] rows and five columns: c0, c1, c3, c4 keys of at most 8 values (c1 equals c0 in about half of the
    rows, c4 equals c3 in most), c2 unique and near 2^63 (sums wrap)"""
    rng = np.random.default_rng(seed)
    out = []
    for r, n in enumerate(RANDOM_SIZES):
        c0 = rng.integers(0, 8, size=n)
        c1 = np.where(rng.integers(0, 2, size=n) == 1, c0, rng.integers(0, 8, size=n))
        c3 = rng.integers(0, 3, size=n)
        c4 = np.where(rng.integers(0, 4, size=n) > 0, c3, rng.integers(0, 3, size=n))
        c2 = rng.permutation(n).astype(np.uint64) + np.uint64(B63 + (r << 20))
        out.append([np.ascontiguousarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3, c4)])
    return out


def random_queries(count=48, seed=434343):
    """(relations, queries): 1..5 bindings, a random tree of one or two predicates an edge, 0..3 one-binding predicates anywhere,
    now and then a predicate that the others imply or one that closes a true cycle, the predicates shuffled, 0..2 filters, 1..4
    views.  The cross product of a query's relations has at most RANDOM_PRODUCT rows: candidates beyond it are drawn again.  That
    is a limit of the brute force by itertools.product, which walks the whole cross product, not of the route; no query is left
    out for the size of an intermediate result (all stay below RANDOM_LIMIT, which the tests assert on every query kept)."""
    rng = np.random.default_rng(seed)
    rels = random_relations()
    keys = (0, 1, 3, 4)
    queries = []
    while len(queries) < count:
        nb = int(rng.choice((1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)))
        bind = [int(x) for x in rng.integers(0, len(RANDOM_SIZES), size=nb)]
        if np.prod([RANDOM_SIZES[r] for r in bind]) > RANDOM_PRODUCT:
            continue
        joins = []
        for b in range(1, nb):
            a = int(rng.integers(0, b))
            for _ in range(int(rng.integers(1, 3))):
                joins.append((a, int(rng.choice(keys)), b, int(rng.choice(keys))))
        for _ in range(int(rng.integers(0, 4))):
            b = int(rng.integers(0, nb))
            joins.append((b, int(rng.choice(keys)), b, int(rng.choice(keys))))
        extra = int(rng.integers(0, 3))
        if extra == 0 and nb >= 3 and len(joins) >= 2:   # implied: the two ends of two predicates that share a term
            for (a, ca, b, cb), (c, cc, d, cd) in itertools.permutations(joins, 2):
                if (b, cb) == (c, cc) and a != d:
                    joins.append((a, ca, d, cd))
                    break
        elif extra == 1 and nb >= 3:                     # most likely a true cycle
            a, b = (int(x) for x in rng.choice(nb, size=2, replace=False))
            joins.append((a, int(rng.choice(keys)), b, int(rng.choice(keys))))
        joins = [joins[k] for k in rng.permutation(len(joins))]
        filters = [(int(rng.integers(0, nb)), 0, "<", int(rng.integers(3, 9))) for _ in range(int(rng.integers(0, 3)))]
        views = [(int(rng.integers(0, nb)), int(rng.integers(0, 5))) for _ in range(int(rng.integers(1, 5)))]
        queries.append((bind, joins, filters, views))
    return rels, queries


def product_answer(cols, query):
    """(sums, rows) by itertools.product over the bindings' filtered rows: every predicate checked on every combination"""
    rels, joins, filters, views = query
    lists = []
    for b, r in enumerate(rels):
        keep = range(len(cols[r][0]))
        for a, c, op, v in filters:
            if a == b:
                x = cols[r][c].tolist()
                keep = [i for i in keep if (x[i] < v if op == "<" else x[i] > v if op == ">" else x[i] == v)]
        lists.append(list(keep))
    py = [[c.tolist() for c in cols[r]] for r in rels]
    sums, rows = [0] * len(views), 0
    for combo in itertools.product(*lists):
        if all(py[a][ca][combo[a]] == py[b][cb][combo[b]] for a, ca, b, cb in joins):
            rows += 1
            for v, (x, c) in enumerate(views):
                sums[v] += py[x][c][combo[x]]
    return [s & M64 for s in sums], rows


def valid(query):
    return track_kinds(query) is not None
