"""What rhj_join_fold_batch_device, rhj_query_fold_plan and the fold route of rhj_query_batch_device (include/rhj_inter.h)
compute, restated without the library: fold_item, a Python-integer model of one item (fold_item_np the same in numpy's wrapping
u64 arithmetic, for the large items); fold_plan, the schedule rule; fold_route, a query run by that plan's rounds; fold_counts,
the fold info and the calls a batch must report.  A factor is (w, src, col), each a u64 numpy array or None; a query is
query_model's (relations, joins, filters, views)."""
import numpy as np

from query_model import INFO_FIELDS, call_counts, track_kinds

M64 = (1 << 64) - 1
MAX_VALUES = MAX_OUTS = 9
MAX_ROWS = 1 << 32


def factor(f, n):
    """f(p) = (w ? w[p] : 1) * (col ? col[src ? src[p] : p] : 1) for p < n, as a u64 array (numpy's products wrap)"""
    w, src, col = f
    out = np.ones(n, dtype=np.uint64) if w is None else np.asarray(w[:n], dtype=np.uint64).copy()
    if col is not None:
        q = np.arange(n) if src is None else np.asarray(src[:n], dtype=np.uint64).astype(np.int64)
        out = out * np.asarray(col, dtype=np.uint64)[q]
    return out


def fold_item(keysR, keysS, values, outs):
    """[(vector, total)] of one item in Python integers: values are factors over S's positions, outs are (value index, factor
    over R's positions); vector[i] = P(i) * A_c(keysR[i]), 0 where the key is not in S"""
    nR, nS = len(keysR), len(keysS)
    V = [factor(f, nS).tolist() for f in values]
    A = [{} for _ in values]
    for j, k in enumerate(np.asarray(keysS, dtype=np.uint64).tolist()):
        for c in range(len(values)):
            A[c][k] = (A[c].get(k, 0) + V[c][j]) & M64
    res = []
    kR = np.asarray(keysR, dtype=np.uint64).tolist()
    for c, f in outs:
        P = factor(f, nR).tolist()
        vec = [(P[i] * A[c].get(kR[i], 0)) & M64 for i in range(nR)]
        res.append((vec, sum(vec) & M64))
    return res


def fold_item_np(keysR, keysS, values, outs):
    """fold_item with numpy's wrapping u64 arithmetic: [(u64 vector, total)]"""
    keysR, keysS = np.asarray(keysR, dtype=np.uint64), np.asarray(keysS, dtype=np.uint64)
    nR, nS = len(keysR), len(keysS)
    uniq, inv = np.unique(keysS, return_inverse=True)
    order = np.argsort(inv, kind="stable")
    starts = np.flatnonzero(np.concatenate([[True], inv[order][1:] != inv[order][:-1]])) if nS else np.zeros(0, dtype=np.int64)
    A = []
    for f in values:
        v = factor(f, nS)[order]
        A.append(np.add.reduceat(v, starts) if nS else np.zeros(0, dtype=np.uint64))      # (u64 sums wrap)
    at = np.searchsorted(uniq, keysR)
    hit = (at < len(uniq))
    hit[hit] = uniq[at[hit]] == keysR[hit]
    res = []
    for c, f in outs:
        a = np.zeros(nR, dtype=np.uint64)
        a[hit] = A[c][at[hit]]
        vec = factor(f, nR) * a
        res.append((vec, int(vec.sum(dtype=np.uint64))))
    return res


def brute_force(keysR, keysS, values, outs):
    """the same by a double loop"""
    nR, nS = len(keysR), len(keysS)
    V = [factor(f, nS).tolist() for f in values]
    res = []
    for c, f in outs:
        P = factor(f, nR).tolist()
        vec = [0] * nR
        for i in range(nR):
            for j in range(nS):
                if int(keysR[i]) == int(keysS[j]):
                    vec[i] = (vec[i] + P[i] * V[c][j]) & M64
        res.append((vec, sum(vec) & M64))
    return res


# ---- the plan ---------------------------------------------------------------------------------------------------------------------

def schedule(nrels, joins, root):
    """(rounds, [(child, parent, round)]) of the tree rooted at root: a child is folded after all of its own children, in a later
    round than the last of them; a parent takes one child a round, the lowest ready binding first"""
    parent, order = {root: root}, [root]
    for x in order:
        for a, _, b, _ in joins:
            other = b if a == x else a if b == x else None
            if other is not None and other not in parent:
                parent[other] = x
                order.append(other)
    waits = {b: sum(1 for c in range(nrels) if c != root and parent[c] == b) for b in range(nrels)}
    folded, steps, rnd = set(), [], 0
    while len(steps) < nrels - 1:
        taken, mine = set(), []
        for c in range(nrels):
            if c == root or c in folded or waits[c] or parent[c] in taken:
                continue
            taken.add(parent[c])
            mine.append((c, parent[c], rnd))
        for c, p, _ in mine:
            folded.add(c)
            waits[p] -= 1
        steps += mine
        rnd += 1
    return rnd, steps


def folds(query):
    """whether the query folds: valid, at least one predicate, every predicate a join of two nodes"""
    kinds = track_kinds(query)
    return bool(kinds) and not any(kinds)


def fold_plan(query):
    """(root, steps) of a folding query, None of any other: the root with the fewest rounds, the lowest binding on a tie"""
    if not folds(query):
        return None
    rels, joins, _, _ = query
    best = None
    for r in range(len(rels)):
        rounds, steps = schedule(len(rels), joins, r)
        if best is None or rounds < best[0]:
            best = (rounds, r, steps)
    return best[1], best[2]


# ---- the route --------------------------------------------------------------------------------------------------------------------

def fold_route(cols, query, item=fold_item_np):
    """(sums, rows, items per round) of a folding query run as the route runs it.  rows is modulo 2^64.  items per round is a dict
    round -> items issued; a query that an empty binding or filter finishes issues none."""
    rels, joins, filters, views = query
    root, steps = fold_plan(query)
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
    zero = ([0] * len(views), 0, issued)
    if any(len(cols[r][0]) == 0 if len(cols[r]) else True for r in rels) or not all(rows.values()):
        return zero
    w = {b: None for b in range(len(rels))}
    acc = {b: {} for b in range(len(rels))}
    col = lambda b, c: cols[rels[b]][c]
    key = lambda b, c: col(b, c)[sel[b].astype(np.int64)] if sel[b] is not None else col(b, c)
    rnd = 0
    while steps:
        now = [s for s in steps if s[2] == rnd]
        steps = [s for s in steps if s[2] != rnd]
        results = []
        for S, P, _ in now:
            last = not steps and (S, P, rnd) == now[-1]
            cP, cS = next((ca, cb) if (a, b) == (P, S) else (cb, ca) for a, ca, b, cb in joins if {a, b} == {P, S})
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
            assert len(values) <= MAX_VALUES and len(outs) <= MAX_OUTS
            results.append((P, last, ov, item(key(P, cP), key(S, cS), values, outs)))
            issued[rnd] = issued.get(rnd, 0) + 1
        for P, last, ov, res in results:
            if res[0][1] == 0:
                return zero
            if last:
                sums = [0] * len(views)
                for (vec, total), v in zip(res[1:], ov[1:]):
                    sums[v] = total
                return sums, res[0][1], issued
            w[P] = np.asarray(res[0][0], dtype=np.uint64)
            for (vec, total), v in zip(res[1:], ov[1:]):
                acc[P][v] = np.asarray(vec, dtype=np.uint64)
        rnd += 1
    raise AssertionError("a plan without a last fold")


def fold_counts(cols, queries):
    """(info, fold info, [(sums, rows)] of the folding queries by position, None for the others) a batch must report with the
    switch on: the folding queries (every binding below 2^32 rows) that are alive after the filters run round by round, one call
    a round that has an item; info counts the calls and levels of the other queries, and the one filter call serves all."""
    which = [i for i, q in enumerate(queries) if folds(q) and all((len(cols[r][0]) if len(cols[r]) else 0) < MAX_ROWS for r in q[0])]
    others = [q for i, q in enumerate(queries) if i not in which]
    info = call_counts(cols, others)[0] if others else dict.fromkeys(INFO_FIELDS, 0)
    rows = lambda r: len(cols[r][0]) if len(cols[r]) else 0
    info["filter_calls"] = int(any(q[2] and all(rows(r) for r in q[0]) for q in queries))      # (a query that binds an empty relation adds no filter)
    answers, per_round, entered = [None] * len(queries), {}, 0
    for i in which:
        sums, rows, issued = fold_route(cols, queries[i])
        answers[i] = (sums, rows)
        entered += bool(issued)
        for r, k in issued.items():
            per_round[r] = per_round.get(r, 0) + k
    return info, {"fold_calls": len(per_round), "fold_items": sum(per_round.values()), "fold_queries": entered}, answers
