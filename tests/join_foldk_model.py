"""What rhj_join_foldk_batch_device, rhj_query_foldk_plan and the fold route with rhj_set_query_fold_keys (include/rhj_inter.h)
compute, restated without the library: foldk_item, a Python-integer model of one item whose keys are tuples of columns
(foldk_item_np the same in numpy's wrapping u64 arithmetic); the home slot of a tuple, with tuples built to share one; foldk_plan,
the plan rule with parallel predicates grouped; foldk_route, a query run by that plan's rounds; foldk_counts, the three info
structs a batch must report.  Keys are lists of nkeys u64 arrays, one per word; factors and queries are join_fold_model's."""
import os

import numpy as np

import join_fold_model as fm
import join_sum_model as jm
from query_model import INFO_FIELDS, call_counts
from source_constants import one

M64 = fm.M64
MAX_KEYS = 4
HEADER = os.path.join(jm.ROOT, "sigmod-2018_amd", "csrc", "rhj_join_foldk_batch.hip.h")


def _check_header():
    """the rules restated below, as the code words them: a change there must be looked at here"""
    with open(HEADER) as f:
        text = f.read()
    who = "tests/join_foldk_model.py"
    one(r"constexpr uint64_t foldk_mix\(uint64_t h, uint64_t word\) \{ return \(h \+ word\) \* JSUM_HASH_MUL; \}", text, "the hash of a tuple", who)
    one(r"constexpr uint64_t foldk_home\(uint64_t h, uint32_t log2_slots\) \{ return h >> \(64 - log2_slots\); \}", text, "the home slot", who)
    one(r"uint64_t h = 0;", text, "the hash's start", who)


_check_header()


def tuples_of(keys):
    """the rows of a side as Python tuples"""
    return list(zip(*[np.asarray(k, dtype=np.uint64).tolist() for k in keys]))


def foldk_item(keysR, keysS, values, outs):
    """[(vector, total)] of one item in Python integers: keysR and keysS are lists of nkeys columns, values factors over S's
    positions, outs (value index, factor over R's positions); vector[i] = P(i) * A_c(tuple of R's row i), 0 where S has no such tuple"""
    tR, tS = tuples_of(keysR), tuples_of(keysS)
    V = [fm.factor(f, len(tS)).tolist() for f in values]
    A = [{} for _ in values]
    for j, k in enumerate(tS):
        for c in range(len(values)):
            A[c][k] = (A[c].get(k, 0) + V[c][j]) & M64
    res = []
    for c, f in outs:
        P = fm.factor(f, len(tR)).tolist()
        vec = [(P[i] * A[c].get(k, 0)) & M64 for i, k in enumerate(tR)]
        res.append((vec, sum(vec) & M64))
    return res


def tuple_ids(keysR, keysS):
    """(idsR, idsS): one u64 per row, equal exactly where the rows' tuples are"""
    both = np.stack([np.concatenate([np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)]) for a, b in zip(keysR, keysS)], axis=1)
    _, inv = np.unique(both, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1).astype(np.uint64)
    return inv[:len(keysR[0])], inv[len(keysR[0]):]


def foldk_item_np(keysR, keysS, values, outs):
    """foldk_item with numpy's wrapping u64 arithmetic: the tuples numbered, then join_fold_model.fold_item_np on the numbers"""
    if len(keysR) == 1:
        return fm.fold_item_np(keysR[0], keysS[0], values, outs)
    idsR, idsS = tuple_ids(keysR, keysS)
    return fm.fold_item_np(idsR, idsS, values, outs)


def brute_force(keysR, keysS, values, outs):
    """the same by a double loop over the rows and a loop over the words"""
    nR, nS, nk = len(keysR[0]), len(keysS[0]), len(keysR)
    V = [fm.factor(f, nS).tolist() for f in values]
    res = []
    for c, f in outs:
        P = fm.factor(f, nR).tolist()
        vec = [0] * nR
        for i in range(nR):
            for j in range(nS):
                if all(int(keysR[t][i]) == int(keysS[t][j]) for t in range(nk)):
                    vec[i] = (vec[i] + P[i] * V[c][j]) & M64
        res.append((vec, sum(vec) & M64))
    return res


# ---- the home slot ----------------------------------------------------------------------------------------------------------------

def tuple_hash(words):
    h = 0
    for w in words:
        h = ((h + int(w)) * jm.MUL) & M64
    return h


def home(words, log2):
    return tuple_hash(words) >> (64 - log2)


def tuples_homed_at(slot, log2, count, nkeys, start=1, lead=None):
    """`count` distinct tuples of nkeys words whose home in a table of 2^log2 slots is `slot`: the leading words are free (lead(k)
    gives tuple k's, default small numbers), the last is chosen so that the hash's top bits are the slot.  Returns nkeys columns."""
    out = []
    for k in range(count):
        first = list(lead(k)) if lead else [(7 * k + 3 * t + 1) & M64 for t in range(nkeys - 1)]
        assert len(first) == nkeys - 1
        want = ((slot << (64 - log2)) | (start + k)) & M64          # (h + last) * MUL == want
        last = (want * jm.MUL_INV - tuple_hash(first)) & M64
        out.append(first + [last])
        assert home(out[-1], log2) == slot
    assert len(set(map(tuple, out))) == count
    return [np.array([t[w] for t in out], dtype=np.uint64) for w in range(nkeys)]


# ---- the plan ---------------------------------------------------------------------------------------------------------------------

def groups_of(query):
    """the kept predicates grouped by unordered binding pair, in the order of each group's first: [((a, b), [predicate indices])],
    or None when a predicate has both sides on one binding or a group has more than MAX_KEYS"""
    _, joins, _, _ = query
    kept, groups = [], {}
    for l, (a, ca, b, cb) in enumerate(joins):
        if a == b:
            return None
        if any((a, ca, b, cb) == joins[m] or (b, cb, a, ca) == joins[m] for m in range(l)):
            continue
        groups.setdefault((min(a, b), max(a, b)), []).append(l)
    if any(len(g) > MAX_KEYS for g in groups.values()):
        return None
    return list(groups.items())


def foldk_plan(query):
    """(root, [(child, parent, round, [predicate indices])]) of a query that folds once parallel predicates are grouped, None of
    any other.  (The caller has a valid query: all bindings in one node at the end.)"""
    rels, joins, _, _ = query
    if not joins:
        return None
    groups = groups_of(query)
    if groups is None or len(groups) != len(rels) - 1:
        return None
    edges = [joins[idx[0]] for _, idx in groups]
    reached, grew = {0}, True                            # nrels - 1 edges that connect all bindings: a spanning tree
    while grew:
        grew = False
        for a, _, b, _ in edges:
            if (a in reached) != (b in reached):
                reached |= {a, b}
                grew = True
    if len(reached) != len(rels):
        return None
    best = None
    for r in range(len(rels)):
        rounds, steps = fm.schedule(len(rels), edges, r)
        if best is None or rounds < best[0]:
            best = (rounds, r, steps)
    by_pair = dict(groups)
    return best[1], [(c, p, rnd, by_pair[(min(c, p), max(c, p))]) for c, p, rnd in best[2]]


def key_columns(query, step):
    """[(parent's column, child's column)] per key word of a step"""
    c, p, _, idx = step
    out = []
    for l in idx:
        a, ca, b, cb = query[1][l]
        out.append((ca, cb) if a == p else (cb, ca))
    return out


# ---- the route --------------------------------------------------------------------------------------------------------------------

def foldk_route(cols, query, item=foldk_item_np):
    """(sums, rows, items per round) of a query run as the fold route runs it with both switches on; items per round is a dict
    round -> [items on one key, items on tuple keys].  join_fold_model.fold_route with a step's key a list of columns."""
    rels, joins, filters, views = query
    root, steps = foldk_plan(query)
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
    steps = list(steps)
    rnd = 0
    while steps:
        now = [s for s in steps if s[2] == rnd]
        steps = [s for s in steps if s[2] != rnd]
        results = []
        for step in now:
            S, P = step[0], step[1]
            last = not steps and step == now[-1]
            kc = key_columns(query, step)
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


def foldk_counts(cols, queries):
    """(info, fold info, foldk info, [(sums, rows)] of the folding queries by position, None for the others) a batch must report
    with both switches on.  The queries with a foldk_plan (every binding below 2^32 rows) fold; a round issues one call for its
    items on one key (counted by the fold info, as with the switch off) and one for its items on tuple keys (the foldk info).
    fold_queries counts every folding query alive after the filters, foldk_queries those among them that join_fold_model.folds
    refuses; info counts the calls and levels of the other queries, and the one filter call serves all."""
    nrows = lambda r: len(cols[r][0]) if len(cols[r]) else 0
    which = [i for i, q in enumerate(queries) if foldk_plan(q) is not None and all(nrows(r) < fm.MAX_ROWS for r in q[0])]
    others = [q for i, q in enumerate(queries) if i not in which]
    info = call_counts(cols, others)[0] if others else dict.fromkeys(INFO_FIELDS, 0)
    info["filter_calls"] = int(any(q[2] and all(nrows(r) for r in q[0]) for q in queries))
    answers, per_round, entered, only = [None] * len(queries), {}, 0, 0
    for i in which:
        sums, rows, issued = foldk_route(cols, queries[i])
        answers[i] = (sums, rows)
        entered += bool(issued)
        only += bool(issued) and not fm.folds(queries[i])
        for r, (one_key, tuples) in issued.items():
            mine = per_round.setdefault(r, [0, 0])
            mine[0] += one_key
            mine[1] += tuples
    fold = {"fold_calls": sum(1 for a, _ in per_round.values() if a), "fold_items": sum(a for a, _ in per_round.values()), "fold_queries": entered}
    foldk = {"foldk_calls": sum(1 for _, b in per_round.values() if b), "foldk_items": sum(b for _, b in per_round.values()), "foldk_queries": only}
    return info, fold, foldk, answers
