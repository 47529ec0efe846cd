"""What rhj_join_foldn_batch_device, rhj_query_foldn_plan and the fold route with rhj_set_query_fold_nodes (include/rhj_inter.h,
DESIGN.md 4.18) compute, restated without the library: foldn_item, one item whose key words each come through a row-id vector of
their own (foldn_item_np the same in numpy's wrapping u64 arithmetic); foldn_plan, the shortest level prefix after which a
query's merged nodes and remaining predicates fold; foldn_route, a query run by that prefix with query_model.py's pair executor
and then by the folds over its nodes; foldn_counts, the six infos a batch must report with all four switches on; random_queries,
small random queries, cyclic ones among them, that itertools.product can answer.  A side's keys are (columns, vectors, rows): a
list of nkeys u64 arrays, a list of nkeys u64 vectors or None, and the side's positions; factors and queries are
join_fold_model's."""
import numpy as np

import join_fold_model as fm
import join_foldk_model as km
import join_folds_model as sm
from query_model import INFO_FIELDS, _match, track_kinds

M64 = fm.M64
MAX_KEYS = km.MAX_KEYS
MAX_TERMS = sm.MAX_TERMS
NO_NODES = {"foldn_calls": 0, "foldn_items": 0, "node_queries": 0, "node_levels": 0}


# ---- the item -----------------------------------------------------------------------------------------------------------------------

def words(cols, sels, n):
    """the nkeys key words of a side's n positions: word t of position p is cols[t][sels[t][p]], cols[t][p] without a vector"""
    out = []
    for c, s in zip(cols, sels):
        c = np.asarray(c, dtype=np.uint64)
        out.append(c[:n] if s is None else c[np.asarray(s[:n], dtype=np.uint64).astype(np.int64)])
    return out


def foldn_item(R, S, values, outs):
    """[(vector, total)] of one item in Python integers; R and S are (columns, vectors, rows)"""
    return km.foldk_item(words(*R), words(*S), values, outs)


def foldn_item_np(R, S, values, outs):
    """foldn_item with numpy's wrapping u64 arithmetic"""
    return km.foldk_item_np(words(*R), words(*S), values, outs)


def brute_force(R, S, values, outs):
    """the same by a double loop over the positions and a loop over the words, every word through its own vector, one element at
    a time"""
    (colsR, selsR, nR), (colsS, selsS, nS) = R, S
    word = lambda cols, sels, t, p: int(cols[t][int(sels[t][p]) if sels[t] is not None else p])
    V = [fm.factor(f, nS).tolist() for f in values]
    res = []
    for c, f in outs:
        P = fm.factor(f, nR).tolist()
        vec = [0] * nR
        for i in range(nR):
            for j in range(nS):
                if all(word(colsR, selsR, t, i) == word(colsS, selsS, t, j) for t in range(len(colsR))):
                    vec[i] = (vec[i] + P[i] * V[c][j]) & M64
        res.append((vec, sum(vec) & M64))
    return res


# ---- the plan -----------------------------------------------------------------------------------------------------------------------

def prefix_plan(query, L):
    """(nodes of the bindings, root, [(child, parent, round, [predicate indices])], [predicates inside a node]) when the query folds
    over its nodes after its first L predicates ran as levels, None when it does not"""
    rels, joins, _, _ = query
    up = {}

    def find(t):
        up.setdefault(t, t)
        while up[t] != t:
            t = up[t]
        return t

    node = list(range(len(rels)))
    for a, ca, b, cb in joins[:L]:
        x, y = find((a, ca)), find((b, cb))
        if x != y:
            up[y] = x
        na, nb = node[a], node[b]
        node = [na if x == nb else x for x in node]       # B's node takes A's id
    selfs, groups, per = [], {}, {}
    for l in range(L, len(joins)):
        a, ca, b, cb = joins[l]
        x, y = find((a, ca)), find((b, cb))
        if x == y:
            continue                                     # said already by the predicates before it
        up[y] = x
        na, nb = node[a], node[b]
        if na == nb:
            per[na] = per.get(na, 0) + 1
            if per[na] > MAX_TERMS:
                return None
            selfs.append(l)
        else:
            g = groups.setdefault((min(na, nb), max(na, nb)), [])
            if len(g) == MAX_KEYS:
                return None
            g.append(l)
    names = sorted(set(node))
    if len(groups) != len(names) - 1:
        return None                                      # a true cycle over the nodes
    if not groups:
        return node, names[0], [], selfs
    rank = {n: k for k, n in enumerate(names)}           # the schedule over the nodes by rank: "the lowest first" means the same
    edges = [(rank[node[joins[idx[0]][0]]], 0, rank[node[joins[idx[0]][2]]], 0) for idx in groups.values()]
    best = None
    for r in range(len(names)):
        rounds, steps = fm.schedule(len(names), edges, r)
        if best is None or rounds < best[0]:
            best = (rounds, r, steps)
    steps = [(names[c], names[p], rnd, groups[(min(names[c], names[p]), max(names[c], names[p]))]) for c, p, rnd in best[2]]
    return node, names[best[1]], steps, selfs


def foldn_plan(query):
    """(levels, nodes of the bindings, root, steps, predicates inside a node) of a valid query: the smallest prefix that passes"""
    for L in range(max(len(query[1]) - 1, 0) + 1):
        plan = prefix_plan(query, L)
        if plan is not None:
            return (L,) + plan
    raise AssertionError("a valid query hands over with one predicate left at the latest: %r" % (query,))


# ---- the route ----------------------------------------------------------------------------------------------------------------------

def run_levels(cols, query, L):
    """the filters and the first L predicates as query_model.trace_query runs them: (ids, node, rows of a node, level steps, whether
    a filter was issued, alive after the filters).  ids[b] are binding b's row ids, aligned within a node; a level step is (kind,
    rows of A's node, rows of B's node, rows of the result); the steps end with the first empty result."""
    rels, joins, filters, _ = query
    ids, issued = {}, False
    empty = any(len(cols[r][0]) == 0 if len(cols[r]) else True for r in rels)
    for b, r in enumerate(rels):
        n = len(cols[r][0]) if len(cols[r]) else 0
        keep = np.ones(n, dtype=bool)
        mine = [f for f in filters if f[0] == b]
        for a, c, op, v in mine:
            x, v = cols[r][c], np.uint64(int(v) & M64)
            keep &= (x < v) if op == "<" else (x > v) if op == ">" else (x == v)
        ids[b] = np.flatnonzero(keep)
        issued |= bool(mine) and not empty
    node = list(range(len(rels)))
    alive = not empty and all(len(ids[b]) for b in ids)
    steps = []
    for a, ca, b, cb in joins[:L] if alive else ():
        ka, kb = cols[rels[a]][ca][ids[a]], cols[rels[b]][cb][ids[b]]
        na, nb = node[a], node[b]
        if na == nb:
            keep = np.flatnonzero(ka == kb)
            for x in range(len(rels)):
                if node[x] == na:
                    ids[x] = ids[x][keep]
            steps.append((1, len(ka), len(kb), len(keep)))
        else:
            ia, ib = _match(ka, kb)
            for x in range(len(rels)):
                if node[x] == na:
                    ids[x] = ids[x][ia]
                elif node[x] == nb:
                    ids[x] = ids[x][ib]
            node = [na if x == nb else x for x in node]
            steps.append((0, len(ka), len(kb), len(ia)))
        if steps[-1][3] == 0:
            break
    return ids, node, steps, issued, alive


def node_folds(cols, query, plan, ids, item=foldn_item_np, first=sm.self_item_np):
    """(sums, rows, items per round, pre-round items) of the nodes' pass: join_folds_model.folds_route with nodes for bindings.  A
    key word, a term's column, a child's view value and a root's lazy view read the column of the member binding named through
    that binding's ids.  items per round is a dict round -> [items on one key, on several words that name one binding a side, on
    words that name several members of a side]."""
    rels, joins, _, views = query
    _, node, root, steps, selfs = plan
    names = sorted(set(node))
    col = lambda b, c: cols[rels[b]][c]
    vec = lambda b: ids[b].astype(np.uint64)
    rows = {n: len(ids[n]) for n in names}
    zeros, issued = [0] * len(views), {}
    w = {n: None for n in names}
    acc = {n: {} for n in names}
    firsts = []
    for n in names:
        terms = [(col(joins[l][0], joins[l][1]), vec(joins[l][0]), col(joins[l][2], joins[l][3]), vec(joins[l][2])) for l in selfs if node[joins[l][0]] == n]
        if not terms and steps:
            continue
        outs = [(None, None, None)] + ([(None, vec(x), col(x, c)) for x, c in views] if not steps else [])
        firsts.append((n, first(rows[n], terms, outs)))
    for n, res in firsts:
        if res[0][1] == 0:
            return zeros, 0, issued, len(firsts)
        if not steps:
            return [t for _, t in res[1:]], res[0][1], issued, len(firsts)
        w[n] = np.asarray(res[0][0], dtype=np.uint64)
    steps = list(steps)
    rnd = 0
    while steps:
        now = [s for s in steps if s[2] == rnd]
        steps = [s for s in steps if s[2] != rnd]
        results = []
        for step in now:
            S, P = step[0], step[1]
            last = not steps and step == now[-1]
            memR, memS, colsR, colsS = [], [], [], []
            for l in step[3]:
                a, ca, b, cb = joins[l]
                (xp, cp), (xs, cs) = ((a, ca), (b, cb)) if node[a] == P else ((b, cb), (a, ca))
                assert node[xp] == P and node[xs] == S
                memR.append(xp); memS.append(xs); colsR.append(col(xp, cp)); colsS.append(col(xs, cs))
            values, value_of = [(w[S], None, None)], {}
            for v, (x, c) in enumerate(views):
                if node[x] == S:
                    value_of[v] = len(values)
                    values.append((w[S], vec(x), col(x, c)))
                elif v in acc[S]:
                    value_of[v] = len(values)
                    values.append((acc[S][v], None, None))
            outs, ov = [(0, (w[P], None, None))], [-1]
            for v, (x, c) in enumerate(views):
                if v in value_of:
                    outs.append((value_of[v], (w[P], None, None)))
                elif v in acc[P]:
                    outs.append((0, (acc[P][v], None, None)))
                elif last and node[x] == P:
                    outs.append((0, (w[P], vec(x), col(x, c))))
                else:
                    continue
                ov.append(v)
            assert len(values) <= fm.MAX_VALUES and len(outs) <= fm.MAX_OUTS
            res = item((colsR, [vec(x) for x in memR], rows[P]), (colsS, [vec(x) for x in memS], rows[S]), values, outs)
            results.append((P, last, ov, res))
            kind = 0 if len(step[3]) == 1 else 1 if len(set(memR)) == 1 and len(set(memS)) == 1 else 2
            issued.setdefault(rnd, [0, 0, 0])[kind] += 1
        for P, last, ov, res in results:
            if res[0][1] == 0:
                return zeros, 0, issued, len(firsts)
            if last:
                sums = [0] * len(views)
                for (_, total), v in zip(res[1:], ov[1:]):
                    sums[v] = total
                return sums, res[0][1], issued, len(firsts)
            w[P] = np.asarray(res[0][0], dtype=np.uint64)
            for (vector, _), v in zip(res[1:], ov[1:]):
                acc[P][v] = np.asarray(vector, dtype=np.uint64)
        rnd += 1
    raise AssertionError("a plan without a last fold")


def foldn_route(cols, query, node_rows=fm.MAX_ROWS, item=foldn_item_np, first=sm.self_item_np):
    """a query that hands over, run as the route runs it: a dict of sums, rows, levels (the level steps it took part in), filtered
    (a filter item was issued), parked (alive when its prefix ended and handed over), stays (a merged node had node_rows rows or
    more at the hand-over: the levels to the end), rounds (items per round) and pre (pre-round items)"""
    plan = foldn_plan(query)
    L = plan[0]
    ids, node, steps, filtered, alive = run_levels(cols, query, L)
    out = {"sums": [0] * len(query[3]), "rows": 0, "levels": steps, "filtered": filtered, "parked": False, "stays": False, "rounds": {}, "pre": 0, "L": L}
    if not alive or (steps and steps[-1][3] == 0):
        return out
    assert node == plan[1]
    if any(len(ids[n]) >= node_rows for n in set(node) if node.count(n) > 1):
        ids, node, steps, _, _ = run_levels(cols, query, len(query[1]))
        out.update(stays=True, levels=steps)
        if steps[-1][3]:
            out.update(rows=len(ids[0]), sums=[int(cols[query[0][a]][c][ids[a]].sum(dtype=np.uint64)) for a, c in query[3]])
        return out
    sums, rows, issued, pre = node_folds(cols, query, plan, ids, item, first)
    out.update(sums=list(sums), rows=rows, parked=True, rounds=issued, pre=pre)
    return out


def level_info(runs):
    """rhj_query_batch_info's level fields of queries that run by levels, query_model.call_counts's rules on level steps: runs is
    [(level steps, levels the query would run)].  A query takes part in a level while it is alive and has a step there; an empty
    result ends it.  A query without a predicate takes part in level 0's apply call."""
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["levels"] = max([n for _, n in runs], default=0)
    for l in range(max(info["levels"], 1)):
        here = [s[l] for s, _ in runs if s is not None and len(s) > l]
        info["eq2_calls"] += any(k == 1 for k, _, _, _ in here)
        info["join_calls"] += any(k == 0 for k, _, _, _ in here)
        info["join_reruns"] += any(k == 0 and out > max(nA, nB) for k, nA, nB, out in here)
        info["apply_calls"] += bool(here) or (l == 0 and any(s is None for s, _ in runs))
    return info


def foldn_counts(cols, queries, node_rows=fm.MAX_ROWS):
    """(info, fold info, foldk info, self info, nodes info, [(sums, rows)]) a batch must report with all four switches on.  A query
    whose bindings all have fewer than 2^32 rows folds from the start by join_folds_model.how(), and hands over when that gives 0;
    any other runs by levels.  The calls of the first fold pass and of the nodes' pass are counted apart (a round of either is up
    to three calls) and summed; fold_queries counts the queries of the first pass alive after the filters and the parked ones,
    foldk_queries and self_queries those of the first pass as before; info counts the levels and calls of the level queries and of
    the prefixes, and the one filter call serves all."""
    nrows = lambda r: len(cols[r][0]) if len(cols[r]) else 0
    answers, runs, filtered = [None] * len(queries), [], False
    passes = ({}, {})
    entered, firsts = {1: 0, 2: 0, 3: 0}, [0, 0]
    nodes = dict(NO_NODES)
    for i, query in enumerate(queries):
        fits = all(nrows(r) < fm.MAX_ROWS for r in query[0])
        kind = sm.how(query) if fits else 0
        if kind:
            sums, rows, issued, pre, alive = sm.folds_route(cols, query, None if kind == 3 else km.foldk_plan(query))
            answers[i] = (list(sums), rows)
            entered[kind] += alive
            firsts[0] += pre
            filtered |= bool(query[2]) and all(nrows(r) for r in query[0])
            for r, (one_key, tuples) in issued.items():
                mine = passes[0].setdefault(r, [0, 0, 0])
                mine[0] += one_key
                mine[1] += tuples
            continue
        if not fits:
            ids, _, steps, f, alive = run_levels(cols, query, len(query[1]))
            done = alive and (not steps or steps[-1][3] > 0)
            answers[i] = ([int(cols[query[0][a]][c][ids[a]].sum(dtype=np.uint64)) if done and len(ids[0]) else 0 for a, c in query[3]], len(ids[0]) if done else 0)
            runs.append((steps if query[1] or not alive else None, len(query[1])))
            filtered |= f
            continue
        run = foldn_route(cols, query, node_rows)
        answers[i] = (run["sums"], run["rows"])
        filtered |= run["filtered"]
        runs.append((run["levels"], len(query[1]) if run["stays"] else run["L"]))
        if run["parked"]:
            nodes["node_queries"] += 1
            nodes["node_levels"] += run["L"]
            firsts[1] += run["pre"]
            for r, kinds in run["rounds"].items():
                mine = passes[1].setdefault(r, [0, 0, 0])
                for k in range(3):
                    mine[k] += kinds[k]
    info = level_info(runs)
    info["filter_calls"] = int(filtered)
    calls = lambda k: sum(1 for p in passes for it in p.values() if it[k])
    items = lambda k: sum(it[k] for p in passes for it in p.values())
    fold = {"fold_calls": calls(0), "fold_items": items(0), "fold_queries": sum(entered.values()) + nodes["node_queries"]}
    foldk = {"foldk_calls": calls(1), "foldk_items": items(1), "foldk_queries": entered[2]}
    self_ = {"self_calls": sum(1 for f in firsts if f), "self_items": sum(firsts), "self_queries": entered[3]}
    nodes["foldn_calls"], nodes["foldn_items"] = calls(2), items(2)
    return info, fold, foldk, self_, nodes, answers


# ---- random queries, cyclic ones among them, that a cross product can answer -----------------------------------------------------------

RANDOM_SIZES = (48, 24, 12, 7, 5, 1)
RANDOM_PRODUCT = 150000                                  # the most rows of a query's cross product
RANDOM_LIMIT = 2 * 10 ** 5                               # every intermediate result stays below this (asserted by the tests)
KEY_COLUMNS = (0, 1, 3)


def random_relations(seed=161616):
    """relation r has RANDOM_SIZES[r] rows and four columns: c0 a key of two values, c1 and c3 equal to c0 in most rows and one of
    three values in the others (so that queries with many predicates, cyclic ones among them, keep rows), c2 unique and near 2^63 (sums
    wrap)"""
    rng = np.random.default_rng(seed)
    out = []
    for r, n in enumerate(RANDOM_SIZES):
        c0 = rng.integers(0, 2, size=n)
        c1, c3 = (np.where(rng.integers(0, 8, size=n) > 0, c0, rng.integers(0, 3, size=n)) for _ in range(2))
        c2 = rng.permutation(n).astype(np.uint64) + np.uint64(sm.B63 + (r << 20))
        out.append([np.ascontiguousarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)])
    return out


def random_queries(count=48, seed=171717):
    """(relations, queries): 1..5 bindings and 0..12 predicates drawn freely over three key columns, any two bindings (or one
    binding twice) a predicate, kept when the query is valid (all bindings in one node at the end) and, once half of `count` fold
    from the start (levels 0), only when it does not; 0..2 filters, 1..4 views.  The
    cross product of a query's relations has at most RANDOM_PRODUCT rows, a limit of the brute force and not of the route."""
    rng = np.random.default_rng(seed)
    rels = random_relations()
    queries, plain = [], 0
    while len(queries) < count:
        nb = int(rng.integers(1, 6))
        bind = [int(x) for x in rng.integers(0, len(RANDOM_SIZES), size=nb)]
        if np.prod([RANDOM_SIZES[r] for r in bind]) > RANDOM_PRODUCT:
            continue
        joins = [(int(rng.integers(0, nb)), int(rng.choice(KEY_COLUMNS)), int(rng.integers(0, nb)), int(rng.choice(KEY_COLUMNS))) for _ in range(int(rng.integers(0, 13)))]
        filters = [(int(rng.integers(0, nb)), 3, "<", int(rng.integers(1, 4))) for _ in range(int(rng.integers(0, 3)))]
        views = [(int(rng.integers(0, nb)), int(rng.integers(0, 4))) for _ in range(int(rng.integers(1, 5)))]
        query = (bind, joins, filters, views)
        if track_kinds(query) is None:
            continue
        plain += foldn_plan(query)[0] == 0
        if foldn_plan(query)[0] == 0 and plain > count // 2:
            continue                                     # (most draws fold from the start: only half of the queries kept may)
        queries.append(query)
    return rels, queries
