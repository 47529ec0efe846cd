"""What rhj_query_batch_device (include/rhj_inter.h) computes, restated without the library: the query lines of a work file, the
node tracking that decides between a join and a two-column equality, and a plain numpy executor (masks, a sort-merge join, sums
modulo 2^64).  A query is (relations, joins [(a, ca, b, cb)], filters [(a, ca, op, value)], views [(a, c)]) with a, b bindings."""
import re

import numpy as np


def parse_work(lines):
    out = []
    for line in lines:
        if "|" not in line:
            continue
        rels, preds, views = line.split("|")
        joins, filters = [], []
        for p in preds.split("&"):
            a, ca, op, b, cb = re.fullmatch(r"(\d+)\.(\d+)([=<>])(\d+)(?:\.(\d+))?", p).groups()
            if cb is None:
                filters.append((int(a), int(ca), op, int(b)))
            else:
                assert op == "="
                joins.append((int(a), int(ca), int(b), int(cb)))
        out.append(([int(r) for r in rels.split()], joins, filters, [tuple(int(x) for x in v.split(".")) for v in views.split()]))
    return out


def track_kinds(query):
    """per predicate 0 (a join of two nodes) or 1 (both bindings in one node: an equality), or None when the bindings are not all
    in one node at the end"""
    rels, joins, _, _ = query
    node = list(range(len(rels)))
    kinds = []
    for a, _, b, _ in joins:
        na, nb = node[a], node[b]
        kinds.append(1 if na == nb else 0)
        node = [na if x == nb else x for x in node]
    return kinds if len(set(node)) == 1 else None


def _match(ka, kb):
    """(ia, ib) of every pair with ka[ia] == kb[ib]"""
    order = np.argsort(kb, kind="stable")
    sb = kb[order]
    lo, hi = np.searchsorted(sb, ka, "left"), np.searchsorted(sb, ka, "right")
    cnt = hi - lo
    ia = np.repeat(np.arange(len(ka)), cnt)
    within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return ia, order[np.repeat(lo, cnt) + within]


def run_query(cols, query):
    """(sums, rows) of one query over cols[r][c] (u64 numpy columns): Python ints below 2^64, all 0 when there is no row"""
    rels, joins, filters, views = query
    ids = {}                                             # binding -> row ids, aligned within a node
    node = list(range(len(rels)))
    for b, r in enumerate(rels):
        keep = np.ones(len(cols[r][0]), dtype=bool)
        for a, c, op, v in filters:
            if a == b:
                x, v = cols[r][c], np.uint64(int(v) & ((1 << 64) - 1))
                keep &= (x < v) if op == "<" else (x > v) if op == ">" else (x == v)
        ids[b] = np.flatnonzero(keep)
    for a, ca, b, cb in joins:
        ka, kb = cols[rels[a]][ca][ids[a]], cols[rels[b]][cb][ids[b]]
        na, nb = node[a], node[b]
        if na == nb:
            keep = np.flatnonzero(ka == kb)
            for x in range(len(rels)):
                if node[x] == na:
                    ids[x] = ids[x][keep]
        else:
            ia, ib = _match(ka, kb)
            for x in range(len(rels)):
                if node[x] == na:
                    ids[x] = ids[x][ia]
                elif node[x] == nb:
                    ids[x] = ids[x][ib]
            node = [na if x == nb else x for x in node]
    assert len(set(node)) == 1
    rows = len(ids[0])
    return [int(cols[rels[a]][c][ids[a]].sum(dtype=np.uint64)) if rows else 0 for a, c in views], rows
