"""What rhj_fold_pred_batch_device and rhj_query_one_wait_plan (include/rhj_inter.h) compute, restated without
the library: pred_item_np, one item in numpy's wrapping u64 arithmetic; pred_item_loop, the same row by row in Python integers;
one_wait, the route's rule over the plans of join_folds_model.  Factors and equality terms are join_folds_model's; a constant term
is (col, sel, op, value) with op one of "<", ">", "=" and the comparison unsigned."""
import numpy as np

import join_fold_model as fm
import join_folds_model as sm

M64 = fm.M64
MAX_CONSTS = 4
MAX_EQS = sm.MAX_TERMS
MAX_OUTS = fm.MAX_OUTS
DEFAULT_ROWS = 4096                                      # the library's default row limit
SMALL_ROWS = 65536                                       # the limit that admits the `small` workload


def mask_np(n, consts, eqs):
    m = np.ones(n, dtype=bool)
    for col, sel, op, value in consts:
        x, v = sm._side(col, sel, n), np.uint64(int(value) & M64)
        m &= (x < v) if op == "<" else (x > v) if op == ">" else (x == v)
    for colA, selA, colB, selB in eqs:
        m &= sm._side(colA, selA, n) == sm._side(colB, selB, n)
    return m


def pred_item_np(n, consts, eqs, outs):
    """[(u64 vector, total)]: vector[i] = m(i) * P(i) for the factors P in outs, m the conjunction of every term"""
    m = mask_np(n, consts, eqs)
    res = []
    for f in outs:
        vec = np.where(m, fm.factor(f, n), np.uint64(0)).astype(np.uint64)
        res.append((vec, int(vec.sum(dtype=np.uint64))))
    return res


def pred_item_loop(n, consts, eqs, outs):
    """the same by a loop over the rows, the terms and the outputs, one Python integer at a time"""
    res = []
    for w, src, col in outs:
        vec = []
        for i in range(n):
            x = 1 if w is None else int(w[i])
            if col is not None:
                x = x * int(col[int(src[i]) if src is not None else i]) & M64
            for c, sel, op, value in consts:
                a, v = int(c[int(sel[i]) if sel is not None else i]), int(value) & M64
                if not (a < v if op == "<" else a > v if op == ">" else a == v):
                    x = 0
            for colA, selA, colB, selB in eqs:
                if int(colA[int(selA[i]) if selA is not None else i]) != int(colB[int(selB[i]) if selB is not None else i]):
                    x = 0
            vec.append(x)
        res.append((vec, sum(vec) & M64))
    return res


def pred_items(query, keys=True, self_=True):
    """the pred items of a query on the route: one per binding with filters or kept one-binding predicates; a query without a join
    is one item whatever it has"""
    rels, joins, filters, _ = query
    mine = {f[0] for f in filters}
    if sm.how(query, keys, self_) == 3:
        mine |= {joins[l][0] for l in sm.folds_plan(query)[2]}
    return 1 if len(rels) == 1 else len(mine)


def one_wait(rows, query, fold=True, keys=True, self_=True, limit=DEFAULT_ROWS):
    """1 when a valid query takes the one-wait route: one of the three plans lets it fold under the switches given, and every
    binding's relation (rows[r] its rows) has between 1 row and the limit; else 0"""
    if not fold or not sm.how(query, keys, self_):
        return 0
    return int(all(1 <= rows[r] <= limit for r in query[0]))
