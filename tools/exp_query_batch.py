"""A batch of queries through rhj_query_batch_device, and batched two-column equalities, against the single calls:
tools/exp_query_batch.py [--reps 30] [--warmup 5] [--out FILE] [--cases abc]
One process, one library, timing level 0; every repetition times two forms of the same work on the same inputs, alternating
single, batch, single ..., each with a host clock around work that ends in a stream synchronisation.  Cases:
  (a) the 50 queries of `small`:
        batch    ONE rhj_query_batch_device call;
        single   the same queries one at a time through the entry points that existed before it: rhj_filter_device per filter,
                 two rhj_build_relation_device + rhj_join_device per join (room for max(nR, nS) pairs, once more with room for
                 the count when that was short), rhj_filter_eq2_device per predicate inside a node, rhj_gather_tables_device
                 per side of every list, rhj_sum_views_device per query.  The loop is driven from Python, as the batch call is
                 entered from Python: its time includes the interpreter's share of about 600 calls.
  (b) 64 equalities of 4096 rows, and 64 of 4 194 304 rows: rhj_filter_eq2_batch_device against the loop of
      rhj_filter_eq2_device;
  (c) one equality of 4 194 304 rows: the batch's mask kernel (k_eq2batch_mask) against the single call's (k_filter_mask_eq2)
      on its own ground.
Outputs are allocated once where the sizes are known; the two forms' answers are compared afterwards.  Prints, and with --out
appends, one line per case: medians, min-max spreads, the ratio."""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
sys.path.insert(0, "oracle")

import numpy as np
import torch

import helpers
from query_model import parse_work

mod = importlib.import_module("sigmod-2018_amd")
u64p = C.POINTER(C.c_uint64)


def ptr(t):
    return None if t is None else t.data_ptr()


class Small:
    """the `small` workload in both forms"""

    def __init__(self, rhj):
        g = helpers.Golden()
        rels = g.small_relations
        self.rhj, self.lib = rhj, rhj.lib
        self.cols = [[torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint64).view(np.int64)).to(rhj.dev) for c in rels["r%d" % r]] for r in range(len(rels))]
        self.queries = parse_work(g.small["work_lines"])
        self.want = g.small["result_lines"]
        self.rels, self.keep_rels = rhj.device_relations(self.cols)
        self.arr, self.keep = mod.query_descs(self.queries)
        self.lines = {}

    def batch(self):
        rc = self.lib.rhj_query_batch_device(self.rels, len(self.cols), self.arr, len(self.queries))
        assert rc == 0, rc
        self.lines["batch"] = [" ".join("NULL" if d.rows == 0 else str(d.sums[k]) for k in range(d.nviews)) for d in self.arr]

    def single(self):
        self.lines["single"] = [self.one(q) for q in self.queries]

    def gather(self, vecs, idx, side, stride, n):
        """the vectors rebuilt through one side of a list"""
        outs = [torch.empty(max(n, 1), dtype=torch.int64, device=self.rhj.dev) for _ in vecs]
        k = len(vecs)
        rc = self.lib.rhj_gather_tables_device((C.c_void_p * k)(*[o.data_ptr() for o in outs]), (C.c_void_p * k)(*[ptr(v) for v in vecs]), k,
                                               C.c_void_p(idx.data_ptr() + 8 * side), stride, n)
        assert rc == 0, rc
        return outs

    def one(self, q):
        rhj, lib = self.rhj, self.lib
        rels, joins, filters, views = q
        col = lambda b, c: self.cols[rels[b]][c]                      # noqa: E731
        vec = dict.fromkeys(range(len(rels)))
        node = {b: b for b in range(len(rels))}
        rows = {b: col(b, 0).shape[0] for b in range(len(rels))}
        for a, ca, op, v in filters:
            ids = rhj.filter_device(col(a, ca), op, v, vec[a])
            if vec[a] is not None:                                   # a second filter on the binding: through the first one's hits
                ids = self.gather([vec[a]], ids, 0, 1, ids.shape[0])[0][:ids.shape[0]]
            vec[a], rows[a] = ids, ids.shape[0]
        for a, ca, b, cb in joins:
            na, nb = node[a], node[b]
            if na == nb:
                n = rows[na]
                out = torch.empty(max(n, 1), dtype=torch.int64, device=rhj.dev)
                hits = C.c_uint64(0)
                rc = lib.rhj_filter_eq2_device(ptr(col(a, ca)), ptr(vec[a]), ptr(col(b, cb)), ptr(vec[b]), n, out.data_ptr(), C.byref(hits))
                assert rc == 0, rc
                idx, stride, m = out, 1, hits.value
            else:
                tup = []
                for x, cx, n in ((a, ca, rows[na]), (b, cb, rows[nb])):
                    t = torch.empty((max(n, 1), 2), dtype=torch.int64, device=rhj.dev)
                    rc = lib.rhj_build_relation_device(ptr(col(x, cx)), ptr(vec[x]), n, t.data_ptr())
                    assert rc == 0, rc
                    tup.append(t[:n])
                cap = max(rows[na], rows[nb])
                idx, m = rhj.join_device(tup[0], tup[1], capacity=cap)
                if m > cap:
                    idx, m = rhj.join_device(tup[0], tup[1], capacity=m)
                stride = 2
            if m == 0:
                return " ".join("NULL" for _ in views)
            for side, nd in ((0, na), (1, nb)):
                xs = [x for x in node if node[x] == nd]
                if side == 1 and na == nb:
                    break
                for x, o in zip(xs, self.gather([vec[x] for x in xs], idx, side, stride, m)):
                    vec[x] = o[:m]
            for x in node:
                if node[x] == nb:
                    node[x] = na
            rows[na] = m
        n = rows[node[views[0][0]]]
        if n == 0:
            return " ".join("NULL" for _ in views)
        k = len(views)
        got = (C.c_uint64 * k)()
        rc = lib.rhj_sum_views_device(k, (C.c_void_p * k)(*[ptr(col(a, c)) for a, c in views]), (C.c_void_p * k)(*[ptr(vec[a]) for a, _ in views]),
                                      (C.c_uint64 * k)(*[n] * k), got)
        assert rc == 0, rc
        return " ".join(str(s) for s in got)

    def compare(self, name):
        assert self.lines["batch"] == self.want, name + ": the batch's lines differ from the recorded ones"
        assert self.lines["single"] == self.want, name + ": the single calls' lines differ from the recorded ones"


class Equalities:
    """count equalities of rows rows each, in both forms; outputs allocated once"""

    def __init__(self, rhj, count, rows):
        self.lib, self.count = rhj.lib, count
        rnd = lambda hi, n: torch.randint(0, hi, (n,), dtype=torch.int64, device=rhj.dev)      # noqa: E731
        shared = min(count, 4)                                        # a few inputs, shared between the items
        self.colA, self.colB = [rnd(4, rows) for _ in range(shared)], [rnd(4, rows) for _ in range(shared)]
        self.sel = [rnd(rows, rows) for _ in range(shared)]
        self.arr = (mod.Eq2Desc * count)()
        self.outs, self.refs, self.hits = [], [], [0] * count
        for k, d in enumerate(self.arr):
            d.d_colA, d.d_selA, d.d_colB, d.d_selB = ptr(self.colA[k % shared]), ptr(self.sel[k % shared]) if k % 2 else None, ptr(self.colB[(k + 1) % shared]), None
            d.n = rows
            self.outs.append(torch.empty(rows, dtype=torch.int64, device=rhj.dev))
            self.refs.append(torch.empty(rows, dtype=torch.int64, device=rhj.dev))
            d.d_out = self.outs[-1].data_ptr()

    def batch(self):
        rc = self.lib.rhj_filter_eq2_batch_device(self.arr, self.count)
        assert rc == 0, rc

    def single(self):
        h = C.c_uint64(0)
        for k, d in enumerate(self.arr):
            rc = self.lib.rhj_filter_eq2_device(d.d_colA, d.d_selA, d.d_colB, d.d_selB, d.n, self.refs[k].data_ptr(), C.byref(h))
            assert rc == 0, rc
            self.hits[k] = h.value

    def compare(self, name):
        for k, d in enumerate(self.arr):
            assert d.hits == self.hits[k] and torch.equal(self.outs[k][:d.hits], self.refs[k][:d.hits]), "%s: item %d differs" % (name, k)


def cases(rhj, which):
    torch.manual_seed(13)
    if "a" in which:
        yield "(a) small: 50 queries", lambda: Small(rhj)
    if "b" in which:
        yield "(b) 64 equalities x 4096 rows", lambda: Equalities(rhj, 64, 4096)
        yield "(b) 64 equalities x 4 194 304 rows", lambda: Equalities(rhj, 64, 1 << 22)
    if "c" in which:
        yield "(c) 1 equality x 4 194 304 rows", lambda: Equalities(rhj, 1, 1 << 22)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--out")
    a = ap.parse_args()
    rhj = mod.RHJ(device=0)
    lib = rhj.lib
    lib.rhj_gather_tables_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_uint64]
    lib.rhj_sum_views_device.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), u64p, u64p]
    lib.rhj_filter_eq2_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, u64p]
    rhj.set_bits(4)
    lines = []
    for name, make in cases(rhj, a.cases):
        lib.rhj_set_timing(0)
        form = make()
        t = {"single": [], "batch": []}
        for rep in range(a.warmup + a.reps):
            for s in ("single", "batch"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                getattr(form, s)()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    t[s].append(dt)
        form.compare(name)
        med = {s: statistics.median(t[s]) for s in t}
        parts = ["%s median %9.3f ms (min %.3f max %.3f, spread %.3f)" % (s, med[s], min(t[s]), max(t[s]), max(t[s]) - min(t[s])) for s in ("single", "batch")]
        line = "%-40s %s | single / batch %.2f | %d + %d reps" % (name, " | ".join(parts), med["single"] / med["batch"], a.warmup, a.reps)
        print(line, flush=True)
        lines.append(line)
        del form
        torch.cuda.empty_cache()
    lib.rhj_set_timing(2)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
