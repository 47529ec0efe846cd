"""rhj_set_query_products: what the switch costs a batch without a cross product, and what the route buys one with:
tools/exp_query_products.py [--reps 30] [--warmup 5] [--cases abc] [--settings levels,one_wait] [--tag NAME] [--out FILE]
The procedure of tools/exp_query_fold_one_wait.py: one process, one library (RHJ_LIB names another build, e.g. the parent commit's,
which has no such switch and runs the `off` forms alone), timing level 0; every repetition times the forms of a case one after
the other on the same device inputs, each with a host clock around work that ends in a stream synchronisation.  Cases, each under
every setting of --settings (levels: no other switch; one_wait: the four fold switches and the one-wait programs, row limit
65 536):
  (a) the 50 queries of `small` through rhj_query_batch_device with the switch off, on, and off again: no query is a cross
      product, so `on` adds the component plan of every query on the host and nothing else; the two `off` forms give the spread
      to read it against;
  (b) the synthetic batch of tests/query_shapes.py (24 queries), likewise;
  (c) 64 cross products of two three-binding chains: relations 0..2 have 4096 rows and 3..5 have 48, keys one to one, a filter
      that keeps 64 + i rows of binding 0, so query i's components have 64 + i and 48 rows and its product about 3000 to 6000:
      `batch` is ONE rhj_query_batch_device call with the switch on; `operators` runs the same queries one at a time through the
      library's reference-named engine as the reference's executor would (Filter, GetRelation, RadixHashJoin,
      InsertJoinToInterResults, CartesianInterResults, then rhj_sum_views_device over the product's row-id tables), the columns
      registered on the device beforehand.
The answers of the forms are compared afterwards.  Prints, and with --out appends, one line per case and setting: per form the
median and the min-max spread, and the ratio of every form to the first."""
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
import query_shapes
from query_model import parse_work
from test_gpu_inter import Engine, make_map

mod = importlib.import_module("sigmod-2018_amd")
u64p = C.POINTER(C.c_uint64)


def dev(rhj, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


def switches(rhj, setting, products):
    folds = setting == "one_wait"
    for setter in (rhj.set_query_fold, rhj.set_query_fold_keys, rhj.set_query_fold_self, rhj.set_query_fold_nodes, rhj.set_query_fold_one_wait):
        setter(folds)
    rhj.set_query_fold_one_wait_rows(65536 if folds else 4096)
    if hasattr(rhj.lib, "rhj_set_query_products"):
        rhj.set_query_products(products)


class SwitchForms:
    """one batch with the products switch off, on and off again (off alone on a library without the switch)"""

    def __init__(self, rhj, cols, queries, setting):
        self.rhj, self.cols, self.queries, self.setting, self.got = rhj, cols, queries, setting, {}
        self.names = ("off", "on", "off again") if hasattr(rhj.lib, "rhj_set_query_products") else ("off", "off again")

    def run(self, form):
        switches(self.rhj, self.setting, form == "on")
        try:
            self.got[form] = self.rhj.query_batch_device(self.cols, self.queries)
        finally:
            switches(self.rhj, "levels", False)

    def compare(self, name):
        for form in self.names[1:]:
            assert self.got[form] == self.got[self.names[0]], "%s: the answers of %s differ" % (name, form)

    def note(self):
        return "%d queries" % len(self.queries)


class ProductForms:
    """64 cross products of two three-binding chains: one batch call against the reference-named operators"""
    names = ("batch", "operators")

    def __init__(self, rhj, setting):
        self.rhj, self.lib, self.setting, self.got = rhj, rhj.lib, setting, {}
        rng = np.random.default_rng(2121)
        self.relations = [[rng.permutation(n), rng.permutation(n), rng.permutation(n), rng.integers(0, 1 << 40, size=n)] for n in (4096,) * 3 + (48,) * 3]
        self.relations = [[np.ascontiguousarray(c, dtype=np.uint64) for c in rel] for rel in self.relations]
        self.cols = [[dev(rhj, c) for c in rel] for rel in self.relations]
        self.views = [(0, 3), (2, 3), (5, 3)]
        self.joins = [(0, 0, 1, 0), (1, 1, 2, 1), (3, 0, 4, 0), (4, 1, 5, 1)]
        self.queries = [(list(range(6)), self.joins, [(0, 2, "<", 64 + i)], self.views) for i in range(64)]
        self.rm, self.keep = make_map(mod, self.relations)
        assert self.lib.rhj_register_relation_map(self.rm, 6) == 0
        self.engine = Engine(mod, self.lib, rhj)
        self.lib.rhj_sum_views_device.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), u64p, u64p]
        self.qrel = (C.c_int * 6)(*range(6))

    def run(self, form):
        if form == "batch":
            switches(self.rhj, self.setting, True)
            try:
                self.got[form] = [(list(s), r) for s, r in self.rhj.query_batch_device(self.cols, self.queries)]
            finally:
                switches(self.rhj, "levels", False)
        else:
            self.got[form] = [self.one(q) for q in self.queries]

    def one(self, query):
        e, L, q, rm = self.engine, self.lib, self.qrel, self.rm
        L.InitInterResults(C.byref(e.head), 6)
        for rel, col, op, value in query[2]:
            fp = mod.FilterPred(rel, col, value, op.encode())
            res = L.Filter(e.head, C.byref(fp), rm, q)
            L.InsertSingleRowIdsToInterResult(C.byref(e.head), rel, res)
            L.FreeResult(res)
        for r1, c1, r2, c2 in query[1]:
            if L.AreActiveInInter(e.head, r1, r2) == 1:
                L.JoinInterNode(C.byref(e.head), rm, r1, c1, r2, c2, q)
                continue
            relR, relS = L.GetRelation(r1, c1, e.head, rm, q), L.GetRelation(r2, c2, e.head, rm, q)
            res = L.RadixHashJoin(relR, relS, None)
            L.InsertJoinToInterResults(e.head, r1, r2, res)
            if e.head.contents.next:
                L.MergeInterNodes(C.byref(e.head))
            L.FreeRelation(relR)
            L.FreeRelation(relS)
            L.FreeResult(res)
        if e.head.contents.next:
            L.CartesianInterResults(C.byref(e.head))
        node = e.head.contents.data.contents
        n, k = int(node.num_tuples), len(query[3])
        got = (C.c_uint64 * k)()
        rc = L.rhj_sum_views_device(k, (C.c_void_p * k)(*[self.cols[b][c].data_ptr() for b, c in query[3]]), (C.c_void_p * k)(*[node.table[b] for b, _ in query[3]]),
                                    (C.c_uint64 * k)(*[n] * k), got)
        assert rc == 0, rc
        L.FreeInterResults(e.head)
        return list(got), n

    def compare(self, name):
        assert self.got["batch"] == self.got["operators"], "%s: the two forms' answers differ" % name
        assert all(rows == (64 + i) * 48 for i, (_, rows) in enumerate(self.got["batch"]))

    def note(self):
        return "64 queries, products of %d to %d rows" % (64 * 48, 127 * 48)

    def close(self):
        self.lib.rhj_unregister_relation_map(self.rm, 6)


def cases(rhj, which, settings):
    for setting in settings:
        if "a" in which:
            g = helpers.Golden()
            rels = g.small_relations
            relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
            cols = [[dev(rhj, c) for c in rel] for rel in relations]
            yield "(a) small: 50 queries, %s" % setting, SwitchForms(rhj, cols, parse_work(g.small["work_lines"]), setting)
        if "b" in which:
            relations, queries = query_shapes.synthetic()
            cols = [[dev(rhj, c) for c in rel] for rel in relations]
            yield "(b) query_shapes synthetic: 24 queries, %s" % setting, SwitchForms(rhj, cols, queries, setting)
        if "c" in which and hasattr(rhj.lib, "rhj_set_query_products"):
            yield "(c) 64 products of two chains of three, %s" % setting, ProductForms(rhj, setting)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--settings", default="levels,one_wait")
    ap.add_argument("--tag", default="this tree")
    ap.add_argument("--out")
    a = ap.parse_args()
    rhj = mod.RHJ(device=0)
    rhj.set_bits(4)
    rhj.lib.rhj_set_timing(0)
    lines = []
    for name, forms in cases(rhj, a.cases, a.settings.split(",")):
        t = {s: [] for s in forms.names}
        for rep in range(a.warmup + a.reps):
            for s in forms.names:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                forms.run(s)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    t[s].append(dt)
        forms.compare(name)
        med = {s: statistics.median(t[s]) for s in t}
        parts = ["%s median %9.3f ms (min %.3f max %.3f, spread %.3f)" % (s, med[s], min(t[s]), max(t[s]), max(t[s]) - min(t[s])) for s in forms.names]
        ratios = " ".join("%s / %s %.2f" % (s, forms.names[0], med[s] / med[forms.names[0]]) for s in forms.names[1:])
        line = "%-10s %-50s %s | %s | %s | %d + %d reps" % (a.tag, name, " | ".join(parts), ratios, forms.note(), a.warmup, a.reps)
        print(line, flush=True)
        lines.append(line)
        if hasattr(forms, "close"):
            forms.close()
        del forms
        rhj.lib.rhj_release()
        torch.cuda.empty_cache()
    rhj.lib.rhj_set_timing(2)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
