"""The fold route with rhj_set_query_fold_one_wait against the route with the four fold switches alone, and
rhj_fold_pred_batch_device against rhj_filter_batch_device:
tools/exp_query_fold_one_wait.py [--reps 30] [--warmup 5] [--cross-reps 10] [--out FILE] [--cases abcd] [--sizes 12,14,16,18,20,22]
The procedure of tools/exp_query_fold_nodes.py: one process, one library, timing level 0; every repetition times the forms of a
case one after the other on the same device inputs (form 1, form 2, ..., form 1, ...), each with a host clock around work that
ends in a stream synchronisation.  Cases:
  (a) the 50 queries of `small` through rhj_query_batch_device with the fold, keys, self and nodes switches on (`four`), with the
      one-wait switch on as well (`one wait`) and with the four once more (`four again`): the difference between the two
      four-switch forms is the spread to read the fifth against;
  (b) the synthetic batch of tests/query_shapes.py (24 queries) with four switches against five;
  (c) the crossover: 64 three-binding chain queries over three relations of 2^k rows, k from --sizes, every binding under a
      filter that passes about 1 % of its rows, then about 50 %; four switches against five with the row limit raised to admit
      the relations (--cross-reps repetitions after 3 warm-up ones);
  (d) 512 items of 4096 rows with two constant terms: rhj_filter_batch_device, which writes hit lists (`filter`), against
      rhj_fold_pred_batch_device with one written output {ones} (`pred`).
The answers of the forms are compared afterwards.  Prints, and with --out appends, one line per case: per form the median and
the min-max spread, and the ratio of every form to the first."""
import argparse
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

mod = importlib.import_module("sigmod-2018_amd")


def dev(rhj, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


class QueryForms:
    """forms: name -> (one-wait switch, row limit); the four fold switches are on in every form"""

    def __init__(self, rhj, cols, queries, forms):
        self.rhj, self.cols, self.queries, self.forms, self.got, self.info = rhj, cols, queries, forms, {}, {}
        self.names = tuple(forms)

    def switches(self, on, one_wait=False, limit=65536):
        for setter in (self.rhj.set_query_fold, self.rhj.set_query_fold_keys, self.rhj.set_query_fold_self, self.rhj.set_query_fold_nodes):
            setter(on)
        self.rhj.set_query_fold_one_wait(one_wait)
        self.rhj.set_query_fold_one_wait_rows(limit)

    def run(self, form):
        self.switches(True, *self.forms[form])
        try:
            self.got[form] = self.rhj.query_batch_device(self.cols, self.queries)
            self.info[form] = self.rhj.lib.rhj_query_batch_last_one_wait_info().contents.as_dict()
        finally:
            self.switches(False)

    def compare(self, name):
        for form in self.names[1:]:
            assert self.got[form] == self.got[self.names[0]], "%s: the answers of %s differ" % (name, form)

    def note(self):
        on = [s for s in self.names if self.forms[s][0]][0]
        i = self.info[on]
        return "%d of %d queries in %d programs, %d waits, %d launches, %d memsets" % (i["queries"], len(self.queries), i["programs"], i["waits"], i["launches"], i["memsets"])


class ItemForms:
    """forms: name -> a function that runs the form and returns what to compare"""

    def __init__(self, forms, keep, count):
        self.forms, self.keep, self.count, self.got = forms, keep, count, {}
        self.names = tuple(forms)

    def run(self, form):
        self.got[form] = self.forms[form]()

    def compare(self, name):
        for form in self.names[1:]:
            assert self.got[form] == self.got[self.names[0]], "%s: the counts of %s differ" % (name, form)

    def note(self):
        return "%d items" % self.count


def chain_case(rhj, k, percent):
    """three relations of 2^k rows: c0 and c1 keys over 2^k values, c2 a permutation of the rows (c2 < t passes t rows), c3 values;
    64 queries 0.c0 = 1.c0, 1.c1 = 2.c1 with c2 < t on every binding, t about percent of the rows and a little different a query"""
    n = 1 << k
    rng = np.random.default_rng(190 + k)
    relations = [[rng.integers(0, n, size=n), rng.integers(0, n, size=n), rng.permutation(n), rng.integers(0, 1 << 40, size=n)] for _ in range(3)]
    cols = [[dev(rhj, c) for c in rel] for rel in relations]
    queries = []
    for i in range(64):
        t = max(n * percent // 100 + i, 1)
        queries.append(([0, 1, 2], [(0, 0, 1, 0), (1, 1, 2, 1)], [(b, 2, "<", t) for b in range(3)], [(0, 3), (2, 3)]))
    return cols, queries


def cases(rhj, which, sizes):
    four, five = (False, 65536), (True, 65536)
    if "a" in which:
        g = helpers.Golden()
        rels = g.small_relations
        relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
        cols = [[dev(rhj, c) for c in rel] for rel in relations]
        yield "(a) small: 50 queries", QueryForms(rhj, cols, parse_work(g.small["work_lines"]), {"four": four, "one wait": five, "four again": four}), None
    if "b" in which:
        relations, queries = query_shapes.synthetic()
        cols = [[dev(rhj, c) for c in rel] for rel in relations]
        yield "(b) query_shapes synthetic: 24 queries", QueryForms(rhj, cols, queries, {"four": four, "one wait": five}), None
    if "c" in which:
        for percent in (1, 50):
            for k in sizes:
                cols, queries = chain_case(rhj, k, percent)
                yield "(c) 64 chains of three, 2^%d rows, %d %% pass" % (k, percent), QueryForms(rhj, cols, queries, {"four": four, "one wait": (True, 1 << k)}), "cross"
    if "d" in which:
        rng = np.random.default_rng(191)
        n, count = 4096, 512
        keep = [dev(rhj, rng.integers(0, 1 << 20, size=n * count)) for _ in range(2)]
        terms = lambda k: [(keep[0][n * k:n * k + n], "<", 1 << 19), (keep[1][n * k:n * k + n], ">", 1 << 18)]
        filters = [(terms(k), None) for k in range(count)]
        preds = [(n, [(c, None, op, v) for c, op, v in terms(k)], [], [((None, None, None), True)]) for k in range(count)]
        yield "(d) 512 items of 4096 rows, two constant terms", ItemForms(
            {"filter": lambda: [h for _, h in rhj.filter_batch_device(filters)], "pred": lambda: [item[0][1] for item in rhj.fold_pred_batch_device(preds)]}, keep, count), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cross-reps", type=int, default=10)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--sizes", default="12,14,16,18,20,22")
    ap.add_argument("--out")
    a = ap.parse_args()
    rhj = mod.RHJ(device=0)
    rhj.set_bits(4)
    rhj.lib.rhj_set_timing(0)
    lines = []
    for name, forms, kind in cases(rhj, a.cases, [int(k) for k in a.sizes.split(",")]):
        warmup, reps = (3, a.cross_reps) if kind == "cross" else (a.warmup, a.reps)
        t = {s: [] for s in forms.names}
        for rep in range(warmup + reps):
            for s in forms.names:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                forms.run(s)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= warmup:
                    t[s].append(dt)
        forms.compare(name)
        med = {s: statistics.median(t[s]) for s in t}
        parts = ["%s median %9.3f ms (min %.3f max %.3f, spread %.3f)" % (s, med[s], min(t[s]), max(t[s]), max(t[s]) - min(t[s])) for s in forms.names]
        ratios = " ".join("%s / %s %.2f" % (s, forms.names[0], med[s] / med[forms.names[0]]) for s in forms.names[1:])
        line = "%-46s %s | %s | %s | %d + %d reps" % (name, " | ".join(parts), ratios, forms.note(), warmup, reps)
        print(line, flush=True)
        lines.append(line)
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
