"""The fold route with rhj_set_query_fold_self against the route without it:
tools/exp_query_fold_self.py [--reps 30] [--warmup 5] [--out FILE] [--cases abc]
The procedure of tools/exp_query_foldk.py: one process, one library, timing level 0; every repetition times the forms of a case
one after the other on the same inputs (form 1, form 2, ..., form 1, ...), each with a host clock around work that ends in a
stream synchronisation.  Cases:
  (a) the 50 queries of `small` through rhj_query_batch_device with the fold and keys switches on (`two`), with the self switch
      on as well (`three`) and with the two once more (`two again`): all three do the same work, and the difference between the
      two two-switch forms is the spread to read the third against;
  (b) the synthetic batch of tests/query_shapes.py (24 queries: self-joins first, last and alone, queries without a join, one
      true cycle) with the fold and keys switches (`two`) against all three (`three`); the level counts of both are printed;
  (c) 512 queries without a join over a relation of 4096 rows, each with one one-binding predicate and two views: by levels (all
      switches off, `levels`) against the new route (`three`).
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
    """forms: name -> (fold, keys, self)"""

    def __init__(self, rhj, cols, queries, forms):
        self.rhj, self.cols, self.queries, self.forms, self.got, self.levels = rhj, cols, queries, forms, {}, {}
        self.names = tuple(forms)

    def run(self, form):
        fold, keys, self_ = self.forms[form]
        self.rhj.set_query_fold(fold)
        self.rhj.set_query_fold_keys(keys)
        self.rhj.set_query_fold_self(self_)
        try:
            self.got[form] = self.rhj.query_batch_device(self.cols, self.queries)
            self.levels[form] = self.rhj.lib.rhj_query_batch_last_info().contents.levels
        finally:
            self.rhj.set_query_fold(False)
            self.rhj.set_query_fold_keys(False)
            self.rhj.set_query_fold_self(False)

    def compare(self, name):
        for form in self.names[1:]:
            assert self.got[form] == self.got[self.names[0]], "%s: the answers of %s differ" % (name, form)

    def note(self):
        return "levels " + " ".join("%s %d" % (s, self.levels[s]) for s in self.names)


def cases(rhj, which):
    two, three = (True, True, False), (True, True, True)
    if "a" in which:
        g = helpers.Golden()
        rels = g.small_relations
        relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
        cols = [[dev(rhj, c) for c in rel] for rel in relations]
        yield "(a) small: 50 queries", QueryForms(rhj, cols, parse_work(g.small["work_lines"]), {"two": two, "three": three, "two again": two})
    if "b" in which:
        relations, queries = query_shapes.synthetic()
        cols = [[dev(rhj, c) for c in rel] for rel in relations]
        yield "(b) query_shapes synthetic: 24 queries", QueryForms(rhj, cols, queries, {"two": two, "three": three})
    if "c" in which:
        rng = np.random.default_rng(15)
        c0 = rng.integers(0, 8, size=4096)
        rel = [c0, np.where(rng.integers(0, 2, size=4096) == 1, c0, 9), rng.permutation(4096) + (1 << 40), rng.integers(0, 8, size=4096)]
        cols = [[dev(rhj, c) for c in rel]]
        queries = [([0], [(0, 0, 0, 1)], [], [(0, 2), (0, 3)]) for _ in range(512)]
        yield "(c) 512 join-less queries x 4096 rows", QueryForms(rhj, cols, queries, {"levels": (False, False, False), "three": three})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--out")
    a = ap.parse_args()
    rhj = mod.RHJ(device=0)
    rhj.set_bits(4)
    rhj.lib.rhj_set_timing(0)
    lines = []
    for name, forms in cases(rhj, a.cases):
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
        line = "%-40s %s | %s | %s | %d + %d reps" % (name, " | ".join(parts), ratios, forms.note(), a.warmup, a.reps)
        print(line, flush=True)
        lines.append(line)
        del forms
        torch.cuda.empty_cache()
    rhj.lib.rhj_set_timing(2)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
