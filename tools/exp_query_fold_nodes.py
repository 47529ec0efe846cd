"""The fold route with rhj_set_query_fold_nodes against the route without it, and rhj_join_foldn_batch_device against
rhj_join_foldk_batch_device:
tools/exp_query_fold_nodes.py [--reps 30] [--warmup 5] [--out FILE] [--cases abcd]
The procedure of tools/exp_query_fold_self.py: one process, one library, timing level 0; every repetition times the forms of a
case one after the other on the same device inputs (form 1, form 2, ..., form 1, ...), each with a host clock around work that
ends in a stream synchronisation.  Cases:
  (a) the 50 queries of `small` through rhj_query_batch_device with the fold, keys and self switches on (`three`), with the nodes
      switch on as well (`four`) and with the three once more (`three again`): all do the same work, and the difference between
      the two three-switch forms is the spread to read the fourth against;
  (b) the synthetic batch of tests/query_shapes.py (24 queries, one true cycle) with three switches against four; the level
      counts of both are printed;
  (c) 16 triangle-plus-chain queries, small enough for the levels (a triangle of three 64-row bindings on keys of 8 values, a
      chain of three more 64-row bindings behind it: some 260 000 rows a query), with three switches (by levels to the end) against four (one level, then folds);
  (d) 512 items of 4096 x 4096 rows on two words, both sides through a row-id vector: rhj_join_foldk_batch_device (`foldk`),
      rhj_join_foldn_batch_device with both words naming that one vector (`foldn shared`) and with a second vector of the same
      values for word 1 (`foldn own`).
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
    """forms: name -> (fold, keys, self, nodes)"""

    def __init__(self, rhj, cols, queries, forms):
        self.rhj, self.cols, self.queries, self.forms, self.got, self.levels = rhj, cols, queries, forms, {}, {}
        self.names = tuple(forms)

    def switches(self, fold, keys, self_, nodes):
        self.rhj.set_query_fold(fold)
        self.rhj.set_query_fold_keys(keys)
        self.rhj.set_query_fold_self(self_)
        self.rhj.set_query_fold_nodes(nodes)

    def run(self, form):
        self.switches(*self.forms[form])
        try:
            self.got[form] = self.rhj.query_batch_device(self.cols, self.queries)
            self.levels[form] = self.rhj.lib.rhj_query_batch_last_info().contents.levels
        finally:
            self.switches(False, False, False, False)

    def compare(self, name):
        for form in self.names[1:]:
            assert self.got[form] == self.got[self.names[0]], "%s: the answers of %s differ" % (name, form)

    def note(self):
        return "levels " + " ".join("%s %d" % (s, self.levels[s]) for s in self.names)


class ItemForms:
    """forms: name -> (method name, items)"""

    def __init__(self, rhj, forms, keep):
        self.rhj, self.forms, self.keep, self.got = rhj, forms, keep, {}
        self.names = tuple(forms)

    def run(self, form):
        entry, items = self.forms[form]
        self.got[form] = [[t for _, t in item] for item in getattr(self.rhj, entry)(items)]

    def compare(self, name):
        for form in self.names[1:]:
            assert self.got[form] == self.got[self.names[0]], "%s: the totals of %s differ" % (name, form)

    def note(self):
        return "%d items" % len(self.forms[self.names[0]][1])


def cases(rhj, which):
    three, four = (True, True, True, False), (True, True, True, True)
    if "a" in which:
        g = helpers.Golden()
        rels = g.small_relations
        relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
        cols = [[dev(rhj, c) for c in rel] for rel in relations]
        yield "(a) small: 50 queries", QueryForms(rhj, cols, parse_work(g.small["work_lines"]), {"three": three, "four": four, "three again": three})
    if "b" in which:
        relations, queries = query_shapes.synthetic()
        cols = [[dev(rhj, c) for c in rel] for rel in relations]
        yield "(b) query_shapes synthetic: 24 queries", QueryForms(rhj, cols, queries, {"three": three, "four": four})
    if "c" in which:
        rng = np.random.default_rng(16)
        relations = [[rng.integers(0, 8, size=n), rng.integers(0, 8, size=n), rng.permutation(n) + (1 << 40), rng.integers(0, 8, size=n)] for n in (64, 64)]
        cols = [[dev(rhj, c) for c in rel] for rel in relations]
        joins = [(0, 0, 1, 0), (1, 1, 2, 1), (0, 3, 2, 3), (2, 0, 3, 0), (3, 1, 4, 1), (4, 3, 5, 3)]
        queries = [([0, 0, 0, 1, 1, 1], joins, [], [(0, 2), (5, 2)]) for _ in range(16)]
        yield "(c) 16 triangle-plus-chain queries", QueryForms(rhj, cols, queries, {"three": three, "four": four})
    if "d" in which:
        rng = np.random.default_rng(17)
        n, count = 4096, 512
        keep = [dev(rhj, rng.integers(0, 64, size=n * count)) for _ in range(4)]            # two words a side, 4096 tuples of 64 x 64
        sel = [dev(rhj, rng.integers(0, n, size=n)) for _ in range(2)]
        own = [s.clone() for s in sel]                    # the same values behind another pointer: a vector of word 1's own
        w = dev(rhj, rng.integers(0, 1 << 62, size=n))
        values, outs = [(None, None, None), (w, None, None)], [(0, (None, None, None), None), (1, (w, None, None), True)]
        k_items, shared, owned = [], [], []
        for k in range(count):
            cR, cS = [c[n * k:n * k + n] for c in keep[:2]], [c[n * k:n * k + n] for c in keep[2:]]
            k_items.append((cR, sel[0], cS, sel[1], values, outs))
            shared.append((cR, [sel[0], sel[0]], cS, [sel[1], sel[1]], values, outs))
            owned.append((cR, [sel[0], own[0]], cS, [sel[1], own[1]], values, outs))
        yield "(d) 512 folds of 4096 x 4096 on two words", ItemForms(rhj, {"foldk": ("join_foldk_batch_device", k_items), "foldn shared": ("join_foldn_batch_device", shared),
                                                                            "foldn own": ("join_foldn_batch_device", owned)}, keep + sel + own + [w])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="abcd")
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
