"""A final join's sums without its pairs against the pair route: tools/exp_join_sum_batch.py [--reps 30] [--warmup 5] [--out FILE]
[--cases abc]
One process, one library, timing level 0; every repetition times two forms of the same work on the same inputs,
  pairs    rhj_join_cols_batch_device with room for every join's count (known beforehand: no second call), then
           rhj_apply_batch_device over the pairs with d_dst NULL: one call each per batch,
  sums     rhj_join_sum_batch_device: one call per batch,
alternating pairs, sums, pairs ..., each with a host clock around work that ends in a stream synchronisation.  Cases:
  (a) the final joins of `small`: per query whose last predicate joins two nodes, the two key vectors and the views' values
      as they stand before that join (tests/join_sum_model.py: final_join_item), materialised as columns;
  (b) 512 items of 4096 x 4096 rows with three terms;
  (c) the 50 queries of `small` through rhj_query_batch_device with rhj_set_query_sum_last off and on (`pairs` is off).
Outputs are allocated once; matches and sums of the two forms are compared afterwards.  Prints, and with --out appends, one
line per case: medians, min-max spreads, the ratio."""
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
import join_sum_model as jm
from query_model import parse_work

mod = importlib.import_module("sigmod-2018_amd")


def dev(rhj, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


class Forms:
    """items [(keysR, keysS, [(side, values)])] as device tensors, prepared for both forms"""

    def __init__(self, rhj, items):
        self.lib, self.items, n = rhj.lib, items, len(items)
        self.sums = (mod.JoinSumDesc * n)()
        self.joins = (mod.JoinColsDesc * n)()
        self.applies = (mod.ApplyDesc * n)()
        self.keep = []
        counts = rhj.join_sum_batch_device([(kR, None, kS, None, []) for kR, kS, _ in items])
        for i, (kR, kS, terms) in enumerate(items):
            m = counts[i][0]
            out = torch.empty((max(m, 1), 2), dtype=torch.int64, device=rhj.dev)
            self.keep.append(out)
            s, j, a = self.sums[i], self.joins[i], self.applies[i]
            s.d_colR, s.nR, s.d_colS, s.nS, s.nterms = kR.data_ptr(), kR.shape[0], kS.data_ptr(), kS.shape[0], len(terms)
            j.d_colR, j.nR, j.d_colS, j.nS, j.d_out, j.out_capacity = kR.data_ptr(), kR.shape[0], kS.data_ptr(), kS.shape[0], out.data_ptr(), m
            a.d_idx, a.n, a.idx_stride, a.nterms = out.data_ptr(), m, 2, len(terms)
            for t, (side, values) in enumerate(terms):
                s.terms[t].side, s.terms[t].d_col = side, values.data_ptr()
                a.terms[t].side, a.terms[t].d_col = side, values.data_ptr()

    def pairs(self):
        rc = self.lib.rhj_join_cols_batch_device(self.joins, len(self.items))
        assert rc == 0, rc
        rc = self.lib.rhj_apply_batch_device(self.applies, len(self.items))
        assert rc == 0, rc

    def sums_(self):
        rc = self.lib.rhj_join_sum_batch_device(self.sums, len(self.items))
        assert rc == 0, rc

    def compare(self, name):
        for i, (_, _, terms) in enumerate(self.items):
            assert self.sums[i].matches == self.joins[i].matches, "%s: matches of item %d differ" % (name, i)
            if self.joins[i].matches:
                assert [self.sums[i].terms[t].sum for t in range(len(terms))] == [self.applies[i].terms[t].sum for t in range(len(terms))], \
                    "%s: sums of item %d differ" % (name, i)


class QueryForms:
    def __init__(self, rhj, cols, queries):
        self.rhj, self.cols, self.queries, self.got = rhj, cols, queries, {}

    def pairs(self):
        self.rhj.set_query_sum_last(False)
        self.got["pairs"] = self.rhj.query_batch_device(self.cols, self.queries)

    def sums_(self):
        self.rhj.set_query_sum_last(True)
        try:
            self.got["sums"] = self.rhj.query_batch_device(self.cols, self.queries)
        finally:
            self.rhj.set_query_sum_last(False)

    def compare(self, name):
        assert self.got["pairs"] == self.got["sums"], "%s: the answers differ" % name


def cases(rhj, which):
    g = helpers.Golden()
    rels = g.small_relations
    relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    queries = parse_work(g.small["work_lines"])
    if "a" in which:
        items = [it for it in (jm.final_join_item(relations, q) for q in queries) if it is not None and len(it[0]) and len(it[1])]
        items = [(dev(rhj, kR), dev(rhj, kS), [(side, dev(rhj, v)) for side, v in terms]) for kR, kS, terms in items]
        yield "(a) small: %d final joins" % len(items), Forms(rhj, items)
    if "b" in which:
        torch.manual_seed(12)
        rnd = lambda hi, n: torch.randint(0, hi, (n,), dtype=torch.int64, device=rhj.dev)      # noqa: E731
        keys = [rnd(4096, 4096) for _ in range(16)]
        vals = [rnd(1 << 62, 4096) for _ in range(8)]
        yield "(b) 512 items x 4096 x 4096 rows x 3 terms", Forms(rhj, [(keys[i % 16], keys[(i + 5) % 16], [(0, vals[i % 8]), (1, vals[(i + 3) % 8]), (0, vals[(i + 1) % 8])])
                                                                         for i in range(512)])
    if "c" in which:
        cols = [[dev(rhj, c) for c in rel] for rel in relations]
        yield "(c) small: 50 queries, switch off / on", QueryForms(rhj, cols, queries)


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
        t = {"pairs": [], "sums": []}
        for rep in range(a.warmup + a.reps):
            for s in ("pairs", "sums"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                getattr(forms, "sums_" if s == "sums" else s)()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    t[s].append(dt)
        forms.compare(name)
        med = {s: statistics.median(t[s]) for s in t}
        parts = ["%s median %9.3f ms (min %.3f max %.3f, spread %.3f)" % (s, med[s], min(t[s]), max(t[s]), max(t[s]) - min(t[s])) for s in ("pairs", "sums")]
        line = "%-46s %s | pairs / sums %.2f | %d + %d reps" % (name, " | ".join(parts), med["pairs"] / med["sums"], a.warmup, a.reps)
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
