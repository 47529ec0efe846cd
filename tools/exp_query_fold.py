"""The fold route against the level route, and the fold primitive against the join sums: tools/exp_query_fold.py [--reps 30]
[--warmup 5] [--out FILE] [--cases abc]
One process, one library, timing level 0; every repetition times the forms of a case one after the other on the same inputs
(form 1, form 2, ..., form 1, ...), each with a host clock around work that ends in a stream synchronisation.  Cases:
  (a) the 50 queries of `small` through rhj_query_batch_device: both switches off (`levels`), rhj_set_query_sum_last on and the
      fold off (`sum_last`), rhj_set_query_fold on (`fold`);
  (b) 512 items of 4096 x 4096 rows: rhj_join_sum_batch_device without a term (`sums`) against rhj_join_fold_batch_device with
      1 value and with 9 values, one output a value that writes its vector;
  (c) one item of 200 000 x 200 000 rows on one key: the same three forms.
The answers of the forms are compared afterwards (case a: all of them; b, c: the row counts).  Prints, and with --out appends,
one line per case: per form the median and the min-max spread, and the ratio of every form to the first."""
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
from query_model import parse_work

mod = importlib.import_module("sigmod-2018_amd")


def dev(rhj, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


class QueryForms:
    names = ("levels", "sum_last", "fold")

    def __init__(self, rhj, cols, queries):
        self.rhj, self.cols, self.queries, self.got = rhj, cols, queries, {}

    def run(self, form):
        self.rhj.set_query_sum_last(form == "sum_last")
        self.rhj.set_query_fold(form == "fold")
        try:
            self.got[form] = self.rhj.query_batch_device(self.cols, self.queries)
        finally:
            self.rhj.set_query_sum_last(False)
            self.rhj.set_query_fold(False)

    def compare(self, name):
        assert self.got["levels"] == self.got["sum_last"] == self.got["fold"], "%s: the answers differ" % name


class ItemForms:
    """items [(keysR, keysS)] as device tensors: the join sums without a term, and folds of 1 and of 9 values with one written
    output a value (value 0 ones, the others a weight vector of S's)"""
    names = ("sums", "fold 1 value", "fold 9 values")

    def __init__(self, rhj, items, weights):
        self.lib, n = rhj.lib, len(items)
        self.sums = (mod.JoinSumDesc * n)()
        self.folds = {1: (mod.JoinFoldDesc * n)(), 9: (mod.JoinFoldDesc * n)()}
        self.keep = []
        for i, (kR, kS) in enumerate(items):
            s = self.sums[i]
            s.d_colR, s.nR, s.d_colS, s.nS, s.nterms = kR.data_ptr(), kR.shape[0], kS.data_ptr(), kS.shape[0], 0
            for nv, arr in self.folds.items():
                d = arr[i]
                d.d_colR, d.nR, d.d_colS, d.nS, d.nvalues, d.nouts = kR.data_ptr(), kR.shape[0], kS.data_ptr(), kS.shape[0], nv, nv
                out = torch.empty((nv, kR.shape[0]), dtype=torch.int64, device=rhj.dev)
                self.keep.append(out)
                for c in range(nv):
                    d.values[c].d_w = weights[c % len(weights)].data_ptr() if c else None
                    d.outs[c].value, d.outs[c].d_out = c, out[c].data_ptr()

    def run(self, form):
        if form == "sums":
            rc = self.lib.rhj_join_sum_batch_device(self.sums, len(self.sums))
        else:
            arr = self.folds[1 if form == "fold 1 value" else 9]
            rc = self.lib.rhj_join_fold_batch_device(arr, len(arr))
        assert rc == 0, rc

    def compare(self, name):
        for i in range(len(self.sums)):
            assert self.sums[i].matches == self.folds[1][i].outs[0].total == self.folds[9][i].outs[0].total, "%s: the rows of item %d differ" % (name, i)


def cases(rhj, which):
    if "a" in which:
        g = helpers.Golden()
        rels = g.small_relations
        relations = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
        cols = [[dev(rhj, c) for c in rel] for rel in relations]
        yield "(a) small: 50 queries", QueryForms(rhj, cols, parse_work(g.small["work_lines"]))
    torch.manual_seed(12)
    rnd = lambda hi, n: torch.randint(0, hi, (n,), dtype=torch.int64, device=rhj.dev)      # noqa: E731
    if "b" in which:
        keys = [rnd(4096, 4096) for _ in range(16)]
        yield "(b) 512 items x 4096 x 4096 rows", ItemForms(rhj, [(keys[i % 16], keys[(i + 5) % 16]) for i in range(512)], [rnd(1 << 62, 4096) for _ in range(8)])
    if "c" in which:
        hot = torch.full((200_000,), 77, dtype=torch.int64, device=rhj.dev)
        yield "(c) 200 000 x 200 000 rows on one key", ItemForms(rhj, [(hot, hot)], [rnd(1 << 62, 200_000) for _ in range(8)])


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
        line = "%-40s %s | %s | %d + %d reps" % (name, " | ".join(parts), ratios, a.warmup, a.reps)
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
