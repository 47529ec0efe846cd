"""The fold route with tuple keys against the fold route without, and the tuple-key fold primitive against the one-key one:
tools/exp_query_foldk.py [--reps 30] [--warmup 5] [--out FILE] [--cases abc]
The procedure of tools/exp_query_fold.py: one process, one library, timing level 0; every repetition times the forms of a case
one after the other on the same inputs (form 1, form 2, ..., form 1, ...), each with a host clock around work that ends in a
stream synchronisation.  Cases:
  (a) the 50 queries of `small` through rhj_query_batch_device with rhj_set_query_fold on (`fold`: 44 queries fold, six run by
      levels) against rhj_set_query_fold_keys on as well (`fold + keys`: all 50 fold);
  (b) 512 items of 4096 x 4096 rows, one value that writes its vector: rhj_join_fold_batch_device (`fold`) against
      rhj_join_foldk_batch_device on 1, 2 and 4 key columns.  Every key column of an item is the same column, so the tuples
      match exactly where the one key does and all forms do the same adds;
  (c) one item of 200 000 x 200 000 rows on one tuple: the same with `foldk 2 keys` alone against `fold`.
The answers of the forms are compared afterwards (case a: all of them; b, c: the totals).  Prints, and with --out appends, one
line per case: per form the median and the min-max spread, and the ratio of every form to the first."""
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
    names = ("fold", "fold + keys")

    def __init__(self, rhj, cols, queries):
        self.rhj, self.cols, self.queries, self.got = rhj, cols, queries, {}

    def run(self, form):
        self.rhj.set_query_fold(True)
        self.rhj.set_query_fold_keys(form == "fold + keys")
        try:
            self.got[form] = self.rhj.query_batch_device(self.cols, self.queries)
        finally:
            self.rhj.set_query_fold(False)
            self.rhj.set_query_fold_keys(False)

    def compare(self, name):
        assert self.got["fold"] == self.got["fold + keys"], "%s: the answers differ" % name


class ItemForms:
    """items [(keysR, keysS)] as device tensors: a fold of one value (ones) with one written output, on the one-key primitive and
    on the tuple-key one with the key column repeated nkeys times"""

    def __init__(self, rhj, items, nkeys=(1, 2, 4)):
        self.lib, n = rhj.lib, len(items)
        self.names = ("fold",) + tuple("foldk %d key%s" % (k, "s" if k > 1 else "") for k in nkeys)
        self.fold = (mod.JoinFoldDesc * n)()
        self.foldk = {name: (mod.JoinFoldKDesc * n)() for name in self.names[1:]}
        self.keep = []
        for i, (kR, kS) in enumerate(items):
            for arr, nk in [(self.fold, 0)] + [(self.foldk[name], k) for name, k in zip(self.names[1:], nkeys)]:
                d = arr[i]
                if nk:
                    d.nkeys = nk
                    for t in range(nk):
                        d.d_colR[t], d.d_colS[t] = kR.data_ptr(), kS.data_ptr()
                else:
                    d.d_colR, d.d_colS = kR.data_ptr(), kS.data_ptr()
                d.nR, d.nS, d.nvalues, d.nouts = kR.shape[0], kS.shape[0], 1, 1
                out = torch.empty((kR.shape[0],), dtype=torch.int64, device=rhj.dev)
                self.keep.append(out)
                d.outs[0].value, d.outs[0].d_out = 0, out.data_ptr()

    def run(self, form):
        if form == "fold":
            rc = self.lib.rhj_join_fold_batch_device(self.fold, len(self.fold))
        else:
            rc = self.lib.rhj_join_foldk_batch_device(self.foldk[form], len(self.fold))
        assert rc == 0, rc

    def compare(self, name):
        for i in range(len(self.fold)):
            for form, arr in self.foldk.items():
                assert self.fold[i].outs[0].total == arr[i].outs[0].total, "%s: the totals of item %d differ (%s)" % (name, i, form)


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
        yield "(b) 512 items x 4096 x 4096 rows", ItemForms(rhj, [(keys[i % 16], keys[(i + 5) % 16]) for i in range(512)])
    if "c" in which:
        hot = torch.full((200_000,), 77, dtype=torch.int64, device=rhj.dev)
        yield "(c) 200 000 x 200 000 rows on one tuple", ItemForms(rhj, [(hot, hot)], nkeys=(2,))


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
