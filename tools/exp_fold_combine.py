"""rhj_set_fold_combine: what the combiner costs where nothing combines and what it buys on skewed keys:
tools/exp_fold_combine.py --parent PARENT.so [--reps 30] [--warmup 5] [--cases abcde] [--out FILE]
DESIGN.md 6's procedure: one process, timing level 0, both libraries loaded (--parent: librhj.so built from the parent commit,
which has no such switch; this tree's from its usual place); every repetition times the forms of a case one after the other on
the same device inputs - `parent`, this tree with the switch `off`, this tree with it `on` - each with a host clock around one
library call that ends in a stream synchronisation, on descriptors built beforehand.  The forms' answers are compared afterwards.
Cases:
  (a) the 50 queries of `small` through rhj_query_batch_device, the four fold switches and the one-wait programs on (row limit 65 536);
  (b) 512 items of 4096 x 4096 rows on distinct keys, 1 value and 9 values, rhj_join_fold_batch_device and (two key columns)
      rhj_join_foldk_batch_device: the price where nothing combines;
  (c) one fold item of 200 000 x 200 000 rows on 1, 2, 16 and 1024 keys interleaved row by row, 1 value and 9 values;
  (d) a child of 4 M rows on 20 keys folded into a parent of 20 rows, 1 value and 9 values;
  (e) one rhj_join_sum_batch_device item of 200 000 x 200 000 rows on 1 key and on 2 keys, one term a side.
Prints, and with --out appends, one line per case: per form the median and the min-max spread, every form's ratio to `parent`,
and the combine info of the `on` form."""
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

mod = importlib.import_module("sigmod-2018_amd")
FORMS = ("parent", "off", "on")


def dev(rhj, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


class Case:
    """a call on descriptors built once; run(form) makes it on the form's library and keeps the answers"""

    def __init__(self, libs, name):
        self.libs, self.name, self.got, self.info = libs, name, {}, None

    def lib(self, form):
        rhj = self.libs["parent" if form == "parent" else "tree"]
        if form != "parent":
            rhj.set_fold_combine(form == "on")
        return rhj

    def after(self, form, rhj):
        if form == "on":
            self.info = rhj.table_batch_last_combine_info()

    def compare(self):
        for form in FORMS[1:]:
            assert self.got[form] == self.got["parent"], "%s: the answers of %s differ from the parent's" % (self.name, form)


class Queries(Case):
    def __init__(self, libs, name, cols, queries):
        super().__init__(libs, name)
        self.cols, self.queries = cols, queries

    def run(self, form):
        rhj = self.lib(form)
        for setter in (rhj.set_query_fold, rhj.set_query_fold_keys, rhj.set_query_fold_self, rhj.set_query_fold_nodes, rhj.set_query_fold_one_wait):
            setter(True)
        rhj.set_query_fold_one_wait_rows(65536)
        self.got[form] = rhj.query_batch_device(self.cols, self.queries)
        self.after(form, rhj)


class Folds(Case):
    """items = [(key columns of R, key columns of S, nR, nS)] as device tensors; every item has the same `weights` over S's
    positions as its values and one output a value, totals only"""

    def __init__(self, libs, name, items, weights, tuple_keys=False):
        super().__init__(libs, name)
        self.keep = (items, weights)
        Desc = mod.JoinFoldKDesc if tuple_keys else mod.JoinFoldDesc
        self.entry = "rhj_join_foldk_batch_device" if tuple_keys else "rhj_join_fold_batch_device"
        self.arr = (Desc * len(items))()
        for d, (kR, kS, nR, nS) in zip(self.arr, items):
            if tuple_keys:
                d.nkeys = len(kR)
                for t, (a, b) in enumerate(zip(kR, kS)):
                    d.d_colR[t], d.d_colS[t] = a.data_ptr(), b.data_ptr()
            else:
                d.d_colR, d.d_colS = kR[0].data_ptr(), kS[0].data_ptr()
            d.nR, d.nS, d.nvalues, d.nouts = nR, nS, len(weights), len(weights)
            for c, w in enumerate(weights):
                d.values[c].d_w = w.data_ptr()
                d.outs[c].value = c

    def run(self, form):
        rhj = self.lib(form)
        rc = getattr(rhj.lib, self.entry)(self.arr, len(self.arr))
        assert rc == 0, rc
        self.got[form] = [[d.outs[c].total for c in range(d.nouts)] for d in self.arr]
        self.after(form, rhj)


class Sums(Case):
    def __init__(self, libs, name, kR, kS, tR, tS):
        super().__init__(libs, name)
        self.keep = (kR, kS, tR, tS)
        self.arr = (mod.JoinSumDesc * 1)()
        d = self.arr[0]
        d.d_colR, d.nR, d.d_colS, d.nS, d.nterms = kR.data_ptr(), kR.shape[0], kS.data_ptr(), kS.shape[0], 2
        d.terms[0].side, d.terms[0].d_col = 0, tR.data_ptr()
        d.terms[1].side, d.terms[1].d_col = 1, tS.data_ptr()

    def run(self, form):
        rhj = self.lib(form)
        rc = rhj.lib.rhj_join_sum_batch_device(self.arr, 1)
        assert rc == 0, rc
        d = self.arr[0]
        self.got[form] = (d.matches, d.terms[0].sum, d.terms[1].sum)
        self.after(form, rhj)


def cases(libs, which):
    rhj = libs["tree"]
    rng = np.random.default_rng(2121)
    wide = lambda n: rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    if "a" in which:
        import helpers
        from query_model import parse_work
        g = helpers.Golden()
        rels = g.small_relations
        cols = [[dev(rhj, np.asarray(c, dtype=np.uint64)) for c in rels["r%d" % r]] for r in range(len(rels))]
        yield Queries(libs, "(a) small: 50 queries, fold switches and one wait", cols, parse_work(g.small["work_lines"]))
    if "b" in which:
        n, rows = 512, 4096
        words = [rng.permutation(n * rows).astype(np.uint64) + np.uint64(1) for _ in range(2)]
        # S's rows of item k are R's in another order (a tuple's words move together): every key of the item once a side
        order = np.concatenate([rng.permutation(rows) + k * rows for k in range(n)])
        keys, ks = [dev(rhj, x) for x in words], [dev(rhj, x[order]) for x in words]
        for nv in (1, 9):
            w = [dev(rhj, wide(rows)) for _ in range(nv)]
            for tuple_keys in (False, True):
                nk = 2 if tuple_keys else 1
                items = [([c[k * rows:(k + 1) * rows] for c in keys[:nk]], [c[k * rows:(k + 1) * rows] for c in ks[:nk]], rows, rows) for k in range(n)]
                yield Folds(libs, "(b) 512 x (4096 x 4096) distinct keys, %s, %d value%s" % ("foldk on 2 words" if tuple_keys else "fold", nv, "s" * (nv > 1)), items, w, tuple_keys)
    if "c" in which:
        rows = 200_000
        for nk in (1, 2, 16, 1024):
            pool = rng.integers(1, 1 << 62, size=nk, dtype=np.uint64)
            kR, kS = dev(rhj, pool[np.arange(rows) % nk]), dev(rhj, pool[(np.arange(rows) + 1) % nk])
            for nv in (1, 9):
                w = [dev(rhj, wide(rows)) for _ in range(nv)]
                yield Folds(libs, "(c) 200 000 x 200 000 on %d key%s, %d value%s" % (nk, "s" * (nk > 1), nv, "s" * (nv > 1)), [([kR], [kS], rows, rows)], w)
    if "d" in which:
        rows = 4 << 20
        pool = rng.integers(1, 1 << 62, size=20, dtype=np.uint64)
        kR, kS = dev(rhj, pool), dev(rhj, pool[rng.integers(0, 20, size=rows)])
        for nv in (1, 9):
            w = [dev(rhj, wide(rows)) for _ in range(nv)]
            yield Folds(libs, "(d) 4 M rows on 20 keys into 20 rows, %d value%s" % (nv, "s" * (nv > 1)), [([kR], [kS], 20, rows)], w)
    if "e" in which:
        rows = 200_000
        for nk in (1, 2):
            pool = rng.integers(1, 1 << 62, size=nk, dtype=np.uint64)
            kR, kS = dev(rhj, pool[np.arange(rows) % nk]), dev(rhj, pool[(np.arange(rows) + 1) % nk])
            yield Sums(libs, "(e) join sums, 200 000 x 200 000 on %d key%s" % (nk, "s" * (nk > 1)), kR, kS, dev(rhj, wide(rows)), dev(rhj, wide(rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="abcde")
    ap.add_argument("--out")
    a = ap.parse_args()
    libs = {"tree": mod.RHJ(device=0), "parent": mod.RHJ(device=0, lib_path=a.parent)}
    assert not hasattr(libs["parent"].lib, "rhj_set_fold_combine"), "--parent names a library that has the switch"
    was = libs["tree"].lib.rhj_get_fold_combine()
    for rhj in libs.values():
        rhj.set_bits(4)
        rhj.lib.rhj_set_timing(0)
    lines = []
    for case in cases(libs, a.cases):
        t = {s: [] for s in FORMS}
        for rep in range(a.warmup + a.reps):
            for s in FORMS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                case.run(s)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    t[s].append(dt)
        case.compare()
        med = {s: statistics.median(t[s]) for s in t}
        parts = ["%s median %9.3f ms (min %.3f max %.3f)" % (s, med[s], min(t[s]), max(t[s])) for s in FORMS]
        ratios = " ".join("%s / parent %.2f" % (s, med[s] / med["parent"]) for s in FORMS[1:])
        line = "%-62s %s | %s | on: %s | %d + %d reps" % (case.name, " | ".join(parts), ratios, case.info, a.warmup, a.reps)
        print(line, flush=True)
        lines.append(line)
        del case
        for rhj in libs.values():
            rhj.lib.rhj_release()
        torch.cuda.empty_cache()
    libs["tree"].set_fold_combine(was)
    for rhj in libs.values():
        rhj.lib.rhj_set_timing(2)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
