"""rhj_set_fold_resident: where one workgroup with the table in LDS beats the three launches over a table in HBM,
and where it loses:  tools/exp_fold_resident.py --parent PARENT.so [--tree TREE.so] [--reps 30] [--warmup 5] [--cases abcd] [--out FILE]
DESIGN.md 6's procedure: one process, timing level 0, both libraries loaded (--parent: librhj.so built from the parent commit,
which has no such switch; this tree's from its usual place); every repetition times the forms of a case one after the other on
the same device inputs - `parent`, this tree with the switch `off`, this tree with it `on` - each with a host clock around one
library call that ends in a stream synchronisation, on descriptors built beforehand.  The forms' answers are compared afterwards.
Cases:
  (a) 512 items of n x n rows on distinct keys with one value, n = 256, 1024, 2048, 4096;
  (b) items with a build side of 4096 rows and the other side of 2^12, 2^14, 2^16 and 2^18 rows, in batches of 8 and of 512 items
      (the sizes beyond the row limit the library was built with run in the table form and show as on / off of 1.00; --tree names
      a build of this tree with FOLD_LDS_MAX_ROWS raised, to measure beyond it): this is what FOLD_LDS_MAX_ROWS is set from;
  (c) one item of 4096 x 65 536 rows on one key, and one on two keys interleaved row by row: same-address LDS atomics
      against the slot combiner (the build side is 4096 rows of the same keys, so that the item is resident);
  (d) the 50 queries of `small` through rhj_query_batch_device with the fold, keys and self switches on, by waits and with the
      one-wait programs at a row limit of 65 536.
Prints, and with --out appends, one line per case: per form the median and the min-max spread, every form's ratio to `parent`,
on / off, and the resident info (and, for the queries, the one-wait info) of the `on` form."""
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
            rhj.set_fold_resident(form == "on")
        return rhj

    def compare(self):
        for form in FORMS[1:]:
            assert self.got[form] == self.got["parent"], "%s: the answers of %s differ from the parent's" % (self.name, form)


class Queries(Case):
    def __init__(self, libs, name, cols, queries, one_wait):
        super().__init__(libs, name)
        self.cols, self.queries, self.one_wait = cols, queries, one_wait

    def run(self, form):
        rhj = self.lib(form)
        for setter in (rhj.set_query_fold, rhj.set_query_fold_keys, rhj.set_query_fold_self):
            setter(True)
        rhj.set_query_fold_one_wait(self.one_wait)
        rhj.set_query_fold_one_wait_rows(65536)
        res, info = rhj.query_batch_device(self.cols, self.queries, with_info=True)
        self.got[form] = [(list(s), r) for s, r in res]
        if form == "on":
            ow = info.one_wait_info
            self.info = "%s launches %d memsets %d rounds %d" % (rhj.table_batch_last_resident_info(), ow["launches"], ow["memsets"], ow["rounds"])
        if form == "off":
            ow = info.one_wait_info
            self.off_info = "launches %d memsets %d" % (ow["launches"], ow["memsets"])


class Folds(Case):
    """items = [(keys of R, keys of S)] as device tensors; every item has one value, a weight over S's positions, and one output
    that writes its vector"""

    def __init__(self, libs, name, items, weight):
        super().__init__(libs, name)
        rhj = libs["tree"]
        self.keep = (items, weight, [])
        self.arr = (mod.JoinFoldDesc * len(items))()
        for d, (kR, kS) in zip(self.arr, items):
            d.d_colR, d.nR, d.d_colS, d.nS, d.nvalues, d.nouts = kR.data_ptr(), kR.shape[0], kS.data_ptr(), kS.shape[0], 1, 1
            d.values[0].d_w = weight.data_ptr()
            out = torch.empty((kR.shape[0],), dtype=torch.int64, device=rhj.dev)
            self.keep[2].append(out)
            d.outs[0].value, d.outs[0].d_out = 0, out.data_ptr()

    def run(self, form):
        rhj = self.lib(form)
        rc = rhj.lib.rhj_join_fold_batch_device(self.arr, len(self.arr))
        assert rc == 0, rc
        self.got[form] = [d.outs[0].total for d in self.arr]
        if form == "on":
            self.info = rhj.table_batch_last_resident_info()


def cases(libs, which):
    rhj = libs["tree"]
    rng = np.random.default_rng(2222)
    wide = lambda n: rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    if "a" in which:
        for rows in (256, 1024, 2048, 4096):
            n = 512
            keys = rng.permutation(n * rows).astype(np.uint64) + np.uint64(1)
            order = np.concatenate([rng.permutation(rows) + k * rows for k in range(n)])
            kR, kS = dev(rhj, keys), dev(rhj, keys[order])
            items = [(kR[k * rows:(k + 1) * rows], kS[k * rows:(k + 1) * rows]) for k in range(n)]
            yield Folds(libs, "(a) 512 x (%d x %d) distinct keys, 1 value" % (rows, rows), items, dev(rhj, wide(rows)))
    if "b" in which:
        build = 4096
        for n in (8, 512):
            for log2 in (12, 14, 16, 18):
                other = 1 << log2
                pool = min(n, 16)                        # the sides are shared among the items, 16 different ones at the most
                # item k: R builds with 4096 distinct keys of its own, S's keys are drawn from them
                kb = dev(rhj, np.concatenate([rng.permutation(build).astype(np.uint64) + np.uint64(p * build + 1) for p in range(pool)]))
                ko = [dev(rhj, rng.integers(1, build + 1, size=other, dtype=np.uint64) + np.uint64(p * build)) for p in range(pool)]
                items = [(kb[(k % pool) * build:(k % pool + 1) * build], ko[k % pool]) for k in range(n)]
                yield Folds(libs, "(b) %d x (4096 x 2^%d), 1 value" % (n, log2), items, dev(rhj, wide(other)))
    if "c" in which:
        rows = 65536
        for nk in (1, 2):
            pool = rng.integers(1, 1 << 62, size=nk, dtype=np.uint64)
            kR, kS = dev(rhj, pool[np.arange(4096) % nk]), dev(rhj, pool[(np.arange(rows) + 1) % nk])
            yield Folds(libs, "(c) 4096 x 65 536 on %d key%s, 1 value" % (nk, "s" * (nk > 1)), [(kR, kS)], dev(rhj, wide(rows)))
    if "d" in which:
        import helpers
        from query_model import parse_work
        g = helpers.Golden()
        rels = g.small_relations
        cols = [[dev(rhj, np.asarray(c, dtype=np.uint64)) for c in rels["r%d" % r]] for r in range(len(rels))]
        for one_wait in (False, True):
            yield Queries(libs, "(d) small: 50 queries, fold + keys + self, %s" % ("one wait at 65 536 rows" if one_wait else "by waits"), cols, parse_work(g.small["work_lines"]), one_wait)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--tree")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--out")
    a = ap.parse_args()
    libs = {"tree": mod.RHJ(device=0, lib_path=a.tree) if a.tree else mod.RHJ(device=0), "parent": mod.RHJ(device=0, lib_path=a.parent)}
    assert not hasattr(libs["parent"].lib, "rhj_set_fold_resident"), "--parent names a library that has the switch"
    was = libs["tree"].lib.rhj_get_fold_resident()
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
        ratios = " ".join("%s / parent %.2f" % (s, med[s] / med["parent"]) for s in FORMS[1:]) + " on / off %.2f" % (med["on"] / med["off"])
        extra = " | off: %s" % case.off_info if hasattr(case, "off_info") else ""
        line = "%-52s %s | %s | on: %s%s | %d + %d reps" % (case.name, " | ".join(parts), ratios, case.info, extra, a.warmup, a.reps)
        print(line, flush=True)
        lines.append(line)
        del case
        for rhj in libs.values():
            rhj.lib.rhj_release()
        torch.cuda.empty_cache()
    libs["tree"].set_fold_resident(was)
    for rhj in libs.values():
        rhj.lib.rhj_set_timing(2)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
