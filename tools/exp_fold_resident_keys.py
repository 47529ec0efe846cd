"""rhj_set_fold_resident_keys: where one workgroup with the table of owners in LDS beats the memset and the three
launches over a table in HBM on TUPLE keys, and where it loses:
  tools/exp_fold_resident_keys.py [--tree TREE.so] [--reps 30] [--sweep-reps 5] [--warmup 5] [--cases abc] [--out FILE]
DESIGN.md 6's procedure: one process, one library, timing level 0; every repetition times the forms of a case one after the other
on the same device inputs, each with a host clock around one library call that ends in a stream synchronisation, on descriptors
built beforehand.  The forms' answers are compared afterwards.  Cases:
  (a) 512 items of n x n rows on distinct tuples of 2 and of 4 key words with one value, n = 256, 1024, 2048, 4096, through
      rhj_join_foldk_batch_device and through rhj_join_foldn_batch_device with two distinct row-id vectors a side; forms `off`, `on`;
  (b) 8 items, one workgroup each, with a build side of 4096 rows on 2 key words and the other side of 2^12 ... 2^16 rows, --sweep-reps
      repetitions; forms `off`, `on`: this is what FOLDK_LDS_MAX_ROWS is set from, the largest power of two at which `on` is no
      slower.  (Sizes beyond the row limit the library was built with run in the table form and show as on / off of 1.00; --tree
      names a build of this tree with FOLDK_LDS_MAX_ROWS raised, to measure beyond it.);
  (c) the 50 queries of `small` and the synthetic batch of tests/query_shapes.py through rhj_query_batch_device with the fold, keys
      and self switches on, by waits and with the one-wait programs at a row limit of 65 536; forms `off`, `old` (rhj_set_fold_resident
      alone) and `both`.
Prints, and with --out appends, one line per case: per form the median and the min-max spread, every form's ratio to `off`, and the
resident infos (and, for the queries, the one-wait info) of the forms."""
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
SWITCHES = {"off": (False, False), "on": (False, True), "old": (True, False), "both": (True, True)}     # (one key, tuple keys)


def dev(rhj, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


class Case:
    """a call on descriptors built once; run(form) makes it under the form's switches and keeps the answers"""
    forms = ("off", "on")

    def __init__(self, rhj, name):
        self.rhj, self.name, self.got, self.info = rhj, name, {}, {}

    def switch(self, form):
        self.rhj.set_fold_resident(SWITCHES[form][0])
        self.rhj.set_fold_resident_keys(SWITCHES[form][1])

    def compare(self):
        for form in self.forms[1:]:
            assert self.got[form] == self.got["off"], "%s: the answers of `%s` differ from those of `off`" % (self.name, form)


class Queries(Case):
    forms = ("off", "old", "both")

    def __init__(self, rhj, name, cols, queries, one_wait):
        super().__init__(rhj, name)
        self.cols, self.queries, self.one_wait = cols, queries, one_wait

    def run(self, form):
        rhj = self.rhj
        self.switch(form)
        for setter in (rhj.set_query_fold, rhj.set_query_fold_keys, rhj.set_query_fold_self):
            setter(True)
        rhj.set_query_fold_one_wait(self.one_wait)
        rhj.set_query_fold_one_wait_rows(65536)
        res, info = rhj.query_batch_device(self.cols, self.queries, with_info=True)
        self.got[form] = [(list(s), r) for s, r in res]
        ow, one, keys = info.one_wait_info, rhj.table_batch_last_resident_info(), rhj.table_batch_last_resident_keys_info()
        self.info[form] = "launches %d memsets %d rounds %d, one key %d resident %d table, tuples %d resident %d table" % (
            ow["launches"], ow["memsets"], ow["rounds"], one["resident_items"], one["table_items"], keys["resident_items"], keys["table_items"])


class Folds(Case):
    """items = [(key columns of R, vectors of R, key columns of S, vectors of S)] as device tensors, a vector per word or None;
    every item has one value, a weight over S's positions, and one output that writes its vector.  nodes: the items go through
    rhj_join_foldn_batch_device with their vectors, else through rhj_join_foldk_batch_device, which has none here."""

    def __init__(self, rhj, name, items, weight, nodes):
        super().__init__(rhj, name)
        self.keep = (items, weight, [])
        self.entry = rhj.lib.rhj_join_foldn_batch_device if nodes else rhj.lib.rhj_join_foldk_batch_device
        self.arr = ((mod.JoinFoldNDesc if nodes else mod.JoinFoldKDesc) * len(items))()
        for d, (cR, vR, cS, vS) in zip(self.arr, items):
            d.nkeys = len(cR)
            for t in range(len(cR)):
                d.d_colR[t], d.d_colS[t] = cR[t].data_ptr(), cS[t].data_ptr()
                if nodes:
                    d.d_selR[t], d.d_selS[t] = vR[t].data_ptr(), vS[t].data_ptr()
            d.nR, d.nS = (vR[0] if nodes else cR[0]).shape[0], (vS[0] if nodes else cS[0]).shape[0]
            d.nvalues, d.nouts = 1, 1
            d.values[0].d_w = weight.data_ptr()
            out = torch.empty((d.nR,), dtype=torch.int64, device=rhj.dev)
            self.keep[2].append(out)
            d.outs[0].value, d.outs[0].d_out = 0, out.data_ptr()

    def run(self, form):
        self.switch(form)
        rc = self.entry(self.arr, len(self.arr))
        assert rc == 0, rc
        self.got[form] = [d.outs[0].total for d in self.arr]
        self.info[form] = str(self.rhj.table_batch_last_resident_keys_info())


def words_of(base, nk):
    """nk key words that are equal exactly where `base` is"""
    radix = {1: 1 << 62, 2: 64, 3: 32, 4: 16}[nk]
    return [(base // np.uint64(radix ** t)) % np.uint64(radix) for t in range(nk - 1)] + [base // np.uint64(radix ** (nk - 1))]


def side(rhj, rng, base, nk, nodes):
    """(key columns, vectors) of one side whose row i carries words_of(base[i]); with nodes, word t is read through one of two
    distinct permutations, and its column is laid out so that the permutation finds the word"""
    words = words_of(base.astype(np.uint64), nk)
    if not nodes:
        return [dev(rhj, w) for w in words], None
    perms = [rng.permutation(len(base)) for _ in range(2)]
    cols = []
    for t, w in enumerate(words):
        c = np.empty_like(w)
        c[perms[t % 2]] = w
        cols.append(dev(rhj, c))
    vecs = [dev(rhj, p.astype(np.uint64)) for p in perms]
    return cols, [vecs[t % 2] for t in range(nk)]


def cases(rhj, which):
    rng = np.random.default_rng(2323)
    wide = lambda n: rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    if "a" in which:
        for nodes in (False, True):
            for nk in (2, 4):
                for rows in (256, 1024, 2048, 4096):
                    n, pool = 512, 16                    # the sides are shared among the items, 16 different ones
                    sides = []
                    for p in range(pool):
                        base = rng.permutation(rows) + 1
                        sides.append(side(rhj, rng, base, nk, nodes) + side(rhj, rng, base[rng.permutation(rows)], nk, nodes))
                    yield Folds(rhj, "(a) %s 512 x (%d x %d) distinct tuples, %d keys, 1 value" % ("foldn" if nodes else "foldk", rows, rows, nk),
                                [sides[k % pool] for k in range(n)], dev(rhj, wide(rows)), nodes)
    if "b" in which:
        build, n, nk = 4096, 8, 2
        for log2 in (12, 13, 14, 15, 16):
            other = 1 << log2
            items = []
            for k in range(n):                           # item k: R builds with 4096 distinct tuples of its own, S's tuples are drawn from them
                items.append(side(rhj, rng, rng.permutation(build) + 1, nk, False) + side(rhj, rng, rng.integers(1, build + 1, size=other), nk, False))
            yield Folds(rhj, "(b) 8 x (4096 x 2^%d), 2 keys, 1 value" % log2, items, dev(rhj, wide(other)), False)
    if "c" in which:
        import helpers
        import query_shapes
        from query_model import parse_work
        g = helpers.Golden()
        rels = g.small_relations
        small = [[dev(rhj, np.asarray(c, dtype=np.uint64)) for c in rels["r%d" % r]] for r in range(len(rels))], parse_work(g.small["work_lines"])
        srels, squeries = query_shapes.reference("synthetic")[:2]
        synthetic = [[dev(rhj, c) for c in rel] for rel in srels], squeries
        for name, (cols, queries) in (("small: 50 queries", small), ("synthetic: %d queries" % len(squeries), synthetic)):
            for one_wait in (False, True):
                yield Queries(rhj, "(c) %s, fold + keys + self, %s" % (name, "one wait at 65 536 rows" if one_wait else "by waits"), cols, queries, one_wait)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sweep-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--out")
    a = ap.parse_args()
    rhj = mod.RHJ(device=0, lib_path=a.tree) if a.tree else mod.RHJ(device=0)
    was = rhj.lib.rhj_get_fold_resident(), rhj.lib.rhj_get_fold_resident_keys()
    rhj.set_bits(4)
    rhj.lib.rhj_set_timing(0)
    lines = []
    for case in cases(rhj, a.cases):
        reps = a.sweep_reps if case.name.startswith("(b)") else a.reps
        t = {s: [] for s in case.forms}
        for rep in range(a.warmup + reps):
            for s in case.forms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                case.run(s)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    t[s].append(dt)
        case.compare()
        med = {s: statistics.median(t[s]) for s in t}
        parts = ["%s median %9.3f ms (min %.3f max %.3f)" % (s, med[s], min(t[s]), max(t[s])) for s in case.forms]
        ratios = " ".join("%s / off %.2f" % (s, med[s] / med["off"]) for s in case.forms[1:])
        line = "%-66s %s | %s | %s | %d + %d reps" % (case.name, " | ".join(parts), ratios, " | ".join("%s: %s" % (s, case.info[s]) for s in case.forms), a.warmup, reps)
        print(line, flush=True)
        lines.append(line)
        del case
        rhj.lib.rhj_release()
        torch.cuda.empty_cache()
    rhj.set_fold_resident(was[0])
    rhj.set_fold_resident_keys(was[1])
    rhj.lib.rhj_set_timing(2)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
