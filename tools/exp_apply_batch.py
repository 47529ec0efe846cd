"""Batched rebuilds and view sums against the loop of single calls: tools/exp_apply_batch.py [--reps 30] [--warmup 5] [--out FILE]
[--cases abc]
One process, one library, timing level 0; every repetition times two forms of the same work on the same inputs,
  loop     per item the existing entry points: one rhj_gather_tables_device per side of the index list that a term reads
           (two per join), and for an item that sums one rhj_sum_views_device over the vectors those gathers wrote (one
           per query); these entry points are what they were before rhj_apply_batch_device existed,
  batch    rhj_apply_batch_device: one call per batch of items (an item that sums writes no table),
alternating loop, batch, loop ..., each with a host clock around work that ends in a stream synchronisation.  Cases:
  (a) the apply batches of `small` as tests/test_gpu_apply_batch.py drives it (one batch per join level: rebuilds of the
      queries that go on, view sums through the pairs of those that finish);
  (b) 512 items x 4096 pairs x 3 tables (two old vectors through the R words, the fresh relation through the S words);
  (c) one item of 100 M pairs and one table through the R words against the single rhj_gather_tables_device call.
Outputs are allocated once; rows and sums of the two forms are compared afterwards.  Prints, and with --out appends, one
line per case: medians, min-max spreads, the ratio."""
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

import torch

import helpers
import test_gpu_apply_batch as drive

mod = importlib.import_module("sigmod-2018_amd")
u64p = C.POINTER(C.c_uint64)


def ptr(t):
    return None if t is None else t.data_ptr()


class Recorder(drive.Engine):
    """the driver's engine, keeping every apply batch's items"""

    def __init__(self, rhj):
        super().__init__(rhj)
        self.batches = []

    def apply_batch(self, items):
        self.batches.append(items)
        return super().apply_batch(items)


def small_batches(rhj):
    g = helpers.Golden()
    rels = g.small_relations
    cols = [[drive.dev(rhj, c) for c in rels["r%d" % r]] for r in range(len(rels))]
    rec = Recorder(rhj)
    lines, _ = drive.run_small(rec, cols, drive.parse_work(g.small["work_lines"]))
    assert lines == g.small["result_lines"]
    return rec.batches


class Forms:
    """one batch of items (the Python binding's form) prepared for both forms, outputs allocated once"""

    def __init__(self, rhj, items):
        self.lib, self.items = rhj.lib, items
        n = len(items)
        new = lambda rows: torch.empty(max(rows, 1), dtype=torch.int64, device=rhj.dev)      # noqa: E731
        # batch: descriptors with their own destinations
        self.arr = (mod.ApplyDesc * max(n, 1))()
        self.batch_rows = []
        self.nothing = new(0)                 # (an empty tensor has no address: the list of a join without a match points here)
        for d, (idx, stride, rows, terms) in zip(self.arr, items):
            d.d_idx, d.n, d.idx_stride, d.nterms = ptr(idx) or (ptr(self.nothing) if idx is not None else None), rows, stride, len(terms)
            outs = []
            for t, (side, src, want, col) in zip(d.terms, terms):
                t.side, t.d_src, t.d_col = side, ptr(src), ptr(col)
                outs.append(new(rows) if want else None)
                t.d_dst = ptr(outs[-1])
            self.batch_rows.append(outs)
        # loop: per item the gather calls (one per side read), then the sum call over what they wrote
        self.calls, self.loop_rows, self.loop_sums = [], [], []
        for idx, stride, rows, terms in items:
            assert idx is not None or not any(want for _, _, want, _ in terms)
            # a vector per term that goes through the list: the rebuilt table, or what the sum call reads
            outs, gathers = [new(rows) if idx is not None else None for _ in terms], []
            for s in range(stride):
                ks = [k for k, t in enumerate(terms) if t[0] == s and outs[k] is not None]
                if ks and rows:
                    gathers.append(((C.c_void_p * len(ks))(*[ptr(outs[k]) for k in ks]), (C.c_void_p * len(ks))(*[ptr(terms[k][1]) for k in ks]), len(ks),
                                    C.c_void_p(idx.data_ptr() + 8 * s), stride, rows))
            ks = [k for k, t in enumerate(terms) if t[3] is not None]
            sums = None
            if ks:
                got = (C.c_uint64 * len(ks))()
                sels = [outs[k] if idx is not None else terms[k][1] for k in ks]
                sums = (len(ks), (C.c_void_p * len(ks))(*[ptr(terms[k][3]) for k in ks]), (C.c_void_p * len(ks))(*[ptr(s) for s in sels]),
                        (C.c_uint64 * len(ks))(*[rows] * len(ks)), got)
            self.calls.append((gathers, sums if rows else None))
            self.loop_rows.append(outs)
            self.loop_sums.append((ks, sums))

    def loop(self):
        for gathers, sums in self.calls:
            for g in gathers:
                rc = self.lib.rhj_gather_tables_device(*g)
                assert rc == 0, rc
            if sums:
                rc = self.lib.rhj_sum_views_device(*sums)
                assert rc == 0, rc

    def batch(self):
        rc = self.lib.rhj_apply_batch_device(self.arr, len(self.items))
        assert rc == 0, rc

    def compare(self, name):
        for i, (idx, stride, rows, terms) in enumerate(self.items):
            for k, (side, src, want, col) in enumerate(terms):
                if want:
                    assert torch.equal(self.batch_rows[i][k][:rows], self.loop_rows[i][k][:rows]), "%s: rows of item %d term %d differ" % (name, i, k)
            ks, sums = self.loop_sums[i]
            if rows and sums:
                assert [self.arr[i].terms[k].sum for k in ks] == list(sums[4]), "%s: sums of item %d differ" % (name, i)


def cases(rhj, which):
    torch.manual_seed(12)
    rnd = lambda hi, n: torch.randint(0, hi, (n,), dtype=torch.int64, device=rhj.dev)      # noqa: E731
    if "a" in which:
        batches = small_batches(rhj)
        yield "(a) small: %d apply batches, %d items" % (len(batches), sum(len(b) for b in batches)), batches
    if "b" in which:
        vecs = [rnd(1 << 20, 8192) for _ in range(8)]
        lists = [rnd(8192, 2 * 4096).reshape(4096, 2) for _ in range(16)]
        yield "(b) 512 items x 4096 pairs x 3 tables", [[(lists[i % 16], 2, 4096, [(0, vecs[i % 8], True, None), (0, vecs[(i + 3) % 8], True, None),
                                                                                     (1, None, True, None)]) for i in range(512)]]
    if "c" in which:
        n = 100_000_000
        yield "(c) 1 item x 100 M pairs x 1 table", [[(rnd(n, 2 * n).reshape(n, 2), 2, n, [(0, rnd(1 << 40, n), True, None)])]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--out")
    a = ap.parse_args()
    rhj = mod.RHJ(device=0)
    lib = rhj.lib
    lib.rhj_gather_tables_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_uint64]
    lib.rhj_sum_views_device.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), u64p, u64p]
    lib.rhj_filter_eq2_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, u64p]
    rhj.set_bits(4)
    lines = []
    for name, batches in cases(rhj, a.cases):
        lib.rhj_set_timing(0)
        forms = [Forms(rhj, items) for items in batches]
        t = {"loop": [], "batch": []}
        for rep in range(a.warmup + a.reps):
            for s in ("loop", "batch"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for f in forms:
                    getattr(f, s)()
                torch.cuda.synchronize()              # (the gather calls are asynchronous; the batch has waited already)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    t[s].append(dt)
        for f in forms:
            f.compare(name)
        med = {s: statistics.median(t[s]) for s in t}
        parts = ["%s median %9.3f ms (min %.3f max %.3f, spread %.3f)" % (s, med[s], min(t[s]), max(t[s]), max(t[s]) - min(t[s])) for s in ("loop", "batch")]
        line = "%-46s %s | loop / batch %.2f | %d + %d reps" % (name, " | ".join(parts), med["loop"] / med["batch"], a.warmup, a.reps)
        print(line, flush=True)
        lines.append(line)
        del forms
        torch.cuda.empty_cache()
    lib.rhj_set_timing(2)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
