"""The statistics of many columns through rhj_column_stats_batch_device against the loop of rhj_column_stats_device calls:
tools/exp_stats_batch.py [--reps 30] [--warmup 5] [--out FILE] [--cases abc]
One process, one library, timing level 0; every repetition times two forms of the same work on the same device columns,
alternating single, batch, single ..., each with a host clock around work that ends in a stream synchronisation.  The
baseline is the loop of single calls (k_col_minmax, k_col_flags, k_count_flags: the code InitRelationMap ran per column before
the batch existed), never the batch itself.  Cases:
  (a) every column of the 14 relations of `small` (tests/golden/small_relations.npz.xz): ONE batched call against one single
      call per column;
  (b) 64 columns of 4 194 304 rows with 1000 distinct values (every workgroup marks the same few bitmap words), and 64 with
      random 64-bit values (folded ranges);
  (c) one column of 67 108 864 rows, narrow (1000 distinct values) and folded (random 64-bit values): the batch's kernels
      against the single call's on its own ground.
The two forms' answers are compared afterwards.  Prints, and with --out appends, one line per case: medians, min-max spreads,
the ratio."""
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

import numpy as np
import torch

import helpers

mod = importlib.import_module("sigmod-2018_amd")
u64p = C.POINTER(C.c_uint64)


class Columns:
    """a list of device columns in both forms"""

    def __init__(self, rhj, cols):
        self.lib, self.cols = rhj.lib, cols
        self.arr = (mod.ColStatsDesc * len(cols))()
        for d, t in zip(self.arr, cols):
            d.d_col, d.n = t.data_ptr(), t.shape[0]
        self.ref = [None] * len(cols)

    def batch(self):
        rc = self.lib.rhj_column_stats_batch_device(self.arr, len(self.cols))
        assert rc == 0, rc

    def single(self):
        l, u, d = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
        for k, t in enumerate(self.cols):
            rc = self.lib.rhj_column_stats_device(t.data_ptr(), t.shape[0], C.byref(l), C.byref(u), C.byref(d))
            assert rc == 0, rc
            self.ref[k] = (l.value, u.value, d.value)

    def compare(self, name):
        for k, d in enumerate(self.arr):
            assert (d.l, d.u, d.d) == self.ref[k], "%s: column %d differs: batch %r, single %r" % (name, k, (d.l, d.u, d.d), self.ref[k])


def small(rhj):
    rels = helpers.Golden().small_relations
    return Columns(rhj, [torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint64).view(np.int64)).to(rhj.dev)
                         for r in range(len(rels)) for c in rels["r%d" % r]])


def narrow(rhj, count, rows):
    return Columns(rhj, [torch.randint(10_000, 11_000, (rows,), dtype=torch.int64, device=rhj.dev) for _ in range(count)])


def wide(rhj, count, rows):
    return Columns(rhj, [torch.randint(-(1 << 63), (1 << 63) - 1, (rows,), dtype=torch.int64, device=rhj.dev) for _ in range(count)])


def cases(rhj, which):
    torch.manual_seed(13)
    if "a" in which:
        yield "(a) small: every column", lambda: small(rhj)
    if "b" in which:
        yield "(b) 64 columns x 4 194 304 rows, 1000 values", lambda: narrow(rhj, 64, 1 << 22)
        yield "(b) 64 columns x 4 194 304 rows, random", lambda: wide(rhj, 64, 1 << 22)
    if "c" in which:
        yield "(c) 1 column x 67 108 864 rows, 1000 values", lambda: narrow(rhj, 1, 1 << 26)
        yield "(c) 1 column x 67 108 864 rows, random", lambda: wide(rhj, 1, 1 << 26)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--out")
    a = ap.parse_args()
    rhj = mod.RHJ(device=0)
    lib = rhj.lib
    lib.rhj_column_stats_device.argtypes = [C.c_void_p, C.c_uint64, u64p, u64p, C.POINTER(C.c_double)]
    lines = []
    for name, make in cases(rhj, a.cases):
        lib.rhj_set_timing(0)
        form = make()
        t = {"single": [], "batch": []}
        for rep in range(a.warmup + a.reps):
            for s in ("single", "batch"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                getattr(form, s)()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    t[s].append(dt)
        form.compare(name)
        med = {s: statistics.median(t[s]) for s in t}
        parts = ["%s median %9.3f ms (min %.3f max %.3f, spread %.3f)" % (s, med[s], min(t[s]), max(t[s]), max(t[s]) - min(t[s])) for s in ("single", "batch")]
        line = "%-48s %d columns | %s | single / batch %.2f | %d + %d reps" % (name, len(form.cols), " | ".join(parts), med["single"] / med["batch"], a.warmup, a.reps)
        print(line, flush=True)
        lines.append(line)
        del form
        torch.cuda.empty_cache()
    lib.rhj_set_timing(2)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
