"""Batched filters against the calls they replace: tools/exp_filter_batch.py [--reps 30] [--warmup 5] [--out FILE]
RHJ_LIB names a library built from the parent commit (as for tools/ab.py: `git archive` the parent, `make` there, copy its
librhj.so to build/).  One process, both libraries loaded, timing level 0; every repetition times
  batch  one rhj_filter_batch_device call of this tree's library over all the filters of a workload,
  loop   the parent's library: one rhj_filter_device call per filter, or for the two-term workload the chained form per
         filter (the reference's way, filter.c:73-77: Filter(), a second Filter() through the row ids of the first, and a
         gather of those row ids through the second's),
alternating batch, loop, batch, loop ..., each with a host clock around work that ends in a stream synchronisation.
Workloads: the 50 filters of `small`; 512 filters of 4096 rows; 64 two-term filters of 4 194 304 rows (two columns of one
relation, 25 % and 50 % selective).  Output buffers are allocated once.  Prints, and with --out appends, one line per workload:
medians, min-max spreads, the ratio, and whether the batch's median is below the loop's by more than the larger spread.

--once: ONE batched call of the 50 filters of `small` and nothing else on the device — the run to put under
`rocprofv3 --kernel-trace --stats` for the launch count (needs no RHJ_LIB)."""
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
M64 = (1 << 64) - 1
ROWS_2TERM = 4_194_304


def dev(r, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(r.dev)


def small50(new):
    """[(terms, rows, hits)] of the 50 filters of `small`, columns on the device"""
    g = helpers.Golden()
    rels = {k: dev(new, v.astype(np.uint64)) for k, v in g.small_relations.items()}
    return [([(rels["r%d" % f["rel"]][f["col"]], f["op"], f["value"])], f["rows"], f["hits"]) for f in g.small["filters"]]


def workloads(new):
    yield "small, its 50 filters", small50(new)
    rng = np.random.default_rng(7)
    table = dev(new, rng.integers(0, 1000, 16 * 4096, dtype=np.uint64)).view(16, 4096)       # 16 distinct columns, shared beyond that
    yield "512 x 4096 rows, one term", [([(table[i % 16], "<", 10 + i % 500)], 4096, None) for i in range(512)]
    a, b = dev(new, rng.integers(0, 1000, ROWS_2TERM, dtype=np.uint64)), dev(new, rng.integers(0, 1000, ROWS_2TERM, dtype=np.uint64))
    yield "64 x 4 194 304 rows, two terms", [([(a, "<", 250 + i), (b, ">", 500 - i)], ROWS_2TERM, None) for i in range(64)]


def fill(arr, filters, out):
    at = 0
    for d, (terms, rows, _) in zip(arr, filters):
        d.n, d.nterms = rows, len(terms)
        for t, (col, op, value) in zip(d.terms, terms):
            t.d_col, t.op, t.value = col.data_ptr(), op.encode(), int(value) & M64
        d.d_out = out.data_ptr() + 8 * at
        at += rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    new = mod.RHJ(device=0, lib_path=mod.LIB_PATH)
    new.lib.rhj_set_timing(0)
    if a.once:
        filters = small50(new)
        out = torch.empty(sum(rows for _, rows, _ in filters), dtype=torch.int64, device=new.dev)
        arr = (mod.FilterDesc * len(filters))()
        fill(arr, filters, out)
        torch.cuda.synchronize()
        assert new.lib.rhj_filter_batch_device(arr, len(filters)) == 0
        assert [d.hits for d in arr] == [h for _, _, h in filters] and {d.path for d in arr} == {7}
        print("one batched call of %d filters: %d hits" % (len(filters), sum(d.hits for d in arr)))
        return
    parent_path = os.environ.get("RHJ_LIB")
    if not parent_path:
        sys.exit("RHJ_LIB must name a librhj.so built from the parent commit")
    old = mod.RHJ(device=0, lib_path=parent_path)
    assert hasattr(new.lib, "rhj_filter_batch_device") and not hasattr(old.lib, "rhj_filter_batch_device"), "which library is which?"
    old.lib.rhj_set_timing(0)
    old.lib.rhj_gather_tables_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_uint64]
    lines = []
    for name, filters in workloads(new):
        n = len(filters)
        total = sum(rows for _, rows, _ in filters)
        out, out_old = (torch.empty(total, dtype=torch.int64, device=new.dev) for _ in range(2))
        arr = (mod.FilterDesc * n)()
        fill(arr, filters, out)
        h = C.c_uint64(0)
        old_hits = [0] * n
        two = len(filters[0][0]) == 2
        if two:                                       # the chain's intermediates: the first filter's row ids, the second's positions in them
            ids1, pos2 = (torch.empty(ROWS_2TERM, dtype=torch.int64, device=new.dev) for _ in range(2))
            dst, src = (C.c_void_p * 1)(), (C.c_void_p * 1)(ids1.data_ptr())

        def batch():
            rc = new.lib.rhj_filter_batch_device(arr, n)
            assert rc == 0, rc

        def loop():
            f, at = old.lib.rhj_filter_device, 0
            for k, (terms, rows, _) in enumerate(filters):
                (c0, op0, v0) = terms[0]
                if not two:
                    rc = f(c0.data_ptr(), None, rows, op0.encode(), int(v0) & M64, out_old.data_ptr() + 8 * at, C.byref(h))
                else:
                    (c1, op1, v1) = terms[1]
                    rc = f(c0.data_ptr(), None, rows, op0.encode(), int(v0) & M64, ids1.data_ptr(), C.byref(h))
                    assert rc == 0, rc
                    rc = f(c1.data_ptr(), ids1.data_ptr(), h.value, op1.encode(), int(v1) & M64, pos2.data_ptr(), C.byref(h))
                    assert rc == 0, rc
                    dst[0] = out_old.data_ptr() + 8 * at
                    rc = old.lib.rhj_gather_tables_device(dst, src, 1, pos2.data_ptr(), 1, h.value)
                    torch.cuda.synchronize()          # (the gather is only enqueued; the filters end in their own synchronisation)
                assert rc == 0, rc
                old_hits[k] = h.value
                at += rows

        t = {"batch": [], "loop": []}
        for rep in range(a.warmup + a.reps):
            for side, fn in (("batch", batch), ("loop", loop)):
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    t[side].append(dt)
        torch.cuda.synchronize()
        at = 0
        for d, (_, rows, known), oh in zip(arr, filters, old_hits):
            assert d.hits == oh and (known is None or known == oh) and d.path == 7, (name, d.hits, oh, d.path)
            assert torch.equal(out[at:at + oh], out_old[at:at + oh]), name + ": the batch's indices differ from the loop's"
            at += rows
        mb, ml = statistics.median(t["batch"]), statistics.median(t["loop"])
        sb, sl = max(t["batch"]) - min(t["batch"]), max(t["loop"]) - min(t["loop"])
        line = ("%-34s %9d hits | batch median %8.3f ms (min %.3f max %.3f, spread %.3f) | parent loop median %8.3f ms (min %.3f max %.3f, spread %.3f) | "
                "loop / batch %.2f | %d + %d reps | batch below loop by more than the larger spread: %s"
                % (name, sum(old_hits), mb, min(t["batch"]), max(t["batch"]), sb, ml, min(t["loop"]), max(t["loop"]), sl, ml / mb, a.warmup, a.reps,
                   "yes" if ml - mb > max(sb, sl) else "NO"))
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
