"""Batched small joins against the loop they replace: tools/exp_batch.py [--reps 30] [--warmup 5] [--out FILE]
RHJ_LIB names a library built from the parent commit (as for tools/ab.py: `git archive` the parent, `make` there, copy its
librhj.so to build/).  One process, both libraries loaded, timing level 0; every repetition times
  batch  one rhj_join_batch_device call of this tree's library over all the joins of a workload,
  loop   one rhj_join_device call of the parent's library per join,
alternating batch, loop, batch, loop ..., each with a host clock around work that ends in the call's own stream
synchronisation.  Workloads: the joins of `small` that go into the batched launches (both relations of at most 65 536 tuples:
85 of the 88) at 4 radix bits, and N x (4096 join 4096) for N = 1, 8, 64, 512.  Output buffers are allocated once, with room
for every join's pairs.  Prints, and with --out appends, one line per workload: medians, min-max spreads, the ratio, and
whether the batch's median is below the loop's by more than the larger spread."""
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


def workloads(new):
    g = helpers.Golden()
    small = []
    for j in g.small["joins"]:
        R, S = g.small_join(j["idx"])
        if new.lib.rhj_batch_takes(4, len(R), len(S)):
            small.append((new.to_device(R), new.to_device(S), j["matches"]))
    yield "small, the %d batched joins at 4 bits" % len(small), small
    rng = np.random.default_rng(7)
    for n in (1, 8, 64, 512):
        rels = []
        for _ in range(min(n, 16)):                  # 16 distinct pairs of relations, shared between the joins beyond that
            R = helpers.make_rel(rng.integers(0, 4096, size=4096, dtype=np.uint64))
            S = helpers.make_rel(rng.integers(0, 4096, size=4096, dtype=np.uint64))
            rels.append((new.to_device(R), new.to_device(S)))
        joins = []
        for i in range(n):
            dR, dS = rels[i % len(rels)]
            joins.append((dR, dS, None))
        yield "%d x (4096 join 4096) at 4 bits" % n, joins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    parent_path = os.environ.get("RHJ_LIB")
    if not parent_path:
        sys.exit("RHJ_LIB must name a librhj.so built from the parent commit")
    new = mod.RHJ(device=0, lib_path=mod.LIB_PATH)
    old = mod.RHJ(device=0, lib_path=parent_path)
    assert hasattr(new.lib, "rhj_join_batch_device") and not hasattr(old.lib, "rhj_join_batch_device"), "which library is which?"
    for r in (new, old):
        r.set_bits(4)
        r.lib.rhj_set_timing(0)
    lines = []
    for name, joins in workloads(new):
        n = len(joins)
        m = C.c_uint64(0)
        counts = []
        for dR, dS, known in joins:                   # sizes of the outputs: counted once, outside the timing
            if known is None:
                assert old.lib.rhj_join_device(dR.data_ptr(), dR.shape[0], dS.data_ptr(), dS.shape[0], None, 0, C.byref(m)) == 0
                known = m.value
            counts.append(known)
        outs = [torch.empty((max(c, 1), 2), dtype=torch.int64, device=new.dev) for c in counts]
        outs_old = [torch.empty_like(o) for o in outs]
        arr = (mod.JoinDesc * n)()
        for d, (dR, dS, _), o, c in zip(arr, joins, outs, counts):
            d.d_R, d.nR, d.d_S, d.nS, d.d_out, d.out_capacity = dR.data_ptr(), dR.shape[0], dS.data_ptr(), dS.shape[0], o.data_ptr(), c
        loop_args = [(dR.data_ptr(), dR.shape[0], dS.data_ptr(), dS.shape[0], o.data_ptr(), c) for (dR, dS, _), o, c in zip(joins, outs_old, counts)]

        def batch():
            rc = new.lib.rhj_join_batch_device(arr, n)
            assert rc == 0, rc

        def loop():
            f = old.lib.rhj_join_device
            for args in loop_args:
                rc = f(*args, C.byref(m))
                assert rc == 0, rc

        t = {"batch": [], "loop": []}
        for rep in range(a.warmup + a.reps):
            for side, fn in (("batch", batch), ("loop", loop)):
                t0 = time.perf_counter()
                fn()                                  # (both end in their own stream synchronisation)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    t[side].append(dt)
        torch.cuda.synchronize()
        for d, c, o, oo in zip(arr, counts, outs, outs_old):
            assert d.matches == c and d.path == 6, (name, d.matches, c, d.path)
            assert torch.equal(o, oo), name + ": the batch's pairs differ from the loop's"
        mb, ml = statistics.median(t["batch"]), statistics.median(t["loop"])
        sb, sl = max(t["batch"]) - min(t["batch"]), max(t["loop"]) - min(t["loop"])
        line = ("%-40s batch median %8.3f ms (min %.3f max %.3f, spread %.3f) | parent loop median %8.3f ms (min %.3f max %.3f, spread %.3f) | "
                "loop / batch %.2f | %d + %d reps | batch below loop by more than the larger spread: %s"
                % (name, mb, min(t["batch"]), max(t["batch"]), sb, ml, min(t["loop"]), max(t["loop"]), sl, ml / mb, a.warmup, a.reps,
                   "yes" if ml - mb > max(sb, sl) else "NO"))
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
