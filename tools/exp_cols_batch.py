"""Batched joins that read columns through row-id vectors against materialising first: tools/exp_cols_batch.py [--reps 30]
[--warmup 5] [--out FILE]
One process, one library, timing level 0; every repetition times three sides over all the joins of a workload,
  build+batch  per join two rhj_build_relation_device calls, then one rhj_join_batch_device call on the relations they wrote
               (what a caller had to do before rhj_join_cols_batch_device),
  cols         one rhj_join_cols_batch_device call on the columns and vectors themselves,
  prebuilt     one rhj_join_batch_device call on relations built beforehand, outside the timing (the floor: what reading
               through the vectors costs),
alternating build+batch, cols, prebuilt, build+batch ..., each with a host clock around work that ends in the call's own stream
synchronisation.  Workloads: the joins of `small` that go into the batched launches (85 of the 88) at 4 radix bits, the columns
being the fixtures' values, once whole (no vectors) and once through a random ascending half of the rows; and
N x (4096 join 4096), each side 4096 ascending rows of an 8192-row column, for N = 1, 8, 64, 512.  Output buffers are
allocated once, with room for every join's pairs, and the three sides' pairs are compared afterwards.  Prints, and with --out
appends, one line per workload: medians, min-max spreads, the ratios, and whether cols' median is below build+batch's by more
than the larger of the two spreads."""
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

SIDES = ("build+batch", "cols", "prebuilt")


def dev(rhj, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


def half(rng, rows):
    """a random ascending half of a column's rows: a filter's output"""
    return np.sort(rng.choice(rows, size=max(rows // 2, 1), replace=False)).astype(np.uint64)


def workloads(rhj):
    """(name, [(colR, selR, colS, selS)]) with device tensors; a vector may be None"""
    g = helpers.Golden()
    rng = np.random.default_rng(11)
    whole, halves = [], []
    for j in g.small["joins"]:
        R, S = g.small_join(j["idx"])
        if not rhj.lib.rhj_batch_takes(4, len(R), len(S)):
            continue
        cR, cS = dev(rhj, R["value"]), dev(rhj, S["value"])
        whole.append((cR, None, cS, None))
        halves.append((cR, dev(rhj, half(rng, len(R))), cS, dev(rhj, half(rng, len(S)))))
    yield "small, %d batched joins at 4 bits, whole columns" % len(whole), whole
    yield "small, %d batched joins, ascending halves" % len(halves), halves
    for n in (1, 8, 64, 512):
        srcs = []
        for _ in range(min(n, 16)):                  # 16 distinct joins, shared between the joins beyond that
            srcs.append(tuple(x for _ in range(2) for x in (dev(rhj, rng.integers(0, 4096, size=8192, dtype=np.uint64)), dev(rhj, half(rng, 8192)))))
        yield "%d x (4096 join 4096 through vectors)" % n, [srcs[i % len(srcs)] for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    rhj = mod.RHJ(device=0)
    lib = rhj.lib
    rhj.set_bits(4)
    lib.rhj_set_timing(0)
    lines = []
    for name, joins in workloads(rhj):
        n = len(joins)
        sizes = [(rhj._cols_side(cR, sR), rhj._cols_side(cS, sS)) for cR, sR, cS, sS in joins]
        rels = {s: [tuple(torch.empty((side[2], 2), dtype=torch.int64, device=rhj.dev) for side in q) for q in sizes] for s in ("build+batch", "prebuilt")}
        build_args = {s: [(side[0], side[1], side[2], t.data_ptr()) for q, ts in zip(sizes, rels[s]) for side, t in zip(q, ts)] for s in rels}

        def build(side):
            for args in build_args[side]:
                rc = lib.rhj_build_relation_device(*args)
                assert rc == 0, rc

        build("prebuilt")
        # sizes of the outputs: counted once, outside the timing
        cnt = (mod.JoinDesc * n)()
        for d, (tR, tS) in zip(cnt, rels["prebuilt"]):
            d.d_R, d.nR, d.d_S, d.nS = tR.data_ptr(), tR.shape[0], tS.data_ptr(), tS.shape[0]
        assert lib.rhj_join_batch_device(cnt, n) == 0
        counts = [d.matches for d in cnt]
        outs = {s: [torch.empty((max(c, 1), 2), dtype=torch.int64, device=rhj.dev) for c in counts] for s in SIDES}
        tup = {}
        for s in ("build+batch", "prebuilt"):
            tup[s] = (mod.JoinDesc * n)()
            for d, (tR, tS), o, c in zip(tup[s], rels[s], outs[s], counts):
                d.d_R, d.nR, d.d_S, d.nS, d.d_out, d.out_capacity = tR.data_ptr(), tR.shape[0], tS.data_ptr(), tS.shape[0], o.data_ptr(), c
        cols = (mod.JoinColsDesc * n)()
        for d, (qR, qS), o, c in zip(cols, sizes, outs["cols"], counts):
            d.d_colR, d.d_selR, d.nR = qR
            d.d_colS, d.d_selS, d.nS = qS
            d.d_out, d.out_capacity = o.data_ptr(), c

        def side_a():
            build("build+batch")
            rc = lib.rhj_join_batch_device(tup["build+batch"], n)
            assert rc == 0, rc

        def side_b():
            rc = lib.rhj_join_cols_batch_device(cols, n)
            assert rc == 0, rc

        def side_c():
            rc = lib.rhj_join_batch_device(tup["prebuilt"], n)
            assert rc == 0, rc

        t = {s: [] for s in SIDES}
        for rep in range(a.warmup + a.reps):
            for s, fn in zip(SIDES, (side_a, side_b, side_c)):
                t0 = time.perf_counter()
                fn()                                  # (all three end in their own stream synchronisation)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    t[s].append(dt)
        torch.cuda.synchronize()
        for k in range(n):
            for arr in (tup["build+batch"], cols, tup["prebuilt"]):
                assert arr[k].matches == counts[k] and arr[k].path == 6, (name, k, arr[k].matches, counts[k], arr[k].path)
            got = [outs[s][k][:counts[k]] for s in SIDES]       # (a join without matches has one row of room that nobody writes)
            assert torch.equal(got[1], got[0]) and torch.equal(got[1], got[2]), name + ": the sides' pairs differ in join %d" % k
        med = {s: statistics.median(t[s]) for s in SIDES}
        spread = {s: max(t[s]) - min(t[s]) for s in SIDES}
        parts = ["%s median %8.3f ms (min %.3f max %.3f, spread %.3f)" % (s, med[s], min(t[s]), max(t[s]), spread[s]) for s in SIDES]
        line = ("%-52s %s | build+batch / cols %.2f | cols / prebuilt %.2f | %d + %d reps | cols below build+batch by more than the larger "
                "spread: %s" % (name, " | ".join(parts), med["build+batch"] / med["cols"], med["cols"] / med["prebuilt"], a.warmup, a.reps,
                                "yes" if med["build+batch"] - med["cols"] > max(spread["build+batch"], spread["cols"]) else "NO"))
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
