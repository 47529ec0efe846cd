"""Two builds of the library on the four plan functions of the fold route, byte for byte, without a device:
tools/cmp_fold_plans.py LIB_A LIB_B [--count 40000] [--seed 20189] [--out FILE]
Calls rhj_query_fold_plan, rhj_query_foldk_plan, rhj_query_folds_plan and rhj_query_foldn_plan of both libraries on --count
queries of tests/test_fold_plans_agree.py's generator, on every query of tests/query_shapes.py and on the `small` workload, every
output structure filled with 0xA5 beforehand, and compares the return values and the raw bytes of the structures (so also what a
refusal leaves alone).  Prints, and with --out appends, the counts; exits 1 on a difference."""
import argparse
import ctypes as C
import importlib
import os
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
sys.path.insert(0, "oracle")

import helpers
import query_shapes
from query_model import parse_work
from test_fold_plans_agree import random_queries

mod = importlib.import_module("sigmod-2018_amd")


def answers(lib, query, nrel):
    """[(return value, bytes of every output)] of the four functions"""
    arr, keep = mod.query_descs([query])
    q = C.byref(arr[0])
    out = []
    for fn, step in ((lib.rhj_query_fold_plan, mod.FoldStep), (lib.rhj_query_foldk_plan, mod.FoldKStep)):
        root, steps = C.c_int(), (step * (mod.QUERY_MAX_RELS - 1))()
        C.memset(C.byref(root), 0xA5, C.sizeof(root))
        C.memset(steps, 0xA5, C.sizeof(steps))
        out.append((fn(q, nrel, None, C.byref(root), steps), bytes(root) + bytes(steps)))
    for fn, plan in ((lib.rhj_query_folds_plan, mod.FoldsPlan()), (lib.rhj_query_foldn_plan, mod.FoldNPlan())):
        C.memset(C.byref(plan), 0xA5, C.sizeof(plan))
        out.append((fn(q, nrel, None, C.byref(plan)), bytes(plan)))
    del keep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=2)
    ap.add_argument("--count", type=int, default=40000)
    ap.add_argument("--seed", type=int, default=20189)
    ap.add_argument("--out")
    a = ap.parse_args()
    libs = [mod.load_library(os.path.abspath(p)) for p in a.libs]
    g = helpers.Golden()
    sets = [("random, seed %d" % a.seed, [(q, 3) for q in random_queries(a.count, a.seed)]),
            ("tests/query_shapes.py", [(q, max(q[0]) + 1) for name in sorted(query_shapes.FAMILIES) for q in query_shapes.FAMILIES[name]()[1]]),
            ("small", [(q, len(g.small_relations)) for q in parse_work(g.small["work_lines"])])]
    lines, differ = [], 0
    for name, queries in sets:
        bad, accepted = 0, [0, 0, 0, 0]
        for query, nrel in queries:
            one, two = (answers(lib, query, nrel) for lib in libs)
            bad += one != two
            for k in range(4):
                accepted[k] += one[k][0] > 0
        differ += bad
        lines.append("%-24s %6d queries, %d differ in a return value or a byte | accepted by %s: fold %d, foldk %d, folds %d, foldn %d"
                     % ((name, len(queries), bad, a.libs[0]) + tuple(accepted)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
