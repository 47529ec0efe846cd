# The sub-bucket path (csrc/rhj_subbucket.hip.h) against the tiled path it replaces (rhj_set_lowradix(0)), alternately, in one
# process, on the same device relations (uniform foreign keys, bench.make_relations):
#   python3 tools/exp_subbucket.py [--reps N] [--only 12]
# Prints per case and path: wall time per join, the library's stage times, G probe tuples/s (the bigger relation / time), and
# the speed-up; a check that both paths returned the same pairs.
import argparse, ctypes as C, importlib, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench

CASES = [(20_000_000, 24_000_000, 9), (40_000_000, 40_000_000, 10), (200_000_000, 200_000_000, 12)]
KEYS = ("ms_hist", "ms_scan", "ms_scatter", "ms_build", "ms_plan", "ms_probe", "ms_offsets", "ms_total")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", type=int, default=0, help="run only the case on this many radix bits")
args = ap.parse_args()
mod = importlib.import_module("sigmod-2018_amd")
rhj = mod.RHJ(device=0)
for nR, nS, bits in CASES:
    if args.only and bits != args.only:
        continue
    w = dict(nR=nR, nS=nS, bits=bits, dist="uniform")
    rhj.set_bits(bits)
    R, S = bench.make_relations(w, rhj.dev, 1234)
    cap = max(nR, nS) + 1024
    outs = {p: torch.empty((cap, 2), dtype=torch.int64, device=rhj.dev) for p in ("new", "tiled")}
    m = C.c_uint64(0)
    times = {"new": [], "tiled": []}
    stats = {}

    def once(p):
        rhj.lib.rhj_set_lowradix(1 if p == "new" else 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = rhj.lib.rhj_join_device(R.data_ptr(), nR, S.data_ptr(), nS, outs[p].data_ptr(), cap, C.byref(m))
        torch.cuda.synchronize()
        assert rc == 0, rc
        times[p].append((time.perf_counter() - t0) * 1e3)
        stats[p] = rhj.stats()

    for p in ("new", "tiled"):                          # warm-up: workspace buffers grown
        once(p)
    times = {"new": [], "tiled": []}
    for _ in range(args.reps):
        for p in ("new", "tiled"):
            once(p)
    rhj.lib.rhj_set_lowradix(1)
    same = torch.equal(outs["new"][:m.value], outs["tiled"][:m.value])
    print("%dM x %dM at %d bits (k = %d), %d pairs, same pairs: %s" % (nR // 10**6, nS // 10**6, bits, rhj.lib.rhj_sub_bits(bits, nR, nS), m.value, same))
    for p in ("new", "tiled"):
        t = sorted(times[p])[len(times[p]) // 2]
        st = stats[p]
        print("  %-5s %-9s median %8.3f ms (min %8.3f)  %6.2f G probe tuples/s   stages %s" % (p, st["path"], t, min(times[p]), max(nR, nS) / t / 1e6,
              " ".join("%s %.3f" % (k[3:], st[k]) for k in KEYS)), flush=True)
    print("  speed-up (median wall time, tiled / new): %.2fx" % (sorted(times["tiled"])[args.reps // 2] / sorted(times["new"])[args.reps // 2]), flush=True)
    del R, S, outs
    torch.cuda.empty_cache()
