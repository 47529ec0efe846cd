"""The items on which the resident form of rhj_join_fold_batch_device is tested (csrc/rhj_fold_lds.hip.h), built with numpy alone:
tests/test_fold_resident_model.py holds every shape to the regime it is named for, tests/test_gpu_fold_resident.py runs them.
An item is test_gpu_join_fold_batch.py's: key columns and row-id vectors (or None) of R and S, values [(w, src, col)], outs
[(value, (w, src, col), whether it has a d_out)], and here the regime its sizes must fall in with the switch on."""
import numpy as np

import fold_resident_model as rm
import join_fold_model as fm
import join_sum_model as jm

M64 = (1 << 64) - 1
ONES = (None, None, None)
RESIDENT, TABLE, EMPTY_SIDE = "resident", "table", "empty side"
ONE_ROW_ITEMS = jm.MAX_ITEMS + 1


def u64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64))


def side_keys(col, sel):
    return col if sel is None else col[sel.astype(np.int64)]


def sizes(it):
    return len(side_keys(*it["R"])), len(side_keys(*it["S"])), len(it["values"])


def model(it):
    """[(vector, total)] per output"""
    return fm.fold_item_np(side_keys(*it["R"]), side_keys(*it["S"]), it["values"], [(c, p) for c, p, _ in it["outs"]])


def regime_of(it):
    nR, nS, nvalues = sizes(it)
    return EMPTY_SIDE if not (nR and nS) else RESIDENT if rm.resident(nR, nS, nvalues) else TABLE


def build_items():
    """the shapes, resident and table items alternating in call order as far as they go, then the one-row items"""
    rng = np.random.default_rng(2024)
    rows = max(rm.MAX_ROWS + 1, 6000)
    items = []
    wide = u64(rng.integers(0, 1 << 63, size=rows)) * np.uint64(2) + np.uint64(1)            # values up to 2^64 - 1
    high = u64(np.where(np.arange(rows) % 3 == 0, M64, 1 << 63))                              # 2^64 - 1 and 2^63 only: products and sums wrap
    ident = u64(rng.permutation(rows))                                                        # a vector into columns of `rows` rows
    holes = u64(rng.integers(0, 3, size=rows)) * wide                                         # a weight that is 0 in a third of the rows
    columns = [wide, high, holes]

    def fac(t, n):
        kind = t % 4                                     # ones, a weight, a column, a weight times a column through a vector
        return (columns[t % 3][:n] if kind in (1, 3) else None, ident[:n] if kind == 3 else None, columns[(t + 1) % 3] if kind >= 2 else None)

    def add(name, regime, kR, kS, nvalues=1, outs=None, selR=None, selS=None):
        kR, kS = u64(kR), u64(kS)
        nR, nS = len(side_keys(kR, selR)), len(side_keys(kS, selS))
        values = [fac(3 + t, nS) for t in range(nvalues)]                                     # (the first: a weight times a column through a vector)
        if outs is None:                                 # every value read, the first by an output of ones and by one with a weight: two outputs on one value
            outs = [(0, ONES, True)] + [(c, fac(c + 1, nR), c % 3 != 2) for c in range(nvalues)][:fm.MAX_OUTS - 1] if nvalues else []
        items.append({"name": name, "regime": regime, "R": (kR, selR), "S": (kS, selS), "values": values, "outs": list(outs)})

    def keys(n, span=3000):
        return rng.integers(1, span, size=n)

    add("1x1 matching", RESIDENT, [7], [7])
    add("1x1 not matching", RESIDENT, [7], [8])
    add("0x5", EMPTY_SIDE, [], [3, 9, 3])
    add("5x0", EMPTY_SIDE, [3, 9, 3, 7, 9], [])
    # the rows and tiles of the workgroup's loops, on either side and on both
    for n in (255, 256, 257, 2047, 2048, 2049, 4096):
        add("%d rows of R, S builds" % n, RESIDENT, keys(n), keys(100))
        add("%d rows of S, R builds" % n, RESIDENT, keys(100), keys(n))
        add("%d rows of both" % n, RESIDENT, keys(n), keys(n))
    # the build side at the LDS cap and one row beyond it
    for v in (1, 3, 9):
        cap = rm.build_cap(v)
        add("R builds at the cap, %d values" % v, RESIDENT, keys(cap), keys(cap + 50), v)
        add("S builds at the cap, %d values" % v, RESIDENT, keys(cap + 50), keys(cap), v)
        add("R builds beyond the cap, %d values" % v, TABLE, keys(cap + 1), keys(cap + 51), v)
        add("S builds beyond the cap, %d values" % v, TABLE, keys(cap + 51), keys(cap + 1), v)
    # the other side at its limit and one row beyond it
    add("S at the row limit", RESIDENT, keys(100, 150), keys(rm.MAX_ROWS, 150))
    add("R at the row limit", RESIDENT, keys(rm.MAX_ROWS, 150), keys(100, 150))
    add("S beyond the row limit", TABLE, keys(100, 150), keys(rm.MAX_ROWS + 1, 150))
    add("R beyond the row limit", TABLE, keys(rm.MAX_ROWS + 1, 150), keys(100, 150))
    add("no value and no output", RESIDENT, keys(300), keys(500), 0)
    add("no output", RESIDENT, keys(300), keys(500), 2, outs=[])
    # keys
    add("R builds, S's keys absent from R", RESIDENT, np.arange(1, 501) * 3, np.arange(1, 3001))
    add("S builds, R's keys absent from S", RESIDENT, np.arange(1, 3001), np.arange(1, 501) * 3)
    add("no key matches", RESIDENT, np.arange(1, 2001) * 2, np.arange(1, 3001) * 2 + 1)
    add("equal sizes", RESIDENT, keys(500, 40), keys(500, 40))
    for special in (jm.EMPTY, M64):
        add("only key %#x" % special, RESIDENT, [special] * 70, [special] * 130)
        add("key %#x in R only" % special, RESIDENT, [1, special, 2, special, 3, 4] * 20, [5, 9, 3, 1, 1] * 30)
        add("key %#x in S only" % special, RESIDENT, [1, 9, 2, 5, 3, 4] * 20, [special, 9, 3, special, special] * 30)
        add("key %#x on both sides, R builds" % special, RESIDENT, [1, special, 2, special, 3, 4] * 20, [special, 9, 3, special, special] * 30)
        add("key %#x on both sides, S builds" % special, RESIDENT, [1, special, 2, special, 3, 4] * 40, [special, 9, 3, special, special] * 30)
    add("one key on every row", RESIDENT, [42] * 4000, [42] * 4096)
    add("one key on every row, S builds", RESIDENT, [42] * 4096, [42] * 2000, 3)
    add("two keys interleaved within a wave", RESIDENT, np.tile([5, 6], 1000), np.tile([5, 6, 6, 5, 7], 800), 2)
    log2 = jm.log2_slots(64)
    coll = jm.keys_homed_at(77, log2, 128)
    add("64 keys of one home slot, R builds", RESIDENT, coll[:64], np.concatenate([coll, coll[40:90]]))
    add("64 keys of one home slot, S builds", RESIDENT, np.concatenate([coll, coll[40:90]]), coll[:64])
    log2 = jm.log2_slots(40)
    last = (1 << log2) - 1
    wrap = np.concatenate([jm.keys_homed_at(s, log2, 6, start=1 + 10 * k) for k, s in enumerate((last - 2, last - 1, last))])
    absent = jm.keys_homed_at(last, log2, 30, start=500)
    add("a run that wraps past the last slot, R builds", RESIDENT, np.concatenate([wrap, wrap, wrap[:4]]), np.concatenate([wrap, wrap[::2], absent, wrap]))
    add("a run that wraps past the last slot, S builds", RESIDENT, np.concatenate([wrap, absent, wrap, wrap, wrap[:4]]), np.concatenate([wrap, wrap[::2], wrap[:4]]))
    # the descriptor's forms
    col = u64(rng.integers(0, 200, size=6000))
    selR, selS = u64(rng.integers(0, 6000, size=700)), u64(rng.integers(0, 6000, size=2500))
    add("key columns through d_sel", RESIDENT, col, col[::-1].copy(), 2, selR=selR, selS=selS)
    add("key columns through d_sel, S builds", RESIDENT, col, col[::-1].copy(), 2, selR=selS, selS=selR)
    cap = rm.build_cap(9)
    nine_o = lambda n: [(8 - t, fac(t, n), t % 3 != 1) for t in range(9)]
    add("nine outputs on nine values, R builds", RESIDENT, keys(cap - 3, 300), keys(2100, 300), 9, outs=nine_o(cap - 3))
    add("nine outputs on nine values, S builds", RESIDENT, keys(2100, 300), keys(cap - 3, 300), 9, outs=nine_o(2100))
    add("no d_out at all", RESIDENT, keys(900, 300), keys(2100, 300), 3, outs=[(c, p, False) for c, p, _ in nine_o(900)[6:]])
    for it in items:
        assert len(it["values"]) <= fm.MAX_VALUES and len(it["outs"]) <= fm.MAX_OUTS and all(c < max(len(it["values"]), 1) for c, _, _ in it["outs"]), it["name"]
    # resident and table items alternate in call order while both last
    res = [it for it in items if it["regime"] != TABLE]
    tab = [it for it in items if it["regime"] == TABLE]
    mixed = []
    for k in range(max(len(res), len(tab))):
        mixed += res[k:k + 1] + tab[k:k + 1]
    # more resident items than a chunk holds: one row a side, the key of every seventh absent
    n = ONE_ROW_ITEMS
    oneR, oneS = u64(np.arange(n) + 10), u64(np.arange(n) + 10 + (np.arange(n) % 7 == 0))
    oneV = u64(rng.integers(0, 1 << 62, size=n)) * np.uint64(4) + np.uint64(3)
    for k in range(n):
        mixed.append({"name": "1x1 #%d" % k, "regime": RESIDENT, "R": (oneR[k:k + 1], None), "S": (oneS[k:k + 1], None),
                      "values": [(oneV[k:k + 1], None, None)], "outs": [(0, ONES, k % 2 == 0), (0, (oneV[k:k + 1], None, None), True)]})
    return mixed
