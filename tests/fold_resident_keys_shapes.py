"""The items on which the resident form of the tuple-key fold batches is tested (csrc/rhj_fold_keys_lds.hip.h), built with numpy
alone: tests/test_fold_resident_keys_model.py holds every shape to the regime it is named for, tests/test_gpu_fold_resident_keys.py
runs them through rhj_join_foldk_batch_device and rhj_join_foldn_batch_device.  An item has, per side, a list of nkeys key columns
and either ONE row-id vector or None ("R", "S": the foldk form) or a list with one vector or None per word ("nR", "nS": the foldn
form; an item without it takes the foldk form's vector for every word, so that both batches must agree bit for bit, and an item
with it runs in the foldn batch only); values [(w, src, col)], outs [(value, (w, src, col), whether it has a d_out)], and the
regime its sizes must fall in with the switch on."""
import numpy as np

import fold_resident_keys_model as rk
import join_foldk_model as km
import join_sum_model as jm
from fold_resident_shapes import EMPTY_SIDE, M64, ONE_ROW_ITEMS, ONES, RESIDENT, TABLE, u64

MAX_OUTS = 9


def vectors(it, side):
    """the row-id vector of every word of a side, in the foldn form"""
    cols, sel = it[side]
    return it["n" + side] if "n" + side in it else [sel] * len(cols)


def rows_of(it, side):
    cols = it[side][0]
    given = [s for s in vectors(it, side) if s is not None]
    return len(given[0]) if given else len(cols[0])


def side_words(it, side):
    """the key words of a side's rows: nkeys arrays"""
    n = rows_of(it, side)
    return [c[:n] if s is None else c[s.astype(np.int64)] for c, s in zip(it[side][0], vectors(it, side))]


def sizes(it):
    return rows_of(it, "R"), rows_of(it, "S"), len(it["values"])


def model(it):
    """[(vector, total)] per output"""
    return km.foldk_item_np(side_words(it, "R"), side_words(it, "S"), it["values"], [(c, p) for c, p, _ in it["outs"]])


def regime_of(it):
    nR, nS, nvalues = sizes(it)
    return EMPTY_SIDE if not (nR and nS) else RESIDENT if rk.resident(nR, nS, nvalues) else TABLE


def build_items():
    """the shapes, resident and table items alternating in call order as far as they go, then the one-row items"""
    rng = np.random.default_rng(2025)
    rows = max(rk.MAX_ROWS + 1, 6000)
    items = []
    wide = u64(rng.integers(0, 1 << 63, size=rows)) * np.uint64(2) + np.uint64(1)            # values up to 2^64 - 1
    high = u64(np.where(np.arange(rows) % 3 == 0, M64, 1 << 63))                              # 2^64 - 1 and 2^63 only: products and sums wrap
    ident = u64(rng.permutation(rows))                                                        # a vector into columns of `rows` rows
    holes = u64(rng.integers(0, 3, size=rows)) * wide                                         # a weight that is 0 in a third of the rows
    columns = [wide, high, holes]

    def fac(t, n):
        kind = t % 4                                     # ones, a weight, a column, a weight times a column through a vector
        return (columns[t % 3][:n] if kind in (1, 3) else None, ident[:n] if kind == 3 else None, columns[(t + 1) % 3] if kind >= 2 else None)

    def add(name, regime, kR, kS, nvalues=1, outs=None, selR=None, selS=None, nR=None, nS=None):
        it = {"name": name, "regime": regime, "R": ([u64(c) for c in kR], selR), "S": ([u64(c) for c in kS], selS)}
        if nR is not None:
            it["nR"], it["nS"] = nR, nS
        rR, rS = rows_of(it, "R"), rows_of(it, "S")
        it["values"] = [fac(3 + t, rS) for t in range(nvalues)]                               # (the first: a weight times a column through a vector)
        if outs is None:                                 # every value read, the first by an output of ones and by one with a weight: two outputs on one value
            outs = [(0, ONES, True)] + [(c, fac(c + 1, rR), c % 3 != 2) for c in range(nvalues)][:MAX_OUTS - 1] if nvalues else []
        it["outs"] = list(outs)
        items.append(it)

    def split(base, nkeys, radix=5):
        """tuples of nkeys words that are equal exactly where `base` is, and share single words far more often"""
        base = np.asarray(base, dtype=np.uint64)
        words = [(base // np.uint64(radix ** t)) % np.uint64(radix) for t in range(nkeys - 1)]
        return words + [base // np.uint64(radix ** (nkeys - 1))]

    def keys(n, nkeys, span=3000):
        return split(rng.integers(0, span, size=n), nkeys)

    def cat(*sides):
        return [np.concatenate(ws) for ws in zip(*sides)]

    def take(side, idx):
        return [w[idx] for w in side]

    add("1x1 matching", RESIDENT, [[7], [9]], [[7], [9]])
    add("1x1 not matching", RESIDENT, [[7], [9]], [[7], [8]])
    add("0x3", EMPTY_SIDE, [[], []], [[3, 9, 3], [1, 1, 1]])
    add("5x0", EMPTY_SIDE, [[3, 9, 3, 7, 9], [1, 2, 3, 4, 5]], [[], []])
    # the rows and tiles of the workgroup's loops, on either side and on both, at 1..4 keys: R builds, S builds, the tie
    for i, n in enumerate((1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2 * rk.TILE + 1)):
        for arr, (nR, nS) in enumerate(((n, 3000), (3000, n), (n, n))):
            for nk in (((1, 4), (2,), (3,))[(arr + i) % 3] if n < 2 * rk.TILE else (1 + (arr + i) % 4,)):
                nv = 1 if jm.log2_slots(min(nR, nS)) <= 13 else 0            # (two tiles plus one on both sides: the owners alone fit)
                regime = RESIDENT if max(nR, nS) <= rk.MAX_ROWS else TABLE   # (the row limit is measured: the walked side may be beyond it)
                add("%d x %d rows, %d keys" % (nR, nS, nk), regime, keys(nR, nk), keys(nS, nk), nv)
    # the build side at the LDS cap and one row beyond it
    for v in (1, 3, 9):
        cap = rk.build_cap(v)
        other = min(cap + 50, rk.MAX_ROWS)               # (a cap at the row limit leaves the tie, where R builds, and no item whose S builds)
        if cap <= rk.MAX_ROWS:
            add("R builds at the cap, %d values" % v, RESIDENT, keys(cap, 2), keys(other, 2), v)
        if cap < rk.MAX_ROWS:
            add("S builds at the cap, %d values" % v, RESIDENT, keys(other, 3), keys(cap, 3), v)
        add("R builds beyond the cap, %d values" % v, TABLE, keys(cap + 1, 2), keys(cap + 51, 2), v)
        add("S builds beyond the cap, %d values" % v, TABLE, keys(cap + 51, 4), keys(cap + 1, 4), v)
    # the other side at its limit and one row beyond it
    add("S at the row limit", RESIDENT, keys(100, 2, 150), keys(rk.MAX_ROWS, 2, 150))
    add("R at the row limit", RESIDENT, keys(rk.MAX_ROWS, 3, 150), keys(100, 3, 150))
    add("S beyond the row limit", TABLE, keys(100, 2, 150), keys(rk.MAX_ROWS + 1, 2, 150))
    add("R beyond the row limit", TABLE, keys(rk.MAX_ROWS + 1, 4, 150), keys(100, 4, 150))
    add("both sides beyond every cap", TABLE, keys(5000, 2), keys(5000, 2))
    # equality decided on the gather: tuples that differ in one word only, the first or the last
    for nk in (2, 3, 4):
        base = [u64(rng.integers(0, 40, size=200)) for _ in range(nk)]
        first = [base[0] + np.uint64(1)] + base[1:]
        last = base[:-1] + [base[-1] + np.uint64(1)]
        add("one word differs, %d keys, R builds" % nk, RESIDENT, base, cat(first, take(base, slice(0, 50)), last, last))
        add("one word differs, %d keys, S builds" % nk, RESIDENT, cat(first, take(base, slice(0, 50)), last, last), base)
    a, b = u64(rng.integers(0, 30, size=300)), u64(rng.integers(0, 30, size=300))
    add("(a, b) against (b, a), R builds", RESIDENT, [a, b], [np.concatenate([b, a[:90]]), np.concatenate([a, b[:90]])])
    add("(a, b) against (b, a), S builds", RESIDENT, [np.concatenate([b, a[:90]]), np.concatenate([a, b[:90]])], [a, b])
    # pairs of distinct tuples with the SAME 64-bit hash: the same home and the same tag, told apart by the gather alone
    for nk in (2, 3):
        log2 = jm.log2_slots(64)
        one = km.tuples_homed_at(77, log2, 64, nk, start=9, lead=lambda k: [1000 + k + t for t in range(nk - 1)])
        two = km.tuples_homed_at(77, log2, 64, nk, start=9, lead=lambda k: [5000 + 3 * k + t for t in range(nk - 1)])
        assert all(km.tuple_hash(x) == km.tuple_hash(y) and x != y for x, y in zip(km.tuples_of(one), km.tuples_of(two)))
        even, odd = np.arange(0, 64, 2), np.arange(1, 64, 2)
        build = cat(take(one, even), take(two, odd))      # one of each pair is absent from the build side
        add("two tuples a hash, %d keys, R builds" % nk, RESIDENT, build, cat(one, two, take(two, even)))
        add("two tuples a hash, %d keys, S builds" % nk, RESIDENT, cat(one, two, take(two, even), take(one, odd)), build)
    # probe chains
    log2 = jm.log2_slots(40)
    last = (1 << log2) - 1
    wrap = cat(*[km.tuples_homed_at(s, log2, 6, 2, start=1 + 10 * k) for k, s in enumerate((last - 2, last - 1, last))])
    absent = km.tuples_homed_at(last - 2, log2, 30, 2, start=500)       # walks the whole run, past the last slot, to a free slot
    head = take(wrap, slice(0, 4))
    add("a run that wraps past the last slot, R builds", RESIDENT, cat(wrap, wrap, head), cat(wrap, take(wrap, slice(0, None, 2)), absent, wrap))
    add("a run that wraps past the last slot, S builds", RESIDENT, cat(wrap, absent, wrap, wrap, head), cat(wrap, wrap, head))
    log2 = jm.log2_slots(300)
    coll = km.tuples_homed_at(5, log2, 400, 3)
    add("300 tuples of one home slot, R builds", RESIDENT, take(coll, slice(0, 300)), cat(coll, take(coll, slice(250, 350))))
    add("300 tuples of one home slot, S builds", RESIDENT, cat(coll, take(coll, slice(250, 350))), take(coll, slice(0, 300)))
    # no tuple is special
    for nk in (1, 2, 4):
        for special in (0, M64):
            mix = lambda seq: [u64([special if x is None else x + t for x in seq]) for t in range(nk)]
            plain = [u64([1, 9, 2, 5, 3, 4] * 20) + np.uint64(t) for t in range(nk)]
            add("tuple of %#x, %d keys, in R only" % (special, nk), RESIDENT, mix([1, None, 2, None, 3, 4] * 20), [p[:90] for p in plain])
            add("tuple of %#x, %d keys, in S only" % (special, nk), RESIDENT, plain, mix([None, 9, 3, None, None] * 30))
            add("tuple of %#x, %d keys, on both sides" % (special, nk), RESIDENT, mix([1, None, 2, None, 3, 4] * 20), mix([None, 9, 3, None, None] * (30 if nk < 4 else 20)))
    hot = lambda n: [u64([42] * n), u64([7] * n), u64([M64] * n)]
    add("one tuple on every row", RESIDENT, hot(4000), hot(4096))
    add("one tuple on every row, S builds", RESIDENT, hot(4096), hot(2000), 3)
    add("two tuples interleaved within a wave", RESIDENT, [np.tile([5, 6], 1000), np.tile([1, 1], 1000)], [np.tile([5, 6, 6, 5, 7], 800), np.tile([1, 1, 1, 1, 1], 800)], 2)
    # the descriptor's forms: one vector a side (both batches) ...
    cols = [u64(rng.integers(0, 12, size=6000)) for _ in range(3)]
    selR, selS = u64(rng.integers(0, 6000, size=700)), u64(rng.integers(0, 6000, size=2500))
    rev = [c[::-1].copy() for c in cols]
    add("d_sel on neither side", RESIDENT, [c[:900] for c in cols], [c[:2500] for c in rev], 2)
    add("d_sel on R", RESIDENT, cols, [c[:2500] for c in rev], 2, selR=selR)
    add("d_sel on S", RESIDENT, [c[:700] for c in cols], rev, 2, selS=selS)
    add("d_sel on both sides, R builds", RESIDENT, cols, rev, 2, selR=selR, selS=selS)
    add("d_sel on both sides, S builds", RESIDENT, cols, rev, 2, selR=selS, selS=selR)
    # ... and one a word (the batch on the keys of nodes only): none, a vector of its own, the previous word's
    four = cols + [u64(rng.integers(0, 3, size=6000))]
    v1, v2, v3 = (u64(rng.integers(0, 6000, size=700)) for _ in range(3))
    w1, w2 = (u64(rng.integers(0, 6000, size=2500)) for _ in range(2))
    add("a vector per word, R builds", RESIDENT, four, [c[::-1].copy() for c in four], 2, nR=[None, v1, v1, v2], nS=[w1, w1, None, w2])
    add("a vector per word, S builds", RESIDENT, four, [c[::-1].copy() for c in four], 2, nR=[w1, None, w2, w2], nS=[v3, v1, v2, None])
    add("a vector per word, two keys", RESIDENT, four[:2], four[:2], 1, nR=[v1, None], nS=[None, w1])
    add("a vector per word beyond the cap", TABLE, four[:3], four[:3], 9, nR=[v1, v2, v2], nS=[w1, w1, w2])
    # values and outputs
    cap = rk.build_cap(9)
    nine_o = lambda n: [(8 - t, fac(t, n), t % 3 != 1) for t in range(9)]
    add("nine outputs on nine values in reverse order, R builds", RESIDENT, keys(cap - 3, 2, 300), keys(2100, 2, 300), 9, outs=nine_o(cap - 3))
    add("nine outputs on nine values in reverse order, S builds", RESIDENT, keys(2100, 4, 300), keys(cap - 3, 4, 300), 9, outs=nine_o(2100))
    add("no value and no output", RESIDENT, keys(300, 2), keys(500, 2), 0)
    add("values without outputs", RESIDENT, keys(300, 3), keys(500, 3), 2, outs=[])
    add("no d_out at all", RESIDENT, keys(900, 2, 300), keys(2100, 2, 300), 3, outs=[(c, p, False) for c, p, _ in nine_o(900)[6:]])
    for it in items:
        assert len(it["values"]) <= 9 and len(it["outs"]) <= MAX_OUTS and all(c < max(len(it["values"]), 1) for c, _, _ in it["outs"]), it["name"]
        assert 1 <= len(it["R"][0]) == len(it["S"][0]) <= km.MAX_KEYS, it["name"]
    # resident and table items alternate in call order while both last
    res = [it for it in items if it["regime"] != TABLE]
    tab = [it for it in items if it["regime"] == TABLE]
    mixed = []
    for k in range(max(len(res), len(tab))):
        mixed += res[k:k + 1] + tab[k:k + 1]
    # more resident items than a chunk holds: one row a side on two keys, the tuple of every seventh absent
    n = ONE_ROW_ITEMS
    oneA, oneR, oneS = u64(np.arange(n) % 5), u64(np.arange(n) + 10), u64(np.arange(n) + 10 + (np.arange(n) % 7 == 0))
    oneV = u64(rng.integers(0, 1 << 62, size=n)) * np.uint64(4) + np.uint64(3)
    for k in range(n):
        mixed.append({"name": "1x1 #%d" % k, "regime": RESIDENT, "R": ([oneA[k:k + 1], oneR[k:k + 1]], None), "S": ([oneA[k:k + 1], oneS[k:k + 1]], None),
                      "values": [(oneV[k:k + 1], None, None)], "outs": [(0, ONES, k % 2 == 0), (0, (oneV[k:k + 1], None, None), True)]})
    return mixed
