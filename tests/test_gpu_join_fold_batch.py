"""rhj_join_fold_batch_device (include/rhj_inter.h, csrc/rhj_join_fold_batch.hip.h): weighted join folds.  Every item is compared
as integers with the model of join_fold_model.py: every vector word and every total.  All items run in ONE batch of mixed sizes
in scrambled order, every d_out between sentinel words that must survive; some of them again alone, and the items without
weights against rhj_join_sum_batch_device on the same pointers."""
import importlib

import numpy as np
import pytest

import join_fold_model as fm
import join_sum_model as jm

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
SENTINEL = 0x5E5E5E5E5E5E5E5E
ONES = (None, None, None)


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def rhj(mod):
    r = mod.RHJ(device=0)
    r.lib.rhj_set_timing(2)
    r.set_bits(4)
    yield r
    r.lib.rhj_set_timing(2)
    r.lib.rhj_set_order(0)
    r.set_bits(4)


def u64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64))


class Device:
    """numpy arrays on the device, every root array uploaded once: a slice of an array is the same slice of its tensor, so
    what items share on the host they share on the device, and a[1:] is a vector offset by one word"""
    def __init__(self, rhj):
        self.rhj, self.roots = rhj, {}

    def __call__(self, a):
        if a is None:
            return None
        root = a.base if a.base is not None else a
        assert root.dtype == np.uint64 and root.ndim == 1 and root.flags.c_contiguous and (len(a) == 0 or a.strides == (8,))
        if id(root) not in self.roots:
            self.roots[id(root)] = (root, self.rhj.torch.from_numpy(root.view(np.int64)).to(self.rhj.dev))
        off = (a.__array_interface__["data"][0] - root.__array_interface__["data"][0]) // 8
        return self.roots[id(root)][1][off:off + len(a)]


def make(name, colR, selR, colS, selS, values, outs):
    """an item: key columns and row-id vectors (or None) of R and S, values [(w, src, col)], outs [(value, (w, src, col), whether
    it has a d_out)]"""
    return {"name": name, "R": (colR, selR), "S": (colS, selS), "values": list(values), "outs": list(outs)}


def side_keys(col, sel):
    return col if sel is None else col[sel.astype(np.int64)]


def model(it):
    """[(vector, total)] per output"""
    return fm.fold_item_np(side_keys(*it["R"]), side_keys(*it["S"]), it["values"], [(c, p) for c, p, _ in it["outs"]])


class Outputs:
    """one device buffer of sentinels; every d_out is a slice of it with a sentinel word before and behind"""
    def __init__(self, rhj, items):
        self.places, at = [], 1
        for it in items:
            nR = len(side_keys(*it["R"]))
            mine = []
            for _, _, given in it["outs"]:
                mine.append(at if given else None)
                if given:
                    at += nR + 1
            self.places.append(mine)
        self.words = at
        self.buf = rhj.torch.full((at,), SENTINEL, dtype=rhj.torch.int64, device=rhj.dev)

    def args(self, dev, items):
        out = []
        for it, mine in zip(items, self.places):
            nR = len(side_keys(*it["R"]))
            outs = [(c, tuple(dev(x) for x in p), None if a is None else self.buf[a:a + nR]) for (c, p, _), a in zip(it["outs"], mine)]
            out.append((dev(it["R"][0]), dev(it["R"][1]), dev(it["S"][0]), dev(it["S"][1]), [tuple(dev(x) for x in f) for f in it["values"]], outs))
        return out

    def host(self):
        return self.buf.cpu().numpy().view(np.uint64)


def check(items, outputs, got, paths, want=None):
    """every total, every vector word, every word that is nobody's (a sentinel), and the vectors of items with an empty side
    (untouched); returns the model's answers"""
    host = outputs.host()
    expect = np.full(outputs.words, SENTINEL, dtype=np.uint64)
    want = want or [model(it) for it in items]
    bad = []
    for it, mine, w, g, p in zip(items, outputs.places, want, got, paths):
        nR, nS = len(side_keys(*it["R"])), len(side_keys(*it["S"]))
        if p != (13 if nR and nS else 0) or [t for _, t in g] != [t for _, t in w]:
            bad.append(it["name"])
        if nR and nS:
            for a, (vec, _) in zip(mine, w):
                if a is not None:
                    expect[a:a + nR] = vec
    assert bad == []
    wrong = np.flatnonzero(host != expect)
    assert len(wrong) == 0, "output words %s differ" % wrong[:8].tolist()
    return want


def build_items():
    rng = np.random.default_rng(2019)
    items = []
    wide = u64(rng.integers(0, 1 << 63, size=6000)) * np.uint64(2) + np.uint64(1)            # values up to 2^64 - 1
    high = u64(np.where(np.arange(6000) % 3 == 0, M64, 1 << 63))                              # 2^64 - 1 and 2^63 only: products and sums wrap
    ident = u64(rng.permutation(6000))                                                        # a vector into columns of 6000 rows
    holes = u64(rng.integers(0, 3, size=6000)) * wide                                         # a weight that is 0 in a third of the rows

    def dressed(nR, nS):
        """two values and three outputs on shared columns of 6000 rows; beyond that size plain ones"""
        if max(nR, nS) > 6000:
            return [ONES], [(0, ONES, True)]
        return ([ONES, (holes[:nS], ident[:nS], high)],
                [(0, ONES, True), (1, (wide[:nR], None, None), True), (0, (None, ident[:nR], wide), False)])

    def plain(name, kR, kS, values=None, outs=None):
        kR, kS = u64(kR), u64(kS)
        v, o = dressed(len(kR), len(kS))
        items.append(make(name, kR, None, kS, None, v if values is None else values, o if outs is None else outs))

    # sides
    five = [3, 9, 3, 7, 9]
    plain("0x5", [], five, [ONES], [(0, ONES, False)])
    plain("5x0", five, [], [ONES], [(0, ONES, True), (0, (wide[:5], None, None), True)])
    plain("1x1 matching", [7], [7])
    plain("1x1 not matching", [7], [8])
    plain("1x5000", [5], rng.integers(0, 10, size=5000))
    plain("5000x1", rng.integers(0, 10, size=5000), [5])
    small, large = rng.integers(0, 50, size=300), rng.integers(0, 50, size=900)
    plain("nR < nS", small, large)
    plain("nR > nS", large, small)
    same, other = rng.integers(0, 40, size=500), rng.integers(0, 40, size=500)
    plain("nR == nS", same, other)
    plain("nR == nS swapped", other, same)
    # tiles
    for n in (2047, 2048, 2049, 4097):
        plain("%d rows of R" % n, rng.integers(0, 3000, size=n), rng.integers(0, 3000, size=100))
        plain("%d rows of S" % n, rng.integers(0, 3000, size=100), rng.integers(0, 3000, size=n))
        plain("%d rows of both" % n, rng.integers(0, 3000, size=n), rng.integers(0, 3000, size=n))
    # keys: the parent's absent from the child (zeros written), the child's absent from the parent where the parent builds
    plain("all distinct, no match", np.arange(1, 2001) * 2, np.arange(1, 3001) * 2 + 1)
    plain("half of the parent's keys absent", np.arange(1, 1001), np.arange(1, 3001) * 2)
    plain("the child's keys absent, the parent builds", np.arange(1, 501) * 3, np.arange(1, 3001))
    for special in sorted({0, M64, jm.EMPTY}):
        plain("only key %#x" % special, [special] * 70, [special] * 130)
        plain("only key %#x on one side" % special, [special] * 70, [5] * 130)
        plain("key %#x among others" % special, [1, special, 2, special, 3, 4] * 20, [special, 9, 3, special, special] * 30)
        plain("key %#x among others, S builds" % special, [1, special, 2, special, 3, 4] * 40, [special, 9, 3, special, special] * 30)
    log2 = jm.log2_slots(300)
    coll = jm.keys_homed_at(77, log2, 600)
    plain("300 colliding keys, R builds", coll[:300], np.concatenate([coll, coll[250:350]]))
    plain("300 colliding keys, S builds", np.concatenate([coll, coll[250:350]]), coll[:300])
    log2 = jm.log2_slots(40)
    last = (1 << log2) - 1
    wrap = np.concatenate([jm.keys_homed_at(s, log2, 6, start=1 + 10 * k) for k, s in enumerate((last - 2, last - 1, last))])
    plain("a run that wraps to slot 0", np.concatenate([wrap, wrap, wrap[:4]]), np.concatenate([wrap[::2], jm.keys_homed_at(last, log2, 30, start=500)]))
    plain("a run that wraps to slot 0, S builds", np.concatenate([wrap, wrap, wrap, wrap[:4]]), np.concatenate([wrap[::2], jm.keys_homed_at(last, log2, 30, start=500)]))
    # arithmetic
    plain("one key in 5000x5000", [42] * 5000, [42] * 5000)
    k300 = np.arange(1, 301)
    plain("1..300 copies against 300..1", np.repeat(k300, k300), np.repeat(k300, k300[::-1]))
    plain("two keys that share waves", np.tile([5, 6], 3000), np.repeat([5, 6, 7], 2000))
    plain("weights of 0 only", rng.integers(0, 20, size=400), rng.integers(0, 20, size=600), [(u64(np.zeros(600)), None, None), ONES],
          [(0, ONES, True), (1, (u64(np.zeros(400)), None, None), True), (1, (None, None, wide[:400]), True)])
    hot = np.full(200_000, 77, dtype=np.uint64)
    bigw = u64(rng.integers(0, 1 << 63, size=200_000)) * np.uint64(2) + np.uint64(1)
    bigsrc = u64(rng.permutation(200_000))
    plain("200 000 x 200 000 on one key", hot, hot, [ONES, (bigw, None, None), (None, bigsrc, bigw)],
          [(0, ONES, False), (0, ONES, True), (1, (bigw, None, None), False), (2, (bigw, bigsrc, bigw), True)])
    # shapes: 1 and 9 values; 0, 1 and 9 outputs; d_out NULL and given; d_sel and d_src NULL and a vector
    colR, colS = u64(rng.integers(0, 200, size=6000)), u64(rng.integers(0, 200, size=6000))
    selR, selS = u64(rng.integers(0, 5990, size=700)), u64(rng.integers(0, 5990, size=900))          # (below 5990: they also index the offset columns)
    srcR, srcS = u64(rng.integers(0, 5990, size=6000)), u64(rng.integers(0, 5990, size=6000))
    columns = [wide, high, colR, colS, holes]
    for with_sel in (False, True):
        nR, nS = (700, 900) if with_sel else (6000, 6000)
        sides = (colR, selR if with_sel else None, colS, selS if with_sel else None)

        def fac(t, n, src):
            kind = t % 4                                 # ones, a weight, a column, a weight times a column through a vector
            return (columns[t % 5][:n] if kind in (1, 3) else None, src[:n] if kind == 3 else None, columns[(t + 1) % 5] if kind >= 2 else None)
        nine_v = [fac(t + 1, nS, srcS) for t in range(9)]
        nine_o = [(8 - t, fac(t, nR, srcR), t % 3 != 1) for t in range(9)]
        for vname, values in (("1 value", [fac(3, nS, srcS)]), ("9 values", nine_v)):
            for oname, outs in (("no output", []), ("1 output", nine_o[:1]), ("9 outputs", nine_o)):
                outs = [(c % len(values), p, given) for c, p, given in outs]
                items.append(make("%s, %s, sel %s" % (vname, oname, with_sel), *sides, values, outs))
        items.append(make("9 outputs without a vector, sel %s" % with_sel, *sides, nine_v, [(c, p, False) for c, p, _ in nine_o]))
    items.append(make("no value and no output", colR, None, colS, selS, [], []))
    items.append(make("vectors offset by one word", colR[1:], selR[1:], colS[3:], None, [(holes[3:], srcS[3:], wide[1:]), (wide[3:], None, None)],
                      [(0, (wide[1:700], srcR[1:700], high[1:]), True), (1, (None, srcR[1:700], high[3:]), True), (1, ONES, False)]))
    # more items than a chunk holds: 4097 of 40x40, each with a constant of its own in the keys
    n = jm.MAX_ITEMS + 1
    base40R, base40S = rng.integers(0, 12, size=40), rng.integers(0, 12, size=40)
    manyR = u64((np.arange(n)[:, None] * 1000 + base40R[None, :] + (np.arange(n)[:, None] % 7 == 0) * base40S[None, :]).reshape(-1))
    manyS = u64((np.arange(n)[:, None] * 1000 + base40S[None, :]).reshape(-1))
    manyV = u64(rng.integers(0, 1 << 62, size=40 * n))
    for k in range(n):
        sl = slice(40 * k, 40 * k + 40)
        items.append(make("40x40 #%d" % k, manyR[sl], None, manyS[sl], None, [ONES, (manyV[sl], None, None)], [(0, ONES, k % 2 == 0), (1, (manyV[sl], None, None), True)]))
    return items


@pytest.fixture(scope="module")
def batch(rhj):
    """(items in the batch's scrambled order, the model's answers, the device's answers and path ids, the Device)"""
    items = build_items()
    order = np.random.default_rng(8).permutation(len(items))
    items = [items[k] for k in order]
    dev = Device(rhj)
    outputs = Outputs(rhj, items)
    args = outputs.args(dev, items)
    rhj.lib.rhj_set_timing(0)
    try:
        got, paths = rhj.join_fold_batch_device(args, with_info=True)
        stats = rhj.stats()
    finally:
        rhj.lib.rhj_set_timing(2)
    return {"items": items, "got": got, "paths": paths, "args": args, "stats": stats, "dev": dev, "outputs": outputs}


def test_the_batch_equals_the_model(batch):
    items = batch["items"]
    assert len(items) > jm.MAX_ITEMS + 50
    want = check(items, batch["outputs"], batch["got"], batch["paths"])
    batch["want"] = want
    names = {it["name"]: k for k, it in enumerate(items)}
    hot = want[names["200 000 x 200 000 on one key"]]
    assert hot[0][1] == 200_000 ** 2 == 4 * 10 ** 10 and (hot[1][0] == np.uint64(200_000)).all()
    assert [t for _, t in want[names["all distinct, no match"]]] == [0, 0, 0]
    assert want[names["the child's keys absent, the parent builds"]][0][1] == 500
    assert [t for _, t in want[names["weights of 0 only"]]][:2] == [0, 0] and want[names["weights of 0 only"]][2][1] != 0
    # both build choices, and the claim launch, ran
    rows = [(len(side_keys(*it["R"])), len(side_keys(*it["S"]))) for it in items]
    assert any(r and s and jm.build_side(r, s) == 0 for r, s in rows) and any(r and s and jm.build_side(r, s) == 1 for r, s in rows)


def test_the_statistics_of_the_call(batch):
    st = batch["stats"]
    rows = [(len(side_keys(*it["R"])), len(side_keys(*it["S"]))) for it in batch["items"]]
    assert st["path"] == "join_fold_batch"
    assert st["n_r"] == sum(r for r, _ in rows) and st["n_s"] == sum(s for _, s in rows)
    assert st["units"] == sum(1 for r, s in rows if r and s)
    assert st["ms_total"] == 0                           # timing level 0


def test_a_chunk_without_a_claim_tile(rhj, batch):
    """every item's child side is the smaller one: the child claims the slots in the add launch and the claim launch is skipped"""
    which = [k for k, it in enumerate(batch["items"]) if 0 < len(side_keys(*it["S"])) < len(side_keys(*it["R"])) and not it["name"].startswith("40x40")]
    assert len(which) >= 10
    items = [batch["items"][k] for k in which]
    outputs = Outputs(rhj, items)
    got, paths = rhj.join_fold_batch_device(outputs.args(batch["dev"], items), with_info=True)
    check(items, outputs, got, paths)


def test_items_alone_give_what_they_give_in_the_batch(rhj, batch):
    names = {it["name"]: k for k, it in enumerate(batch["items"])}
    n = jm.MAX_ITEMS
    picked = ["40x40 #0", "40x40 #%d" % (n - 1), "40x40 #%d" % n, "1x1 matching", "5x0", "300 colliding keys, S builds", "a run that wraps to slot 0",
              "4097 rows of both", "200 000 x 200 000 on one key", "9 values, 9 outputs, sel True", "no value and no output", "only key 0x0"]
    for k in [names[x] for x in picked] + [0, n - 1, n, len(batch["items"]) - 1]:      # (and the pair around the batch's first cut)
        items = [batch["items"][k]]
        outputs = Outputs(rhj, items)
        got, paths = rhj.join_fold_batch_device(outputs.args(batch["dev"], items), with_info=True)
        check(items, outputs, got, paths)
        assert [t for _, t in got[0]] == [t for _, t in batch["got"][k]], items[0]["name"]


def test_state_between_calls(rhj, batch, oracle):
    items = batch["items"][:300]
    outputs = Outputs(rhj, items)
    args = outputs.args(batch["dev"], items)
    want = [model(it) for it in items]

    def again():
        outputs.buf.fill_(SENTINEL)
        got, paths = rhj.join_fold_batch_device(args, with_info=True)
        check(items, outputs, got, paths, want)
        return paths
    again()
    again()                                              # twice back to back
    rhj.lib.rhj_release()
    rhj.torch.cuda.synchronize()
    again()                                              # after the arena was dropped
    try:
        for level in (0, 1, 2):
            rhj.lib.rhj_set_timing(level)
            paths = again()
            st = rhj.stats()
            assert (st["ms_total"] > 0) == (level >= 1)
            assert rhj.lib.rhj_last_stats().contents.reserved == 13
            assert st["units"] == sum(1 for p in paths if p == 13)
    finally:
        rhj.lib.rhj_set_timing(2)
    # an ordinary join afterwards
    rhj.set_bits(4)
    R = oracle.generate(10000, 0, 0, 0.0, 5)
    S = oracle.generate(10000, 1, 10000, 0.0, 6)
    t, m = rhj.join_device(rhj.to_device(R), rhj.to_device(S))
    ref = oracle.join(R, S, 4)
    assert m == len(ref) and (rhj.pairs_to_numpy(t) == ref).all()


def test_items_without_weights_equal_the_join_sums(rhj, batch):
    """every weight NULL, value 0 and output 0 plain ones, up to eight column outputs on value 0: the totals are
    rhj_join_sum_batch_device's matches and side-0 sums on the same pointers, and with the sides swapped its side-1 sums"""
    rng = np.random.default_rng(5)
    dev = batch["dev"]
    cols = [u64(rng.integers(0, 1 << 63, size=6000)) * np.uint64(2) + np.uint64(1) for _ in range(3)]
    src = u64(rng.integers(0, 6000, size=6000))
    fold_items, sum_items, swapped = [], [], []
    for nR, nS, nterms in ((1, 1, 0), (300, 900, 1), (900, 300, 8), (500, 500, 3), (2049, 4097, 8), (6000, 70, 2)):
        kR, kS = u64(rng.integers(0, 60, size=nR)), u64(rng.integers(0, 60, size=nS))
        terms = [(src[:nR] if t % 2 else None, cols[t % 3]) for t in range(nterms)]
        fold_items.append(make("%dx%d" % (nR, nS), kR, None, kS, None, [ONES], [(0, ONES, False)] + [(0, (None, s, c), False) for s, c in terms]))
        sum_items.append((dev(kR), None, dev(kS), None, [(0, dev(s), dev(c)) for s, c in terms]))
        swapped.append((dev(kS), None, dev(kR), None, [(1, dev(s), dev(c)) for s, c in terms]))
    outputs = Outputs(rhj, fold_items)
    got = rhj.join_fold_batch_device(outputs.args(dev, fold_items))
    for sums in (rhj.join_sum_batch_device(sum_items), rhj.join_sum_batch_device(swapped)):
        for it, g, (matches, s) in zip(fold_items, got, sums):
            assert [t for _, t in g] == [matches] + list(s), it["name"]
    assert got[2][0][1] > 0 and len(got[2]) == 9


def test_tables_of_half_the_arena_cut_after_two(rhj):
    """three items whose tables take half the arena's budget each, between two small ones: the second chunk begins at the third"""
    rows = jm.ARENA_BYTES // 2 // 16 // 4 + 1                # the fewest rows a table of 16-byte slots (one value) of half the budget is built from
    assert 16 << jm.table_log2(rows, rows + 9) == jm.ARENA_BYTES // 2 and 16 << jm.table_log2(rows - 1, rows) == jm.ARENA_BYTES // 4
    keys = u64(np.arange(rows + 5) % 4096 + 1)
    vals = u64(np.arange(rows + 5)) * np.uint64(0x9E3779B97F4A7C15)
    small = u64([3, 4, 4, 5])
    items = [make("small", small, None, keys[:9], None, [(vals[:9], None, None)], [(0, ONES, True)]),
             make("half a", keys[:rows], None, keys[:rows], None, [(vals[:rows], None, None)], [(0, ONES, False)]),
             make("half b", keys[:rows], None, keys[1:rows + 2], None, [(None, None, vals)], [(0, (vals[:rows], None, None), False)]),
             make("half c", keys[2:rows + 4], None, keys[:rows], None, [ONES], [(0, ONES, True)]),
             make("small again", small, None, keys[:9], None, [(vals[:9], None, None)], [(0, ONES, True)])]
    dev = Device(rhj)
    outputs = Outputs(rhj, items)
    got, paths = rhj.join_fold_batch_device(outputs.args(dev, items), with_info=True)
    check(items, outputs, got, paths)


def test_both_table_batches_share_one_arena(rhj):
    """three calls in one process with nothing released between them: (a) 64 folds of 2049 x 4097 rows with nine values leave
    the arena full of 80-byte slots whose words are not zero; (b) three join sums and then (c) two folds with one value place
    16-byte slots over them.  A chunk clears exactly the tables it placed, so (b) and (c) must read none of what (a) left.
    Keys are drawn from [0, 60), the empty key on every side of more than one row; the sizes sit on the 2048-row tile and on the tie
    of the build side.  (c)'s one value is 0 in every row ("zero values": an item without a value can have no output), so a
    single word of (a) read as an A_c shows in a d_out, all of whose words must be written zeros."""
    rng = np.random.default_rng(64)
    dev = Device(rhj)

    def keys(n):
        k = u64(rng.integers(0, 60, size=n))
        if n > 1:
            k[int(rng.integers(0, n))] = jm.EMPTY
        return k
    # (a)
    weights = [u64(rng.integers(1, 1 << 63, size=4097)) * np.uint64(2) + np.uint64(1) for _ in range(3)]
    src = u64(rng.permutation(4097))
    nine = [ONES] + [(weights[c % 3], src if c % 2 else None, weights[(c + 1) % 3] if c >= 4 else None) for c in range(1, fm.MAX_VALUES)]
    outs = [(0, ONES, True), (fm.MAX_VALUES - 1, (weights[0][:2049], None, None), True), (4, ONES, False)]
    folds = [make("2049x4097 #%d" % k, keys(2049), None, keys(4097), None, nine, outs) for k in range(64)]
    assert len(nine) == fm.MAX_VALUES and 64 * (80 << jm.table_log2(2049, 4097)) < jm.ARENA_BYTES      # one chunk
    outputs = Outputs(rhj, folds)
    got, paths = rhj.join_fold_batch_device(outputs.args(dev, folds), with_info=True)
    check(folds, outputs, got, paths)
    assert all(t != 0 for g in got for _, t in g)
    # (b)
    cols = [u64(rng.integers(0, 1 << 63, size=2048)) * np.uint64(2) + np.uint64(1) for _ in range(2)]
    sums, want = [], []
    for nR, nS in ((300, 900), (900, 300), (2048, 2048)):
        kR, kS = keys(nR), keys(nS)
        sums.append((dev(kR), None, dev(kS), None, [(0, None, dev(cols[0])), (1, None, dev(cols[1]))]))
        want.append(jm.join_sum(kR, kS, [(0, cols[0][:nR]), (1, cols[1][:nS])]))
    assert [(m, list(s)) for m, s in rhj.join_sum_batch_device(sums)] == [(m, list(s)) for m, s in want]
    assert rhj.stats()["path"] == "join_sum_batch" and rhj.stats()["matches"] == sum(m for m, _ in want) & M64
    # (c)
    zeros = u64(np.zeros(2048))
    last = [make("1x1", keys(1), None, keys(1), None, [(zeros[:1], None, None)], [(0, ONES, True)]),
            make("2049x2048", keys(2049), None, keys(2048), None, [(zeros, None, None)], [(0, ONES, True)])]
    outputs = Outputs(rhj, last)
    got, paths = rhj.join_fold_batch_device(outputs.args(dev, last), with_info=True)
    want = check(last, outputs, got, paths)
    assert all(t == 0 and not vec.any() for w in want for vec, t in w)
