"""rhj_join_sum_batch_device (include/rhj_inter.h, csrc/rhj_join_sum_batch.hip.h): the row count and the view sums of final joins
without their pairs.  Every item is compared as integers with the numpy model of join_sum_model.py; the items of at most two
million pairs also with the route the call replaces, rhj_join_cols_batch_device followed by rhj_apply_batch_device.  All items
run in ONE batch of mixed sizes in scrambled order; some of them again alone."""
import importlib

import numpy as np
import pytest

import join_sum_model as jm

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
PAIR_ROUTE_MOST = 2_000_000


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


def make(name, colR, selR, colS, selS, terms):
    """an item: key columns and row-id vectors (or None) of R and S, terms [(side, src or None, col)]"""
    return {"name": name, "R": (colR, selR), "S": (colS, selS), "terms": list(terms)}


def side_keys(col, sel):
    return col if sel is None else col[sel]


def model(it):
    keys = [side_keys(*it["R"]), side_keys(*it["S"])]
    terms = [(side, col[src] if src is not None else col[:len(keys[side])]) for side, src, col in it["terms"]]
    return jm.join_sum(keys[0], keys[1], terms)


def on_device(dev, it):
    return (dev(it["R"][0]), dev(it["R"][1]), dev(it["S"][0]), dev(it["S"][1]), [(side, dev(src), dev(col)) for side, src, col in it["terms"]])


def build_items():
    rng = np.random.default_rng(2018)
    items = []
    wide = u64(rng.integers(0, 1 << 63, size=6000)) * np.uint64(2) + np.uint64(1)            # values up to 2^64 - 1
    high = u64(np.where(np.arange(6000) % 3 == 0, M64, 1 << 63))                              # 2^64 - 1 and 2^63 only: w * v and the running sums wrap
    ident = u64(rng.permutation(6000))                                                        # a vector into columns of 6000 rows

    def two_terms(nR, nS):
        """one term a side on columns of at least 6000 rows, through nothing and through a vector"""
        return [(0, None, wide), (1, ident[:nS], high)] if max(nR, nS) <= 6000 else []

    def plain(name, kR, kS, terms=None):
        kR, kS = u64(kR), u64(kS)
        items.append(make(name, kR, None, kS, None, two_terms(len(kR), len(kS)) if terms is None else terms))

    # sides
    five = [3, 9, 3, 7, 9]
    plain("0x5", [], five, [])
    plain("5x0", five, [], [])
    plain("1x1 matching", [7], [7])
    plain("1x1 not matching", [7], [8])
    plain("1x5000", [5], rng.integers(0, 10, size=5000))
    plain("5000x1", rng.integers(0, 10, size=5000), [5])
    small, large = rng.integers(0, 50, size=300), rng.integers(0, 50, size=900)
    plain("nR < nS", small, large)
    plain("nR > nS", large, small)
    same = rng.integers(0, 40, size=500)
    other = rng.integers(0, 40, size=500)
    plain("nR == nS", same, other)
    plain("nR == nS swapped", other, same)
    # tiles
    for n in (2047, 2048, 2049, 4097):
        plain("%d rows of R" % n, rng.integers(0, 3000, size=n), rng.integers(0, 3000, size=100))
        plain("%d rows of S" % n, rng.integers(0, 3000, size=100), rng.integers(0, 3000, size=n))
        plain("%d rows of both" % n, rng.integers(0, 3000, size=n), rng.integers(0, 3000, size=n))
    # the table's size
    for n in (1023, 1024, 1025):
        distinct = rng.permutation(1 << 20)[:n] + 1
        plain("%d distinct build keys" % n, distinct, rng.integers(1, 1 << 20, size=3000).tolist() + distinct[::3].tolist())
    plain("all distinct, no match", np.arange(1, 2001) * 2, np.arange(1, 3001) * 2 + 1)
    # keys
    for special in sorted({0, M64, jm.EMPTY}):
        plain("only key %#x" % special, [special] * 70, [special] * 130)
        plain("only key %#x on one side" % special, [special] * 70, [5] * 130)
        plain("key %#x among others" % special, [1, special, 2, special, 3, 4] * 20, [special, 9, 3, special, special] * 30)
    log2 = jm.log2_slots(300)
    coll = jm.keys_homed_at(77, log2, 600)
    plain("300 colliding keys, R builds", coll[:300], np.concatenate([coll, coll[250:350]]))
    plain("300 colliding keys, S builds", np.concatenate([coll, coll[250:350]]), coll[:300])
    log2 = jm.log2_slots(40)
    last = (1 << log2) - 1
    wrap = np.concatenate([jm.keys_homed_at(s, log2, 6, start=1 + 10 * k) for k, s in enumerate((last - 2, last - 1, last))])
    plain("a run that wraps to slot 0", np.concatenate([wrap, wrap, wrap[:4]]), np.concatenate([wrap[::2], jm.keys_homed_at(last, log2, 30, start=500)]))
    # counts
    plain("one key in 5000x5000", [42] * 5000, [42] * 5000)
    plain("one key in 70000x70000", [42] * 70000, [42] * 70000, [])
    k300 = np.arange(1, 301)
    plain("1..300 copies against 300..1", np.repeat(k300, k300), np.repeat(k300, k300[::-1]), [])
    plain("zipf", np.minimum(rng.zipf(1.3, size=20000), 5000), np.minimum(rng.zipf(1.3, size=20000), 5000), [])
    # terms: 0, 8 on side 0, 8 on side 1, alternating; d_src NULL and a vector; d_sel NULL and a vector
    colR, colS = u64(rng.integers(0, 200, size=6000)), u64(rng.integers(0, 200, size=6000))
    selR, selS = u64(rng.integers(0, 5990, size=700)), u64(rng.integers(0, 5990, size=900))          # (below 5990: they also index the offset columns)
    srcR, srcS = u64(rng.integers(0, 5990, size=6000)), u64(rng.integers(0, 5990, size=6000))
    columns = [wide, high, colR, colS]
    for shape, sides in (("no term", []), ("8 terms of R", [0] * 8), ("8 terms of S", [1] * 8), ("alternating terms", [0, 1] * 4)):
        for with_src in (False, True):
            for with_sel in (False, True):
                nR, nS = (700, 900) if with_sel else (6000, 6000)
                terms = [(s, ((srcR, srcS)[s][:(nR, nS)[s]] if with_src else None), columns[(t + s) % 4]) for t, s in enumerate(sides)]
                items.append(make("%s, src %s, sel %s" % (shape, with_src, with_sel), colR, selR if with_sel else None, colS, selS if with_sel else None, terms))
    items.append(make("the key columns summed, one column twice", colR, selR, colS, selS,
                      [(0, selR, colR), (1, selS, colS), (0, selR, colR), (1, None, colR), (0, None, colS)]))
    items.append(make("vectors offset by one word", colR[1:], selR[1:], colS[3:], None, [(0, srcR[1:700], wide[1:]), (1, srcS[3:], high[1:])]))
    # the join whose pairs do not fit anywhere: 199 000 rows of one key on either side, unique keys on the rest
    hot = np.full(200_000, 77, dtype=np.uint64)
    hotR, hotS = hot.copy(), hot.copy()
    hotR[::200] = np.arange(1000) + 1000                 # 1000 unique keys a side, 500 of them shared
    hotS[100::200] = np.arange(1000) + 1500
    bigv = u64(rng.integers(0, 1 << 63, size=200_000)) * np.uint64(2) + np.uint64(1)
    bigsrc = u64(rng.permutation(200_000))
    items.append(make("the join whose pairs do not fit", hotR, None, hotS, None,
                      [(0, None, bigv), (0, bigsrc, bigv), (0, None, hotR), (1, None, bigv), (1, bigsrc, bigv), (1, None, hotS)]))
    # more items than a chunk holds: 4097 of 40x40, each with a constant of its own in the keys
    n = jm.MAX_ITEMS + 1
    base40R, base40S = rng.integers(0, 12, size=40), rng.integers(0, 12, size=40)
    manyR = u64((np.arange(n)[:, None] * 1000 + base40R[None, :] + (np.arange(n)[:, None] % 7 == 0) * base40S[None, :]).reshape(-1))
    manyS = u64((np.arange(n)[:, None] * 1000 + base40S[None, :]).reshape(-1))
    manyV = u64(rng.integers(0, 1 << 62, size=40 * n))
    for k in range(n):
        sl = slice(40 * k, 40 * k + 40)
        items.append(make("40x40 #%d" % k, manyR[sl], None, manyS[sl], None, [(0, None, manyV[sl]), (1, None, manyV[sl])]))
    return items


@pytest.fixture(scope="module")
def batch(rhj):
    """(items in the batch's scrambled order, the model's answers, the device's answers and path ids, the Device)"""
    items = build_items()
    order = np.random.default_rng(7).permutation(len(items))
    items = [items[k] for k in order]
    want = [model(it) for it in items]
    dev = Device(rhj)
    args = [on_device(dev, it) for it in items]
    rhj.lib.rhj_set_timing(0)
    try:
        got, paths = rhj.join_sum_batch_device(args, with_info=True)
        stats = rhj.stats()
    finally:
        rhj.lib.rhj_set_timing(2)
    return {"items": items, "want": want, "got": got, "paths": paths, "args": args, "stats": stats, "dev": dev}


def test_the_batch_equals_the_model(batch):
    assert len(batch["items"]) > jm.MAX_ITEMS + 50
    bad = [it["name"] for it, w, g in zip(batch["items"], batch["want"], batch["got"]) if (w[0], list(w[1])) != (g[0], list(g[1]))]
    assert bad == []
    names = {it["name"]: k for k, it in enumerate(batch["items"])}
    assert batch["want"][names["one key in 70000x70000"]][0] == 70000 ** 2 > 1 << 32
    m = batch["want"][names["the join whose pairs do not fit"]][0]
    assert m == 199_000 ** 2 + 500 and batch["got"][names["the join whose pairs do not fit"]][0] == m
    assert batch["want"][names["all distinct, no match"]] == (0, [0, 0])
    # every path id: 12 but for the items with an empty side
    for it, p in zip(batch["items"], batch["paths"]):
        assert p == (0 if it["name"] in ("0x5", "5x0") else 12), it["name"]


def test_the_statistics_of_the_call(batch):
    st = batch["stats"]
    rows = [(len(side_keys(*it["R"])), len(side_keys(*it["S"]))) for it in batch["items"]]
    assert st["path"] == "join_sum_batch"
    assert st["n_r"] == sum(r for r, _ in rows) and st["n_s"] == sum(s for _, s in rows)
    assert st["matches"] == sum(w[0] for w in batch["want"]) & M64
    assert st["units"] == sum(1 for r, s in rows if r and s)
    assert st["ms_total"] == 0                           # timing level 0


def test_the_batch_equals_the_pair_route(rhj, batch):
    """rhj_join_cols_batch_device with room for the count, then rhj_apply_batch_device over the pairs: the contract's own words"""
    which = [k for k, w in enumerate(batch["want"]) if w[0] <= PAIR_ROUTE_MOST and batch["items"][k]["name"] != "the join whose pairs do not fit"]
    assert len(which) > jm.MAX_ITEMS
    args = batch["args"]
    pairs = rhj.join_cols_batch_device([args[k][:4] for k in which], capacities=[max(batch["want"][k][0], 1) for k in which])
    apply_items, apply_who = [], []
    for k, (p, m) in zip(which, pairs):
        assert m == batch["got"][k][0], batch["items"][k]["name"]
        if m and args[k][4]:
            apply_items.append((p, 2, m, [(side, src, False, col) for side, src, col in args[k][4]]))
            apply_who.append(k)
    res = rhj.apply_batch_device(apply_items)
    for k, terms in zip(apply_who, res):
        assert [s for _, s in terms] == list(batch["got"][k][1]), batch["items"][k]["name"]


def test_items_alone_give_what_they_give_in_the_batch(rhj, batch):
    names = {it["name"]: k for k, it in enumerate(batch["items"])}
    n = jm.MAX_ITEMS
    for name in ("40x40 #0", "40x40 #%d" % (n - 1), "40x40 #%d" % n, "40x40 #%d" % (n // 2), "1x1 matching", "5x0", "300 colliding keys, S builds",
                 "a run that wraps to slot 0", "4097 rows of both", "the join whose pairs do not fit", "alternating terms, src True, sel True"):
        k = names[name]
        (got,), (path,) = rhj.join_sum_batch_device([batch["args"][k]], with_info=True)
        assert got == batch["got"][k] and path == batch["paths"][k], name
    # the first and the last item of the batch's own order, and the pair around its first cut
    for k in (0, n - 1, n, len(batch["items"]) - 1):
        (got,) = rhj.join_sum_batch_device([batch["args"][k]])
        assert got == batch["got"][k], batch["items"][k]["name"]


def test_state_between_calls(rhj, batch, oracle):
    args = batch["args"]
    part = args[:300]
    want = batch["got"][:300]
    assert rhj.join_sum_batch_device(part) == want and rhj.join_sum_batch_device(part) == want       # twice back to back
    rhj.lib.rhj_release()
    rhj.torch.cuda.synchronize()
    assert rhj.join_sum_batch_device(part) == want                                                  # after the arena was dropped
    try:
        for level in (0, 1, 2):
            rhj.lib.rhj_set_timing(level)
            assert rhj.join_sum_batch_device(part) == want
            st = rhj.stats()
            assert (st["ms_total"] > 0) == (level >= 1)
            assert rhj.lib.rhj_last_stats().contents.reserved == 12
            assert st["units"] == sum(1 for p in batch["paths"][:300] if p == 12) and st["matches"] == sum(m for m, _ in want) & M64
    finally:
        rhj.lib.rhj_set_timing(2)
    # an ordinary join afterwards
    rhj.set_bits(4)
    R = oracle.generate(10000, 0, 0, 0.0, 5)
    S = oracle.generate(10000, 1, 10000, 0.0, 6)
    t, m = rhj.join_device(rhj.to_device(R), rhj.to_device(S))
    ref = oracle.join(R, S, 4)
    assert m == len(ref) and (rhj.pairs_to_numpy(t) == ref).all()


def test_tables_of_half_the_arena_cut_after_two(rhj):
    """three items whose tables take half the arena's budget each, between two small ones: the second chunk begins at the third"""
    rows = jm.ARENA_BYTES // 2 // jm.SLOT_BYTES // 4 + 1     # the fewest rows a table of half the budget is built from
    assert jm.table_bytes(rows, rows + 9) == jm.ARENA_BYTES // 2 and jm.table_bytes(rows - 1, rows) == jm.ARENA_BYTES // 4
    keys = u64(np.arange(rows + 5) % 4096 + 1)
    vals = u64(np.arange(rows + 5)) * np.uint64(0x9E3779B97F4A7C15)
    small = u64([3, 4, 4, 5])
    items = [make("small", small, None, keys[:9], None, [(1, None, vals)]),
             make("half a", keys[:rows], None, keys[:rows], None, [(0, None, vals)]),
             make("half b", keys[:rows], None, keys[1:rows + 2], None, [(1, None, vals)]),
             make("half c", keys[2:rows + 4], None, keys[:rows], None, []),
             make("small again", small, None, keys[:9], None, [(1, None, vals)])]
    dev = Device(rhj)
    got = rhj.join_sum_batch_device([on_device(dev, it) for it in items])
    for it, g in zip(items, got):
        w = model(it)
        assert (w[0], list(w[1])) == (g[0], list(g[1])), it["name"]
