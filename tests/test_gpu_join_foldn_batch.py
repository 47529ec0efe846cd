"""rhj_join_foldn_batch_device (include/rhj_inter.h, csrc/rhj_join_foldn_batch.hip.h): weighted join folds on tuple keys whose
words each have a row-id vector of their own.  Every item is compared as integers with the model of join_foldn_model.py: every
vector word, every total and every word behind an output.  All items run in ONE batch of mixed sizes, key counts and vector
patterns in scrambled order, more of them than a chunk holds; the items whose words all share one vector a side run again through
rhj_join_foldk_batch_device on the same pointers and must give the same words.

Within an item all key columns have one length and every vector's values stay below it, and a side has no more positions than
that: whichever vector a word is read through, right or wrong, the read stays inside its column."""
import importlib

import numpy as np
import pytest

import join_foldn_model as nm
import join_sum_model as jm

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
SENTINEL = 0x5E5E5E5E5E5E5E5E
ONES = (None, None, None)
PATH = 16
LENGTH = 5000                                            # the rows of a shared key column


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
    """numpy arrays on the device, every root array uploaded once: a slice of an array is the same slice of its tensor"""
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


def side(cols, sels, n=None):
    """a side: key columns, one vector or None per column, and its positions (the vectors' length, else n)"""
    cols, sels = [u64(c) for c in cols], list(sels)
    given = [s for s in sels if s is not None]
    rows = len(given[0]) if given else (len(cols[0]) if n is None else n)
    assert len(cols) == len(sels) and all(len(s) == rows for s in given) and all(len(c) == len(cols[0]) >= rows for c in cols)
    assert all(int(s.max()) < len(cols[0]) for s in given if len(s))           # any vector on any column stays inside it
    return cols, sels, rows


def shares_one_vector(s):
    return all(v is s[1][0] for v in s[1])


def model(it):
    return nm.foldn_item_np(it["R"], it["S"], it["values"], [(c, p) for c, p, _ in it["outs"]])


class Outputs:
    """one device buffer of sentinels; every d_out is a slice of it with a sentinel word before and behind"""
    def __init__(self, rhj, items):
        self.places, at = [], 1
        for it in items:
            mine = []
            for _, _, given in it["outs"]:
                mine.append(at if given else None)
                if given:
                    at += it["R"][2] + 1
            self.places.append(mine)
        self.words = at
        self.buf = rhj.torch.full((at,), SENTINEL, dtype=rhj.torch.int64, device=rhj.dev)

    def args(self, dev, items, one_vector=False):
        """the items as join_foldn_batch_device takes them; one_vector: as join_foldk_batch_device does"""
        out = []
        for it, mine in zip(items, self.places):
            (cR, sR, nR), (cS, sS, nS) = it["R"], it["S"]
            outs = [(c, tuple(dev(x) for x in p), None if a is None else self.buf[a:a + nR]) for (c, p, _), a in zip(it["outs"], mine)]
            values = [tuple(dev(x) for x in f) for f in it["values"]]
            if one_vector:
                out.append(([dev(c if sR[0] is not None else c[:nR]) for c in cR], dev(sR[0]), [dev(c if sS[0] is not None else c[:nS]) for c in cS], dev(sS[0]), values, outs))
            else:
                out.append(([dev(c if any(s is not None for s in sR) else c[:nR]) for c in cR], [dev(s) for s in sR],
                            [dev(c if any(s is not None for s in sS) else c[:nS]) for c in cS], [dev(s) for s in sS], values, outs))
        return out

    def host(self):
        return self.buf.cpu().numpy().view(np.uint64)


def check(items, outputs, got, paths, want=None, path=PATH):
    """every total, every vector word, every word that is nobody's (a sentinel); returns the model's answers"""
    host = outputs.host()
    expect = np.full(outputs.words, SENTINEL, dtype=np.uint64)
    want = want or [model(it) for it in items]
    bad = []
    for it, mine, w, g, p in zip(items, outputs.places, want, got, paths):
        nR, nS = it["R"][2], it["S"][2]
        if p != (path if nR and nS else 0) or [t for _, t in g] != [t for _, t in w]:
            bad.append(it["name"])
        if nR and nS:
            for a, (vec, _) in zip(mine, w):
                if a is not None:
                    expect[a:a + nR] = vec
    assert bad == []
    wrong = np.flatnonzero(host != expect)
    assert len(wrong) == 0, "output words %s differ" % wrong[:8].tolist()
    return want


PATTERNS = ("n", "o", "on", "no", "op", "oo", "nop", "oop", "opo", "ooo", "nnn", "opp", "noop", "oooo", "opop", "ppnn", "oppp", "onoo")


def build_items():
    rng = np.random.default_rng(2025)
    items = []
    wide = u64(rng.integers(0, 1 << 63, size=LENGTH)) * np.uint64(2) + np.uint64(1)
    ident = u64(rng.permutation(LENGTH))
    holes = u64(rng.integers(0, 3, size=LENGTH)) * wide
    vector = lambda n: u64(rng.integers(0, LENGTH, size=n))

    def vectors(pattern, n):
        """a vector per word: n none, p the previous word's (none when that has none), o one of its own"""
        out = []
        for t, ch in enumerate(pattern):
            out.append(None if ch == "n" else out[t - 1] if ch == "p" and t else vector(n))
        return out

    def dressed(nR, nS):
        """two values and three outputs on shared columns"""
        return ([ONES, (holes[:nS], ident[:nS], wide)],
                [(0, ONES, True), (1, (wide[:nR], None, None), True), (0, (None, ident[:nR], wide), False)])

    def add(name, R, S, values=None, outs=None):
        v, o = dressed(R[2], S[2])
        items.append({"name": name, "R": R, "S": S, "values": v if values is None else values, "outs": o if outs is None else outs})

    def draw(nk, span=5, rows=LENGTH):
        return [rng.integers(0, span, size=rows) for _ in range(nk)]

    # sides at the wave, round, tile and two-tile edges; every key count; every pattern on R only, on S only and on both; either side
    # building, and the tie
    sizes = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097)
    k = 0
    for n in sizes:
        for m in (sizes[(sizes.index(n) + 5) % len(sizes)], n):
            for where in ("R", "S", "both"):
                pat = PATTERNS[k % len(PATTERNS)]
                k += 1
                nk = len(pat)
                plain = "n" * nk
                add("%d x %d rows, %s on %s" % (n, m, pat, where),
                    side(draw(nk), vectors(pat if where != "S" else plain, n), n), side(draw(nk), vectors(pat if where != "R" else plain, m), m))
    assert k >= 3 * len(PATTERNS)
    add("0 x 5 rows", side([[], []], [None, None]), side(draw(2, rows=5), [None, None]), values=[ONES], outs=[(0, ONES, False)])
    add("5 x 0 rows", side(draw(3), vectors("ono", 5), 5), side([[], [], []], [None] * 3), values=[ONES], outs=[(0, ONES, True)])
    # tuples that differ only in the ONE word that has a vector of its own: read through word 0's vector (or through none) the
    # word is another row's value, and the tuple another tuple
    for nk in (2, 3, 4):
        for w in range(1, nk):
            cols = [np.full(LENGTH, 7) for _ in range(nk)]
            cols[w] = np.arange(LENGTH) % 97
            for shared in ("n", "o"):
                def one_own(n):
                    base = None if shared == "n" else vector(n)
                    return [vector(n) if t == w else base for t in range(nk)]
                few = [np.full(LENGTH, 7) for _ in range(nk)]
                few[w] = np.arange(LENGTH) % 97 % 31
                add("word %d of %d alone has its vector (others %s), the build side's" % (w, nk, shared), side(cols, one_own(300), 300), side(few, one_own(900), 900))
                add("word %d of %d alone has its vector (others %s), the probing side's" % (w, nk, shared), side(cols, one_own(900), 900), side(few, one_own(300), 300))
                add("word %d of %d alone has its vector (others %s), S builds and owns it" % (w, nk, shared), side(few, [None] * nk, 900), side(cols, one_own(300), 300))
    # the all-zero and the all-ones tuple, through vectors that pick them out of columns of other values
    for nk in (1, 2, 4):
        cols = [np.where(np.arange(LENGTH) % 3 == 0, 0, np.where(np.arange(LENGTH) % 3 == 1, M64, 5)).astype(np.uint64) for _ in range(nk)]
        third = lambda n, r: [u64(3 * rng.integers(0, LENGTH // 3, size=n) + r) for _ in range(nk)]
        mixed = lambda n: [u64(rng.integers(0, LENGTH - 2, size=n)) for _ in range(nk)]
        add("all-zero and all-ones tuples among others, %d keys, R builds" % nk, side(cols, mixed(200)), side(cols, mixed(700)))
        add("all-zero and all-ones tuples among others, %d keys, S builds" % nk, side(cols, mixed(700)), side(cols, mixed(200)))
        add("only the all-zero tuple, %d keys" % nk, side(cols, third(70, 0)), side(cols, third(130, 0)))
        add("only the all-ones tuple, %d keys" % nk, side(cols, third(130, 1)), side(cols, third(70, 1)))
    # one tuple on every row: the hot-slot path
    hot = [np.full(LENGTH, 11), np.full(LENGTH, 22), np.full(LENGTH, 33)]
    add("one hot tuple on both sides, R builds", side(hot, vectors("ooo", 3000)), side(hot, vectors("opo", 3001)))
    add("one hot tuple on both sides, S builds", side(hot, vectors("non", 3002), 3002), side(hot, vectors("oon", 3000)))
    # 0..9 values and outputs in every form of the factor, d_out given or not
    columns = [wide, holes, ident]
    srcR, srcS = u64(rng.integers(0, LENGTH - 10, size=3000)), u64(rng.integers(0, LENGTH - 10, size=3000))

    def fac(t, n, src):
        kind = t % 4
        return (columns[t % 3][:n] if kind in (1, 3) else None, src[:n] if kind == 3 else None, columns[(t + 1) % 3] if kind >= 2 else None)
    for count in range(10):
        keys = draw(2, 20)
        values = [fac(t + 1, 3000, srcS) for t in range(count)]
        outs = [(count - 1 - t, fac(t, 3000, srcR), t % 3 != 1) for t in range(count)]
        add("%d values, %d outputs" % (count, count), side(keys, vectors("oo", 3000)), side(keys, vectors("no", 3000), 3000), values=values, outs=outs)
    add("1 value, no output", side(draw(2), vectors("oo", 100)), side(draw(2), vectors("oo", 100)), values=[ONES], outs=[])
    # more items than a chunk holds: 40 x 40 on two keys over slices of 40 rows, word 1 through a vector of its own on both sides
    n = jm.MAX_ITEMS - len(items) + 5
    b40R, b40S = rng.integers(0, 4, size=(2, 40)), rng.integers(0, 4, size=(2, 40))
    manyR = [u64((np.arange(n)[:, None] * 1000 * (1 - w) + b40R[w][None, :]).reshape(-1)) for w in range(2)]
    manyS = [u64((np.arange(n)[:, None] * 1000 * (1 - w) + b40S[w][None, :]).reshape(-1)) for w in range(2)]
    manyV = u64(rng.integers(0, 1 << 62, size=40 * n))
    selR, selS = u64(rng.integers(0, 40, size=40 * n)), u64(rng.integers(0, 40, size=40 * n))
    for k in range(n):
        sl = slice(40 * k, 40 * k + 40)
        items.append({"name": "40x40 #%d" % k, "R": side([c[sl] for c in manyR], [None, selR[sl]]), "S": side([c[sl] for c in manyS], [selS[sl] if k % 2 else None, selS[sl]]),
                      "values": [ONES, (manyV[sl], None, None)], "outs": [(0, ONES, k % 2 == 0), (1, (manyV[sl], None, None), True)]})
    return items


@pytest.fixture(scope="module")
def batch(rhj):
    items = build_items()
    order = np.random.default_rng(9).permutation(len(items))
    items = [items[k] for k in order]
    dev = Device(rhj)
    outputs = Outputs(rhj, items)
    args = outputs.args(dev, items)
    rhj.lib.rhj_set_timing(0)
    try:
        got, paths = rhj.join_foldn_batch_device(args, with_info=True)
        stats = rhj.stats()
    finally:
        rhj.lib.rhj_set_timing(2)
    return {"items": items, "got": got, "paths": paths, "stats": stats, "dev": dev, "outputs": outputs}


def test_the_batch_equals_the_model_and_the_tuple_key_batch(rhj, batch):
    items = batch["items"]
    launched = sum(1 for it in items if it["R"][2] and it["S"][2])
    assert jm.MAX_ITEMS < launched <= jm.MAX_ITEMS + 16 and len(items) == jm.MAX_ITEMS + 5        # a chunk is cut after 4096 launched items
    want = check(items, batch["outputs"], batch["got"], batch["paths"])
    names = {it["name"]: k for k, it in enumerate(items)}
    assert want[names["one hot tuple on both sides, R builds"]][0][1] == 3000 * 3001
    assert want[names["only the all-zero tuple, 4 keys"]][0][1] == 70 * 130
    sides = [(it["R"][2], it["S"][2]) for it in items]
    assert any(r and s and r < s for r, s in sides) and any(r and s and s < r for r, s in sides) and any(r and r == s for r, s in sides)
    assert {len(it["R"][0]) for it in items} == {1, 2, 3, 4}
    # a word read through word 0's vector, or through none, would have changed these answers
    for it, w in zip(items, want):
        if not it["name"].startswith("word "):
            continue
        for which in ("R", "S"):
            cols, sels, n = it[which]
            if len({id(s) for s in sels}) == 1:
                continue
            wrong = dict(it, **{which: (cols, [sels[0]] * len(sels), n)})
            assert [t for _, t in model(wrong)] != [t for _, t in w], it["name"]
    # the items whose words all share one vector a side: rhj_join_foldk_batch_device on the same pointers, bit for bit
    same = [it for it in items if shares_one_vector(it["R"]) and shares_one_vector(it["S"])]
    assert len(same) >= 12 and any(it["R"][1][0] is not None for it in same) and any(len(it["R"][0]) == 4 for it in same)
    outs_n, outs_k = Outputs(rhj, same), Outputs(rhj, same)
    got_n, paths_n = rhj.join_foldn_batch_device(outs_n.args(batch["dev"], same), with_info=True)
    got_k, paths_k = rhj.join_foldk_batch_device(outs_k.args(batch["dev"], same, one_vector=True), with_info=True)
    assert [[t for _, t in g] for g in got_n] == [[t for _, t in g] for g in got_k]
    assert [p and PATH for p in paths_k] == paths_n and set(paths_k) <= {0, 14}
    assert (outs_n.host() == outs_k.host()).all()
    check(same, outs_n, got_n, paths_n)


def test_the_statistics_of_the_call(batch):
    st = batch["stats"]
    sides = [(it["R"][2], it["S"][2]) for it in batch["items"]]
    assert st["path"] == "join_foldn_batch"
    assert st["n_r"] == sum(r for r, _ in sides) and st["n_s"] == sum(s for _, s in sides)
    assert st["units"] == sum(1 for r, s in sides if r and s)
    assert st["ms_total"] == 0                           # timing level 0
