"""GPU: the split paths — the low-radix path (r <= 8, csrc/rhj_lowradix.hip.h) and the sub-bucket path (r = 9..13,
csrc/rhj_subbucket.hip.h) — at the split widths k the rule (rhj_sub_bits) gives, and on the edges their kernels decide on:
probe-side ties, pass B's 4096-tuple chunks, one-tuple and one-sided buckets, a hot bucket, a split that does not split,
16 and 17 matches, row ids at and beyond 32 bits, keys that collide in the internal join's hash, and the partition knobs.

Every result is compared bit for bit, order included: with oracle.join up to ~90 M tuples a side, beyond that with the
canonical-order model of tests/canon.py on the device (held to the oracle by tests/test_canon_model.py).  Every case asserts
the path it meant to reach and the k its sizes give, so a change of the rule fails here instead of losing coverage."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import hashkeys as hk
from canon import canonical_join
from pyoracle import TUPLE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
CHUNK = 4096                      # SB_CHUNK: pass B's chunk and the emit sequence's slot (rhj_subbucket.hip.h)
LDS_CAP = (160 * 1024 - 2048 - 128) * 2 // 9     # FUSED_LDS_CAP (rhj_device.hip): the largest build side the fused kernel's LDS index takes


def split_path(r):
    return "lowradix" if r <= 8 else "subbucket"


@pytest.fixture(scope="module")
def rhj():
    mod = importlib.import_module("sigmod-2018_amd")
    r = mod.RHJ(device=0)
    r.lib.rhj_set_lowradix(1)
    r.lib.rhj_set_count_in_pass1(1)
    yield r
    r.lib.rhj_set_lowradix(1)
    r.lib.rhj_set_count_in_pass1(1)


def expect_k(rhj, r, nR, nS, k):
    got = rhj.lib.rhj_sub_bits(r, nR, nS)
    assert got == k, "rhj_sub_bits(%d, %d, %d) = %d, the case was built for k = %d" % (r, nR, nS, got, k)


def check_stats(rhj, r, what, taken=True):
    """The last join ran on r radix bits, on r's split path (taken) or, refused there, on another one."""
    st = rhj.stats()
    assert st["radix_bits"] == r, (what, st["radix_bits"])
    if taken:
        assert st["path"] == split_path(r), (what, st["path"])
    else:
        assert st["path"] not in ("lowradix", "subbucket"), (what, st["path"])


def rel(keys, ids=None):
    out = np.zeros(len(keys), dtype=TUPLE)
    out["value"] = keys
    out["row_id"] = np.arange(len(keys), dtype=np.uint64) if ids is None else ids
    return out


def as_pairs(p):
    return np.ascontiguousarray(p).view(np.uint64).reshape(-1, 2)


def dev_pairs(rhj, R, S, **kw):
    dR = R if not isinstance(R, np.ndarray) else rhj.to_device(R)
    dS = S if not isinstance(S, np.ndarray) else rhj.to_device(S)
    t, m = rhj.join_device(dR, dS, **kw)
    return t.cpu().numpy().view(np.uint64).reshape(-1, 2), m


def same(got, want, what):
    assert got.shape == want.shape, "%s: %d pairs, expected %d" % (what, len(got), len(want))
    if not np.array_equal(got, want):
        i = int(np.nonzero((got != want).any(axis=1))[0][0])
        raise AssertionError("%s: first difference at pair %d: %r, expected %r" % (what, i, got[i], want[i]))


def join_checked(rhj, oracle, R, S, r, k, what, want=None, path=None):
    """The join on r bits against the oracle (or `want`), on the path the rule sends it to."""
    expect_k(rhj, r, len(R), len(S), k)
    rhj.set_bits(r)
    if want is None:
        want = as_pairs(oracle.join(R, S, r))
    got, m = dev_pairs(rhj, R, S)
    st = rhj.stats()
    assert st["path"] == (path or split_path(r)) and st["radix_bits"] == r, (what, st["path"], st["radix_bits"])
    assert m == len(want), what
    same(got, want, what)
    return want


def random_keys(rng, n, r, buckets):
    mask = np.uint64((1 << r) - 1)
    return (rng.integers(0, M64, size=n, dtype=np.uint64, endpoint=True) & ~mask) | buckets


def build(seed, r, hR, hS, share=None, override=None):
    """R and S bucket by bucket: hR[b] random 64-bit keys of bucket b in R; hS[b] keys of b in S, drawn from R's keys of b
    (fresh keys of b where R has none).  share {b: (s, k)}: every key of bucket b has bits [r, r + k) == s.  override
    {b: (R keys, S keys)}: bucket b holds exactly these.  Row ids are positions; both relations shuffled."""
    rng = np.random.default_rng(seed)
    nb = 1 << r
    hR, hS = np.array(hR, dtype=np.int64), np.array(hS, dtype=np.int64)
    override = override or {}
    for b, (kr, ks) in override.items():
        hR[b], hS[b] = len(kr), len(ks)
    bR = np.repeat(np.arange(nb, dtype=np.uint64), hR)
    kR = random_keys(rng, len(bR), r, bR)
    bS = np.repeat(np.arange(nb, dtype=np.uint64), hS)
    kS = random_keys(rng, len(bS), r, bS)
    for b, (s, k) in (share or {}).items():
        m = np.uint64(((1 << k) - 1) << r)
        for keys, bb in ((kR, bR), (kS, bS)):
            sel = bb == np.uint64(b)
            keys[sel] = (keys[sel] & ~m) | np.uint64(s << r)
    offR = np.concatenate([[0], np.cumsum(hR)])
    offS = np.concatenate([[0], np.cumsum(hS)])
    bi = bS.astype(np.int64)
    has = hR[bi] > 0
    pick = offR[bi] + (rng.random(len(bS)) * hR[bi]).astype(np.int64)
    kS[has] = kR[pick[has]]
    for b, (kr, ks) in override.items():
        kR[offR[b]:offR[b + 1]] = kr
        kS[offS[b]:offS[b + 1]] = ks
    return rel(rng.permutation(kR)), rel(rng.permutation(kS))


# ---- a. every split width ----------------------------------------------------------------------------------------------
# (r, k, tuples a side): the smallest round size the rule gives that k for
# (grouped by size: one pair of relations is kept at a time)
# 9..13 bits: with the model's cases below and test_gpu_subbucket.py's k = 1 at 9, 10 and 12 bits, every (r, k) the rule gives.
# 1..8 bits (the low-radix path): every r and every k from 1 to 8, at 600 K and 12 M a side (test_sub_bits.py pins the rule there).
ORACLE_WIDTHS = [(1, 4, 600_000), (2, 3, 600_000), (3, 2, 600_000), (4, 1, 600_000),
                 (1, 8, 12_000_000), (2, 8, 12_000_000), (3, 7, 12_000_000), (4, 6, 12_000_000), (5, 5, 12_000_000),
                 (6, 4, 12_000_000), (7, 3, 12_000_000), (8, 2, 12_000_000),
                 (9, 2, 24_000_000), (9, 3, 42_000_000), (10, 2, 42_000_000), (11, 1, 69_000_000), (9, 4, 83_000_000),
                 (10, 3, 83_000_000), (11, 2, 83_000_000)]
_FK = {}


def fk_relations(oracle, n, r):
    """n x n uniform foreign keys (S drawn from R's n unique keys): per bucket either side may be the bigger one.  Returns
    R, S and the oracle's result on r bits (kept for the next case on the same relations)."""
    if _FK.get("n") != n:
        _FK.clear()
        _FK.update(n=n, R=oracle.generate(n, 0, 0, 0.0, 1000 + n % 997), S=oracle.generate(n, 1, n, 0.0, 2000 + n % 991))
    if r not in _FK:
        _FK[r] = as_pairs(oracle.join(_FK["R"], _FK["S"], r))
    return _FK["R"], _FK["S"], _FK[r]


@pytest.mark.parametrize("r,k,n", ORACLE_WIDTHS, ids=["r%d_k%d" % (r, k) for r, k, _ in ORACLE_WIDTHS])
def test_every_width_against_the_oracle(rhj, oracle, r, k, n):
    R, S, want = fk_relations(oracle, n, r)
    join_checked(rhj, oracle, R, S, r, k, "r=%d k=%d" % (r, k), want=want)


def test_duplicates_on_both_sides_at_k3(rhj, oracle):
    """Poisson duplicates on both sides (about 1.3 a key, far below 16 matches): several matches per probe tuple copied from
    the internal join's list at k = 3."""
    R = oracle.generate(42_000_000, 4, 32_000_000, 0.0, 301)
    S = oracle.generate(42_000_000, 4, 32_000_000, 0.0, 302)
    join_checked(rhj, oracle, R, S, 9, 3, "duplicates")


MODEL_WIDTHS = [(9, 5, 170_000_000), (10, 4, 170_000_000), (11, 3, 170_000_000), (12, 2, 170_000_000), (13, 1, 280_000_000)]


@pytest.mark.parametrize("n", sorted({n for _, _, n in MODEL_WIDTHS}))
def test_every_width_against_the_model(rhj, n):
    """Beyond the oracle's reach: uniform foreign keys generated on the device, every pair compared with the canonical-order
    model on the device.  r = 13 never counts pass 2's digits in pass 1 (count_in_pass1 = bits <= 12)."""
    torch = rhj.torch
    cases = [(r, k) for r, k, nn in MODEL_WIDTHS if nn == n]
    free, _ = torch.cuda.mem_get_info()
    # inputs, the library's buffers (partitions, intermediates, scratch pairs, stash, emit map, output) and the model's arrays:
    # 411 B a tuple measured at the peak on 280 M a side (81 B inputs, 204 B after the join, 411 B after the model)
    need = n * 480 + (8 << 30)
    if free < need:
        pytest.skip("needs ~%d GB of free device memory" % (need >> 30))
    import bench
    w = dict(nR=n, nS=n, bits=cases[0][0], dist="uniform")
    R, S = bench.make_relations(w, rhj.dev, 17)
    for r, k in cases:
        expect_k(rhj, r, n, n, k)
        rhj.set_bits(r)
        t, m = rhj.join_device(R, S, capacity=n)
        st = rhj.stats()
        assert st["path"] == "subbucket" and st["radix_bits"] == r, (r, st["path"])
        assert m == n
        want = canonical_join(R[:, 0], R[:, 1], S[:, 0], S[:, 1], r)
        assert want.shape == t.shape and torch.equal(t, want), "r=%d k=%d differs from the model" % (r, k)
        del t, want
        torch.cuda.empty_cache()


# ---- b. probe-side ties, chunk edges, tiny, one-sided and hot buckets --------------------------------------------------
def edge_layout(r, base, seed):
    """Bucket counts around `base` (every seventh bucket a tie) and the special buckets; returns hR, hS, {name: bucket}."""
    rng = np.random.default_rng(seed)
    nb = 1 << r
    hR = base + rng.integers(-base // 20, base // 20, size=nb)
    hS = base + rng.integers(-base // 20, base // 20, size=nb)
    hS[::7] = hR[::7]
    special = [("tie", base - 7, base - 7), ("R_one_more", base + 1, base), ("S_one_more", base, base + 1)]
    for m in (1, 2, 11):
        c = m * CHUNK
        special += [("tie_%d_minus" % m, c - 1, c - 1), ("tie_%d" % m, c, c), ("tie_%d_plus" % m, c + 1, c + 1),
                    ("R_%d_S_minus" % m, c, c - 1), ("R_minus_S_%d" % m, c - 1, c), ("R_plus_S_%d" % m, c + 1, c),
                    ("R_%d_S_plus" % m, c, c + 1)]
    special += [("one_one", 1, 1), ("one_R", 1, 5), ("one_S", 5, 1), ("only_R", 1, 0), ("only_S", 0, 1),
                ("R_empty", 0, base // 2), ("S_empty", base // 2, 0), ("both_empty", 0, 0), ("hot", base, 1_200_000)]
    names = {}
    step = nb // len(special)
    for i, (name, a, b) in enumerate(special):
        bb = i * step + 3
        hR[bb], hS[bb] = a, b
        names[name] = bb
    return hR, hS, names


EDGE = {9: (47_000, 2), 6: (72_000, 2)}          # r: (tuples a bucket, k); 6 bits: the low-radix path
_EDGE_CACHE = {}


def edge_relations(rhj, oracle, r):
    if r not in _EDGE_CACHE:
        _EDGE_CACHE.clear()
        base, k = EDGE[r]
        hR, hS, names = edge_layout(r, base, 40 + r)
        R, S = build(50 + r, r, hR, hS)
        expect_k(rhj, r, len(R), len(S), k)
        _EDGE_CACHE[r] = (R, S, names, as_pairs(oracle.join(R, S, r)))
    return _EDGE_CACHE[r]


@pytest.mark.parametrize("r", sorted(EDGE))
def test_ties_chunk_edges_and_a_hot_bucket(rhj, oracle, r):
    """hR == hS (R probes) and hR == hS +- 1 in many buckets; sides of m * 4096 - 1, m * 4096 and m * 4096 + 1 tuples; buckets
    of one tuple, with R or S empty, empty; one hot bucket of 1.2 M S tuples (about 300 probe chunks) against an ordinary
    build side.  k_sb_meta, k_sb_scatter and k_lr_parent must agree on every probe side."""
    R, S, names, want = edge_relations(rhj, oracle, r)
    mask = np.uint64((1 << r) - 1)
    hR = np.bincount((R["value"] & mask).astype(np.int64), minlength=1 << r)
    hS = np.bincount((S["value"] & mask).astype(np.int64), minlength=1 << r)
    assert hR[names["tie"]] == hS[names["tie"]] and hS[names["hot"]] >= 1_000_000 and hR[names["R_empty"]] == 0
    assert ((hR == hS) & (hR > 0)).sum() >= (1 << r) // 8
    join_checked(rhj, oracle, R, S, r, EDGE[r][1], "edges at r=%d" % r, want=want)


def test_bucket_range_shares_on_the_hot_and_empty_buckets(rhj, oracle):
    """Shares at k = 2 whose bounds sit on the hot bucket and on empty buckets: each on the sub-bucket path, together the
    whole result."""
    r = 9
    R, S, names, want = edge_relations(rhj, oracle, r)
    rhj.set_bits(r)
    dR, dS = rhj.to_device(R), rhj.to_device(S)
    h, e, s0 = names["hot"], names["both_empty"], names["S_empty"]
    cuts = sorted({0, h, h + 1, e, e + 1, s0, (1 << r)})
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        t, m = rhj.join_device(dR, dS, bucket_range=(lo, hi))
        check_stats(rhj, r, (lo, hi))
        assert m == t.shape[0]
        parts.append(t.cpu().numpy().view(np.uint64).reshape(-1, 2))
    same(np.concatenate(parts), want, "shares")


# ---- c. the split that does not split ----------------------------------------------------------------------------------
SPLIT = {9: (47_000, 2), 4: (75_000, 2)}


@pytest.mark.parametrize("r", sorted(SPLIT))
@pytest.mark.parametrize("fits", [True, False])
def test_split_that_does_not_split(rhj, oracle, r, fits):
    """Some buckets' keys all share bits [r, r + k): one sub-bucket holds the whole bucket, its siblings are empty.  A build
    side beyond the LDS index there makes the path refuse (the tiled path answers, exact); one that fits stays on the path."""
    base, k = SPLIT[r]
    rng = np.random.default_rng(60 + r)
    nb = 1 << r
    hR = base + rng.integers(-base // 20, base // 20, size=nb)
    hS = hR + rng.integers(-50, 50, size=nb)
    share = {}
    for i, b in enumerate((1, nb // 2 + 1, nb - 2)):
        share[b] = (i % (1 << k), k)
        if fits:
            hR[b], hS[b] = LDS_CAP // 2, LDS_CAP // 2 + 2 * i     # the build side (S on the tie, R where S is bigger) fits the index
        else:
            hR[b] = hS[b] = LDS_CAP + 1000
    R, S = build(70 + r, r, hR, hS, share=share)
    if fits:
        join_checked(rhj, oracle, R, S, r, k, "shared sub-bucket, fits")
    else:
        expect_k(rhj, r, len(R), len(S), k)
        rhj.set_bits(r)
        got, m = dev_pairs(rhj, R, S)
        check_stats(rhj, r, "shared sub-bucket beyond the index", taken=False)
        same(got, as_pairs(oracle.join(R, S, r)), "shared sub-bucket beyond the index")


# ---- d. matches per probe tuple ----------------------------------------------------------------------------------------
MATCH = {9: (47_000, 2), 4: (75_000, 2)}


def match_relations(r, fan, seed):
    """Bucket bR (R probes: hR > hS): one R key appears `fan` times in S.  Bucket bS (S probes): one S key appears `fan`
    times in R.  Everything else is a foreign-key join with a few matches a probe tuple."""
    base, _ = MATCH[r]
    rng = np.random.default_rng(seed)
    nb = 1 << r
    hR = base + rng.integers(-base // 20, base // 20, size=nb)
    hS = hR - 100
    bR, bS = 5, nb - 6
    hS[bS] = hR[bS] + 200
    R, S = build(seed + 1, r, hR, hS)
    mask = np.uint64(nb - 1)
    kR, kS = R["value"], S["value"]
    inR = np.nonzero((kR & mask) == np.uint64(bR))[0]
    inS = np.nonzero((kS & mask) == np.uint64(bR))[0]
    x = kR[inR[0]]
    fresh = random_keys(rng, len(inS), r, np.uint64(bR))
    kS[inS] = np.where(kS[inS] == x, fresh, kS[inS])              # x nowhere in S ...
    kS[inS[1:fan + 1]] = x                                        # ... but `fan` times
    inR = np.nonzero((kR & mask) == np.uint64(bS))[0]
    inS = np.nonzero((kS & mask) == np.uint64(bS))[0]
    y = kR[inR[0]]
    kR[inR[1:fan]] = y                                            # y `fan` times in R
    kS[inS[len(inS) // 2]] = y
    assert (kS == x).sum() == fan and (kR == y).sum() == fan
    return R, S, int(R["row_id"][(kR == x)][0])


@pytest.mark.parametrize("r", sorted(MATCH))
def test_sixteen_matches_accepted_and_capacity(rhj, oracle, r):
    """Exactly 16 matches for one tuple of an R-probing bucket and for one of an S-probing bucket (the count byte keeps 7
    bits): the path takes them, exactly; the capacity protocol on this list — count only, one pair short, a cut inside
    the 16-match run — reports every pair and writes the exact prefix."""
    R, S, xid = match_relations(r, 16, 80 + r)
    want = join_checked(rhj, oracle, R, S, r, MATCH[r][1], "16 matches")
    M = len(want)
    run = np.nonzero(want[:, 0] == np.uint64(xid))[0]
    assert len(run) == 16 and run[-1] - run[0] == 15
    dR, dS = rhj.to_device(R), rhj.to_device(S)
    _, m = rhj.join_device(dR, dS, count_only=True)
    assert m == M
    check_stats(rhj, r, "count only")
    for cap in (M - 1, int(run[0]) + 7):
        got, m = dev_pairs(rhj, dR, dS, capacity=cap)
        assert m == M, cap
        check_stats(rhj, r, "capacity %d" % cap)
        same(got, want[:cap], "capacity %d" % cap)


@pytest.mark.parametrize("r", sorted(MATCH))
def test_seventeen_matches_refused(rhj, oracle, r):
    R, S, _ = match_relations(r, 17, 90 + r)
    expect_k(rhj, r, len(R), len(S), MATCH[r][1])
    rhj.set_bits(r)
    got, m = dev_pairs(rhj, R, S)
    check_stats(rhj, r, "17 matches", taken=False)
    same(got, as_pairs(oracle.join(R, S, r)), "17 matches")


# ---- e. row ids --------------------------------------------------------------------------------------------------------
IDS = {9: (24_000_000, 2), 4: (1_200_000, 2)}
_IDS_CACHE = {}


def id_relations(oracle, r, tmp_path_factory):
    """Foreign keys with positional row ids, their oracle result, and the three saved for child processes.  The result of
    the same keys under other row ids is this one's pairs mapped through them: the order depends on positions alone."""
    if r not in _IDS_CACHE:
        n = IDS[r][0]
        R = oracle.generate(n, 0, 0, 0.0, 111 + r)
        S = oracle.generate(n + n // 7, 1, n, 0.0, 112 + r)
        W = as_pairs(oracle.join(R, S, r))
        d = tmp_path_factory.mktemp("ids%d" % r)
        for name, a in (("R", R), ("S", S), ("W", W)):
            np.save(str(d / (name + ".npy")), a)
        _IDS_CACHE[r] = (R, S, W, str(d))
    return _IDS_CACHE[r]


def relabel(W, idR, idS):
    return np.stack([idR[W[:, 0]], idS[W[:, 1]]], axis=1)


@pytest.mark.parametrize("r", sorted(IDS))
def test_narrow_row_ids_not_positions(rhj, oracle, tmp_path_factory, r):
    """Row ids below 2^32, 2^32 - 1 among them, a bijection of the positions and not the positions: the path takes them."""
    R, S, W, _ = id_relations(oracle, r, tmp_path_factory)
    R, S = R.copy(), S.copy()
    for x, c in ((R, 2654435761), (S, 40503)):
        n = len(x)
        off = (0xFFFFFFFF - (n // 2) * c) % (1 << 32)
        x["row_id"] = ((np.arange(n, dtype=np.uint64) * np.uint64(c) + np.uint64(off)) & np.uint64(0xFFFFFFFF))
    assert R["row_id"].max() == 0xFFFFFFFF and S["row_id"].max() == 0xFFFFFFFF
    join_checked(rhj, oracle, R, S, r, IDS[r][1], "narrow row ids", want=relabel(W, R["row_id"], S["row_id"]))


CHILD = r'''
import importlib, os, sys
import numpy as np
d, r, k, order = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
R0, S0, W = (np.load(os.path.join(d, x + ".npy")) for x in ("R", "S", "W"))
mod = importlib.import_module("sigmod-2018_amd")
rhj = mod.RHJ(device=0)
rhj.set_bits(r)
assert rhj.lib.rhj_sub_bits(r, len(R0), len(S0)) == k, "the relations were built for k = %d" % k
split = "lowradix" if r <= 8 else "subbucket"
WIDE = np.uint64(1 << 40)
for name in order.split(","):
    R, S = R0.copy(), S0.copy()
    nR, nS = len(R), len(S)
    if name == "ends":
        R["row_id"][:10] += WIDE
        S["row_id"][-3:] += WIDE
    elif name == "middle_only":                 # beyond the first and last 2048 row ids k_rowid_sample reads
        R["row_id"][nR // 2:nR // 2 + 5] += WIDE
        S["row_id"][nS // 3] += WIDE
    elif name == "one_in_S":
        S["row_id"][nS // 2] = np.uint64(0xFFFFFFFF00000001)
    want = np.stack([R["row_id"][W[:, 0]], S["row_id"][W[:, 1]]], axis=1)
    t, m = rhj.join_device(rhj.to_device(R), rhj.to_device(S), capacity=len(W))
    got = t.cpu().numpy().view(np.uint64).reshape(-1, 2)
    path = rhj.stats()["path"]
    assert rhj.stats()["radix_bits"] == r, (name, rhj.stats()["radix_bits"])
    assert m == len(W) and got.shape == want.shape and np.array_equal(got, want), (name, path, "differs")
    assert (path == split) == (name == "narrow"), (name, path)
    print(name, path, flush=True)
print("ok")
'''


@pytest.mark.parametrize("r", sorted(IDS))
@pytest.mark.parametrize("order", ["ends,narrow,one_in_S,narrow", "narrow,middle_only,narrow"])
def test_wide_row_ids_in_a_fresh_process(oracle, tmp_path_factory, r, order):
    """Wide row ids leave the split path, exact, whether the sample sees them (at the ends) or only pass 1 does (middle
    only, row_id_overflow); a narrow join after a wide one takes the split path again.  A fresh process each, so the
    process-wide "a join needed 16-byte intermediates" state is known at its first join."""
    _, _, _, d = id_relations(oracle, r, tmp_path_factory)
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "oracle")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    res = subprocess.run([sys.executable, "-c", CHILD, d, str(r), str(IDS[r][1]), order], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0 and b"ok" in res.stdout, (res.stdout.decode()[-800:], res.stderr.decode()[-1500:])


# ---- f. hash collisions in the internal join ---------------------------------------------------------------------------
COLLIDE = {9: (47_000, 2), 4: (75_000, 2)}


@pytest.mark.parametrize("r", sorted(COLLIDE))
def test_colliding_keys_in_one_sub_bucket(rhj, oracle, r):
    """The internal join is k_join_fused<false, true>: FjIndexT<false>, the mix64 form (slot = umulhi(h >> 32, hs), hs = the
    build side).  Planted in sub-bucket (s << r) | b at T = r + k bits, on its build side (S probes bucket b): 600 keys of
    one slot with the clamped tag, probed with 300 absent keys of the same slot and tag; 60 pairs of keys with equal low
    words and different high words that share a slot and a tag."""
    base, k = COLLIDE[r]
    T = r + k
    rng = np.random.default_rng(120 + r)
    nb = 1 << r
    b, s = nb // 3, (1 << k) - 1
    sub = (s << r) | b
    n_c, n_abs, n_pairs, filler = 600, 300, 60, 3000
    bc = n_c + 2 * n_pairs + filler                            # the planted sub-bucket's build count = its slot count
    lo, span = hk.mix64_slot_range(bc // 2, bc)
    cl = hk.mix64_keys(sub, T, n_c + n_abs, lo, span, 0xFFFE, seed=r)
    assert len(cl) == n_c + n_abs
    present, absent = cl[:n_c], cl[n_c:]
    pairs = hk.mix64_lowword_pairs(sub, T, bc, n_pairs, seed=r).reshape(-1)
    mT = np.uint64((1 << T) - 1)
    fill = (rng.integers(0, M64, size=filler, dtype=np.uint64, endpoint=True) & ~mT) | np.uint64(sub)
    others = random_keys(rng, base, r, np.uint64(b))           # the bucket's other sub-buckets
    others = others[((others >> np.uint64(r)) & np.uint64((1 << k) - 1)) != np.uint64(s)]
    Rk = np.concatenate([present, pairs, fill, others])
    assert len(np.unique(Rk)) == len(Rk) and np.all((Rk & mT)[:bc] == np.uint64(sub))
    Sk = rng.permutation(np.concatenate([Rk, present, pairs, absent, Rk[rng.integers(0, len(Rk), size=len(Rk) // 4)]]))
    assert len(Sk) > len(Rk)
    hR = base + rng.integers(-base // 20, base // 20, size=nb)
    R, S = build(130 + r, r, hR, hR + 10, override={b: (rng.permutation(Rk), Sk)})
    join_checked(rhj, oracle, R, S, r, k, "colliding keys in sub-bucket %d" % sub)


# ---- g. partition knobs and entry points -------------------------------------------------------------------------------
def test_without_counting_in_pass_1(rhj, oracle):
    """rhj_set_count_in_pass1(0): pass 2's counts from the digit bytes (k_hist_runs) under the sub-bucket path at k = 2."""
    R, S, want = fk_relations(oracle, 24_000_000, 9)
    rhj.lib.rhj_set_count_in_pass1(0)
    try:
        join_checked(rhj, oracle, R, S, 9, 2, "count_in_pass1 off", want=want)
    finally:
        rhj.lib.rhj_set_count_in_pass1(1)


def test_host_relations_at_k2(rhj, oracle):
    R, S, want = fk_relations(oracle, 24_000_000, 9)
    expect_k(rhj, 9, len(R), len(S), 2)
    rhj.set_bits(9)
    got = as_pairs(rhj.RadixHashJoin(R, S))
    check_stats(rhj, 9, "RadixHashJoin")
    same(got, want, "RadixHashJoin")


MSD_CHILD = r'''
import importlib, os, sys
import numpy as np
d = sys.argv[1]
R, S, W = (np.load(os.path.join(d, x + ".npy")) for x in ("R", "S", "W"))
mod = importlib.import_module("sigmod-2018_amd")
rhj = mod.RHJ(device=0)
rhj.set_bits(9)
assert rhj.lib.rhj_sub_bits(9, len(R), len(S)) == 2
t, m = rhj.join_device(rhj.to_device(R), rhj.to_device(S), capacity=len(W))
got = t.cpu().numpy().view(np.uint64).reshape(-1, 2)
st = rhj.stats()
assert st["path"] == "subbucket" and st["radix_bits"] == 9, (st["path"], st["radix_bits"])
assert m == len(W) and np.array_equal(got, W)
print("ok")
'''


def test_msd_partition_in_a_child(oracle, tmp_path_factory):
    """RHJ_MSD=1 (pass 1 of the r-bit partition on the high bits) under the sub-bucket path at k = 2."""
    _, _, _, d = id_relations(oracle, 9, tmp_path_factory)
    env = dict(os.environ, RHJ_MSD="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "oracle")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    res = subprocess.run([sys.executable, "-c", MSD_CHILD, d], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=300)
    assert res.returncode == 0 and b"ok" in res.stdout, res.stderr.decode()[-1500:]
