"""The inputs of tests/test_gpu_fused_edges.py, built on the CPU: one planted bucket (or a few) that puts a unit of the fused
join on one of its capacity edges, in a thin random background that avoids those buckets.  tests/test_fused_model.py asserts on
the CPU that tests/fused_model.py places every shape in the regime its name states; the device test imports the same builders,
so a shape cannot drift out of its regime unnoticed.

A shape's `expect` is a list with one dict per unit of the planted bucket, attribute of fused_model's unit -> exact value
(or a callable that takes the unit), and `walk` the units of the whole join that k_join_walk takes."""
import functools
from collections import namedtuple

import numpy as np

import fused_model as fm
import hashkeys as hk
from helpers import make_rel

C = fm.constants()
Shape = namedtuple("Shape", "name R S bits knobs b expect walk extra")

# kernel variants: bits, knobs, hash family, one row id >= 2^32
TWO = {"small": 0, "fused": 2}
VARIANTS = {
    "small_res": (8, {}, "h32", False),                            # k_join_fused<true, false> behind the small path's partition
    "small_gather": (8, {"resident": 0}, "mix64", False),          # <false, false>
    "two_res": (9, dict(TWO), "h32", False),                       # two-pass partition, 12-byte tuples: <true, true>
    "two_gather": (9, dict(TWO, resident=0), "mix64", False),      # <false, true>
    "two_res_wide": (9, dict(TWO), "h32", True),                   # the join runs again on 16-byte tuples: <true, false>, two-pass
    "two_gather_wide": (9, dict(TWO, resident=0), "mix64", True),
    "small_res_4": (4, {}, "h32", False),                          # 4 bits: 4096-tuple units (family e only)
    "small_gather_4": (4, {"resident": 0}, "mix64", False),
}
GATHER = ("small_gather", "two_gather", "two_gather_wide")
RESIDENT = ("small_res", "two_res", "two_res_wide")
BOTH = ("small_res", "small_gather", "two_res", "two_gather")
ALL8 = RESIDENT + GATHER                                       # every variant at 8 bits and more


def path_of(variant):
    return "small" if variant.startswith("small") else "fused"


# ---- keys -------------------------------------------------------------------------------------------------------------------
def rand_keys(rng, b, bits, n):
    """n distinct random keys of bucket b (below 2^60)."""
    k = np.unique(rng.integers(0, 1 << (59 - bits), size=n + n // 4 + 16, dtype=np.uint64) << np.uint64(bits) | np.uint64(b))
    assert len(k) >= n
    return rng.permutation(k)[:n]


def h32_clones(base, bits, n, seed):
    """n distinct keys with base's bucket and H32 value: base xor combinations of hashkeys.h32_basis (hashkeys.h32_clones draws
    them without replacement from all 2^(32 - bits) combinations, which costs a permutation of that many)."""
    basis = hk.h32_basis(bits)
    rng = np.random.default_rng(seed)
    combos = np.unique(rng.integers(0, 1 << len(basis), size=2 * n + 16))
    assert len(combos) >= n
    combos = rng.permutation(combos)[:n]
    keys = np.full(n, base, dtype=np.uint64)
    for i, v in enumerate(basis):
        keys[((combos >> i) & 1).astype(bool)] ^= np.uint64(v)
    return keys


def slot_keys(family, b, bits, hs, slot, raw_tags, per, seed):
    """For every raw tag of raw_tags: `per` distinct keys of bucket b in slot `slot` (of hs) with that tag, under the family's hash."""
    out = []
    for i, t in enumerate(raw_tags):
        if family == "mix64":
            lo, span = hk.mix64_slot_range(slot, hs)
            k = hk.mix64_keys(b, bits, per, lo, span, t, seed=seed + i)
        else:
            top = -(-(slot << 16) // hs)                              # the smallest h >> 16 with (h >> 16) * hs >> 16 == slot
            base = hk.h32_keys(b, bits, [(top << 16) | t], 1, seed + i)[0]
            k = h32_clones(int(base), bits, per, seed + i)
        assert len(k) == per and len(np.unique(k)) == per
        s, tg = fm.slot_tag(k, bits, hs, family == "h32")
        assert (s == slot).all() and (tg == t + 1).all()
        out.append(k)
    return out


def off_slot(keys, bits, hs, h32, slots, n):
    """The first n of `keys` that do not fall into one of `slots` at hs."""
    s, _ = fm.slot_tag(keys, bits, hs, h32)
    k = keys[~np.isin(s, np.asarray(slots))]
    assert len(k) >= n
    return k[:n]


def keep_order_mix(rng, segments):
    """One key array out of several: every segment's keys keep their relative order, the segments are mixed at random."""
    arr = np.concatenate([np.asarray(s, dtype=np.uint64) for s in segments])
    sid = np.concatenate([np.full(len(s), i) for i, s in enumerate(segments)])
    pos = rng.permutation(len(arr))
    out = np.empty(len(arr), dtype=np.uint64)
    out[pos[np.lexsort((pos, sid))]] = arr
    return out


def background(rng, bits, nR, nS, avoid):
    """Background keys outside the buckets `avoid`: R's distinct but for a tenth that appear twice, half of S's drawn from R's
    (with replacement) and half fresh, so the background's units have tuples with two and more matches as well."""
    mask = np.uint64((1 << bits) - 1)

    def fresh(n):
        k = np.unique(rng.integers(0, 1 << 60, size=n + n // 4 + 64, dtype=np.uint64))
        k = k[~np.isin(k & mask, np.array(sorted(avoid), dtype=np.uint64))]
        return rng.permutation(k)[:n]

    r = fresh(nR)
    r = np.concatenate([r, r[:nR // 10]])
    s = np.concatenate([r[rng.integers(0, len(r), size=nS // 2)], fresh(nS - nS // 2)])
    return rng.permutation(r), rng.permutation(s)


def assemble(rng, variant, planted, nR=20_000, nS=26_000):
    """R and S: the background and the planted buckets (b, R keys, S keys), whose keys keep the order they are given in."""
    bits, knobs, family, wide = VARIANTS[variant]
    bgR, bgS = background(rng, bits, nR, nS, {b for b, _, _ in planted})
    R = make_rel(keep_order_mix(rng, [bgR] + [x for _, x, _ in planted]))
    S = make_rel(keep_order_mix(rng, [bgS] + [y for _, _, y in planted]))
    if wide:                                                          # one row id beyond 32 bits, on a planted tuple
        i = int(np.nonzero((R["value"] & np.uint64((1 << bits) - 1)) == np.uint64(planted[0][0]))[0][0])
        R["row_id"][i] = np.uint64((1 << 32) + 7)
    return R, S


def shape(name, variant, rng, planted, expect, walk, extra=None, **kw):
    bits, knobs, family, wide = VARIANTS[variant]
    R, S = assemble(rng, variant, planted, **kw)
    return Shape(name, R, S, bits, dict(knobs), planted[0][0], expect, walk, extra or {})


def irregular_cluster(family, b, bits, hs, n_foreign, seed, raw_tag=0x1234, slot=7):
    """K and n_foreign foreign keys of one slot and tag."""
    k = slot_keys(family, b, bits, hs, slot, [raw_tag], 1 + n_foreign, seed)[0]
    return k[0], k[1:]


# ---- a. the overflow buffer --------------------------------------------------------------------------------------------------
OVF_TOTALS = {"ent-1": C.FJ_OVF_ENT - 1, "ent": C.FJ_OVF_ENT, "ent+1": C.FJ_OVF_ENT + 1,
              "cap-1": C.FJ_OVF_CAP - 1, "cap": C.FJ_OVF_CAP, "cap+1": C.FJ_OVF_CAP + 1}


def overflow(variant, which, npatch=0):
    """A gather unit whose probe tuples ask for exactly OVF_TOTALS[which] overflow entries: t16 of them hit keys with 16 copies
    (15 entries each), t2 keys with 2 copies, the last tuple of the unit among the former; npatch irregular tuples (one entry
    each) besides."""
    bits, knobs, family, wide = VARIANTS[variant]
    assert family == "mix64"
    T = OVF_TOTALS[which]
    rng = np.random.default_rng(T * 7 + npatch)
    b = 37
    keys = rand_keys(rng, b, bits, 1000 + 14 + 600 + 3000)
    k16, k2, single, miss = keys[:1000], keys[1000:1014], keys[1014:1614], keys[1614:]
    main = rng.permutation(np.concatenate([np.repeat(k16, 16), np.repeat(k2, 2), single]))
    bc = len(main) + (3 if npatch else 0)
    t16, t2 = divmod(T - npatch, 15)
    probe = [k16[np.arange(t16 - 1) % 1000], k2[:t2], single, miss[rng.integers(0, len(miss), size=bc + 400 - (t16 - 1) - t2 - 600 - npatch - 1)]]
    build = main
    if npatch:
        K, F = irregular_cluster(family, b, bits, bc, 1, seed=T)
        build = np.concatenate([[K], main[:8000], F, main[8000:], [K]])
        probe.append(np.full(npatch, K, dtype=np.uint64))
    probe = np.concatenate([rng.permutation(np.concatenate(probe)), k16[:1]])     # (the unit's last tuple has 16 matches)
    assert len(build) == bc and bc <= len(probe) <= C.FJ_SPAN
    walk = T > C.FJ_OVF_ENT or npatch > C.FJ_PATCH_CAP
    exp = [{"count": len(probe), "bc": bc, "resident": False, "ovf_total": T, "npatch": npatch, "route": "walk" if walk else "stream_ovf"}]
    return shape("overflow-%s-%s" % (which, variant), variant, rng, [(b, probe, build)], exp, int(walk),
                 {"background_ovf": True})


# ---- b. the patch list -------------------------------------------------------------------------------------------------------
def patch_count(variant, n):
    """n irregular tuples: key K twice on the build side, a foreign key of K's slot and tag at a build position between the two
    copies; n probe tuples of K."""
    bits, knobs, family, wide = VARIANTS[variant]
    rng = np.random.default_rng(100 + n)
    b = 91
    keys = rand_keys(rng, b, bits, 5000)
    single, miss = keys[:2000], keys[2000:]
    bc = 2003
    K, F = irregular_cluster(family, b, bits, bc, 1, seed=n)
    build = np.concatenate([[K], single[:900], F, single[900:], [K]])
    probe = rng.permutation(np.concatenate([np.full(n, K, dtype=np.uint64), single, miss[:1000]]))
    walk = n > C.FJ_PATCH_CAP
    exp = [{"bc": bc, "resident": False, "npatch": n, "ovf_total": n, "route": "walk" if walk else "stream_ovf"}]
    return shape("patch-%d-%s" % (n, variant), variant, rng, [(b, probe, build)], exp, int(walk))


def patch_positions(variant):
    """Irregular tuples at the unit's indices 0, 255, 256 and 65 535, with the foreign hit before the first match (rounds 1, 2),
    between the two (rounds 0, 2) and behind the last (rounds 0, 1)."""
    bits, knobs, family, wide = VARIANTS[variant]
    rng = np.random.default_rng(7)
    b = 5
    keys = rand_keys(rng, b, bits, 3000 + 3000)
    single, miss = keys[:3000], keys[3000:]
    bc = 3009
    (ka, fa), (kb_, fb), (kc, fc) = [irregular_cluster(family, b, bits, bc, 1, seed=20 + i, raw_tag=0x2000 + i, slot=11 + i) for i in range(3)]
    # candidates come in descending build position: [F K K] for ka, [K F K] for kb_, [K K F] for kc
    build = np.concatenate([[ka, ka, kb_, fc[0]], single[:1500], [fb[0], kc], single[1500:], [kc, kb_, fa[0]]])
    probe = np.concatenate([single, miss])[rng.integers(0, 6000, size=C.FJ_SPAN)]
    at = {0: ka, 255: kb_, 256: kc, C.FJ_SPAN - 1: kb_}
    for i, k in at.items():
        probe[i] = k

    def rounds(u):
        return [int(u.bm[i]) for i in sorted(at)] == [0b110, 0b101, 0b011, 0b101] and all(u.irregular[i] for i in at)

    exp = [{"count": C.FJ_SPAN, "bc": bc, "npatch": 4, "route": "stream_ovf", "check": rounds}]
    return shape("patch-positions-%s" % variant, variant, rng, [(b, probe, build)], exp, 0)


def patch_round(variant, r):
    """The second match of K found in round r: r - 1 foreign keys of K's slot and tag between K's two copies.  Round 15 stays on
    the patch list, round 16 has no overflow run."""
    bits, knobs, family, wide = VARIANTS[variant]
    rng = np.random.default_rng(200 + r)
    b = 123
    keys = rand_keys(rng, b, bits, 2500)
    single, miss = keys[:1500], keys[1500:]
    bc = 1500 + 2 + r - 1
    K, F = irregular_cluster(family, b, bits, bc, r - 1, seed=r)
    build = np.concatenate([[K], single[:700], F, single[700:], [K]])
    probe = rng.permutation(np.concatenate([np.full(5, K, dtype=np.uint64), single, miss]))
    walk = r > C.FJ_OVF_J
    exp = [{"bc": bc, "npatch": 0 if walk else 5, "route": "walk" if walk else "stream_ovf",
            "check": lambda u: set(int(x) for x in u.bm[u.c == 2][u.fp[u.c == 2]]) == {1 | (1 << r)}}]
    return shape("patch-round%d-%s" % (r, variant), variant, rng, [(b, probe, build)], exp, int(walk))


def patch_mayres(variant="small_res"):
    """Residency on, a planted build side above the resident limit: a gather unit of a MAYRES kernel, where one irregular tuple
    sends the unit to the walk (l. 1312)."""
    bits, knobs, family, wide = VARIANTS[variant]
    rng = np.random.default_rng(31)
    b = 200
    bc = fm.resident_limit() + 53
    keys = rand_keys(rng, b, bits, bc + 1000)
    single, miss = keys[:bc - 3], keys[bc - 3:]
    K, F = irregular_cluster(family, b, bits, bc, 1, seed=3)
    build = np.concatenate([[K], single[:4000], F, single[4000:], [K]])
    probe = rng.permutation(np.concatenate([[K], single, miss[:700]]))
    exp = [{"bc": bc, "resident": False, "npatch": 0, "route": "walk", "check": lambda u: int((u.fp & (u.c >= 2)).sum()) == 1}]
    return shape("patch-mayres-%s" % variant, variant, rng, [(b, probe, build)], exp, 1)


# ---- c. the index build --------------------------------------------------------------------------------------------------------
SLOT_LENGTHS = (16, 17, 64, 65, 1023, 1024, 1025, "bc")
SLOT_FORMS = ("copies", "tags", "same_tag")


def long_slot(variant, n, form):
    """One slot of exactly n entries: one key's copies; three keys with different tags; three keys of one tag, interleaved in
    build position.  n == "bc": the slot is the whole build side.  The probe side asks for every key, so the order of the
    matches (descending build position) shows the ranking."""
    bits, knobs, family, wide = VARIANTS[variant]
    h32 = family == "h32"
    whole = n == "bc"
    n_ = 1500 if whole else n
    rng = np.random.default_rng(n_ * 3 + SLOT_FORMS.index(form))
    b = 66
    nfill = 0 if whole else 500
    bc = n_ + nfill
    hs = max(bc, 64)
    slot = 0 if whole else 9
    if form == "copies":
        ks = slot_keys(family, b, bits, hs, slot, [0x3000], 1, seed=n_)[0]
        parts = [n_]
    elif form == "tags":
        ks = np.concatenate(slot_keys(family, b, bits, hs, slot, [0x3000, 0x3001, 0x2FFF], 1, seed=n_))
        parts = [n_ - 2 * (n_ // 3), n_ // 3, n_ // 3]
    else:
        ks = slot_keys(family, b, bits, hs, slot, [0x3000], 3, seed=n_)[0]
        parts = [n_ - 2 * (n_ // 3), n_ // 3, n_ // 3]
    slot_entries = rng.permutation(np.concatenate([np.full(p, k, dtype=np.uint64) for k, p in zip(ks, parts)]))
    keys = rand_keys(rng, b, bits, 3 * nfill + 2000)
    fill = off_slot(keys[:3 * nfill], bits, hs, h32, [slot], nfill) if nfill else keys[:0]
    miss = keys[3 * nfill:]
    build = keep_order_mix(rng, [slot_entries, fill])
    probe = rng.permutation(np.concatenate([ks, ks, fill, miss[:n_ + 100]]))
    cmax = max(parts)
    if form == "same_tag":
        route = "walk"
    elif family == "h32":
        route = "res_dup"
    else:
        route = "walk" if cmax > C.FJ_OVF_J + 1 else "stream_ovf"
    if form == "same_tag" and not h32 and n_ <= C.FJ_OVF_J + 1:       # every match within round 15: the patch list takes the six tuples
        route = "stream_ovf"
    exp = [{"bc": bc, "hs": hs, "resident": h32, "route": route,
            "check": lambda u: int(u.slot_len[slot]) == n_ and int(u.slot_len.max()) == n_ and int(u.c.max()) == cmax}]
    return shape("slot-%s-%s-%s" % (n, form, variant), variant, rng, [(b, probe, build)], exp, int(route == "walk"))


def many_long_slots(variant):
    """Several slots above 64 entries in one bucket, slot 0 and slot hs - 1 among them: the workgroup ranks them one after the
    other (next = pick + 1)."""
    bits, knobs, family, wide = VARIANTS[variant]
    h32 = family == "h32"
    rng = np.random.default_rng(77)
    b = 12
    lens = {0: 70, 5: 130, 300: 66, None: 100}                      # slot -> copies (None: hs - 1)
    nfill = 400
    bc = nfill + sum(lens.values())
    hs = bc
    slots = [hs - 1 if s is None else s for s in lens]
    ks = [slot_keys(family, b, bits, hs, s, [0x1111], 1, seed=s)[0][0] for s in slots]
    keys = rand_keys(rng, b, bits, 3 * nfill + 1500)
    fill = off_slot(keys[:3 * nfill], bits, hs, h32, slots, nfill)
    build = rng.permutation(np.concatenate([np.full(n, k, dtype=np.uint64) for k, n in zip(ks, lens.values())] + [fill]))
    probe = rng.permutation(np.concatenate([ks, ks, fill, keys[3 * nfill:]]))
    route = "res_dup" if h32 else "walk"
    exp = [{"bc": bc, "hs": hs, "route": route,
            "check": lambda u: [int(u.slot_len[s]) for s in slots] == list(lens.values()) and int((u.slot_len > C.WAVE).sum()) == 4}]
    return shape("slots-many-%s" % variant, variant, rng, [(b, probe, build)], exp, int(route == "walk"))


def build_sizes():
    lim = fm.resident_limit()
    return {"1": 1, "63": 63, "64": 64, "65": 65, "res": lim, "res+1": lim + 1, "cap": C.FUSED_LDS_CAP}


def build_size(variant, which):
    """Build sides of 1, 63, 64 and 65 tuples (the floor of 64 slots), at the residency limit and one above, and of FUSED_LDS_CAP
    tuples, the largest the plan gives the fused path; two of them (from 64 on) are copies of one key."""
    bits, knobs, family, wide = VARIANTS[variant]
    bc = build_sizes()[which]
    rng = np.random.default_rng(bc)
    b = 150
    keys = rand_keys(rng, b, bits, bc + 600)
    build = keys[:bc].copy()
    if bc >= 64:
        build[bc // 2] = build[3]
    probe = rng.permutation(np.concatenate([keys[:bc], keys[:min(bc, 300)], keys[bc:]]))
    hs, fits = fm.geometry(bc)
    res = family == "h32" and fits
    exp = [{"bc": bc, "hs": hs, "resident": res}]
    if which == "res":
        assert fits and not fm.geometry(bc + 1)[1]
    return shape("build-%s-%s" % (which, variant), variant, rng, [(b, probe, build)], exp, None)


# ---- d. resident runs and the count byte ---------------------------------------------------------------------------------------
RUNS = (2, 64, 65, 128, 129, 126, 127, 128, 300)


def runs_clean(variant):
    """Clean runs of 2 .. 300 copies (128 twice: two keys), emitted by fj_emit_res with the exact count from the run."""
    bits, knobs, family, wide = VARIANTS[variant]
    rng = np.random.default_rng(41)
    b = 99
    keys = rand_keys(rng, b, bits, len(RUNS) + 900 + 1500)
    ks, fill, miss = keys[:len(RUNS)], keys[len(RUNS):len(RUNS) + 900], keys[len(RUNS) + 900:]
    build = rng.permutation(np.concatenate([np.repeat(ks, RUNS), fill]))
    probe = rng.permutation(np.concatenate([ks, ks, fill, miss]))
    exp = [{"resident": True, "route": "res_dup", "check": lambda u: sorted(int(x) for x in u.c[u.c >= 2]) == sorted(RUNS + RUNS)
            and not u.fp[u.c >= 2].any()}]
    return shape("runs-clean-%s" % variant, variant, rng, [(b, probe, build)], exp, 0)


def run_foreign(variant, n):
    """A run of n copies with one foreign same-tag entry inside it: fp, the unit walks, and a stashed count of 127 is recounted."""
    bits, knobs, family, wide = VARIANTS[variant]
    rng = np.random.default_rng(300 + n)
    b = 44
    bc = 800 + n + 1
    K, F = irregular_cluster(family, b, bits, bc, 1, seed=n, slot=3)
    fill = off_slot(rand_keys(rng, b, bits, 2400), bits, bc, family == "h32", [3], 800 + 600)
    fill, miss = fill[:800], fill[800:]
    run = np.concatenate([np.full(n // 2, K, dtype=np.uint64), F, np.full(n - n // 2, K, dtype=np.uint64)])
    build = keep_order_mix(rng, [run, fill])
    probe = rng.permutation(np.concatenate([[K, K], fill, miss]))
    exp = [{"bc": bc, "resident": True, "route": "walk",
            "check": lambda u: sorted(int(x) for x in u.c[u.fp]) == [n, n] and set(int(x) for x in u.run_len[u.fp]) == {n + 1}}]
    return shape("run-foreign-%d-%s" % (n, variant), variant, rng, [(b, probe, build)], exp, 1)


def run_late_first(variant, copies, nforeign):
    """A key whose run starts with nforeign >= 64 foreign same-tag entries (they sit at higher build positions): its first match
    is found by the wave step of fj_count_res (the `had` branch)."""
    bits, knobs, family, wide = VARIANTS[variant]
    rng = np.random.default_rng(400 + copies * 100 + nforeign)
    b = 45
    bc = 700 + copies + nforeign
    K, F = irregular_cluster(family, b, bits, bc, nforeign, seed=nforeign + copies, slot=4)
    fill = off_slot(rand_keys(rng, b, bits, 2200), bits, bc, family == "h32", [4], 700 + 500)
    fill, miss = fill[:700], fill[700:]
    build = np.concatenate([fill[:300], np.full(copies, K, dtype=np.uint64), fill[300:], F])
    probe = rng.permutation(np.concatenate([[K, K, K], fill, miss]))
    route = "walk" if copies >= 2 else "stream"
    exp = [{"bc": bc, "resident": True, "route": route,
            "check": lambda u: set(int(x) for x in u.first_round[u.fp & (u.c > 0)]) == {nforeign} and int(u.c[u.fp].max()) == copies}]
    return shape("run-late-%d-%d-%s" % (copies, nforeign, variant), variant, rng, [(b, probe, build)], exp, int(route == "walk"))


ROUND_TOTALS = (63, 64, 65, 127, 128, 129)


def res_rounds(variant):
    """64-tuple rounds of fj_emit_res built one by one (probe tuples 64 r .. 64 r + 63 of the unit): round 0 all 64 lanes with
    100 matches; round 1 only lane 63 with more than one; rounds 2..7 totals of 63, 64, 65, 127, 128 and 129 pairs; round 8
    lanes 3, 17 and 40 with runs of 200, 300 and 70 at once, and round 9 lane 3 again (another tuple of the same lane)."""
    bits, knobs, family, wide = VARIANTS[variant]
    rng = np.random.default_rng(55)
    b = 70
    sizes = {"k100": 100, "k5": 5, "k200": 200, "k300": 300, "k70": 70}
    for t in ROUND_TOTALS:
        sizes["t%d" % t] = t - 62
    keys = rand_keys(rng, b, bits, len(sizes) + 600 + 1500)
    k = dict(zip(sizes, keys[:len(sizes)]))
    fill, miss = keys[len(sizes):len(sizes) + 600], keys[len(sizes) + 600:]
    build = rng.permutation(np.concatenate([np.full(n, k[name], dtype=np.uint64) for name, n in sizes.items()] + [fill]))
    rounds = [np.full(64, k["k100"], dtype=np.uint64), np.concatenate([fill[:63], [k["k5"]]])]
    for t in ROUND_TOTALS:
        r = np.concatenate([fill[100:162], [k["t%d" % t]], miss[:1]])
        rounds.append(r)
    r8 = fill[200:264].copy(); r8[3], r8[17], r8[40] = k["k200"], k["k300"], k["k70"]
    r9 = miss[10:74].copy(); r9[3] = k["k300"]
    rounds += [r8, r9]
    probe = np.concatenate(rounds + [rng.permutation(np.concatenate([fill, miss]))])
    want_tot = [6400, 68] + list(ROUND_TOTALS) + [64 - 3 + 570, 300]

    def check(u):
        tot = [int(u.c[64 * r:64 * r + 64].sum()) for r in range(10)]
        return tot == want_tot and int((u.c[64:128] > 1).sum()) == 1 and u.c[127] == 5 and (u.c[:64] == 100).all()

    exp = [{"resident": True, "route": "res_dup", "check": check}]
    return shape("res-rounds-%s" % variant, variant, rng, [(b, probe, build)], exp, 0)


GATHER_MANY = (17, 126, 127, 128, 300)


def gather_many(variant, n):
    """A probe tuple with n > 16 matches on the gather path: the unit walks, counts from 127 on are recounted through G.load."""
    bits, knobs, family, wide = VARIANTS[variant]
    rng = np.random.default_rng(500 + n)
    b = 18
    keys = rand_keys(rng, b, bits, 1 + 700 + 1200)
    K, fill, miss = keys[0], keys[1:701], keys[701:]
    build = rng.permutation(np.concatenate([np.full(n, K, dtype=np.uint64), fill]))
    probe = rng.permutation(np.concatenate([[K, K], fill, miss]))
    exp = [{"resident": False, "route": "walk", "ovf_total": 2 * (n - 1), "check": lambda u: int(u.c.max()) == n}]
    return shape("gather-many-%d-%s" % (n, variant), variant, rng, [(b, probe, build)], exp, 1)


# ---- e. units and groups -------------------------------------------------------------------------------------------------------
UNIT_SIZES = (1, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, 2 * 65536 + 1)
UNIT_SIZES_4 = (4095, 4096, 4097, 3 * 4096 + 1)


def unit_sizes(variant, pc):
    """A bucket whose probe side has pc tuples, every fourth of them (and the first tuple of every unit but the first) with two
    matches: ceil(pc / span) units, the multi-match tuples include a unit's last tuple and the next one's first."""
    bits, knobs, family, wide = VARIANTS[variant]
    rng = np.random.default_rng(pc * 5 + bits)
    b = 3
    nd = min(300, pc // 8)
    keys = rand_keys(rng, b, bits, 2 * nd + 1 + 300)
    dup, single, miss = keys[:nd], keys[nd:2 * nd + 1], keys[2 * nd + 1:]
    build = rng.permutation(np.concatenate([dup, dup, single]))
    others = np.concatenate([single, miss])
    probe = others[rng.integers(0, len(others), size=pc)]
    if nd:
        i4 = np.arange(3, pc, 4)
        probe[i4] = dup[rng.integers(0, nd, size=len(i4))]
    nbg = (3000, 4000) if bits == 4 else (20_000, 26_000)
    span = 4096 if bits == 4 else C.FJ_SPAN
    if nd:
        for first in range(span, pc, span):
            probe[first] = dup[0]
    nunits = -(-pc // span)
    exp = [{"off": i * span, "count": min(span, pc - i * span), "bc": 2 * nd + len(single)} for i in range(nunits)]
    if nd:
        for i in range(nunits):
            exp[i]["check"] = (lambda i: lambda u: (i == 0 or u.c[0] == 2) and (u.count < span or u.c[span - 1] == 2))(i)
    return shape("units-%d-%s" % (pc, variant), variant, rng, [(b, probe, build)], exp, 0, {"span": span}, nR=nbg[0], nS=nbg[1])


# ---- f. deferred emit and the double buffer ---------------------------------------------------------------------------------
KINDS = ("none", "fk", "ovf", "irregular", "m17", "resdup", "empty")


def kind_bucket(rng, family, b, bits, kind, side_max):
    """(probe keys, build keys) of one bucket of the given kind; the probe side is the bigger one."""
    nb = int(rng.integers(side_max // 4, side_max // 2))
    extra = int(rng.integers(1, side_max // 2))
    keys = rand_keys(rng, b, bits, 3 * side_max)
    fill, miss = keys[:nb], keys[nb:]
    build = [fill]
    hits = []
    if kind == "ovf":
        build.append(fill[:10]); hits = [fill[:10]]
    elif kind == "m17":
        build.append(np.full(16, fill[0], dtype=np.uint64)); hits = [fill[:1]]
    elif kind == "resdup":
        build.append(np.full(39, fill[1], dtype=np.uint64)); hits = [fill[1:2]] * 3
    bld = rng.permutation(np.concatenate(build))
    if kind == "irregular":
        bc = nb + 3
        K, F = irregular_cluster(family, b, bits, max(bc, 64), 1, seed=b)
        bld = np.concatenate([[K], fill[:nb // 2], F, fill[nb // 2:], [K]])
        hits = [np.array([K, K], dtype=np.uint64)]
    if kind == "none":
        probe = miss[:len(bld) + extra]
    elif kind == "empty":
        return miss[:nb], miss[:0]
    else:
        nh = sum(len(h) for h in hits)
        probe = rng.permutation(np.concatenate(hits + [fill[rng.integers(0, nb, size=len(bld) + extra - nh - 5)], miss[:5]]))
    assert len(probe) > len(bld) and len(probe) <= side_max + 60
    return probe, bld


def kinds_join(bits, resident, seed, side_max, kinds=None):
    """Every bucket of the radix populated, its kind drawn from KINDS; which relation probes is drawn as well."""
    family = "h32" if resident else "mix64"
    rng = np.random.default_rng(seed)
    bins = 1 << bits
    if kinds is None:
        kinds = [KINDS[i] for i in rng.integers(0, len(KINDS), size=bins)]
    Rs, Ss = [], []
    for b in range(bins):
        probe, build = kind_bucket(rng, family, b, bits, kinds[b], side_max)
        r, s = (probe, build) if rng.integers(0, 2) else (build, probe)
        Rs.append(r); Ss.append(s)
    return make_rel(keep_order_mix(rng, Rs)), make_rel(keep_order_mix(rng, Ss)), kinds


def deferred(resident):
    knobs = dict(TWO)
    if not resident:
        knobs["resident"] = 0
    R, S, kinds = kinds_join(10, resident, 5 + resident, 300)
    return Shape("deferred-%s" % ("res" if resident else "gather"), R, S, 10, knobs, 0, None, None, {"kinds": kinds})


def unit_kinds(kinds):
    return [k for k in kinds if k != "empty"]


def pairs_at(kinds, d):
    u = unit_kinds(kinds)
    return {(u[i], u[i + d]) for i in range(len(u) - d)}


def deferred_batch(resident, njoins=3):
    """The same mix on 8 bits, njoins joins of one batch: four workgroups a join take the units in turn, a workgroup's next unit
    is the one 1 to BJ_WGS places behind.  The seeds are the first ones whose kinds have every ordered pair at each distance."""
    want = {(a, b) for a in KINDS[:-1] for b in KINDS[:-1]}
    out, seed = [], 1000 * (1 + resident)
    while len(out) < njoins:
        seed += 1
        kinds = [KINDS[i] for i in np.random.default_rng(seed).integers(0, len(KINDS), size=256)]
        if all(pairs_at(kinds, d) == want for d in range(1, C.BJ_WGS + 1)):
            out.append(kinds_join(8, resident, seed, 100, kinds))
    return out


# ---- g. the speculation -----------------------------------------------------------------------------------------------------
SPEC_BITS = 9
SPEC_B = 301


@functools.lru_cache(maxsize=1)
def spec_background():
    """A primary-key R of 1.2 M keys and a foreign-key S of 2.2 M, outside bucket SPEC_B."""
    rng = np.random.default_rng(99)
    k = np.unique(rng.integers(0, 1 << 60, size=1_300_000, dtype=np.uint64))
    k = rng.permutation(k[(k & np.uint64((1 << SPEC_BITS) - 1)) != np.uint64(SPEC_B)])[:1_200_000]
    return k, k[rng.integers(0, len(k), size=2_200_000)]


SPEC_KINDS = ("rec511", "rec512", "rec513", "lookback", "split", "totals")


def spec_planted(kind, rng):
    """(R keys, S keys) of bucket SPEC_B, which R probes, and what the speculation does on it."""
    b, bits = SPEC_B, SPEC_BITS
    if kind.startswith("rec"):
        n = int(kind[3:])
        r = rand_keys(rng, b, bits, 3000)
        mult = np.zeros(3000, dtype=np.int64)
        mult[:256] = 1; mult[512:1256] = 1
        mult[256:511] = 3                                            # group 1: 255 tuples with two records each
        mult[511] = n - 510 + 1
        return r, rng.permutation(np.repeat(r, mult)), {"records": (1, n), "last_spec": 1}
    if kind == "lookback":
        r = rand_keys(rng, b, bits, 34_000)
        mult = np.zeros(len(r), dtype=np.int64)
        mult[:30_000] = 1
        mult[np.arange(133) * 256 + 7] = 2
        return r, rng.permutation(np.repeat(r, mult)), {"groups": 133, "last_spec": 1}
    if kind == "split":
        r = rand_keys(rng, b, bits, C.FJ_SPAN + 500)
        return r, rng.permutation(r[:3000]), {"units": 2, "last_spec": 2}
    r = rand_keys(rng, b, bits, 3001)                                 # totals: one S tuple with two partners, one with none
    R = np.concatenate([r[:3000], r[:1]])
    return R, rng.permutation(np.concatenate([r[:2000], r[3000:]])), {"last_spec": 1}


def spec(kind, resident):
    rng = np.random.default_rng(SPEC_KINDS.index(kind))
    bgR, bgS = spec_background()
    pr, ps, extra = spec_planted(kind, rng)
    R = make_rel(keep_order_mix(rng, [bgR, pr]))
    S = make_rel(keep_order_mix(rng, [bgS, ps]))
    knobs = {"spec": 1}
    if not resident:
        knobs["resident"] = 0
    walk = 1 if (kind == "rec513" and not resident) else 0
    return Shape("spec-%s-%s" % (kind, "res" if resident else "gather"), R, S, SPEC_BITS, knobs, SPEC_B, None, walk, extra)


# ---- the cases: id -> (family, builder, arguments); both test files run every one --------------------------------------------
CASES = {}


def _reg(fam, fn, *args):
    CASES["%s:%s(%s)" % (fam, fn.__name__, ",".join(str(a) for a in args))] = (fn, args)


for _v in GATHER:
    for _w in OVF_TOTALS:
        _reg("a", overflow, _v, _w)
    for _n in (C.FJ_PATCH_CAP - 1, C.FJ_PATCH_CAP, C.FJ_PATCH_CAP + 1):
        _reg("b", patch_count, _v, _n)
    _reg("b", overflow, _v, "ent", C.FJ_PATCH_CAP)
    _reg("b", patch_positions, _v)
    for _r in (C.FJ_OVF_J, C.FJ_OVF_J + 1):
        _reg("b", patch_round, _v, _r)
    for _n in GATHER_MANY:
        _reg("d", gather_many, _v, _n)
for _v in RESIDENT:
    _reg("b", patch_mayres, _v)
for _v in ALL8:
    for _n in SLOT_LENGTHS:
        for _f in SLOT_FORMS:
            _reg("c", long_slot, _v, _n, _f)
    for _w in build_sizes():
        _reg("c", build_size, _v, _w)
    _reg("c", many_long_slots, _v)
for _v in RESIDENT:
    _reg("d", runs_clean, _v)
    for _n in sorted(set(RUNS)):
        _reg("d", run_foreign, _v, _n)
    for _c, _nf in ((1, 64), (1, 70), (5, 64)):
        _reg("d", run_late_first, _v, _c, _nf)
    _reg("d", res_rounds, _v)
for _v in VARIANTS:
    for _pc in (UNIT_SIZES_4 if _v.endswith("_4") else UNIT_SIZES):
        _reg("e", unit_sizes, _v, _pc)


def build(case_id):
    fn, args = CASES[case_id]
    return fn(*args)
