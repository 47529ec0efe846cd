"""The tiled join path's plan (sigmod-2018_amd/csrc/rhj_join_tiled.hip.h: plan_body, lds_slots_for; rhj_device.hip: join_setup,
join_tiled) restated in Python, with its constants read from the sources by regular expression.  Nothing here imports the
library: tests/test_tiled_model.py checks the restatement on the CPU, tests/test_gpu_tiled_edges.py builds its cases on the
edges this module derives and compares rhj_last_stats() with plan()'s totals.  A changed constant moves the edges with it.

What the plan decides per bucket b with cR, cS > 0 tuples:
  side    S probes ("flip") when cR < cS, R probes when cR >= cS (rhjoin.c:86); pc = the probe side's size, bc = the build side's
  mode    1 (32-bit table built in LDS, lds_slots_for(bc) slots and T32_PAD replica entries behind them) when bc <= lds_cap,
          2 (64-bit table in HBM of 2^lg slots, 2^lg the power of two >= 2 bc, built by ceil(bc / BUILD_CHUNK) build units)
  units   ceil(pc / PR_UNIT) probe units
lds_cap is tiled_cap (the plan was made for the tiled path: rhj_set_fused(0), tiny buckets), fused_cap (the fused or small
path handed over) or forced_cap (rhj_set_force_hbm_table(1))."""
import os
import re
from collections import namedtuple

import numpy as np

from source_constants import c_int as _c_int, one as _one

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sigmod-2018_amd", "csrc")
SOURCES = ("rhj_join_fused.hip.h", "rhj_join_tiled.hip.h", "rhj_device.hip")      # in include order


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


Constants = namedtuple("Constants", "LDS_BUDGET FJ_LDS_EXTRA FUSED_LDS LDS_MAX_SLOTS FUSED_LDS_CAP BUILD_CHUNK PR_UNIT T32_PAD "
                                    "SLOT_FLOOR SLOT_ADD SLOT_GRANULE SCAN_BLOCK tiled_cap fused_cap forced_cap")


def parse_constants(read=_read):
    """The constants of the tiled path from the sources (`read(name)` returns a source file's text)."""
    text = {n: read(n) for n in SOURCES}
    names = {}
    for n in SOURCES:                                    # every integer constexpr, in source order: later ones use earlier ones
        for m in re.finditer(r"constexpr\s+(?:int|uint32_t|uint64_t|size_t)\s+(\w+)\s*=\s*([^;]+);", text[n]):
            try:
                names[m.group(1)] = _c_int(m.group(2), names)
            except (ValueError, NameError, SyntaxError, TypeError, ZeroDivisionError):
                pass                                     # (casts, sizeof, names of other headers: nothing the plan uses)
    dev, tiled = text["rhj_device.hip"], text["rhj_join_tiled.hip.h"]
    # join_setup: lds_cap = want_fused ? FUSED_LDS_CAP : force_hbm ? 0 : LDS_MAX_SLOTS * 4 / 5
    m = _one(r"lds_cap\s*=\s*s\.want_fused\s*\?\s*([^:;]+?)\s*:\s*g\.force_hbm\s*\?\s*([^:;]+?)\s*:\s*([^;]+);", dev, "join_setup's lds_cap")
    fused_cap, forced_cap, tiled_cap = (_c_int(x, names) for x in m.groups())
    # lds_slots_for: s = bc + (bc >> 1) + ADD; s = (s + G - 1) & ~(G - 1); min(max(s, FLOOR), max_slots)
    body = _one(r"(?s)lds_slots_for\s*\([^)]*\)\s*\{(.*?)\n\}", re.sub(r"//[^\n]*", "", tiled), "lds_slots_for").group(1)
    body = " ".join(body.split())
    add = int(_one(r"\(bc \+ \(bc >> 1\)\) \+ (\d+)u;", body, "lds_slots_for's constant").group(1))
    g = _one(r"s = \(s \+ (\d+)u\) & ~(\d+)u;", body, "lds_slots_for's granule")
    if g.group(1) != g.group(2):
        raise AssertionError("lds_slots_for rounds with two different masks")
    floor = int(_one(r"return min\(max\(s, (\d+)u\), max_slots\);", body, "lds_slots_for's floor").group(1))
    # launch_offsets: counts a scan block
    sb = _one(r"nblocks = \(uint32_t\)\(\(max_n \+ (\d+)\) / (\d+) \?", dev, "launch_offsets' block")
    if int(sb.group(1)) + 1 != int(sb.group(2)):
        raise AssertionError("launch_offsets rounds with two different block sizes")
    need = ("LDS_BUDGET", "FJ_LDS_EXTRA", "FUSED_LDS", "LDS_MAX_SLOTS", "FUSED_LDS_CAP", "BUILD_CHUNK", "PR_UNIT", "T32_PAD")
    missing = [n for n in need if n not in names]
    if missing:
        raise AssertionError("tests/tiled_model.py no longer finds %s in the sources" % missing)
    return Constants(*[names[n] for n in need], floor, add, int(g.group(1)) + 1, int(sb.group(2)), tiled_cap, fused_cap, forced_cap)


_CONSTANTS = None


def constants():
    global _CONSTANTS
    if _CONSTANTS is None:
        _CONSTANTS = parse_constants()
    return _CONSTANTS


def lds_slots_for(bc, c=None):
    c = c or constants()
    s = bc + (bc >> 1) + c.SLOT_ADD
    s = (s + c.SLOT_GRANULE - 1) & ~(c.SLOT_GRANULE - 1)
    return min(max(s, c.SLOT_FLOOR), c.LDS_MAX_SLOTS)


def tab64_lg(bc):
    """log2 of a 64-bit table's slot count: the power of two >= 2 bc (64 - clzll(2 bc - 1))"""
    return (2 * bc - 1).bit_length()


def last_floor_build(c=None):
    """The largest build side whose 32-bit table has the floor's slots (one more tuple: one granule more)."""
    c = c or constants()
    bc = 1
    while lds_slots_for(bc + 1, c) == c.SLOT_FLOOR:
        bc += 1
    return bc


def first_full_build(c=None):
    """The smallest build side whose 32-bit table has LDS_MAX_SLOTS slots: from here on tables stop growing."""
    c = c or constants()
    bc = (c.LDS_MAX_SLOTS - c.SLOT_ADD - c.SLOT_GRANULE) * 2 // 3 - 2
    assert lds_slots_for(bc, c) < c.LDS_MAX_SLOTS
    while lds_slots_for(bc, c) < c.LDS_MAX_SLOTS:
        bc += 1
    return bc


def first_clamped_build(c=None):
    """The smallest build side for which lds_slots_for's min() cuts: bc + bc / 2 + SLOT_ADD, rounded up, is beyond LDS_MAX_SLOTS."""
    c = c or constants()
    bc = first_full_build(c)
    while ((bc + (bc >> 1) + c.SLOT_ADD + c.SLOT_GRANULE - 1) & ~(c.SLOT_GRANULE - 1)) <= c.LDS_MAX_SLOTS:
        bc += 1
    return bc


Plan = namedtuple("Plan", "flip pc bc mode slots lg units_of build_units_of units hbm_units max_build table_slots tab32_slots "
                          "hbm_slots lds_buckets")


def plan(histR, histS, lds_cap, c=None):
    """plan_body over two histograms.  Per bucket (arrays of len(histR); 0 where a side is empty): flip, pc, bc, mode, slots
    (mode 1), lg (mode 2), units_of, build_units_of.  Totals as rhj_last_stats() reports them after a tiled join: units,
    hbm_units, max_build, table_slots (= tab32_slots + hbm_slots)."""
    c = c or constants()
    cR, cS = (np.asarray(h, dtype=np.int64) for h in (histR, histS))
    assert cR.shape == cS.shape
    n = len(cR)
    flip = np.zeros(n, dtype=bool)
    pc, bc, mode, slots, lg, nu, nbu = (np.zeros(n, dtype=np.int64) for _ in range(7))
    for b in range(n):
        r, s = int(cR[b]), int(cS[b])
        if r == 0 or s == 0:
            continue
        flip[b] = r < s
        pc[b], bc[b] = (s, r) if flip[b] else (r, s)
        nu[b] = -(-int(pc[b]) // c.PR_UNIT)
        if bc[b] <= lds_cap:
            mode[b], slots[b] = 1, lds_slots_for(int(bc[b]), c)
        else:
            mode[b], lg[b] = 2, tab64_lg(int(bc[b]))
            nbu[b] = -(-int(bc[b]) // c.BUILD_CHUNK)
    tab32 = int((slots[mode == 1] + c.T32_PAD).sum())
    hbm = int(sum(1 << int(x) for x in lg[mode == 2]))
    return Plan(flip, pc, bc, mode, slots, lg, nu, nbu, int(nu.sum()), int(nbu.sum()), int(bc.max()) if n else 0, tab32 + hbm,
                tab32, hbm, int((mode == 1).sum()))


def histograms(R_keys, S_keys, bits):
    mask = np.uint64((1 << bits) - 1)
    return tuple(np.bincount((np.asarray(k, dtype=np.uint64) & mask).astype(np.int64), minlength=1 << bits) for k in (R_keys, S_keys))


def tab32_arena_bound(nR, nS, bits):
    """join_tiled's allocation for the 32-bit tables, in entries: nmin + nmin / 2 + 80 bins + 64"""
    nmin = min(int(nR), int(nS))
    return nmin + nmin // 2 + 80 * (1 << bits) + 64


def xcd_deal(nu, per=None):
    """k_probe's unit of every workgroup x of its grid of ceil(nu / 8) * 8 (None: the workgroup returns at once): XCD x & 7 takes
    the (x & 7)-th run of per = ceil(nu / 8) units."""
    per = (nu + 7) // 8 if per is None else per
    out = []
    for x in range((nu + 7) // 8 * 8):
        u = (x & 7) * per + (x >> 3)
        out.append(None if (x >> 3) >= per or u >= nu else u)
    return out


# ---- relations with exact bucket sizes, and the cases of tests/test_gpu_tiled_edges.py ------------------------------------
def bucket_keys(rng, b, bits, n):
    """n distinct keys of bucket b: (distinct random word << bits) | b"""
    w = np.zeros(0, dtype=np.uint64)
    while len(w) < n:
        w = np.unique(np.concatenate([w, rng.integers(1 << 20, 1 << (62 - bits), size=n + 64, dtype=np.uint64)]))
    return (rng.permutation(w)[:n] << np.uint64(bits)) | np.uint64(b)


def sized_bucket(rng, b, bits, cR, cS, dup=0.02, hit=0.6):
    """Keys of bucket b, exactly cR for R and cS for S.  The build side (R when cR < cS, as the plan chooses) is distinct keys
    but for a share `dup` of repeats; a share `hit` of the probe side is drawn from the build keys, the rest is absent keys."""
    nb, npr = (cR, cS) if cR < cS else (cS, cR)
    nd = min(int(nb * dup), nb - 1) if nb > 1 else 0
    keys = bucket_keys(rng, b, bits, (nb - nd) + npr)
    base, absent = keys[:nb - nd], keys[nb - nd:]
    build = rng.permutation(np.concatenate([base, base[rng.integers(0, len(base), size=nd)]]))
    take = rng.random(npr) < hit
    probe = np.where(take, base[rng.integers(0, len(base), size=npr)], absent)
    return (build, probe) if cR < cS else (probe, build)


def sized_relations(rng, bits, sizes, **kw):
    """sizes: {bucket: (cR, cS)}.  Returns the shuffled key columns of R and S."""
    rk, sk = [np.zeros(0, dtype=np.uint64)], [np.zeros(0, dtype=np.uint64)]
    for b, (cR, cS) in sorted(sizes.items()):
        r, s = sized_bucket(rng, b, bits, cR, cS, **kw)
        rk.append(r)
        sk.append(s)
    return rng.permutation(np.concatenate(rk)), rng.permutation(np.concatenate(sk))


def build_edges(cap, c=None):
    """(a): the build sides on lds_slots_for's floor and clamp and around a route's lds_cap"""
    c = c or constants()
    f, full = last_floor_build(c), first_full_build(c)
    return [1, f, f + 1, full, full + 1, cap - 1, cap, cap + 1]


def sides_by_parity(builds, c=None):
    """Bucket i's build side is R's for even i and S's for odd i; the probe side has 1, PR_UNIT - 1 or PR_UNIT + 1 tuples more."""
    c = c or constants()
    extra = (1, c.PR_UNIT - 1, c.PR_UNIT + 1)
    out = {}
    for i, bc in enumerate(builds):
        pc = bc + extra[i % 3]
        out[i] = (bc, pc) if i % 2 == 0 else (pc, bc)
    return out


def sides_with_ties(builds, c=None):
    """As sides_by_parity with the sides swapped, and two buckets (the second and the last but one) with cR == cS: R probes."""
    out = {i: (s, r) for i, (r, s) in sides_by_parity(builds, c).items()}
    for i in (1, len(builds) - 2):
        out[i] = (builds[i], builds[i])
    return out


def chunk_edges(c=None):
    """(b): build sides around one and two build chunks and around the 16-bit position limit of a 32-bit table's entries"""
    c = c or constants()
    k = c.BUILD_CHUNK
    return [k - 1, k, k + 1, 2 * k, 2 * k + 1, 65534, 65535, 65536]


def probe_edges(c=None):
    """(b): (cR, cS) with probe sides of exactly 1, PR_UNIT - 1, PR_UNIT, PR_UNIT + 1, 2 PR_UNIT, 2 PR_UNIT + 1"""
    c = c or constants()
    u = c.PR_UNIT
    return {0: (1, 1), 1: (100, u - 1), 2: (u, u), 3: (u + 1, u), 4: (2 * u, 2 * u), 5: (u + 5, 2 * u + 1), 6: (u - 1, 3)}


def unit_total_sizes(units, bits=4, c=None):
    """(b): tiny buckets, `units` probe units in all (one a bucket, the first bucket PR_UNIT + 1 probe tuples when there are
    more units than buckets)"""
    c = c or constants()
    bins = 1 << bits
    assert 1 <= units <= bins + 1
    sizes = {b: (1 + b % 3, 1 + (b + 1) % 3) for b in range(min(units, bins))}
    if units > bins:
        sizes[0] = (c.PR_UNIT + 1, 5)
    return sizes


def scan_block_keys(n_buckets, bits, extra_unit=False, c=None):
    """(c): the first n_buckets buckets hold one key on both sides, 1..3 times a side — 1, 2, 3, 4, 6 or 9 pairs, neighbours
    different — so every bucket is one unit with a count of its own; the buckets behind them hold a tuple on one side or none.
    extra_unit: bucket 0 gets PR_UNIT more probe tuples without a partner (one more unit)."""
    c = c or constants()
    bins = 1 << bits
    assert n_buckets <= bins
    reps = [(1, 1), (2, 1), (3, 1), (2, 2), (3, 2), (3, 3), (1, 2), (1, 3), (2, 3)]
    rk, sk = [], []
    for b in range(bins):
        key = ((b * 7919 + 12345) << bits) | b
        if b < n_buckets:
            r, s = reps[b % len(reps)]
            rk += [key] * r
            sk += [key] * s
        elif b % 3 == 0:
            rk.append(key)
        elif b % 3 == 1:
            sk.append(key)
    if extra_unit:
        rk += [((1 << 40) + (i << bits)) for i in range(c.PR_UNIT)]
    return np.array(rk, dtype=np.uint64), np.array(sk, dtype=np.uint64)


# ---- (d) clusters homed in a table's last slots ----------------------------------------------------------------------------
WRAP_SIZES = ((1, False), (4, False), (5, False), (8, False), (9, False), (13, False), (5, True), (9, True))   # (distinct keys, one of them three times)
WRAP_LOW = ((0, +0x100), (0, -0x100), (1, -0x100), (2, +0x100), (3, -0x100), (3, +1))   # (home slot, tag - the cluster's tag) of the keys behind the wrap
WRAP_ABSENT = 3                        # absent keys of the cluster's home and tag


def _keys_at(table, b, bits, n, home, size, tag, seed):
    """n distinct keys of bucket b homed at slot `home` of a 32-bit table of `size` slots with 16-bit tag `tag`, or of a 64-bit
    table of 2^size slots with 32-bit tag `tag`"""
    import hashkeys as hk
    if table == 32:
        k = hk.mix64_keys(b, bits, n, *hk.mix64_slot_range(home, size), tag, seed=seed)
    else:
        k = hk.mix64_keys(b, bits, n, top_lo=home << (32 - size), top_span=1 << (32 - size), tag16=0, seed=seed, low32=tag)
    assert len(k) == n, "only %d of %d keys" % (len(k), n)
    return k


def table_of(table, bc, c=None):
    """(what _keys_at calls size, the slot count) of the table a build side of bc tuples gets"""
    if table == 32:
        s = lds_slots_for(bc, c)
        return s, s
    lg = tab64_lg(bc)
    return lg, 1 << lg


def wrap_cluster(table, b, bits, j, size, dup, filler, seed, c=None):
    """The planted bucket of case (d) for a table kind (32 / 64): R's keys (the build side) and S's (the probe side).
    Build: `size` distinct keys homed at slot slots - 1 - j with one tag (the first three times when dup), the WRAP_LOW keys
    homed at slots 0..3 with tags above and below it, `filler` random keys.  Probe: every build key, every second twice,
    WRAP_ABSENT absent keys of the cluster's home and tag, and absent keys of that home with the smallest and the largest tag
    and with the tags next to the cluster's.  Returns a dict with those parts, the home and the table's size."""
    rng = np.random.default_rng(seed)
    bc = size + (2 if dup else 0) + len(WRAP_LOW) + filler
    tsize, slots = table_of(table, bc, c)
    home = slots - 1 - j
    tag, tmax = (0x8000, 0xFFFF) if table == 32 else (0x80000000, 0xFFFFFFFF)
    same = _keys_at(table, b, bits, size + WRAP_ABSENT, home, tsize, tag, seed)
    cluster, absent_same = same[:size], same[size:]
    low = np.concatenate([_keys_at(table, b, bits, 1, h, tsize, tag + d, seed + 10 + i) for i, (h, d) in enumerate(WRAP_LOW)])
    other = np.concatenate([_keys_at(table, b, bits, 2, home, tsize, t, seed + 20 + i) for i, t in enumerate((0, tmax, tag + 1, tag - 1))])
    fill = bucket_keys(rng, b, bits, filler)
    build = np.concatenate([cluster, np.repeat(cluster[:1], 2 if dup else 0), low, fill])
    assert len(build) == bc and len(np.unique(np.concatenate([cluster, absent_same, low, other, fill]))) == size + WRAP_ABSENT + len(low) + len(other) + filler
    for keys, homes, tags in ((same, home, tag), (low, [h for h, _ in WRAP_LOW], [tag + d for _, d in WRAP_LOW]),
                              (other, home, np.repeat([0, tmax, tag + 1, tag - 1], 2))):
        assert np.array_equal(table_home(table, keys, tsize), np.broadcast_to(np.uint64(homes), keys.shape)), "home"
        assert np.array_equal(_tag(table, keys), np.broadcast_to(np.uint64(tags), keys.shape)), "tag"
        assert np.all((keys & np.uint64((1 << bits) - 1)) == np.uint64(b))
    present = np.unique(build)
    probe = rng.permutation(np.concatenate([present, present[::2], absent_same, other, other[:3]]))
    assert len(probe) > bc                                    # S probes the bucket
    return dict(R=rng.permutation(build), S=probe, cluster=cluster, absent_same=absent_same, low=low, other=other, home=home,
                tsize=tsize, slots=slots, bc=bc, tag=tag)


# ---- (e) match counts at the stash's limits ---------------------------------------------------------------------------------
STASH_REPEATS = (1, 2, 16, 17, 254, 255, 256, 257, 300)


def table_home(table, keys, tsize):
    """the home slot of keys in a 32-bit table of tsize slots (t32_home) or a 64-bit table of 2^tsize slots (Tab64::home)"""
    import hashkeys as hk
    h = hk.mix64(keys)
    return hk.mix_slot(h, tsize) if table == 32 else hk.tab64_home(h, tsize)


def _tag(table, keys):
    import hashkeys as hk
    h = hk.mix64(keys)
    return hk.mix_raw_tag(h) if table == 32 else hk.tab64_tag(h)


def stash_bucket(table, b, bits, flagged, seed, c=None):
    """One bucket: two build keys for every count of STASH_REPEATS, repeated that often, and 400 single keys, shuffled; the
    probe side, 4 units and some, has eight tuples of every repeated key, one of every second single key and absent keys.
    All keys are small integers with pairwise different table tags, so no unit's count pass meets a tag hit on another key.
    flagged: every second unit (1, 3) also gets two absent keys with the home and tag of a repeated key — these units verify
    again while they emit, their neighbours do not.  Returns (R keys, S keys, units)."""
    import hashkeys as hk
    c = c or constants()
    rng = np.random.default_rng(seed)
    cand = (np.arange(1, 30001, dtype=np.uint64) << np.uint64(bits)) | np.uint64(b)
    _, first = np.unique(_tag(table, cand), return_index=True)
    cand = cand[np.sort(first)]                               # pairwise different tags
    nh = 2 * len(STASH_REPEATS)
    hot, single, absent = cand[:nh], cand[nh:nh + 400], cand[nh + 400:]
    reps = np.repeat(STASH_REPEATS, 2)
    build = rng.permutation(np.concatenate([np.repeat(hot, reps), single]))
    bc = len(build)
    units = 4
    pc = units * c.PR_UNIT + 77
    units += 1
    assert pc > bc
    nflag = 2 * (units // 2) if flagged else 0
    n_abs = pc - 8 * nh - 200 - nflag
    assert 0 < n_abs <= len(absent)
    probe = list(rng.permutation(np.concatenate([np.repeat(hot, 8), single[::2], absent[:n_abs]])))
    if flagged:
        tsize, _ = table_of(table, bc, c)
        pos = 0
        for u in range(1, units, 2):
            for off, k in ((5, hot[-1]), (c.PR_UNIT // 2, hot[0])):            # beside the 300-fold key and beside a single match
                h = int(hk.mix64(k)[0])
                if table == 32:
                    f = hk.mix64_keys(b, bits, units, h >> 32, 1, (h >> 16) & 0xFFFF, seed=seed + u)
                else:
                    home = h >> (64 - tsize)
                    f = hk.mix64_keys(b, bits, units, home << (32 - tsize), 1 << (32 - tsize), 0, seed=seed + u, low32=h & 0xFFFFFFFF)
                f = f[f != k]
                probe.insert(u * c.PR_UNIT + off, f[pos % len(f)])
            pos += 1
    probe = np.array(probe, dtype=np.uint64)
    assert len(probe) == pc
    unit_of = np.arange(pc) // c.PR_UNIT
    for k in hot:                                             # every repeated key is probed from both kinds of unit
        assert len(set(unit_of[probe == k] & 1)) == 2
    return build, probe, units


# ---- (f) the joins of the fresh process ------------------------------------------------------------------------------------
def hot_bucket_relations(rng, bits, n, hot, hot_build, hot_probe_extra=3000):
    """Key columns of R and S, n tuples each, uniform over the buckets but for bucket `hot`: hot_build distinct keys in R and
    hot_build + hot_probe_extra in S (R builds it).  Half of S's other keys are R's, half are fresh."""
    mask = np.uint64((1 << bits) - 1)

    def bg(m):
        k = np.unique(rng.integers(0, 1 << 63, size=m + m // 4 + 1024, dtype=np.uint64))
        k = k[(k & mask) != np.uint64(hot)]
        assert len(k) >= m
        return rng.permutation(k)[:m]
    hr = bucket_keys(rng, hot, bits, hot_build + 500)
    hr, fresh = hr[:hot_build], hr[hot_build:]
    ns = hot_build + hot_probe_extra
    hs = np.concatenate([hr[rng.integers(0, hot_build, size=ns - 500)], fresh])
    bR = bg(n - hot_build)
    m = n - ns
    bS = np.concatenate([bR[rng.integers(0, len(bR), size=m // 2)], bg(m - m // 2)])
    return rng.permutation(np.concatenate([bR, hr])), rng.permutation(np.concatenate([bS, hs]))
