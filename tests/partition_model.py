"""The radix partition's launch plan (sigmod-2018_amd/csrc/rhj_device.hip: run_partition, partition_pass; the kernels of
rhj_partition.hip.h) restated in Python, with its constants read from the sources by regular expression, a vectorised
reference of the stable partition, and the key builders and shape tables of tests/test_gpu_partition_edges.py.  Nothing here
imports the library: tests/test_partition_model.py checks on the CPU that every row of every table lands in the regime its
name claims, the GPU file runs the same rows.  A changed constant moves plan() with it, and a row that no longer reaches its
regime fails on the CPU.

Pass 1 of the two-pass partition takes the low `lo` bits of the radix (pass-1 digit d1 = key & (2^lo - 1)), pass 2 the `hi`
bits above them (d2); pass-2 tile (d1, j), number d1 * groups + j, is the runs of digit d1 of the pass-1 tiles of group j."""
import os
import re
from collections import namedtuple

import numpy as np

from tiled_model import _c_int

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sigmod-2018_amd", "csrc")
SOURCES = ("rhj_common.hip.h", "rhj_partition.hip.h", "rhj_join_tiled.hip.h", "rhj_device.hip")      # in include order


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    m = re.search(pattern, text)
    if not m:
        raise AssertionError("tests/partition_model.py no longer finds %s in the sources" % what)
    return m


NAMES = ("WAVE", "PT_BLOCK", "PT_TILE", "PT_MAX_BITS", "PT_MAX_GROUP", "PT_STRIP", "FH_SLICES", "SR_TILE", "SR_MINW", "SR_RUNOFF",
         "HR_BLOCK", "LDS_BUDGET", "SMALL_TILES")
Constants = namedtuple("Constants", NAMES + ("STRIP2_TILES", "STRIP4_TILES", "GROUP_NUM", "GROUP_DEN", "CHUNK_TILES", "MAX_CHUNKS",
                                             "HIST_GRID", "HR_CHUNK", "HR_MIN_CHUNK", "HR_WANT", "HR_GRID", "GS_THREADS", "XCDS"))


def parse_constants(read=_read):
    """The constants of the partition from the sources (`read(name)` returns a source file's text)."""
    text = {n: read(n) for n in SOURCES}
    names = {}
    for n in SOURCES:                                    # every integer constexpr, in source order: later ones use earlier ones
        for m in re.finditer(r"constexpr\s+(?:int|uint32_t|uint64_t|size_t)\s+(\w+)\s*=\s*([^;]+);", text[n]):
            try:
                names[m.group(1)] = _c_int(m.group(2), names)
            except (ValueError, NameError, SyntaxError, TypeError, ZeroDivisionError):
                pass
    missing = [n for n in NAMES if n not in names]
    if missing:
        raise AssertionError("tests/partition_model.py no longer finds %s in the sources" % missing)
    dev, part = text["rhj_device.hip"], text["rhj_partition.hip.h"]
    m = _one(r"strip_tiles = most_tiles >= (\d+) \? PT_STRIP : most_tiles >= (\d+) \? \(PT_STRIP < 2 \? PT_STRIP : 2u\) : 1u;", dev,
             "run_partition's strip_tiles")
    strip4, strip2 = int(m.group(1)), int(m.group(2))
    g = _one(r"uint32_t group = (\d+)u \* bins1 / (\d+)u;", dev, "run_partition's group")
    _one(r"if \(group > PT_MAX_GROUP - 1\) group = PT_MAX_GROUP - 1;", dev, "run_partition's group clamp")
    _one(r"a\.parts = \(group \+ a\.strip - 1\) / a\.strip;\s*a\.per = \(a\.groups \+ FH_SLICES - 1\) / FH_SLICES;", dev, "run_partition's parts and per")
    ch = _one(r"uint32_t chunks = \(max_tiles \+ (\d+)\) / (\d+);", dev, "partition_pass' chunks")
    if int(ch.group(1)) + 1 != int(ch.group(2)):
        raise AssertionError("partition_pass rounds its chunks with two different sizes")
    mc = _one(r"if \(chunks > (\d+)\) chunks = (\d+);", dev, "partition_pass' chunk clamp")
    hg = _one(r"hist_grid = max_tiles < (\d+) \? max_tiles : (\d+);", dev, "partition_pass' histogram grid")
    if mc.group(1) != mc.group(2) or hg.group(1) != hg.group(2):
        raise AssertionError("partition_pass clamps with two different values")
    _one(r"return \(size_t\)SR_TILE \* 16 \+ \(PT_WAVES \+ 3\) \* bins \* 4 \+ \(PT_BLOCK / 64 \+ 2\) \* 8 \+ 2 \* \(SR_RUNOFF \+ PT_MAX_GROUP\) \* 4 \+ 16;",
         dev, "scatter_runs_lds_bytes")
    _one(r"per_cu = \(uint32_t\)\(LDS_BUDGET / scatter_runs_lds_bytes\(hi\)\);", dev, "the scatter's workgroups a CU")
    _one(r"if \(per_cu > \(uint32_t\)SR_MINW \* 256u / PT_BLOCK\) per_cu = \(uint32_t\)SR_MINW \* 256u / PT_BLOCK;", dev, "the scatter's occupancy clamp")
    _one(r"want = \(\(max2 < sgrid \? max2 : sgrid\) \+ 7u\) & ~7u;", dev, "the scatter's grid")
    _one(r"xcd = blockIdx\.x & 7u, per_xcd = gridDim\.x >> 3;", part, "k_scatter_runs' deal over the XCDs")
    hw = _one(r"hw = \(max2 \+ HR_BLOCK / WAVE - 1\) / \(HR_BLOCK / WAVE\);", dev, "k_hist_runs' grid") and \
        _one(r"dim3\(hw < (\d+) \? hw : (\d+), nrel\)", dev, "k_hist_runs' grid clamp")
    hr = _one(r"uint32_t chunk = (\d+);\s*while \(chunk > (\d+)u && r\.tiles / chunk < (\d+)u\) chunk >>= 1;", part, "k_hist_runs' chunk")
    gs = _one(r"cpt = min\(8u, bins\), lanes = bins / cpt, rows = (\d+)u / lanes;", part, "k_group_scan's rows")
    _one(r"uint32_t S = max\(1u, min\(rows / R, r\.parts\)\);\s*if \(S < 4u\) S = 1;", part, "k_group_scan's shares")
    return Constants(*[names[n] for n in NAMES], strip2, strip4, int(g.group(1)), int(g.group(2)), int(ch.group(2)), int(mc.group(1)),
                     int(hg.group(1)), int(hr.group(1)), int(hr.group(2)), int(hr.group(3)), int(hw.group(1)), int(gs.group(1)), 8)


_CONSTANTS = None


def constants():
    global _CONSTANTS
    if _CONSTANTS is None:
        _CONSTANTS = parse_constants()
    return _CONSTANTS


def tiles_for(n, c=None):
    c = c or constants()
    return max(1, -(-int(n) // c.PT_TILE))


def scatter_runs_lds_bytes(hi, c=None):
    c = c or constants()
    return c.SR_TILE * 16 + (c.PT_BLOCK // c.WAVE + 3) * (1 << hi) * 4 + (c.PT_BLOCK // 64 + 2) * 8 + 2 * (c.SR_RUNOFF + c.PT_MAX_GROUP) * 4 + 16


OnePass = namedtuple("OnePass", "passes bits tiles chunks per hist_grid hist_strides scan_rounds empty_chunks")
TwoPass = namedtuple("TwoPass", "passes bits tiles lo hi bins1 bins2 group groups strip parts last_strip per tiles2 count_in_pass1 "
                                "sgrid busiest wave_runs rows R S rounds chunk hist_grid hist_strides")


def plan(bits, n, cus=256, count_in_pass1=True, lo_bits=0, c=None):
    """run_partition for ONE relation of n tuples (the other relation of a join changes `strip` only: the larger tile count
    selects it).  Two relations in one launch: plan2()."""
    return plan_tiles(bits, tiles_for(n, c), cus, count_in_pass1, lo_bits, c)


def plan_tiles(bits, tiles, cus=256, count_in_pass1=True, lo_bits=0, c=None, most_tiles=None):
    c = c or constants()
    most = max(tiles, most_tiles or 0)
    if bits <= c.PT_MAX_BITS and not lo_bits:                         # partition_pass (without a plan: no small route)
        chunks = min(max((most + c.CHUNK_TILES - 1) // c.CHUNK_TILES, 1), c.MAX_CHUNKS)
        per = -(-tiles // chunks)
        grid = min(most, c.HIST_GRID)
        return OnePass(1, bits, tiles, chunks, per, grid, -(-tiles // grid), -(-chunks // c.WAVE),
                       sum(1 for q in range(chunks) if q * per >= tiles))
    lo = lo_bits or bits // 2
    hi = bits - lo
    bins1, bins2 = 1 << lo, 1 << hi
    group = (7 * bins1 // 8) if lo_bits else (c.GROUP_NUM * bins1 // c.GROUP_DEN)
    group = min(max(group, 1), c.PT_MAX_GROUP - 1)
    strip = c.PT_STRIP if most >= c.STRIP4_TILES else min(c.PT_STRIP, 2) if most >= c.STRIP2_TILES else 1
    groups = -(-tiles // group)
    parts = -(-group // strip)
    per = -(-groups // c.FH_SLICES)
    tiles2 = bins1 * groups
    cip1 = bool(count_in_pass1) and bits <= 12
    per_cu = max(1, min(c.LDS_BUDGET // scatter_runs_lds_bytes(hi, c), c.SR_MINW * 256 // c.PT_BLOCK))
    sgrid = (min(tiles2, cus * per_cu) + 7) & ~7
    # k_group_scan, slice 0's first round
    cpt = min(8, bins2)
    rows = c.GS_THREADS // (bins2 // cpt)
    j1 = min(per, groups)
    R = min(rows, j1)
    S = max(1, min(rows // R, parts))
    if S < 4:
        S = 1
    chunk = c.HR_CHUNK
    while chunk > c.HR_MIN_CHUNK and tiles2 // chunk < c.HR_WANT:
        chunk >>= 1
    hgrid = min(-(-tiles2 // (c.HR_BLOCK // c.WAVE)), c.HR_GRID)
    return TwoPass(2, bits, tiles, lo, hi, bins1, bins2, group, groups, strip, parts, group - (parts - 1) * strip, per, tiles2, cip1,
                   sgrid, -(-tiles2 // sgrid), group <= c.WAVE, rows, R, S if cip1 else None, -(-j1 // rows), chunk, hgrid,
                   -(-tiles2 // (hgrid * chunk)))


def plan2(bits, nR, nS, **kw):
    """Two relations in one launch: (plan of R, plan of S), both with the larger relation's strip / chunks / grids."""
    tR, tS = tiles_for(nR), tiles_for(nS)
    return plan_tiles(bits, tR, most_tiles=tS, **kw), plan_tiles(bits, tS, most_tiles=tR, **kw)


def scatter_sequences(p):
    """k_scatter_runs: the pass-2 tiles of every workgroup that has any, in the order it takes them"""
    per_xcd = p.sgrid >> 3
    out = []
    for x in range(p.sgrid):
        first = (x & 7) * per_xcd + (x >> 3)
        if first < p.tiles2:
            out.append(list(range(first, p.tiles2, p.sgrid)))
    return out


# ---- the reference ------------------------------------------------------------------------------------------------------------
def stable_partition(keys, row_ids, bits):
    """The stable partition of (keys, row_ids) on key & (2^bits - 1): ([n, 2] permuted tuples, hist, psum) with psum = -1 for an
    empty bucket, as rhj_partition_device returns it.  numpy arrays (uint64 or int64) give uint64 tuples and int64 hist / psum;
    torch int64 tensors give int64 tensors on their device."""
    nb = 1 << bits
    if isinstance(keys, np.ndarray):
        k = np.ascontiguousarray(keys).view(np.uint64) if keys.dtype != np.uint64 else keys
        r = np.ascontiguousarray(row_ids).view(np.uint64) if row_ids.dtype != np.uint64 else row_ids
        d = (k & np.uint64(nb - 1)).astype(np.int64)
        o = np.argsort(d, kind="stable")
        hist = np.bincount(d, minlength=nb).astype(np.int64)
        psum = np.cumsum(hist) - hist
        psum[hist == 0] = -1
        return np.stack([k[o], r[o]], axis=1), hist, psum
    import torch
    d = keys & (nb - 1)
    o = torch.sort(d, stable=True).indices
    hist = torch.bincount(d, minlength=nb)
    psum = torch.cumsum(hist, 0) - hist
    psum[hist == 0] = -1
    return torch.stack([keys[o], row_ids[o]], dim=1), hist, psum


# ---- keys: 47 bits, random above the radix (a tuple misplaced inside its bucket shows), row ids are the positions ------------------
KEY_BITS = 47


def _above(rng, n, low_bits):
    return rng.integers(0, 1 << (KEY_BITS - low_bits), size=n, dtype=np.uint64) << np.uint64(low_bits)


def keys_uniform(rng, n, bits):
    return rng.integers(0, 1 << KEY_BITS, size=n, dtype=np.uint64)


def keys_equal(rng, n, bits, bucket):
    return _above(rng, n, bits) | np.uint64(bucket)


def keys_last(rng, n, bits):
    return keys_equal(rng, n, bits, (1 << bits) - 1)


def keys_absent(rng, n, bits, lo, absent):
    """uniform, but no key has the digit `absent` in its low `lo` bits (those take the digit absent ^ 1)"""
    k = keys_uniform(rng, n, bits)
    hit = (k & np.uint64((1 << lo) - 1)) == np.uint64(absent)
    k[hit] ^= np.uint64(1)
    return k


def odd_cell_bucket(bits):
    """a bucket whose (d1, d2) cell of pass 1's 16-bit counts has an odd index: d2 = 3 (1 at hi = 1 ... never: hi >= 4), d1 = 5"""
    lo = bits // 2
    return (3 << lo) | 5


def keys_pair(rng, n, bits):
    """two buckets by position parity whose cells share one 32-bit word: d1 = 6, d2 = 2 and 3"""
    lo = bits // 2
    d2 = np.uint64(2) + (np.arange(n, dtype=np.uint64) & np.uint64(1))
    return _above(rng, n, bits) | (d2 << np.uint64(lo)) | np.uint64(6)


_ZIPF = {}


def zipf_ranks(n, theta=0.9, domain=1 << 16, seed=11):
    """the first n of one sequence of Zipf(theta) ranks (drawn once a process: the draw is the slow part)"""
    have = _ZIPF.get((theta, domain, seed))
    if have is None or len(have) < n:
        w = 1.0 / np.arange(1, domain + 1, dtype=np.float64) ** theta
        cdf = np.cumsum(w)
        have = np.searchsorted(cdf, np.random.default_rng(seed).random(n) * cdf[-1]).astype(np.uint64)
        _ZIPF.clear()
        _ZIPF[(theta, domain, seed)] = have
    return have[:n]


def keys_zipf(rng, n, bits, theta=0.9):
    """Zipf(theta) over 65 536 keys; which keys, and so which buckets are hot, differs with the radix width"""
    mult = np.uint64(0x9E3779B97F4A7C15 + 2 * bits)
    return ((zipf_ranks(n, theta) + np.uint64(1)) * mult) & np.uint64((1 << KEY_BITS) - 1)


def keys_marked(rng, bits, lo, dstar, marked):
    """marked: bool per position.  The marked tuples have pass-1 digit dstar, the others any other digit; everything above
    the low lo bits is random."""
    n = len(marked)
    other = rng.integers(0, (1 << lo) - 1, size=n, dtype=np.uint64)
    other += (other >= np.uint64(dstar)).astype(np.uint64)
    return _above(rng, n, lo) | np.where(marked, np.uint64(dstar), other)


def keys_count(rng, n, bits, lo, dstar, count):
    marked = np.zeros(n, dtype=bool)
    marked[rng.permutation(n)[:count]] = True
    return keys_marked(rng, bits, lo, dstar, marked)


def keys_hot_absent(rng, n, bits, lo, hot, absent, share=0.3):
    """a share of the tuples has pass-1 digit `hot`, none has `absent`, the rest any other digit"""
    assert hot != absent
    other = rng.integers(0, (1 << lo) - 1, size=n, dtype=np.uint64)
    other += (other >= np.uint64(absent)).astype(np.uint64)
    d1 = np.where(rng.random(n) < share, np.uint64(hot), other)
    return _above(rng, n, lo) | d1


def digit1(keys, bits):
    return (keys & np.uint64((1 << (bits // 2)) - 1)).astype(np.int64)


def tile_counts(marked, c=None):
    """marked tuples of every pass-1 tile"""
    c = c or constants()
    pad = (-len(marked)) % c.PT_TILE
    return np.concatenate([marked, np.zeros(pad, dtype=bool)]).reshape(-1, c.PT_TILE).sum(axis=1)


def strip_cell_max(keys, bits, p, c=None):
    """The largest 16-bit cell of k_local_part's strip counts: (strip of tiles, d1, d2) -> tuples"""
    c = c or constants()
    k = np.asarray(keys, dtype=np.uint64)
    cell = (k & np.uint64((1 << bits) - 1)).astype(np.int64)          # (d2 << lo | d1: a renumbering of the kernel's d1 << hi | d2)
    tile = np.arange(len(k), dtype=np.int64) // c.PT_TILE
    strip = (tile // p.group) * p.parts + (tile % p.group) // p.strip
    return int(np.bincount(strip * (1 << bits) + cell).max())


# ---- the shape tables -----------------------------------------------------------------------------------------------------------
def group_of(bits, c=None):
    return plan_tiles(bits, 1, c=c).group


# A: tile, group and slice edges
A_BITS = (9, 10, 11, 12, 13, 14, 15)
A_KINDS = ("uniform", "equal", "absent", "last")


def a_sizes(bits, c=None):
    c = c or constants()
    T, G = c.PT_TILE, group_of(bits, c)
    return [1, 63, T - 1, T, T + 1, G * T - 1, G * T, G * T + 1, 8 * G * T, 8 * G * T + 1, 9 * G * T + 1]


def a_keys(kind, bits, n, seed=1):
    rng = np.random.default_rng(seed + 17 * bits)
    lo = bits // 2
    if kind == "uniform":
        return keys_uniform(rng, n, bits)
    if kind == "equal":
        return keys_equal(rng, n, bits, odd_cell_bucket(bits))
    if kind == "absent":
        return keys_absent(rng, n, bits, lo, 3)
    assert kind == "last"
    return keys_last(rng, n, bits)


# B: strips.  (tiles, last tile full, key kind, also with rhj_set_count_in_pass1(0))
B_BITS = (9, 10, 12)
B_ROWS = {
    "strip 1": [(1023, True, "uniform", True), (1023, False, "equal", False), (1023, True, "pair", False), (1023, False, "zipf", False)],
    "strip 2": [(1024, True, "equal", False), (1024, False, "uniform", False), (1025, True, "zipf", True), (1025, False, "pair", False),
                (2047, True, "pair", False), (2047, False, "equal", False)],
    "strip 4": [(2048, True, "uniform", False), (2048, False, "equal", False), (2049, True, "equal", False), (2049, False, "zipf", False),
                (2050, True, "pair", True), (2050, False, "uniform", False), (2051, True, "zipf", False), (2051, False, "pair", False)],
}
B_REGIME_STRIP = {"strip 1": 1, "strip 2": 2, "strip 4": 4}
B_KINDS = ("uniform", "equal", "pair", "zipf")
B_LAST_STRIP = {9: (4, 3), 10: (8, 2), 12: (15, 4)}       # at strip 4: (parts, tiles of a group's last strip); 12 bits: no short strip
B_MAX_TILES = 2051


def b_size(tiles, full, c=None):
    c = c or constants()
    return tiles * c.PT_TILE if full else (tiles - 1) * c.PT_TILE + 1


def b_keys(kind, bits, n, seed=2):
    """the first n keys of the kind's key set of B_MAX_TILES tiles (a prefix of each kind is of the same kind)"""
    rng = np.random.default_rng(seed + 17 * bits)
    if kind == "uniform":
        return keys_uniform(rng, n, bits)
    if kind == "equal":
        return keys_equal(rng, n, bits, odd_cell_bucket(bits))
    if kind == "pair":
        return keys_pair(rng, n, bits)
    assert kind == "zipf"
    return keys_zipf(rng, n, bits)


# B, wide row ids: (name, tiles, tuples of the last tile, position of the one row id >= 2^32) per strip regime.  The position is
# outside the first and last 2048 tuples (k_rowid_sample reads those), so pass 1 has to find it.
def b_wide_rows(c=None):
    c = c or constants()
    T = c.PT_TILE
    rows = []
    for tiles in (1023, 1025, 2050):
        n = (tiles - 1) * T + 3000
        p = plan(12, n, c=c)
        first = 3 * p.group + p.strip * (p.parts // 2)            # the first tile of a strip in the middle of group 3
        rows.append(("first tile of a strip", tiles, n, first * T + 3001))
        rows.append(("last, partial tile", tiles, n, (tiles - 1) * T + 100))
    return rows


B_WIDE_BITS = 12
WIDE = 1 << 40

# C: pass-2 batch edges, D: runs — one group
C_BITS = (9, 12, 14)


def c_counts(bits, c=None):
    c = c or constants()
    T = c.SR_TILE
    return [0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, group_of(bits, c) * c.PT_TILE]


def c_dstars(bits):
    return [0, (1 << (bits // 2)) - 1]


def c_keys(bits, dstar, count, c=None):
    c = c or constants()
    n = group_of(bits, c) * c.PT_TILE
    return keys_count(np.random.default_rng(3 + bits + 1000 * dstar + count), n, bits, bits // 2, dstar, count)


D_BITS = (9, 14)
D_PLACES = ("every third tile", "runs 63 64 65", "one full tile", "last tuple")
D_DSTAR = 5


def d_marked(place, bits, c=None):
    c = c or constants()
    G, T = group_of(bits, c), c.PT_TILE
    rng = np.random.default_rng(4 + bits)
    m = np.zeros((G, T), dtype=bool)
    if place == "every third tile":
        for t in range(0, G, 3):
            m[t, rng.integers(0, T)] = True
    elif place == "runs 63 64 65":
        for t in range(G):
            m[t, rng.permutation(T)[:63 + t % 3]] = True
    elif place == "one full tile":
        m[G // 2, :] = True
    else:
        assert place == "last tuple"
        m[G - 1, T - 1] = True
    return m.reshape(-1)


def d_keys(place, bits, c=None):
    return keys_marked(np.random.default_rng(5 + bits), bits, bits // 2, D_DSTAR, d_marked(place, bits, c))


# E: a workgroup of k_scatter_runs with several tiles
E_BITS = (9, 12, 14)
E_TILES = {500: (2, 2), 1447: (3, 4)}                  # pass-1 tiles -> (fewest, most) tiles of the workgroups that have two or more
E_KINDS = ("uniform", "hot, first digit absent", "hot, last digit absent")
E_LAST = 1234                                          # tuples of the last, partial tile


def e_size(tiles, c=None):
    c = c or constants()
    return (tiles - 1) * c.PT_TILE + E_LAST


def e_digits(kind, bits):
    """(hot, absent) pass-1 digits of a "hot + absent" key set: the first and the last digit, so that both kinds of tile lie in
    the sequences of the workgroups that take several tiles (the first and the last pass-2 tiles)"""
    bins1 = 1 << (bits // 2)
    return (bins1 - 1, 0) if "first" in kind else (0, bins1 - 1)


def e_keys(kind, bits, n):
    rng = np.random.default_rng(6 + bits)
    if kind == "uniform":
        return keys_uniform(rng, n, bits)
    hot, absent = e_digits(kind, bits)
    return keys_hot_absent(rng, n, bits, bits // 2, hot, absent)


# F: one pass
F_BITS = (1, 4, 6, 8)
F_TILES = (1, 2, 16, 17, 1024, 1025, 2048, 2049)
F_KINDS = ("uniform", "equal", "absent", "last")
F_REGIMES = {1: "one chunk", 2: "one chunk", 16: "one chunk", 17: "two chunks", 1024: "one scan round", 1025: "carry in scan_bins",
             2048: "full grid", 2049: "grid stride"}


def f_sizes(c=None):
    return [b_size(t, full, c) for t in F_TILES for full in (True, False)]


def f_keys(kind, bits, n):
    rng = np.random.default_rng(7 + bits)
    if kind == "uniform":
        return keys_uniform(rng, n, bits)
    if kind == "equal":
        return keys_equal(rng, n, bits, (1 << bits) // 3)
    if kind == "absent":
        return keys_absent(rng, n, bits, bits, (1 << bits) - 1 if bits > 1 else 1)
    assert kind == "last"
    return keys_last(rng, n, bits)


# G: large, wholly on the device: (name, bits, tiles, tuples less (-) or more (+) than tiles full tiles)
def g_rows(c=None):
    c = c or constants()
    T = c.PT_TILE
    big = 8193 * T - 5
    return [("chunk clamp", 4, big), ("chunk clamp", 8, big), ("no shares", 9, big), ("no shares", 11, big),
            ("shares", 10, big), ("shares", 12, big), ("hist_runs chunk 8", 14, 15361 * T + 1)]


# H: two relations in one launch
H_BITS = (9, 12, 14)
H_ONE_PASS_BITS = 8                                    # partition_pass with two relations beyond SMALL_TILES: the fused path on <= 8 bits


def h_sizes(c=None):
    c = c or constants()
    big = 2049 * c.PT_TILE + 3
    return [(1, big), (4097, big), (big, 1), (big, 4097)]
