"""The small join's partition (sigmod-2018_amd/csrc/rhj_small.hip.h: small_hist_body, small_selfhist, small_colsum, the plan
workgroup of small_scatter_body; rhj_device.hip: join_setup, join_small) restated in Python, with its constants read from the
sources by regular expression, the key builders and the shape tables of tests/test_gpu_small_edges.py.  Nothing here imports
the library: tests/test_small_model.py checks on the CPU that every shape lands in the regime its name claims and that the
column sums as written here add up, the GPU file runs the same shapes.  A changed constant moves the geometry with it, and a
shape that no longer reaches its regime fails on the CPU.

The column sums: cnt[tile][digit] is what k_small_hist left.  A scatter workgroup (tile t) needs, per digit, the tuples in the
tiles before t and in all tiles; the plan's workgroup needs the second only, for both relations at once.  Either cuts the tile
range into Q slices of per = ceil(tiles / Q) rows — Q = min(threads / lanes, SM_PARTS) with lanes = bins / 4 threads a slice
(four digits a thread; one digit a thread and lanes = bins below 2 bits), threads = SM_BLOCK for a scatter workgroup and
PLAN_THREADS per relation for the plan's — and reads a slice in rounds of SM_ROWS rows (the plan's: 2 * SM_ROWS) that are in
flight together; below 2 bits the rows are read one by one."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

import fused_model as fm
from source_constants import c_int, one

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sigmod-2018_amd", "csrc")
SOURCES = ("rhj_common.hip.h", "rhj_partition.hip.h", "rhj_small.hip.h", "rhj_batch.hip.h")      # in include order

NEED = ("SM_BLOCK", "SM_V", "SM_TILE", "SM_MAX_TILES", "SM_PARTS", "SM_ROWS", "SM_SELF_TILES", "BJ_MAX_TILES", "PT_MAX_BITS")
Constants = namedtuple("Constants", NEED + ("PLAN_THREADS", "SMALL_TILES", "FUSED_LDS_CAP"))

PLAN_THREADS = 512                   # threads per relation in the plan's workgroup: `tid >> 9` and `512u` in small_scatter_body


def _one(pattern, text, what):
    return one(pattern, text, what, "tests/small_model.py")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def plan_threads_in_source(text):
    """The plan workgroup's halves as small_scatter_body words them: (1 << shift, mask + 1, the divisor of either Q)."""
    m = _one(r"const uint32_t rel = tid >> (\d+), tt = tid & (\d+)u;", text, "the plan workgroup's halves")
    a = _one(r"Q = min\((\d+)u / lanes, SM_PARTS\);", text, "the plan workgroup's Q")
    b = _one(r"Q = min\((\d+)u >> bits, SM_PARTS\);", text, "the plan workgroup's Q below 2 bits")
    return 1 << int(m.group(1)), int(m.group(2)) + 1, int(a.group(1)), int(b.group(1))


def parse_constants(read=_read):
    text = {n: read(n) for n in SOURCES}
    names = {}
    for n in SOURCES:
        for m in re.finditer(r"constexpr\s+(?:int|uint32_t|uint64_t|size_t)\s+(\w+)\s*=\s*([^;]+);", text[n]):
            try:
                names[m.group(1)] = c_int(m.group(2), names)
            except (ValueError, NameError, SyntaxError, TypeError, ZeroDivisionError):
                pass
    missing = [n for n in NEED if n not in names]
    if missing:
        raise AssertionError("tests/small_model.py no longer finds %s in the sources" % missing)
    sm = text["rhj_small.hip.h"]
    got = plan_threads_in_source(sm)
    if set(got) != {PLAN_THREADS} or 2 * PLAN_THREADS != names["SM_BLOCK"]:
        raise AssertionError("tests/small_model.py: the plan workgroup has %r threads a relation in the sources, %d here" % (got, PLAN_THREADS))
    # the rules this module restates, as the code words them: a change there must be looked at here
    for pat, what in ((r"Q = min\(\(uint32_t\)SM_BLOCK / lanes, SM_PARTS\);", "small_colsum's Q"),
                      (r"Q = min\(\(uint32_t\)SM_BLOCK >> bits, SM_PARTS\);", "small_colsum's Q below 2 bits"),
                      (r"const uint32_t per = \(r\.tiles \+ Q - 1u\) / Q;\s*const uint32_t row0 = min\(q \* per, r\.tiles\), row1 = min\(row0 \+ per, r\.tiles\);",
                       "the slices' rows"),
                      (r"for \(uint32_t rb = row0; rb < row1; rb \+= SM_ROWS\)", "small_colsum's rounds"),
                      (r"for \(uint32_t rb = row0; rb < row1; rb \+= 2 \* SM_ROWS\)", "the plan workgroup's rounds"),
                      (r"if \(rb \+ j < t\) \{ bf\.x \+= v\[j\]\.x;", "small_colsum's rows before the tile"),
                      (r"if \(bits >= 2\) \{\s*const uint32_t lanes = bins >> 2;", "the four-digit lanes"),
                      (r"psum\[\(size_t\)rel \* bins \+ tt\] = rel \? ex - r0\.n : ex;", "the plan workgroup's prefix of S")):
        _one(pat, sm, what)
    f = fm.constants()
    return Constants(*[names[n] for n in NEED], PLAN_THREADS, min(f.SMALL_TILES, names["SM_MAX_TILES"]), f.FUSED_LDS_CAP)


_CONSTANTS = None


def constants():
    global _CONSTANTS
    if _CONSTANTS is None:
        _CONSTANTS = parse_constants()
    return _CONSTANTS


# ---- the host's rules -----------------------------------------------------------------------------------------------------------
def tiles(n, c=None):
    c = c or constants()
    return (int(n) + c.SM_TILE - 1) // c.SM_TILE


def self_hist(nR, nS, c=None):
    """join_small: no k_small_hist launch, the scatter workgroups count the digits themselves"""
    c = c or constants()
    return max(tiles(nR, c), tiles(nS, c)) <= c.SM_SELF_TILES


def takes(bits, nR, nS, c=None):
    """join_setup's s.small under the default knobs (the split paths go first where they apply: rhj_sub_bits, tests/test_sub_bits.py)"""
    c = c or constants()
    return 1 <= bits <= c.PT_MAX_BITS and nR > 0 and nS > 0 and tiles(nR, c) <= c.SMALL_TILES and tiles(nS, c) <= c.SMALL_TILES


Geometry = namedtuple("Geometry", "Q per slices rounds round_rows")      # slices: (row0, row1) of every slice; rounds: loads rounds of every slice


def colsum_geometry(ntiles, bits, who, c=None):
    c = c or constants()
    assert who in ("scatter", "plan")
    bins = 1 << bits
    threads = c.SM_BLOCK if who == "scatter" else c.PLAN_THREADS
    lanes = bins >> 2 if bits >= 2 else bins
    Q = min(threads // lanes, c.SM_PARTS)
    per = (ntiles + Q - 1) // Q
    slices = []
    for q in range(Q):
        row0 = min(q * per, ntiles)
        slices.append((row0, min(row0 + per, ntiles)))
    step = 1 if bits < 2 else c.SM_ROWS if who == "scatter" else 2 * c.SM_ROWS
    return Geometry(Q, per, slices, [-(-(r1 - r0) // step) for r0, r1 in slices], step)


def colsum_many(cnt, ts, bits, who, c=None, geom=None):
    """colsum for several tiles at once: (before[len(ts)][bins], all[bins]).  A slice's rows are met in ascending order, so the
    rows `rb + j < t` of a slice are the ones met before row t: `before` of every t is read off the running sum there."""
    g = geom or colsum_geometry(len(cnt), bits, who, c)
    cnt = np.asarray(cnt, dtype=np.uint32)
    ts = [int(t) for t in np.asarray(ts).reshape(-1)]
    bins = 1 << bits
    assert cnt.shape[1] == bins
    bf = np.zeros((len(ts), bins), dtype=np.uint32)                      # sum over q of part[q]
    al = np.zeros(bins, dtype=np.uint32)                                 # sum over q of part[Q + q]
    zero = np.zeros(bins, dtype=np.uint32)
    for row0, row1 in g.slices:
        part_al = np.zeros(bins, dtype=np.uint32)
        at = {}                                                          # row -> the slice's sum when that row is met
        for rb in range(row0, row1, g.round_rows):
            v = [cnt[rb + j] if rb + j < row1 else zero for j in range(g.round_rows)]     # the round's loads, all in flight
            for j in range(g.round_rows):
                at[rb + j] = part_al.copy()
                part_al += v[j]
        for i, t in enumerate(ts):
            if t > row0:
                bf[i] += at.get(t, part_al) if t < row1 else part_al
        al += part_al
    return bf, al


def colsum(cnt, t, bits, who, c=None, geom=None):
    """small_colsum (who = "scatter") or the plan workgroup's sums (who = "plan": it uses `all` only) over cnt[tiles][bins]:
    per digit, the tuples in the tiles before t and in all tiles, slice by slice and round by round as the kernel walks them."""
    bf, al = colsum_many(cnt, [t], bits, who, c, geom)
    return bf[0], al


def tile_hist(keys, bits, c=None, digits=None):
    """cnt[tile][digit] as small_hist_body leaves it: the digit is taken from the low 32 bits of the value"""
    c = c or constants()
    bins = 1 << bits
    d = (np.asarray(keys, dtype=np.uint64).astype(np.uint32) & np.uint32(bins - 1)).astype(np.int64) if digits is None else digits
    t = np.arange(len(d), dtype=np.int64) // c.SM_TILE
    return np.bincount(t * bins + d, minlength=tiles(len(d), c) * bins).reshape(-1, bins).astype(np.uint32)


def selfhist(keys, t, bits, c=None):
    """small_selfhist: the workgroup of tile t counts every tile of the relation itself"""
    c = c or constants()
    bins = 1 << bits
    keys = np.asarray(keys, dtype=np.uint64)
    before, all_ = np.zeros(bins, dtype=np.uint32), np.zeros(bins, dtype=np.uint32)
    for tt in range(tiles(len(keys), c)):
        beg = tt * c.SM_TILE
        end = min(beg + c.SM_TILE, len(keys))
        h = np.bincount((keys[beg:end].astype(np.uint32) & np.uint32(bins - 1)).astype(np.int64), minlength=bins).astype(np.uint32)
        all_ += h
        if tt < t:
            before += h
    return before, all_


# ---- keys: below 2^47, random above the radix and above bit 32, row ids are the positions --------------------------------------------
SMALL_N = 4096
KINDS = ("uniform", "tile_digit", "one_digit_last", "one_digit_first", "last_tile_only")
NO_PARTNER = np.uint64(1 << 46)      # set in no key of distinct_keys()

_DRAWS = {}


def _draw(which, n):
    """the first n of one seeded sequence of 32-bit words (drawn once a process, for the largest relation)"""
    have = _DRAWS.get(which)
    if have is None or len(have) < n:
        c = constants()
        have = np.random.default_rng(1000 + which).integers(0, 1 << 32, size=max(n, c.SM_MAX_TILES * c.SM_TILE + 1), dtype=np.uint32)
        _DRAWS[which] = have
    return have[:n]


def distinct_keys(bits, n, seed=5):
    """n distinct keys, key i in digit i mod bins: a serial number in bits 8..31, random bits between the radix and bit 8 and
    in bits 32..45"""
    bins = 1 << bits
    rng = np.random.default_rng(seed + 31 * bits)
    assert n <= 1 << 24
    i = np.arange(n, dtype=np.uint64)
    serial = rng.permutation(n).astype(np.uint64)
    mid = rng.integers(0, 256, size=n, dtype=np.uint64) & np.uint64(0xFF & ~(bins - 1))
    high = rng.integers(0, 1 << 14, size=n, dtype=np.uint64)
    return (high << np.uint64(32)) | (serial << np.uint64(8)) | mid | (i & np.uint64(bins - 1))


_SMALL = {}


def small_keys(bits):
    """the small side: SMALL_N distinct keys, SMALL_N / bins in every digit — one tile"""
    if bits not in _SMALL:
        _SMALL[bits] = distinct_keys(bits, SMALL_N)
    return _SMALL[bits]


def digits(kind, bits, n, c=None):
    c = c or constants()
    bins = 1 << bits
    if kind == "uniform":
        return (_draw(0, n) % np.uint32(bins)).astype(np.int64)
    if kind == "tile_digit":
        return (np.arange(n, dtype=np.int64) // c.SM_TILE) % bins
    if kind == "one_digit_last":
        return np.full(n, bins - 1, dtype=np.int64)
    if kind == "one_digit_first":
        return np.zeros(n, dtype=np.int64)
    assert kind == "last_tile_only"
    d = (_draw(0, n) % np.uint32(bins - 1)).astype(np.int64)
    d[(tiles(n, c) - 1) * c.SM_TILE:] = bins - 1
    return d


def large_keys(kind, bits, n, partner=None, c=None):
    """The large side: digits by `kind`, every key drawn from the partner's keys of its digit (partner: the other relation's
    distinct keys, key i in digit i mod bins; default small_keys(bits)).  A digit the partner has no key of gets keys that
    match nothing.  (Against small_keys() the last few results are kept: do not write into them.)"""
    if partner is None and c is None:
        return _large_keys_small(kind, bits, n)
    return _large_keys(kind, bits, n, small_keys(bits) if partner is None else np.asarray(partner, dtype=np.uint64), c)


@functools.lru_cache(maxsize=3)
def _large_keys_small(kind, bits, n):
    k = _large_keys(kind, bits, n, small_keys(bits), None)
    k.setflags(write=False)
    return k


def _large_keys(kind, bits, n, partner, c):
    bins = 1 << bits
    d = digits(kind, bits, n, c)
    have = (len(partner) - np.arange(bins, dtype=np.int64) + bins - 1) // bins          # partner keys of every digit
    r = _draw(1, n).astype(np.int64)
    pick = r % np.maximum(have, 1)[d]
    keys = partner[np.minimum(d + bins * pick, len(partner) - 1)]
    none = have[d] == 0
    if none.any():
        keys = np.where(none, NO_PARTNER | (r.astype(np.uint64) << np.uint64(8)) | d.astype(np.uint64), keys)
    return keys


Expected = namedtuple("Expected", "path units max_build")


def expected(kR, kS, bits, c=None):
    """What the plan's workgroup reports of a join on the small path: stats()["path"] ("small", or None where the join is not
    the small path's to finish), ["units"], ["max_build"]."""
    c = c or constants()
    bins = 1 << bits
    mask = np.uint32(bins - 1)
    cR = np.bincount((np.asarray(kR, dtype=np.uint64).astype(np.uint32) & mask).astype(np.int64), minlength=bins)
    cS = np.bincount((np.asarray(kS, dtype=np.uint64).astype(np.uint32) & mask).astype(np.int64), minlength=bins)
    both = (cR > 0) & (cS > 0)
    span = fm.fused_span_for(bins, len(kR), len(kS))
    hi, lo = np.maximum(cR, cS)[both], np.minimum(cR, cS)[both]
    small = takes(bits, len(kR), len(kS), c) and bool((lo <= c.FUSED_LDS_CAP).all())
    return Expected("small" if small else None, int((-(-hi // span)).sum()), int(lo.max()) if len(lo) else 0)


# ---- the shape tables -------------------------------------------------------------------------------------------------------------
def size_of(ntiles, full, c=None):
    c = c or constants()
    return ntiles * c.SM_TILE if full else (ntiles - 1) * c.SM_TILE + 1


# A: the self-counted path and its end.  (nR, nS); the first relation's keys are of the kind, the second's are distinct
A_BITS = (1, 2, 8)
A_KINDS = ("uniform", "tile_digit")


def a_sizes(c=None):
    c = c or constants()
    T, top = c.SM_TILE, c.SM_SELF_TILES * c.SM_TILE
    return [(T, T), (T + 1, T // 2), (top, top), (top, 1), (top + 1, top), (top + 1, T // 2)]


def a_keys(kind, bits, n, m):
    """(keys of the relation of n tuples, of the kind; m distinct keys of the other relation)"""
    other = small_keys(bits) if m == SMALL_N else distinct_keys(bits, m)
    return large_keys(kind, bits, n, other), other


# B: slice edges, C: round edges and the top: a large side of T tiles, full or with a one-tuple last tile, against small_keys()
B_TILES = (3, 8, 9, 15, 16, 17)
B_BITS = (1, 2, 3, 7, 8)
B_KINDS = KINDS
C_BITS = (1, 2, 8)
C_ROWS = {                                               # tiles -> (last tile: full / one tuple, kinds)
    128: ((True,), ("uniform", "tile_digit")),
    129: ((True, False), ("uniform", "tile_digit", "last_tile_only")),
    256: ((True,), ("uniform", "tile_digit")),
    257: ((True, False), ("uniform", "tile_digit")),
    512: ((True,), ("uniform", "tile_digit", "last_tile_only")),
}

# D: two large sides: R of D_TILES[0] tiles of distinct keys, S of D_TILES[1] tiles drawn from them; built on 8 bits (the digits
# of 7 and 2 bits are its low bits)
D_TILES = (129, 257)
D_KINDS = ("uniform", "tile_digit")
D_BITS = {8: "small", 7: "small", 2: "tiled"}            # 2 bits: with rhj_set_lowradix(0)


@functools.lru_cache(maxsize=2)
def d_keys(kind):
    c = constants()
    kR = distinct_keys(8, D_TILES[0] * c.SM_TILE, seed=6)
    return kR, large_keys(kind, 8, D_TILES[1] * c.SM_TILE, kR)


# E: through columns: (family, tiles) and what rhj_join_cols_device reads them through
E_A_TILES = (2, 3)
E_B_TILES = (3, 17)
E_C_TILES = (129,)
E_SELS = ("whole column", "row-id vector")

# F: row ids beyond 2^32 on the large side
F_TILES = (17, 129)
F_BITS = (2, 8)
WIDE = 1 << 40

# G: cnt reuse: (tiles, bits) back to back
G_STEPS = ((512, 8), (3, 2), (257, 1), (17, 8), (2, 8), (129, 2))

# H: batched
H_BITS = (1, 2, 8)
H_TILES = (1, 2, 3, 7, 8)


def h_joins(bits):
    """[(kind, tiles, last tile full, large side is R)] in the scrambled order of one batched call: every tile count with a full
    and a one-tuple last tile, all five kinds, orders alternating, and tile_digit in the other order as well"""
    rows = [(kind, t, full) for kind in KINDS for t in H_TILES for full in (True, False)]
    rows = [(k, t, f, i % 2 == 0) for i, (k, t, f) in enumerate(rows)]
    rows += [(k, t, f, not o) for k, t, f, o in rows if k == "tile_digit"]
    order = np.random.default_rng(80 + bits).permutation(len(rows))
    return [rows[i] for i in order]


def all_tile_counts():
    return sorted(set(B_TILES) | set(C_ROWS) | set(H_TILES) | {2} | {t for t, _ in G_STEPS})
