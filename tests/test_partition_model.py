"""tests/partition_model.py against the sources it restates, against the oracle, and against the regimes the shape tables of
tests/test_gpu_partition_edges.py claim to reach: every row of every table is held to its name by plan().  CPU only."""
import numpy as np
import pytest

import partition_model as pm
from helpers import make_rel

C = pm.constants()
T = C.PT_TILE


def test_parsed_constants():
    """The values at this commit and what the kernels rely on; a changed constant fails here with the new values in the message."""
    assert (C.WAVE, C.PT_BLOCK, C.PT_TILE, C.PT_MAX_BITS, C.PT_MAX_GROUP, C.PT_STRIP) == (64, 512, 4096, 8, 256, 4), C
    assert (C.FH_SLICES, C.SR_TILE, C.SR_MINW, C.SR_RUNOFF, C.HR_BLOCK, C.LDS_BUDGET, C.SMALL_TILES) == (8, 4096, 4, 264, 256, 160 * 1024, 1024), C
    assert (C.STRIP2_TILES, C.STRIP4_TILES, C.GROUP_NUM, C.GROUP_DEN) == (1024, 2048, 15, 16), C
    assert (C.CHUNK_TILES, C.MAX_CHUNKS, C.HIST_GRID, C.HR_CHUNK, C.HR_MIN_CHUNK, C.HR_WANT, C.HR_GRID, C.GS_THREADS) == (16, 512, 2048, 32, 4, 2048, 4096, 1024), C
    # a strip's counts are 16-bit cells; the run table's offsets are 16-bit; SR_RUNOFF holds the total behind PT_MAX_GROUP runs
    assert C.PT_STRIP * C.PT_TILE < 65536 and C.PT_TILE < 65536 and C.SR_RUNOFF > C.PT_MAX_GROUP and C.SR_TILE == C.PT_TILE
    # two scatter workgroups a CU at every width
    assert all(C.LDS_BUDGET // pm.scatter_runs_lds_bytes(hi) >= 2 for hi in range(1, C.PT_MAX_BITS + 1))
    assert [pm.group_of(b) for b in range(9, 16)] == [15, 30, 30, 60, 60, 120, 120]
    assert all(pm.group_of(b) < C.PT_MAX_GROUP - 1 for b in range(9, 16))           # the clamp: no default width reaches it


def test_constants_follow_the_sources():
    """Moving a constant in (a copy of) the sources moves the plan; a pattern that no longer matches fails loudly."""
    def moved(name, old, new):
        def read(n):
            t = pm._read(n)
            if n == name:
                assert old in t
                t = t.replace(old, new)
            return t
        return pm.parse_constants(read)
    c = moved("rhj_partition.hip.h", "PT_STRIP = 4;", "PT_STRIP = 8;")
    assert pm.plan(9, 2048 * T, c=c).strip == 8 and pm.plan(9, 2048 * T, c=c).parts == 2
    c = moved("rhj_device.hip", "most_tiles >= 2048 ? PT_STRIP", "most_tiles >= 4096 ? PT_STRIP")
    assert pm.plan(12, 2048 * T, c=c).strip == 2 and pm.plan(12, 4096 * T, c=c).strip == 4
    c = moved("rhj_partition.hip.h", "FH_SLICES = 8;", "FH_SLICES = 4;")
    assert pm.plan(9, 8 * 15 * T, c=c).per == 2
    c = moved("rhj_device.hip", "if (chunks > 512) chunks = 512;", "if (chunks > 256) chunks = 256;")
    assert pm.plan(4, 8193 * T, c=c).chunks == 256
    with pytest.raises(AssertionError, match="no longer finds"):
        moved("rhj_device.hip", "uint32_t group = 15u * bins1 / 16u;", "uint32_t group = bins1;")
    with pytest.raises(AssertionError, match="no longer finds"):
        moved("rhj_partition.hip.h", "if (S < 4u) S = 1;", "if (S < 2u) S = 1;")


def test_plan_on_known_sizes():
    p = pm.plan(12, 100_000_000)                                    # README's 100M relation at 12 bits
    assert (p.lo, p.hi, p.group, p.strip, p.parts, p.groups, p.per, p.tiles2) == (6, 6, 60, 4, 15, 407, 51, 64 * 407)
    assert (p.sgrid, p.busiest, p.wave_runs, p.rows, p.R, p.S, p.rounds) == (512, 51, True, 128, 51, 1, 1)
    p = pm.plan(14, 300_000)
    assert (p.lo, p.hi, p.group, p.groups, p.tiles2, p.strip, p.count_in_pass1, p.wave_runs, p.S) == (7, 7, 120, 1, 128, 1, False, False, None)
    assert (p.sgrid, p.busiest, p.chunk, p.hist_grid) == (128, 1, 4, 32)
    p = pm.plan(8, 1_000_003)
    assert (p.tiles, p.chunks, p.per, p.hist_grid, p.hist_strides, p.scan_rounds) == (245, 16, 16, 245, 1, 1)
    assert pm.plan(9, 1).tiles == 1 and pm.plan(9, 0).tiles == 1
    assert pm.plan(8, 3 << 20, lo_bits=8).passes == 2 and pm.plan(8, 3 << 20, lo_bits=8).group == 224
    # what the issue states about the tests that existed before: none of their sizes reaches a strip or a second tile
    for n in (1, 63, 4097, 300_000, 1_000_003, 1_200_000):
        for bits in range(9, 16):
            p = pm.plan(bits, n)
            assert p.strip == 1 and p.busiest == 1, (bits, n)


def test_scatter_sequences_visit_every_tile_once():
    for bits, tiles in ((9, 500), (12, 1447), (14, 77), (9, 1)):
        p = pm.plan_tiles(bits, tiles)
        seq = pm.scatter_sequences(p)
        assert sorted(t for s in seq for t in s) == list(range(p.tiles2))
        assert max(len(s) for s in seq) == p.busiest and len(seq) <= p.sgrid and p.sgrid % 8 == 0


def tuples_of(rel):
    return np.stack([rel["value"], rel["row_id"]], axis=1)


@pytest.mark.parametrize("bits", [1, 4, 8, 9, 12, 15])
def test_stable_partition_equals_the_oracle(oracle, bits):
    for n in (1, 4097, 300_000):
        rng = np.random.default_rng(bits * 1000 + n % 97)
        for kind, keys in (("uniform", pm.keys_uniform(rng, n, bits)), ("equal", pm.keys_equal(rng, n, bits, (1 << bits) - 2)),
                           ("absent", pm.keys_absent(rng, n, bits, bits, 0))):
            rel = make_rel(keys)
            want, whist, wpsum = oracle.partition(rel, bits)
            got, hist, psum = pm.stable_partition(rel["value"], rel["row_id"], bits)
            assert np.array_equal(got, tuples_of(want)), (kind, n, bits)
            assert np.array_equal(hist.astype(np.uint64), whist) and np.array_equal(psum, wpsum), (kind, n, bits)
            if kind == "absent":
                assert psum[0] == -1 and hist[0] == 0
    # the torch back end gives the same bytes
    import torch
    keys = pm.keys_zipf(np.random.default_rng(bits), 50_000, bits)
    ids = np.arange(len(keys), dtype=np.uint64)
    a, ah, ap = pm.stable_partition(keys, ids, bits)
    b, bh, bp = pm.stable_partition(torch.from_numpy(keys.view(np.int64)), torch.from_numpy(ids.view(np.int64)), bits)
    assert np.array_equal(a.view(np.int64), b.numpy()) and np.array_equal(ah, bh.numpy()) and np.array_equal(ap, bp.numpy())


# ---- every row of every shape table lands in the regime its name claims -----------------------------------------------------------
@pytest.mark.parametrize("bits", pm.A_BITS)
def test_table_a_regimes(bits):
    G = pm.group_of(bits)
    sizes = pm.a_sizes(bits)
    assert sizes == [1, 63, T - 1, T, T + 1, G * T - 1, G * T, G * T + 1, 8 * G * T, 8 * G * T + 1, 9 * G * T + 1]
    p = [pm.plan(bits, n) for n in sizes]
    assert [x.tiles for x in p] == [1, 1, 1, 1, 2, G, G, G + 1, 8 * G, 8 * G + 1, 9 * G + 1]
    assert [x.groups for x in p] == [1, 1, 1, 1, 1, 1, 1, 2, 8, 9, 10]                       # one group to two, eight to nine
    assert [x.per for x in p] == [1] * 9 + [2, 2]                                             # per goes 1 -> 2 ...
    assert [-(-x.groups // x.per) for x in p][-3:] == [8, 5, 5]                               # ... and slices end up empty
    assert all(x.passes == 2 and x.count_in_pass1 == (bits <= 12) for x in p)
    assert all(not pm.plan(bits, n, count_in_pass1=False).count_in_pass1 for n in sizes)
    for kind in pm.A_KINDS:
        k = pm.a_keys(kind, bits, 3 * T)
        d = (k & np.uint64((1 << bits) - 1)).astype(np.int64)
        if kind == "equal":
            assert len(set(d)) == 1 and (d[0] >> (bits // 2)) & 1 == 1
        elif kind == "last":
            assert set(d) == {(1 << bits) - 1}
        elif kind == "absent":
            assert 3 not in set(pm.digit1(k, bits)) and len(set(pm.digit1(k, bits))) == (1 << (bits // 2)) - 1
        assert int(k.max()) >> 32 != 0 and int(k.max()) < 1 << pm.KEY_BITS                    # random bits above bit 32


@pytest.mark.parametrize("bits", pm.B_BITS)
def test_table_b_regimes(bits):
    kinds = {r: set() for r in pm.B_ROWS}
    off = set()
    seen_tiles = {}
    for regime, rows in pm.B_ROWS.items():
        for tiles, full, kind, both in rows:
            n = pm.b_size(tiles, full)
            p = pm.plan(bits, n)
            assert p.tiles == tiles and p.strip == pm.B_REGIME_STRIP[regime] and p.count_in_pass1, (regime, tiles)
            assert n == tiles * T if full else n == (tiles - 1) * T + 1
            kinds[regime].add(kind)
            seen_tiles.setdefault(tiles, set()).add(full)
            if both:
                off.add(regime)
                assert not pm.plan(bits, n, count_in_pass1=False).count_in_pass1
    assert all(k == set(pm.B_KINDS) for k in kinds.values()), kinds                          # every (strip regime x key kind)
    assert off == set(pm.B_ROWS)                                                             # once per regime without the pass-1 counts
    assert sorted(seen_tiles) == [1023, 1024, 1025, 2047, 2048, 2049, 2050, 2051]
    assert all(v == {True, False} for v in seen_tiles.values())                              # last tile full, and one tuple
    assert {t % 4 for t, *_ in pm.B_ROWS["strip 4"]} == {0, 1, 2, 3}
    p = pm.plan_tiles(bits, 2048)
    assert (p.parts, p.last_strip) == pm.B_LAST_STRIP[bits]
    assert (p.strip == 4 and p.group % 4 != 0) == (bits in (9, 10))                          # "strip 4, short last strip"
    # a relation that ends inside a strip
    assert any(((t - 1) % p.group) % p.strip != p.strip - 1 for t in (2049, 2050, 2051))


@pytest.mark.parametrize("bits", pm.B_BITS)
def test_table_b_cells(bits):
    """all equal: the count strip * PT_TILE sits in the upper half of a word whose lower half stays 0; pair: two cells of one
    word with 2 PT_TILE each a strip of four; the largest 16-bit cell is strip * PT_TILE < 65536"""
    lo, hi = bits // 2, bits - bits // 2
    for tiles in (1024, 2048):
        p = pm.plan_tiles(bits, tiles)
        n = 4 * p.group * T                                                                  # (four groups of the relation: a strip's counts do not depend on the rest)
        k = pm.b_keys("equal", bits, n)
        d1, d2 = pm.digit1(k, bits), ((k >> np.uint64(lo)) & np.uint64((1 << hi) - 1)).astype(np.int64)
        cell = (d1 << hi) | d2
        assert len(set(cell)) == 1 and cell[0] & 1 == 1
        assert pm.strip_cell_max(k, bits, p) == p.strip * T < 65536
        k = pm.b_keys("pair", bits, n)
        d1, d2 = pm.digit1(k, bits), ((k >> np.uint64(lo)) & np.uint64((1 << hi) - 1)).astype(np.int64)
        cell = (d1 << hi) | d2
        assert sorted(set(cell)) == [int(cell.min()), int(cell.min()) + 1] and cell.min() % 2 == 0
        assert pm.strip_cell_max(k, bits, p) == p.strip * T // 2 and np.bincount(cell & 1).tolist() == [n // 2, n // 2]
    for kind in ("uniform", "zipf"):
        k = pm.b_keys(kind, bits, 64 * T)
        assert pm.strip_cell_max(k, bits, pm.plan_tiles(bits, 2048)) <= 4 * T
        assert int(k.max()) >> 32 != 0
    z = pm.b_keys("zipf", bits, 200_000)
    top = np.bincount((z & np.uint64((1 << bits) - 1)).astype(np.int64)).max()
    assert top > 20 * 200_000 / (1 << bits)                                                  # skewed: a bucket 20 times the mean


def test_table_b_wide_rows():
    seen = set()
    for name, tiles, n, pos in pm.b_wide_rows():
        p = pm.plan(pm.B_WIDE_BITS, n)
        assert p.tiles == tiles and 2048 <= pos < n - 2048                                   # k_rowid_sample does not see it
        tile = pos // T
        if name == "first tile of a strip":
            in_group = tile % p.group
            assert in_group % p.strip == 0 and in_group + p.strip <= p.group and tile + p.strip <= tiles       # a whole strip behind it
        else:
            assert tile == tiles - 1 and n % T != 0
        seen.add((name, p.strip))
    assert seen == {(nm, s) for nm in ("first tile of a strip", "last, partial tile") for s in (1, 2, 4)}


@pytest.mark.parametrize("bits", pm.C_BITS)
def test_table_c_counts(bits):
    G = pm.group_of(bits)
    n = G * T
    p = pm.plan(bits, n)
    assert p.groups == 1 and p.tiles == G and p.strip == 1 and p.busiest == 1
    assert pm.c_counts(bits) == [0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, n]
    assert pm.c_dstars(bits) == [0, p.bins1 - 1]
    for dstar in pm.c_dstars(bits):
        for cnt in pm.c_counts(bits):
            k = pm.c_keys(bits, dstar, cnt)
            h = np.bincount(pm.digit1(k, bits), minlength=p.bins1)
            assert len(k) == n and h[dstar] == cnt                                           # the exact total of pass-2 tile (d*, 0)
            assert -(-cnt // C.SR_TILE) == {0: 0, 1: 1, T - 1: 1, T: 1, T + 1: 2, 2 * T - 1: 2, 2 * T: 2, 2 * T + 1: 3}.get(cnt, G)
            if cnt < n:
                assert (h > 0).sum() == p.bins1 - (cnt == 0)                                  # the rest is spread over the other digits


@pytest.mark.parametrize("bits", pm.D_BITS)
def test_table_d_runs(bits):
    G = pm.group_of(bits)
    p = pm.plan(bits, G * T)
    assert p.groups == 1 and p.wave_runs == (bits == 9) and (G > 64) == (bits == 14)
    for place in pm.D_PLACES:
        m = pm.d_marked(place, bits)
        k = pm.d_keys(place, bits)
        assert np.array_equal(pm.digit1(k, bits) == pm.D_DSTAR, m)
        runs = pm.tile_counts(m)
        assert len(runs) == G
        if place == "every third tile":
            assert runs.tolist() == [1 if t % 3 == 0 else 0 for t in range(G)]
            assert runs.sum() <= 64 and (runs > 0).sum() > 4                                 # more than four runs under one 64-element round
        elif place == "runs 63 64 65":
            assert runs.tolist() == [63 + t % 3 for t in range(G)]
            starts = np.cumsum(runs) - runs
            assert set(starts % 64) == {0, 63}                                               # run borders on a round's first element and on its last
        elif place == "one full tile":
            assert runs.tolist() == [T if t == G // 2 else 0 for t in range(G)] and 0 < G // 2 < G - 1
        else:
            assert runs.tolist() == [0] * (G - 1) + [1] and m[-1]


@pytest.mark.parametrize("bits", pm.E_BITS)
def test_table_e_regimes(bits):
    for tiles, (fewest, most) in pm.E_TILES.items():
        n = pm.e_size(tiles)
        p = pm.plan(bits, n)
        assert p.tiles == tiles and n % T == pm.E_LAST and p.tiles2 > p.sgrid == 512
        seq = [s for s in pm.scatter_sequences(p) if len(s) >= 2]
        assert p.busiest == most >= 2 and min(len(s) for s in seq) >= fewest and seq         # "second tile": the busiest takes >= 2
        for kind in pm.E_KINDS[1:]:
            hot, absent = pm.e_digits(kind, bits)
            k = pm.e_keys(kind, bits, n)
            h = np.bincount(pm.digit1(k, bits), minlength=p.bins1)
            assert h[absent] == 0 and (h > 0).sum() == p.bins1 - 1 and 0.29 < h[hot] / n < 0.31 + 0.7 / (p.bins1 - 1)
            empty = set(range(absent * p.groups, (absent + 1) * p.groups))                   # pass-2 tiles without a tuple
            hot_tiles = set(range(hot * p.groups, (hot + 1) * p.groups))
            # tiles of many batches among one-batch tiles
            assert 0.3 * min(p.group, tiles) * T / C.SR_TILE > 3
            if "first" in kind:
                assert any(s[0] in empty for s in seq)                                       # an empty tile is a workgroup's first tile
            else:
                assert any(s[-1] in empty for s in seq)                                      # ... and a workgroup's last tile
            assert any(hot_tiles & set(s) and set(s) - hot_tiles for s in seq)                # a many-batch tile beside others in one sequence


@pytest.mark.parametrize("bits", pm.F_BITS)
def test_table_f_regimes(bits):
    assert pm.f_sizes() == [n for t in pm.F_TILES for n in (t * T, (t - 1) * T + 1)]
    for tiles in pm.F_TILES:
        for full in (True, False):
            p = pm.plan(bits, pm.b_size(tiles, full))
            assert p.passes == 1 and p.tiles == tiles
            what = pm.F_REGIMES[tiles]
            if what == "one chunk":
                assert p.chunks == 1
            elif what == "two chunks":
                assert p.chunks == 2 and p.per == 9
            elif what == "one scan round":
                assert p.chunks == 64 and p.scan_rounds == 1
            elif what == "carry in scan_bins":
                assert p.chunks == 65 and p.scan_rounds >= 2
            elif what == "full grid":
                assert p.hist_grid == 2048 and p.hist_strides == 1
            else:
                assert what == "grid stride" and p.hist_grid == 2048 and p.hist_strides == 2
    for kind in pm.F_KINDS:
        k = pm.f_keys(kind, bits, 2 * T)
        d = set((k & np.uint64((1 << bits) - 1)).astype(np.int64))
        assert len(d) == {"uniform": 1 << bits, "equal": 1, "absent": (1 << bits) - 1, "last": 1}[kind]
        if kind == "last":
            assert d == {(1 << bits) - 1}


def test_table_g_regimes():
    seen = []
    for name, bits, n in pm.g_rows():
        p = pm.plan(bits, n)
        seen.append((name, bits))
        if name == "chunk clamp":
            assert p.passes == 1 and p.chunks == 512 and p.per == 17 and p.empty_chunks > 0 and p.scan_rounds == 8 and p.hist_strides == 5
        elif name == "no shares":
            assert p.count_in_pass1 and p.S == 1 and p.R > 1 and p.rows // p.R < 4 and p.strip == 4
        elif name == "shares":
            assert p.count_in_pass1 and p.S >= 4 and p.R > 1 and p.rows % p.R != 0
        else:
            assert name == "hist_runs chunk 8" and not p.count_in_pass1 and p.chunk == 8 and p.hist_strides == 1 and p.busiest > 2
        assert n < 1 << 32
    assert seen == [("chunk clamp", 4), ("chunk clamp", 8), ("no shares", 9), ("no shares", 11), ("shares", 10), ("shares", 12),
                    ("hist_runs chunk 8", 14)]


def test_table_h_regimes():
    for bits in pm.H_BITS:
        for nR, nS in pm.h_sizes():
            pR, pS = pm.plan2(bits, nR, nS)
            small, large = (pR, pS) if nR < nS else (pS, pR)
            assert small.tiles in (1, 2) and large.tiles == 2050 and small.strip == large.strip == 4
            # the launch has the large side's strips; the small side's workgroups beyond its own write zero counts or return
            assert small.groups * small.parts < large.groups * large.parts
    pR, pS = pm.plan2(pm.H_ONE_PASS_BITS, 4097, pm.h_sizes()[0][1])
    assert pR.passes == 1 and pS.tiles > C.SMALL_TILES and pR.chunks == pS.chunks == 129 and pS.hist_strides == 2 and pR.hist_strides == 1
