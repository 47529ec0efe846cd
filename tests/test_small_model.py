"""tests/small_model.py against the sources it restates, against plain sums, against the oracle, and against the regimes the
shapes of tests/test_gpu_small_edges.py claim to reach.  CPU only."""
import numpy as np
import pytest

import small_model as sm
from helpers import make_rel

C = sm.constants()
T = C.SM_TILE
WHO = ("scatter", "plan")


def test_parsed_constants():
    """The values at this commit; a changed constant fails here with the new values in the message."""
    assert (C.SM_BLOCK, C.SM_V, C.SM_TILE, C.SM_MAX_TILES, C.SM_PARTS, C.SM_ROWS, C.SM_SELF_TILES) == (1024, 8, 8192, 512, 16, 8, 2), C
    assert (C.BJ_MAX_TILES, C.PT_MAX_BITS, C.PLAN_THREADS, C.SMALL_TILES) == (8, 8, 512, 512), C
    assert sm.SMALL_N * 2 == T and sm.SMALL_N % (1 << C.PT_MAX_BITS) == 0           # the small side: half a tile, every digit alike


def test_plan_threads_pattern_matches_the_source():
    """`tid >> 9`, `tid & 511u` and the two `512u` of the plan workgroup's Q all say PLAN_THREADS, half the workgroup"""
    assert sm.plan_threads_in_source(sm._read("rhj_small.hip.h")) == (sm.PLAN_THREADS,) * 4
    assert 2 * sm.PLAN_THREADS == C.SM_BLOCK


def test_constants_follow_the_sources():
    def moved(old, new, name="rhj_small.hip.h"):
        def read(n):
            t = sm._read(n)
            if n == name:
                assert old in t
                t = t.replace(old, new)
            return t
        return sm.parse_constants(read)
    c = moved("SM_PARTS = 16;", "SM_PARTS = 8;")
    assert sm.colsum_geometry(17, 2, "scatter", c).per == 3
    c = moved("SM_ROWS = 8;", "SM_ROWS = 4;")
    assert sm.colsum_geometry(128, 8, "scatter", c).rounds[0] == 2
    c = moved("SM_SELF_TILES = 2;", "SM_SELF_TILES = 3;")
    assert sm.self_hist(3 * T, 1, c) and not sm.self_hist(3 * T + 1, 1, c)
    with pytest.raises(AssertionError, match="threads a relation"):
        moved("const uint32_t rel = tid >> 9, tt = tid & 511u;", "const uint32_t rel = tid >> 8, tt = tid & 255u;")
    with pytest.raises(AssertionError, match="threads a relation"):
        moved("Q = min(512u / lanes, SM_PARTS);", "Q = min(256u / lanes, SM_PARTS);")
    with pytest.raises(AssertionError, match="no longer finds"):
        moved("rb += 2 * SM_ROWS", "rb += SM_ROWS")
    with pytest.raises(AssertionError, match="no longer finds"):
        moved("row1 = min(row0 + per, r.tiles);", "row1 = row0 + per;")


# ---- every shape in the regime its name claims ------------------------------------------------------------------------------------
def used(g):
    return [s for s in g.slices if s[1] > s[0]]


def test_self_count_shapes():
    top = C.SM_SELF_TILES * T
    assert sm.a_sizes() == [(8192, 8192), (8193, 4096), (16384, 16384), (16384, 1), (16385, 16384), (16385, 4096)]
    want = [True, True, True, True, False, False]
    for (nR, nS), self_ in zip(sm.a_sizes(), want):
        assert sm.self_hist(nR, nS) == sm.self_hist(nS, nR) == self_, (nR, nS)
        assert all(sm.takes(b, nR, nS) and sm.takes(b, nS, nR) for b in sm.A_BITS)
    assert sm.tiles(top) == C.SM_SELF_TILES and sm.tiles(top + 1) == C.SM_SELF_TILES + 1      # the first histogram launch: a one-tuple last tile
    assert sm.tiles(T) == 1 and sm.tiles(T + 1) == 2 and sm.tiles(1) == 1
    assert set(sm.E_A_TILES) == {max(sm.tiles(a), sm.tiles(b)) for a, b in sm.a_sizes()} - {1}


def test_slice_edge_shapes():
    """B: Q = 16 slices for a scatter workgroup at every width; the plan's workgroup has 8 at 8 bits"""
    for bits in sm.B_BITS:
        Q = {t: sm.colsum_geometry(t, bits, "scatter") for t in sm.B_TILES}
        assert all(g.Q == C.SM_PARTS == 16 for g in Q.values())
        assert Q[3].per == 1 and len(used(Q[3])) == 3                                  # per == 1, 13 empty slices
        assert Q[15].per == 1 and len(used(Q[15])) == 15
        assert Q[16].per == 1 and len(used(Q[16])) == 16                               # the last tile count of one row a slice
        assert Q[17].per == 2 and used(Q[17]) == [(2 * q, 2 * q + 2) for q in range(8)] + [(16, 17)]    # slices 0..8, the last of one row
        assert len(Q[17].slices) - len(used(Q[17])) == 7
        assert all(r <= 1 for t in sm.B_TILES for r in (Q[t].rounds if bits >= 2 else []))
        P = {t: sm.colsum_geometry(t, bits, "plan") for t in sm.B_TILES}
        if bits == 8:
            assert all(g.Q == 8 for g in P.values())
            assert P[8].per == 1 and len(used(P[8])) == 8
            assert P[9].per == 2 and used(P[9]) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 9)] and len(P[9].slices) == 8
            assert P[17].per == 3 and used(P[17])[-1] == (15, 17)
        else:
            assert all(P[t].slices == Q[t].slices for t in sm.B_TILES)
    # the narrow widths: one thread a digit below 2 bits (rows read one by one), one lane a slice at 2 bits
    assert sm.colsum_geometry(17, 1, "scatter").round_rows == 1 and sm.colsum_geometry(17, 2, "scatter").round_rows == C.SM_ROWS
    assert sm.colsum_geometry(17, 1, "plan").round_rows == 1 and sm.colsum_geometry(17, 2, "plan").round_rows == 2 * C.SM_ROWS


def test_round_edge_shapes():
    """C: the second round of loads, and the top of the path"""
    R = C.SM_ROWS
    for bits in sm.C_BITS:
        S = {t: sm.colsum_geometry(t, bits, "scatter") for t in sm.C_ROWS}
        P = {t: sm.colsum_geometry(t, bits, "plan") for t in sm.C_ROWS}
        assert (S[128].per, S[129].per, S[256].per, S[257].per, S[512].per) == (R, R + 1, 2 * R, 2 * R + 1, 4 * R)
        assert used(S[129])[-1] == (126, 129) and used(S[257])[-1] == (255, 257) and len(used(S[129])) == 15
        if bits >= 2:
            assert set(S[128].rounds) == {1} and S[129].rounds[0] == 2                 # per = SM_ROWS + 1: a second round of one row
            assert set(S[256].rounds) == {2} and S[257].rounds[0] == 3
        if bits == 8:                                                                  # Q = 8, rounds of 2 * SM_ROWS: the edge is at 128 -> 129
            assert P[128].per == 2 * R and set(P[128].rounds) == {1}
            assert P[129].per == 2 * R + 1 and P[129].rounds == [2] * 7 + [1] and used(P[129])[-1] == (119, 129)
            assert P[257].per == 33 and P[257].rounds[0] == 3
        else:                                                                          # Q = 16: at 256 -> 257
            assert P[256].per == 2 * R and P[257].per == 2 * R + 1
            if bits >= 2:
                assert set(P[128].rounds) == set(P[256].rounds) == {1} and set(P[129].rounds) == {0, 1}      # (129: one empty slice)
                assert P[257].rounds[:15] == [2] * 15 and used(P[257])[-1] == (255, 257)
    top = C.SM_MAX_TILES * T
    assert C.SM_MAX_TILES == C.SMALL_TILES == 512 and max(sm.C_ROWS) == C.SM_MAX_TILES
    for bits in sm.C_BITS:
        assert sm.takes(bits, top, sm.SMALL_N) and sm.takes(bits, sm.SMALL_N, top)
        assert not sm.takes(bits, top + 1, sm.SMALL_N) and not sm.takes(bits, sm.SMALL_N, top + 1)
    assert not sm.takes(C.PT_MAX_BITS + 1, T, T)


def test_other_shapes():
    """D..H"""
    nR, nS = sm.D_TILES[0] * T, sm.D_TILES[1] * T
    for kind in sm.D_KINDS:
        kR, kS = sm.d_keys(kind)
        assert len(np.unique(kR)) == nR == len(kR) and len(kS) == nS and np.isin(kS, kR).all()
        for bits, path in sm.D_BITS.items():
            e = sm.expected(kR, kS, bits)
            assert sm.takes(bits, nR, nS) and not sm.self_hist(nR, nS)
            assert (e.path == "small") == (path == "small"), (kind, bits, e)           # 2 bits: a build side beyond the LDS index
            if path != "small":
                assert e.max_build > C.FUSED_LDS_CAP
    assert set(sm.E_B_TILES) <= set(sm.B_TILES) and set(sm.E_C_TILES) <= set(sm.C_ROWS) and set(sm.F_TILES) <= set(sm.B_TILES) | set(sm.C_ROWS)
    assert sm.G_STEPS == ((512, 8), (3, 2), (257, 1), (17, 8), (2, 8), (129, 2))
    assert sm.G_STEPS[0][0] == C.SM_MAX_TILES and sm.self_hist(sm.G_STEPS[4][0] * T, sm.SMALL_N)
    for bits in sm.H_BITS:
        rows = sm.h_joins(bits)
        assert len(rows) == 60 and max(sm.H_TILES) == C.BJ_MAX_TILES
        assert {(k, t, f) for k, t, f, _ in rows} == {(k, t, f) for k in sm.KINDS for t in sm.H_TILES for f in (True, False)}
        assert {(k, o) for k, _, _, o in rows} == {(k, o) for k in sm.KINDS for o in (True, False)}
        assert rows != sorted(rows)
        for _, t, f, _ in rows:
            n = sm.size_of(t, f)
            assert sm.tiles(n) == t and n <= C.BJ_MAX_TILES * T and sm.self_hist(n, sm.SMALL_N) == (t <= C.SM_SELF_TILES)


# ---- the keys ------------------------------------------------------------------------------------------------------------------------
def test_key_kinds():
    for bits in sm.B_BITS:
        bins = 1 << bits
        small = sm.small_keys(bits)
        d = (small.astype(np.uint32) & np.uint32(bins - 1)).astype(np.int64)
        assert len(np.unique(small)) == sm.SMALL_N and (np.bincount(d, minlength=bins) == sm.SMALL_N // bins).all()
        assert (small >> np.uint64(32)).max() > 0 and small.max() < 1 << 46
        for n in (17 * T, 16 * T + 1):
            for kind in sm.KINDS:
                k = sm.large_keys(kind, bits, n)
                assert np.isin(k, small).all() and np.array_equal(k[:3 * T], sm.large_keys(kind, bits, n)[:3 * T])
                cnt = sm.tile_hist(k, bits)
                assert cnt.shape == (17, bins) and int(cnt.sum()) == n and int(cnt[-1].sum()) == n - 16 * T
                if kind == "tile_digit":                                               # one column a row, the next row another
                    assert all(cnt[t, t % bins] == cnt[t].sum() for t in range(17))
                elif kind == "one_digit_last":
                    assert (cnt[:, bins - 1] == cnt.sum(1)).all()
                elif kind == "one_digit_first":
                    assert (cnt[:, 0] == cnt.sum(1)).all()
                elif kind == "last_tile_only":
                    assert (cnt[:-1, bins - 1] == 0).all() and cnt[-1, bins - 1] == n - 16 * T
                else:
                    assert (cnt[:-1] > 0).all() or bits == 8
    # a partner without keys of some digit: those tuples match nothing
    k, other = sm.a_keys("tile_digit", 2, 2 * T, 1)
    assert len(other) == 1 and (k[:T] == other[0]).all() and not np.isin(k[T:], other).any() and k.max() < 1 << 47


# ---- the column sums as written, against plain sums ----------------------------------------------------------------------------------
def cnt_of(kind, bits, ntiles, full):
    """the large side's histogram rows (test_key_kinds: the keys' digits are digits())"""
    return sm.tile_hist(None, bits, digits=sm.digits(kind, bits, sm.size_of(ntiles, full)))


def tiles_asked(ntiles, bits):
    ts = {0, 1, ntiles - 1}
    for who in WHO:
        for r0, r1 in sm.colsum_geometry(ntiles, bits, who).slices:
            ts |= {r0 - 1, r0, r0 + 1, r1 - 1, r1, r1 + 1}
    return sorted(t for t in ts if 0 <= t < ntiles)


@pytest.mark.parametrize("bits", sm.B_BITS)
def test_colsum_adds_up(bits):
    for ntiles in sm.all_tile_counts():
        for full in (True, False):
            for kind in ("uniform", "tile_digit", "last_tile_only"):
                cnt = cnt_of(kind, bits, ntiles, full)
                assert len(cnt) == ntiles
                ts = tiles_asked(ntiles, bits)
                run = np.concatenate([np.zeros((1, 1 << bits), dtype=np.int64), np.cumsum(cnt.astype(np.int64), axis=0)])
                for who in WHO:
                    bf, al = sm.colsum_many(cnt, ts, bits, who)
                    what = (ntiles, full, kind, bits, who)
                    assert np.array_equal(al, cnt.sum(0)), what
                    assert np.array_equal(bf, run[ts]), what
    cnt = cnt_of("tile_digit", bits, 17, False)
    for t in (0, 16):
        bf, al = sm.colsum(cnt, t, bits, "scatter")
        assert np.array_equal(bf, cnt[:t].sum(0)) and np.array_equal(al, cnt.sum(0))


@pytest.mark.parametrize("bits", sm.A_BITS)
def test_selfhist_adds_up(bits):
    for n in (1, T // 2, T, T + 1, 2 * T):
        for kind in sm.A_KINDS:
            k = sm.large_keys(kind, bits, n)
            cnt = sm.tile_hist(k, bits)
            for t in range(sm.tiles(n)):
                bf, al = sm.selfhist(k, t, bits)
                assert np.array_equal(bf, cnt[:t].sum(0)) and np.array_equal(al, cnt.sum(0))


@pytest.mark.parametrize("bits", (1, 2, 8))
def test_structured_rows_show_a_wrong_row_range(bits):
    """What the key kinds are for: sums over one row too few, a dropped second round or a skipped short tail are wrong on
    tile_digit rows by a multiple of a tile, and on last_tile_only rows in the last digit — on the restatement, not the device."""
    for ntiles, who in ((17, "scatter"), (129, "scatter"), (129, "plan"), (257, "plan")):
        g = sm.colsum_geometry(ntiles, bits, who)
        last = max(q for q, s in enumerate(g.slices) if s[1] > s[0])
        short = list(g.slices)
        short[last] = (short[last][0], short[last][1] - 1)                     # the last slice's tail
        one_round = [(r0, min(r1, r0 + g.round_rows)) for r0, r1 in g.slices]  # no second round
        for kind in ("tile_digit", "last_tile_only"):
            cnt = cnt_of(kind, bits, ntiles, False)
            for wrong in (short, one_round):
                if wrong == list(g.slices):
                    continue
                _, al = sm.colsum(cnt, 0, bits, who, geom=g._replace(slices=wrong))
                diff = cnt.sum(0).astype(np.int64) - al
                assert diff.any(), (ntiles, who, kind)
                if kind == "last_tile_only" and wrong is short:
                    assert diff[-1] == 1 and not diff[:-1].any()


# ---- every large-side tuple has one partner --------------------------------------------------------------------------------------------
def fk_shapes():
    for t in sm.B_TILES:
        for bits in sm.B_BITS:
            for kind in sm.B_KINDS:
                for full in (True, False):
                    yield kind, bits, sm.size_of(t, full)
    for t, (fulls, kinds) in sm.C_ROWS.items():
        for bits in sm.C_BITS:
            for kind in kinds:
                for full in fulls:
                    yield kind, bits, sm.size_of(t, full)


def check_fk(oracle, kL, kS, bits, what, orders=(True, False)):
    """(which relation is R does not change who has a partner: the callers take the orders in turn, shape by shape)"""
    L, S = make_rel(kL), make_rel(kS)
    for large_is_r in orders:
        pairs = oracle.join(L, S, bits) if large_is_r else oracle.join(S, L, bits)
        ids = pairs["row_idR" if large_is_r else "row_idS"]
        assert len(pairs) == len(L), what
        assert (np.bincount(ids.astype(np.int64), minlength=len(L)) == 1).all(), what
    e = sm.expected(kL, kS, bits)
    assert e.path == "small" and e.max_build <= sm.SMALL_N >> bits and e.units >= 1, (what, e)


def test_slice_edge_shapes_are_foreign_key_joins(oracle):
    for i, (kind, bits, n) in enumerate(s for s in fk_shapes() if s[2] <= max(sm.B_TILES) * T):
        check_fk(oracle, sm.large_keys(kind, bits, n), sm.small_keys(bits), bits, (kind, bits, n), orders=(i % 2 == 0,))


@pytest.mark.parametrize("bits", sm.C_BITS)
def test_round_edge_shapes_are_foreign_key_joins(oracle, bits):
    big = [(kind, n) for kind, b, n in fk_shapes() if n > max(sm.B_TILES) * T and b == bits]
    for i, (kind, n) in enumerate(big):
        check_fk(oracle, sm.large_keys(kind, bits, n), sm.small_keys(bits), bits, (kind, bits, n), orders=(i % 2 == 0,))
    for n in (C.SM_MAX_TILES * T + 1,):                                                # beyond the top
        k = sm.large_keys("tile_digit", bits, n)
        assert sm.expected(k, sm.small_keys(bits), bits).path is None
        assert len(oracle.join(make_rel(k), make_rel(sm.small_keys(bits)), bits)) == n
