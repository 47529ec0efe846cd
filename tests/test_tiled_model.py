"""tests/tiled_model.py against the sources it restates and against the properties the GPU cases of
tests/test_gpu_tiled_edges.py rely on.  CPU only."""
import re

import numpy as np
import pytest

import hashkeys as hk
import tiled_model as tm

C = tm.constants()


def test_parsed_constants():
    """The values at this commit; a changed constant fails here with the new derived values in the message."""
    assert (C.LDS_MAX_SLOTS, C.tiled_cap, C.fused_cap, C.forced_cap) == (40960, 32768, 35925, 0), C
    assert C.fused_cap == C.FUSED_LDS_CAP and C.tiled_cap == C.LDS_MAX_SLOTS * 4 // 5
    assert (C.PR_UNIT, C.BUILD_CHUNK, C.T32_PAD, C.SCAN_BLOCK) == (1024, 4096, 8, 1024), C
    assert (C.SLOT_FLOOR, C.SLOT_ADD, C.SLOT_GRANULE) == (64, 4, 4), C
    # rhj_device.hip's static_assert: a 32-bit table's entry holds position + 1 in 16 bits
    assert C.tiled_cap <= 65534 and C.fused_cap <= 65534
    # k_build_lds dumps 16-byte groups, Tab32::load_chunk reads them: every size is a multiple of 4
    assert C.SLOT_GRANULE % 4 == 0 and C.SLOT_FLOOR % 4 == 0 and C.LDS_MAX_SLOTS % 4 == 0 and C.T32_PAD % 4 == 0


def test_the_header_comment_states_the_unit():
    m = re.search(r"constexpr int PR_UNIT = PR_BLOCK \* PR_V;\s*// (\d+) probe tuples per unit", tm._read("rhj_join_tiled.hip.h"))
    assert m and int(m.group(1)) == C.PR_UNIT


def test_constants_follow_the_sources():
    """Moving a constant in (a copy of) the sources moves the model's edges."""
    def moved(name, old, new):
        def read(n):
            t = tm._read(n)
            if n == name:
                assert old in t
                t = t.replace(old, new)
            return t
        return tm.parse_constants(read)
    c = moved("rhj_device.hip", "LDS_BUDGET = 160 * 1024;", "LDS_BUDGET = 128 * 1024;")
    assert (c.LDS_MAX_SLOTS, c.tiled_cap, c.fused_cap) == (32768, 26214, (128 * 1024 - C.FJ_LDS_EXTRA - 128) * 2 // 9)
    assert tm.build_edges(c.tiled_cap, c)[-3:] == [26213, 26214, 26215] and tm.first_full_build(c) < tm.first_full_build(C)
    c = moved("rhj_join_tiled.hip.h", "PR_V = 4;", "PR_V = 8;")
    assert c.PR_UNIT == 2048 and tm.probe_edges(c)[3] == (2049, 2048)
    c = moved("rhj_device.hip", "BUILD_CHUNK = 4096;", "BUILD_CHUNK = 1000;")
    assert tm.chunk_edges(c)[:5] == [999, 1000, 1001, 2000, 2001]
    c = moved("rhj_join_tiled.hip.h", "T32_PAD = 8;", "T32_PAD = 12;")
    assert tm.plan([3], [5], c.tiled_cap, c).table_slots == 64 + 12
    c = moved("rhj_join_tiled.hip.h", "+ 4u;", "+ 8u;")
    assert c.SLOT_ADD == 8 and tm.last_floor_build(c) < tm.last_floor_build(C)


def test_lds_slots_for():
    f = tm.lds_slots_for
    assert [f(bc) for bc in (1, 39, 40, 41, 43, 44)] == [64, 64, 64, 68, 68, 72]
    assert tm.last_floor_build() == 40
    # the table stops growing at 27 302 build tuples (27302 + 13651 + 4 = 40957, rounded up to the granule: LDS_MAX_SLOTS), the
    # min() first cuts at 27 305, and from 27 307 on the load factor is above 2/3
    assert tm.first_full_build() == 27302 and f(27301) == 40956 and f(27302) == 40960 == C.LDS_MAX_SLOTS
    assert tm.first_clamped_build() == 27305
    assert all(3 * bc <= 2 * f(bc) for bc in range(1, 27307)) and 3 * 27307 > 2 * f(27307)
    assert all(f(bc) % 4 == 0 and f(bc) > bc for bc in list(range(1, 3000)) + list(range(27000, C.fused_cap + 1)))
    assert C.tiled_cap / f(C.tiled_cap) == 0.8
    assert round(C.fused_cap / f(C.fused_cap), 3) == 0.877 and C.fused_cap < f(C.fused_cap)


def test_tab64_sizing():
    assert [1 << tm.tab64_lg(bc) for bc in (1, 2, 3, 4, 5, 4096, 4097, 65535, 65536, 65537)] == \
        [2, 4, 8, 8, 16, 8192, 16384, 131072, 131072, 262144]
    for bc in (1, 2, 3, 1000, 4096, 4097, 65536):
        assert (1 << tm.tab64_lg(bc)) >= 2 * bc > (1 << tm.tab64_lg(bc)) // 2


def test_plan_on_a_hand_made_histogram():
    histR = [0, 5, 7, 7, 40000, 3000, 1, 0]
    histS = [9, 0, 7, 8, 50000, 1000, 1, 0]
    p = tm.plan(histR, histS, C.tiled_cap)
    assert list(p.flip) == [False, False, False, True, True, False, False, False]
    assert list(p.pc) == [0, 0, 7, 8, 50000, 3000, 1, 0] and list(p.bc) == [0, 0, 7, 7, 40000, 1000, 1, 0]
    assert list(p.mode) == [0, 0, 1, 1, 2, 1, 1, 0]
    assert p.units == 1 + 1 + 49 + 3 + 1 and p.hbm_units == 10 and p.max_build == 40000 and p.lds_buckets == 4
    assert p.table_slots == 131072 + (64 + 8) * 3 + (1504 + 8)
    q = tm.plan(histR, histS, C.forced_cap)
    assert list(q.mode) == [0, 0, 2, 2, 2, 2, 2, 0] and q.tab32_slots == 0 and q.hbm_units == 1 + 1 + 10 + 1 + 1
    assert q.table_slots == 16 + 16 + 131072 + 2048 + 2
    assert tm.plan(histR, histS, 40000).hbm_units == 0 and tm.plan(histR, histS, 39999).hbm_units == 10


def gpu_case_sizes():
    """(name, bits, {bucket: (cR, cS)}, lds_cap) of the GPU cases that are built from bucket sizes"""
    for cap in (C.tiled_cap, C.fused_cap):
        for lay in (tm.sides_by_parity, tm.sides_with_ties):
            for lds_cap in (cap, C.forced_cap):
                yield "a", 3, lay(tm.build_edges(cap)), lds_cap
    for lds_cap in (C.tiled_cap, C.forced_cap):
        yield "b chunks", 3, tm.sides_by_parity(tm.chunk_edges()), lds_cap
        yield "b probes", 3, tm.probe_edges(), lds_cap
        for u in (1, 7, 8, 9, 17):
            yield "b units", 4, tm.unit_total_sizes(u), lds_cap
    for bits in (12, 14):
        yield "f", bits, {5: (33000, 36000), **{b: (73, 73) for b in range(6, 1 << bits)}}, C.tiled_cap
    yield "f", 9, {5: (C.fused_cap + 1, C.fused_cap + 3001), **{b: (1200, 1200) for b in range(6, 512)}}, C.fused_cap


def test_tab32_arena_bound():
    """join_tiled's 32-bit arena (nmin + nmin / 2 + 80 bins + 64 entries) holds every plan's tables, pads included; per bucket
    that is slots + T32_PAD <= bc + bc / 2 + 80."""
    assert all(tm.lds_slots_for(bc) + C.T32_PAD <= bc + bc // 2 + 80 for bc in range(1, C.fused_cap + 1))
    for name, bits, sizes, cap in gpu_case_sizes():
        hR, hS = np.zeros(1 << bits, dtype=np.int64), np.zeros(1 << bits, dtype=np.int64)
        for b, (r, s) in sizes.items():
            hR[b], hS[b] = r, s
        p = tm.plan(hR, hS, cap)
        assert p.tab32_slots <= tm.tab32_arena_bound(hR.sum(), hS.sum(), bits), (name, bits, cap)
        assert p.units <= (1 << bits) + (hR.sum() + hS.sum()) // C.PR_UNIT + 2                    # plan_args: max_units
        assert p.hbm_units <= (1 << bits) + min(hR.sum(), hS.sum()) // C.BUILD_CHUNK + 2           # plan_args: max_bunits
    for n in (1023, 1024, 1025, 2048):
        for extra in (False, True):
            R, S = tm.scan_block_keys(n, 11, extra)
            hR, hS = tm.histograms(R, S, 11)
            p = tm.plan(hR, hS, C.tiled_cap)
            assert p.units == n + extra and p.tab32_slots <= tm.tab32_arena_bound(len(R), len(S), 11)
    for table in (32, 64):
        R, S, units = tm.stash_bucket(table, 3, 3, True, 5)
        p = tm.plan(*tm.histograms(R, S, 3), C.tiled_cap)
        assert p.units == units and p.tab32_slots <= tm.tab32_arena_bound(len(R), len(S), 3)


@pytest.mark.parametrize("nu", list(range(1, 41)) + [1023, 1024, 1025])
def test_xcd_deal_visits_every_unit_once(nu):
    got = tm.xcd_deal(nu)
    assert len(got) == (nu + 7) // 8 * 8
    assert sorted(u for u in got if u is not None) == list(range(nu))
    if nu % 8 and nu > 8:                          # what the map would do with per = nu / 8: units are left out
        short = tm.xcd_deal(nu, per=nu // 8)
        assert sorted(u for u in short if u is not None) != list(range(nu))


def test_scan_block_counts_differ_between_neighbours():
    R, S = tm.scan_block_keys(C.SCAN_BLOCK + 1, 11)
    hR, hS = tm.histograms(R, S, 11)
    pairs = (hR * hS)[:C.SCAN_BLOCK + 1]
    assert pairs.min() >= 1 and np.all(np.diff(pairs) != 0) and set(pairs) == {1, 2, 3, 4, 6, 9}
    assert np.all((hR * hS)[C.SCAN_BLOCK + 1:] == 0) and (hR + hS)[C.SCAN_BLOCK + 1:].max() == 1


@pytest.mark.parametrize("table", [32, 64])
@pytest.mark.parametrize("filler", [0, 150])
def test_wrap_clusters_land_where_they_claim(table, filler):
    """home = slots - 1 - j with one tag, at the model's table size for the bucket's build side; the keys behind the wrap at
    slots 0..3 with tags on both sides of it (wrap_cluster asserts the same for every GPU case it builds)."""
    b, bits = 5, 3
    for j in range(4):
        for size, dup in ((1, False), (13, False), (9, True)):
            w = tm.wrap_cluster(table, b, bits, j, size, dup, filler, seed=j)
            assert w["bc"] == len(w["R"]) and len(w["S"]) > len(w["R"])
            h = hk.mix64(np.concatenate([w["cluster"], w["absent_same"]]))
            if table == 32:
                assert w["slots"] == tm.lds_slots_for(w["bc"]) and (w["slots"] == C.SLOT_FLOOR) == (filler == 0)
                assert set(hk.mix_slot(h, w["slots"])) == {w["slots"] - 1 - j} and set(hk.mix_raw_tag(h)) == {w["tag"]}
                assert list(hk.mix_slot(hk.mix64(w["low"]), w["slots"])) == [s for s, _ in tm.WRAP_LOW]
                assert (w["slots"] - 1 - j) & 3 == 3 - j                      # Tab32::skip
            else:
                assert w["slots"] == 1 << tm.tab64_lg(w["bc"])
                assert set(hk.tab64_home(h, w["tsize"])) == {w["slots"] - 1 - j} and set(hk.tab64_tag(h)) == {w["tag"]}
                assert list(hk.tab64_home(hk.mix64(w["low"]), w["tsize"])) == [s for s, _ in tm.WRAP_LOW]
            assert not np.isin(w["absent_same"], w["R"]).any() and not np.isin(w["other"], w["R"]).any()
            assert (np.sort(w["R"])[1:] == np.sort(w["R"])[:-1]).sum() == (2 if dup else 0)


@pytest.mark.parametrize("table", [32, 64])
def test_stash_bucket(table):
    for flagged in (False, True):
        R, S, units = tm.stash_bucket(table, 3, 3, flagged, 5)
        assert len(S) > len(R) and units == -(-len(S) // C.PR_UNIT) >= 4
        keys, counts = np.unique(R, return_counts=True)
        assert sorted(counts[counts > 1]) == sorted(r for r in tm.STASH_REPEATS if r > 1 for _ in range(2))
        # a unit's count pass is flagged by a probe key that shares its tag with ANOTHER build key
        tagR = {int(t): int(k) for k, t in zip(keys, tm._tag(table, keys))}
        assert len(tagR) == len(keys)
        flagging = np.array([int(t) in tagR and tagR[int(t)] != int(k) for k, t in zip(S, tm._tag(table, S))])
        unit = np.arange(len(S)) // C.PR_UNIT
        assert sorted(set(unit[flagging])) == ([u for u in range(units) if u % 2] if flagged else [])
