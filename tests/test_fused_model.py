"""tests/fused_model.py on the CPU: its constants against the sources, its geometry against hand-computed values, and every
shape of tests/fused_shapes.py in the regime its name states — the exact overflow total, patch count, slot length, run length,
records a group, units a bucket and route — with the model's pair list held to helpers.spec_join."""
import numpy as np
import pytest

import fused_model as fm
import fused_shapes as fs
from helpers import spec_join

C = fm.constants()


def test_constants_come_from_the_sources():
    assert C.FJ_OVF_ENT == C.FJ_OVF_CAP - C.FJ_PATCH_CAP // 2          # the patch words are the tail of the overflow buffer
    assert C.FJ_GROUPS * C.GROUP == C.FJ_SPAN and C.GROUP == C.FJ_V * C.WAVE
    assert C.FJ_BATCH == C.FJ_BLOCK * C.FJ_V and C.FUSED_LDS == C.LDS_BUDGET - C.FJ_LDS_EXTRA
    assert C.FUSED_LDS_CAP == (C.FUSED_LDS - 128) * 2 // 9 and C.FUSED_LDS_CAP <= 65534
    assert C.COUNT_SAT == 127 and C.FJ_OVF_J + 1 == C.FJ_LONG          # 16 matches: the last with an overflow run / an inserted slot
    assert C.FJ_RUN_LOCK == C.WAVE


def test_a_missing_constant_fails_loudly():
    def read(name):
        return fm._read(name).replace("FJ_PATCH_CAP = 128", "FJ_PATCH_CAP_X = 128")
    with pytest.raises((AssertionError, NameError)):
        fm.parse_constants(read)

    def read2(name):
        return fm._read(name).replace("nmin / bins <= 7000", "nmin / bins < 7001")
    with pytest.raises(AssertionError):
        fm.parse_constants(read2)

    def read3(name):
        return fm._read(name).replace("npatch > FJ_PATCH_CAP", "npatch >= FJ_PATCH_CAP")
    with pytest.raises(AssertionError):
        fm.parse_constants(read3)


def test_geometry():
    assert fm.geometry(1) == (64, True) and fm.geometry(63)[0] == 64 and fm.geometry(64)[0] == 64 and fm.geometry(65)[0] == 65
    lim = fm.resident_limit()
    assert fm.geometry(lim)[1] and not fm.geometry(lim + 1)[1]
    bcp = (lim + 3) & ~3
    assert bcp * 20 + (lim + 3) // 2 * 4 + 64 <= C.FUSED_LDS                  # 20 bytes a tuple, 2 a slot
    hs, fits = fm.geometry(C.FUSED_LDS_CAP)
    assert not fits and hs < C.FUSED_LDS_CAP and hs >= C.FUSED_LDS_CAP // 4   # fewer, longer slots; never below a quarter
    assert 4 * ((C.FUSED_LDS_CAP + 3) & ~3) + 4 * 8 + 2 * (hs + 2) + 64 <= C.FUSED_LDS + 32
    assert fm.fused_span_for(256, 10 ** 6, 10 ** 6) == C.FJ_SPAN and fm.fused_span_for(16, 20_000, 16_000) == C.FJ_BATCH
    assert fm.fused_span_for(16, 512 * 3 * 4096, 5) == 3 * C.FJ_BATCH and fm.fused_span_for(16, 512 * (3 * 4096 + 1), 5) == 4 * C.FJ_BATCH


def test_window_rule_against_a_literal_walk():
    """Index.probe (vectorised) against fj_lookup / fj_round restated entry by entry: windows of FJ_WIN, a window's hits
    lowest index first, the next window once the mask is empty and more than FJ_WIN entries were left."""
    rng = np.random.default_rng(1)
    bits, b, hs = 8, 9, 64
    ks = fs.slot_keys("mix64", b, bits, hs, 5, [0x10, 0x11], 12, seed=1)
    build = rng.permutation(np.concatenate([np.repeat(ks[0][:6], 3), ks[1][:7], fs.rand_keys(rng, b, bits, 20)]))
    X = fm.Index(build, bits, hs, False)
    ent_tag, ent_pos = (fm.slot_tag(build, bits, hs, False)[1])[X.order], X.order
    start = np.concatenate([[0], np.cumsum(X.slot_len)])
    probe = np.concatenate([ks[0], ks[1]])
    c, fp, bm, L, first, _ = X.probe(probe)
    slots, tags = fm.slot_tag(probe, bits, hs, False)
    for i, key in enumerate(probe):
        at, n = int(start[slots[i]]), int(X.slot_len[slots[i]])
        rnd, cc, ffp, bbm = 0, 0, False, 0
        while True:
            hits = [j for j in range(min(n, C.FJ_WIN)) if ent_tag[at + j] == tags[i]]
            for j in hits:
                eq = build[ent_pos[at + j]] == key
                cc += eq; ffp = ffp or not eq; bbm |= int(eq) << min(rnd, 31); rnd += 1
            if n <= C.FJ_WIN:
                break
            at, n = at + C.FJ_WIN, n - C.FJ_WIN
        assert (cc, ffp, bbm, rnd) == (c[i], fp[i], int(bm[i]), L[i]), i
    assert L.max() == 18 and X.slot_len[5] >= 25 and fp.any() and (c == 3).any()       # three windows and more, foreign hits between matches


def check_expect(m, s):
    units = m.units_of(s.b)
    assert len(units) == len(s.expect), (s.name, len(units))
    for u, e in zip(units, s.expect):
        for k, v in e.items():
            if k == "check":
                assert v(u), (s.name, "check")
            else:
                assert getattr(u, k) == v, (s.name, k, getattr(u, k), v)
    if s.walk is not None:                                # (a background bucket may add a walked unit of its own: a 16-bit tag collision)
        assert sum(u.route == "walk" for u in units) == s.walk, s.name
        assert m.walk_units >= s.walk


def pairs_hold(s, buckets):
    """The model's pair list against helpers.spec_join, on the planted bucket and a few others (spec_join is a Python loop)."""
    mask = np.uint64((1 << s.bits) - 1)
    keep = np.array(sorted(buckets), dtype=np.uint64)
    R, S = s.R[np.isin(s.R["value"] & mask, keep)], s.S[np.isin(s.S["value"] & mask, keep)]
    want = spec_join(R, S, s.bits)
    got = fm.model(R, S, s.bits, s.knobs).pairs
    assert len(got) == len(want) and np.array_equal(got[:, 0], want["row_idR"]) and np.array_equal(got[:, 1], want["row_idS"]), s.name


@pytest.mark.parametrize("case", list(fs.CASES))
def test_shape_is_in_its_regime(case):
    s = fs.build(case)
    m = fm.model(s.R, s.S, s.bits, s.knobs, with_pairs=False)
    assert m.fused_ok and m.path == ("small" if s.bits <= C.PT_MAX_BITS else "fused")
    assert len(s.R) + len(s.S) < 260_000
    check_expect(m, s)
    if s.extra.get("background_ovf"):
        others = [u for u in m.units if u.bucket != s.b]
        assert sum(u.ovf_total > 0 for u in others) > len(others) // 2
    bins = 1 << s.bits
    pairs_hold(s, {s.b, (s.b + 1) % bins, (s.b + 97) % bins})


@pytest.mark.parametrize("resident", [0, 1])
def test_deferred_mix(resident):
    s = fs.deferred(resident)
    m = fm.model(s.R, s.S, s.bits, s.knobs, with_pairs=False)
    kinds = s.extra["kinds"]
    assert m.path == "fused" and m.mayres == bool(resident) and not m.try_spec
    assert max(m.cR.max(), m.cS.max()) <= 400 and ((m.cR > 0) | (m.cS > 0)).all()
    assert len(m.units) == len(fs.unit_kinds(kinds)) and len(m.units) > 3 * 256        # some four units a workgroup
    want = {"none": {"stream"}, "fk": {"stream"}, "ovf": {"res_dup" if resident else "stream_ovf"},
            "irregular": {"walk" if resident else "stream_ovf"}, "m17": {"res_dup" if resident else "walk"},
            "resdup": {"res_dup" if resident else "walk"}}
    for u in m.units:
        assert u.route in want[kinds[u.bucket]], (u.bucket, kinds[u.bucket], u.route)
        if kinds[u.bucket] == "irregular" and not resident:
            assert u.npatch == 2
    assert set(kinds) == set(fs.KINDS) and m.walk_units == sum(u.route == "walk" for u in m.units) > 50
    pairs_hold(s, set(range(40)))


@pytest.mark.parametrize("resident", [0, 1])
def test_deferred_batch_mix(resident):
    joins = fs.deferred_batch(resident)
    want = {(a, b) for a in fs.KINDS[:-1] for b in fs.KINDS[:-1]}
    for R, S, kinds in joins:
        assert max(len(R), len(S)) <= C.BJ_MAX_TILES * C.SM_TILE
        m = fm.model(R, S, 8, {"resident": resident}, batch=True, with_pairs=False)
        assert m.path == "batch" and [kinds[u.bucket] for u in m.units] == fs.unit_kinds(kinds)
        for d in range(1, C.BJ_WGS + 1):                       # every ordered pair of kinds, at every distance a workgroup's next unit can have
            assert {(kinds[m.units[i].bucket], kinds[m.units[i + d].bucket]) for i in range(len(m.units) - d)} == want
        assert m.walk_units > 20


@pytest.mark.parametrize("resident", [0, 1])
@pytest.mark.parametrize("kind", fs.SPEC_KINDS)
def test_spec_shape(kind, resident):
    s = fs.spec(kind, resident)
    m = fm.model(s.R, s.S, s.bits, s.knobs, with_pairs=False)
    assert m.try_spec and m.spec_rel == 1 and m.mayres == bool(resident) and m.path == "fused"
    units = m.units_of(s.b)
    assert all(not u.flip and not u.fkp for u in units)                   # R probes the planted bucket
    assert sum(1 for u in m.units if not u.fkp) == len(units)             # and only that one
    assert m.last_spec == s.extra["last_spec"] and m.walk_units == s.walk
    if "records" in s.extra:
        g, n = s.extra["records"]
        assert len(units) == 1 and int(units[0].records[g]) == n and int(np.delete(units[0].records, g).max()) == 0
        assert units[0].cannot == (n > C.FJ_REC_CAP) and units[0].resident == bool(resident)
        assert units[0].route == ("res_dup" if resident else "stream_ovf")
    if "groups" in s.extra:
        assert len(units[0].records) == s.extra["groups"] >= 130 and (units[0].records > 0).all() and not units[0].cannot
        assert not units[0].resident
    if "units" in s.extra:
        assert len(units) == s.extra["units"] and units[1].off == C.FJ_SPAN
    if kind == "totals":
        assert units[0].total == units[0].bc and (units[0].c[units[0].c > 0] == 1).all()
        i, cnt = np.unique(s.R["value"][(s.R["value"] & np.uint64(511)) == np.uint64(s.b)], return_counts=True)
        assert cnt.max() == 2                                            # the hypothesis is false, the check cannot see it
    pairs_hold(s, {s.b})
