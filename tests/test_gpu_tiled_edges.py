"""GPU: the tiled join path (csrc/rhj_join_tiled.hip.h: k_plan, k_build_lds, k_build_hbm, k_probe; k_offsets_* of
rhj_common.hip.h; join_tiled of rhj_device.hip) with buckets placed ON its constants: the build sides where a bucket changes
its table kind or its table stops growing, probe sides around a unit, unit counts around the XCD deal's eighths and the offset
scan's block, clusters homed in a table's last slots, match counts around the stash's 8 bits, and the handover from the fused
and small paths, in a fresh process too.

Every case asserts (run_case): the pairs are the oracle's, order included, through helpers.guarded_join at capacity M and at
M - 1 (return code, *matches, sentinel rows on both sides, the inputs unchanged); stats()["path"] is the path the case is
built for; and after a tiled join units, hbm_units, max_build and table_slots equal the totals of tests/tiled_model.py's plan
over the case's histograms.  The edges come from that model, which reads the constants from the sources: a changed constant
moves the cases.  tests/test_tiled_model.py checks the model and the key constructors on the CPU.

Relations are built bucket by bucket with exact sizes (tiled_model.sized_relations) on 3 radix bits unless a case says otherwise.
"""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_hash_collisions as collisions
import tiled_model as tm
from helpers import guarded_join, make_rel, pairs_to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = tm.constants()
BITS = 3
STAT_KEYS = ("units", "hbm_units", "max_build", "table_slots")

# rhj_set_* knobs and their defaults; every case restores all of them
DEFAULTS = collisions.DEFAULTS
restore = collisions.restore

# how a join gets to the tiled path: the knobs, and the lds_cap its plan is made with
ROUTES = {
    "planned": ({"fused": 0}, C.tiled_cap),
    "after_fused": ({"small": 0, "lowradix": 0}, C.fused_cap),
    "after_small": ({"lowradix": 0}, C.fused_cap),
    "forced_hbm": ({"force_hbm_table": 1}, C.forced_cap),
}


@pytest.fixture(scope="module")
def rhj():
    mod = importlib.import_module("sigmod-2018_amd")
    r = mod.RHJ(device=0)
    restore(r)
    yield r
    restore(r)


@pytest.fixture
def knobs(rhj):
    def set_(**kw):
        for k, v in kw.items():
            getattr(rhj.lib, "rhj_set_" + k)(v)
    try:
        yield set_
    finally:
        restore(rhj)


def run_case(rhj, oracle, R, S, bits, lds_cap, what, path="tiled"):
    """One join at capacity M and at M - 1 against the oracle, its path and (tiled) its plan's totals against the model.
    R, S: relations or key columns (row id = position).  Returns the model's plan."""
    if R.dtype.names is None:
        R, S = make_rel(R), make_rel(S)
    rhj.set_bits(bits)
    want = oracle.join(R, S, bits)
    M = len(want)
    assert M >= 2, what
    p = tm.plan(*tm.histograms(R["value"], S["value"], bits), lds_cap)
    model = {k: getattr(p, k) for k in STAT_KEYS}
    dR, dS = rhj.to_device(R), rhj.to_device(S)
    want_t = pairs_to_device(rhj, want)

    def call(out, cap, m):
        return rhj.lib.rhj_join_device(dR.data_ptr(), len(R), dS.data_ptr(), len(S), out, cap, m)

    for cap in (M, M - 1):
        try:
            guarded_join(rhj, call, dR, dS, cap, want_t)
        except AssertionError as e:
            raise AssertionError("%s: %s; the model's plan: %r" % (what, e, model)) from None
        st = rhj.stats()
        assert st["path"] == path and st["radix_bits"] == bits, "%s: ran as %r on %d bits, the case is built for %r" % (what, st["path"], st["radix_bits"], path)
        if path == "tiled":
            got = {k: st[k] for k in STAT_KEYS}
            assert got == model, "%s, capacity %d: the plan's totals are %r, the model's %r" % (what, cap, got, model)
    return p


# ---- (a) build-side edges, one join per route ------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["parity", "ties"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_build_side_edges(rhj, oracle, knobs, route, layout):
    """Eight buckets whose build sides are 1, the last on lds_slots_for's floor and the next, the first with LDS_MAX_SLOTS slots
    and the next, and lds_cap - 1, lds_cap, lds_cap + 1 of the route (forced_hbm: of the planned route; every bucket gets a
    64-bit table).  parity: R builds the even buckets and S the odd ones, the probe sides 1, PR_UNIT - 1 or PR_UNIT + 1 longer;
    ties: the other way round, and two buckets (the floor's and lds_cap's) with cR == cS, which R probes."""
    kn, cap = ROUTES[route]
    builds = tm.build_edges(cap if cap else C.tiled_cap)
    sizes = (tm.sides_by_parity if layout == "parity" else tm.sides_with_ties)(builds)
    Rk, Sk = tm.sized_relations(np.random.default_rng(len(route) * 10 + len(layout)), BITS, sizes)
    knobs(**kn)
    p = run_case(rhj, oracle, Rk, Sk, BITS, cap, "%s, %s" % (route, layout))
    assert list(p.bc) == builds
    if cap:
        assert list(p.mode) == [1] * 7 + [2] and p.hbm_units == -(-(cap + 1) // C.BUILD_CHUNK)
        assert int(p.slots[3]) == C.LDS_MAX_SLOTS > int(p.slots[2]) and int(p.slots[6]) == C.LDS_MAX_SLOTS
    else:
        assert list(p.mode) == [2] * 8 and p.tab32_slots == 0
    assert list(p.flip) == [(r < s) for r, s in (sizes[i] for i in range(8))] and (layout == "parity" or list(p.pc)[6] == builds[6])


@pytest.mark.parametrize("layout", ["parity", "ties"])
@pytest.mark.parametrize("route", ["after_fused", "after_small"])
def test_the_handover_routes_keep_a_join_of_lds_cap(rhj, oracle, knobs, route, layout):
    """The edge from its other side: without the bucket of lds_cap + 1 build tuples the largest is FUSED_LDS_CAP and the join
    stays where it was."""
    kn, cap = ROUTES[route]
    builds = tm.build_edges(cap)[:-1]
    sizes = (tm.sides_by_parity if layout == "parity" else tm.sides_with_ties)(builds + [0])
    del sizes[7]
    Rk, Sk = tm.sized_relations(np.random.default_rng(len(route) * 10 + len(layout) + 1), BITS, sizes)
    assert tm.plan(*tm.histograms(Rk, Sk, BITS), cap).max_build == cap == C.FUSED_LDS_CAP
    knobs(**kn)
    run_case(rhj, oracle, Rk, Sk, BITS, cap, "%s without lds_cap + 1, %s" % (route, layout), path={"after_fused": "fused", "after_small": "small"}[route])
    assert rhj.stats()["max_build"] == cap


def test_table_growth_stops(rhj, oracle, knobs):
    """The build sides around the three edges of lds_slots_for's upper end: the first table of LDS_MAX_SLOTS slots, the first
    size the min() cuts, and the first load factor above 2/3."""
    full, cut = tm.first_full_build(), tm.first_clamped_build()
    over = next(bc for bc in range(full, C.tiled_cap) if 3 * bc > 2 * tm.lds_slots_for(bc))
    builds = [full - 1, full, cut - 1, cut, over - 1, over, over + 1, C.tiled_cap]
    Rk, Sk = tm.sized_relations(np.random.default_rng(3), BITS, tm.sides_by_parity(builds))
    knobs(fused=0)
    p = run_case(rhj, oracle, Rk, Sk, BITS, C.tiled_cap, "growth stops")
    assert list(p.slots) == [C.LDS_MAX_SLOTS - C.SLOT_GRANULE] + [C.LDS_MAX_SLOTS] * 7


# ---- (b) chunk, unit and table-size edges ------------------------------------------------------------------------------------
TABLES = {"hbm64": ({"force_hbm_table": 1}, C.forced_cap), "lds32": ({"fused": 0}, C.tiled_cap)}


@pytest.mark.parametrize("table", list(TABLES))
def test_build_chunk_and_position_edges(rhj, oracle, knobs, table):
    """Build sides of BUILD_CHUNK - 1, BUILD_CHUNK, + 1, two chunks, two and one tuple (64-bit tables built by one, two and three
    workgroups, sized 2^13 and, one tuple on, 2^14), and 65 534, 65 535, 65 536: beyond the 16-bit position of a 32-bit table's
    entries, so these are 64-bit tables also with rhj_set_fused(0), next to the 32-bit tables of the small ones."""
    kn, cap = TABLES[table]
    builds = tm.chunk_edges()
    Rk, Sk = tm.sized_relations(np.random.default_rng(4), BITS, tm.sides_by_parity(builds))
    knobs(**kn)
    p = run_case(rhj, oracle, Rk, Sk, BITS, cap, "chunk edges, " + table)
    assert list(p.bc) == builds
    assert list(p.mode) == ([2] * 8 if table == "hbm64" else [1] * 5 + [2] * 3)
    assert list(p.lg[5:]) == [17, 17, 17] and list(p.build_units_of[5:]) == [16, 16, 16]
    if table == "hbm64":
        assert list(p.build_units_of[:5]) == [1, 1, 2, 2, 3] and list(p.lg[:5]) == [13, 13, 14, 14, 15]


@pytest.mark.parametrize("table", list(TABLES))
def test_probe_unit_edges(rhj, oracle, knobs, table):
    """Probe sides of exactly 1, PR_UNIT - 1, PR_UNIT, PR_UNIT + 1, 2 PR_UNIT and 2 PR_UNIT + 1 tuples: last units of one tuple,
    of all but one, and full ones."""
    kn, cap = TABLES[table]
    sizes = tm.probe_edges()
    Rk, Sk = tm.sized_relations(np.random.default_rng(5), BITS, sizes, hit=0.8)
    knobs(**kn)
    p = run_case(rhj, oracle, Rk, Sk, BITS, cap, "probe edges, " + table)
    u = C.PR_UNIT
    assert list(p.pc[:7]) == [1, u - 1, u, u + 1, 2 * u, 2 * u + 1, u - 1] and list(p.units_of[:7]) == [1, 1, 1, 2, 2, 3, 1]


@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("units", [1, 7, 8, 9, 17])
def test_unit_totals_around_the_xcd_deal(rhj, oracle, knobs, table, units):
    """Tiny relations on 4 bits with 1, 7, 8, 9 and 17 probe units in all: k_probe's grid is ceil(units / 8) * 8 workgroups and
    its map from workgroup to unit must reach every unit when that is not a multiple of 8."""
    kn, cap = TABLES[table]
    Rk, Sk = tm.sized_relations(np.random.default_rng(units), 4, tm.unit_total_sizes(units), dup=0.5, hit=0.9)
    Rk, Sk = np.concatenate([Rk, Rk[:1]]), np.concatenate([Sk, Rk[:1]])                  # (a pair for certain)
    knobs(**kn)
    p = run_case(rhj, oracle, Rk, Sk, 4, cap, "%d units, %s" % (units, table))
    assert p.units == units


# ---- (c) the offset scan's block ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("units", [C.SCAN_BLOCK - 1, C.SCAN_BLOCK, C.SCAN_BLOCK + 1, 2 * C.SCAN_BLOCK + 1])
def test_scan_block_edges(rhj, oracle, knobs, units):
    """11 bits, one unit a bucket, 1, 2, 3, 4, 6 or 9 pairs a unit and never the neighbour's count: launch_offsets scans SCAN_BLOCK
    unit counts a workgroup and adds the blocks' bases in a launch of its own, so a base that is off by a unit or a block that
    is not added shows in the pairs.  2 * SCAN_BLOCK + 1: every bucket of the radix and one of two units."""
    bits = 11
    extra = units > (1 << bits)
    Rk, Sk = tm.scan_block_keys(units - extra, bits, extra)
    rng = np.random.default_rng(units)
    knobs(fused=0)
    p = run_case(rhj, oracle, rng.permutation(Rk), rng.permutation(Sk), bits, C.tiled_cap, "%d units" % units)
    assert p.units == units and p.hbm_units == 0


# ---- (d) clusters homed in a table's last slots -------------------------------------------------------------------------------
@pytest.mark.parametrize("filler", [0, 150], ids=["floor_table", "filled_table"])
@pytest.mark.parametrize("j", [0, 1, 2, 3])
@pytest.mark.parametrize("table", [32, 64], ids=["lds32", "hbm64"])
def test_wrap_around_clusters(rhj, oracle, knobs, table, j, filler):
    """A bucket of a random 60 K x 80 K join whose build side holds 1, 4, 5, 8, 9 or 13 keys of one tag homed at slot
    slots - 1 - j (Tab32 skips 3 - j entries of its first group of four) — and once 5 and 9 with one of them three times, whose
    pairs come in descending build position across the wrap —, keys homed at slots 0..3 with greater and smaller tags, and
    `filler` random keys; probed by every build key, by absent keys of the cluster's home and tag (they flag their unit) and of
    the smallest, the greatest and the neighbouring tags (tiled_model.wrap_cluster).  k_build_lds wraps s + 1 == slots,
    the dump replicates the first entries behind the table, load_chunk reads them there and the walk goes on at
    advance(s0, CH - skip); Tab64 wraps by mask."""
    b = 5
    kn, cap = TABLES["lds32" if table == 32 else "hbm64"]
    knobs(**kn)
    for size, dup in tm.WRAP_SIZES:
        w = tm.wrap_cluster(table, b, BITS, j, size, dup, filler, seed=100 * j + 10 * size + dup)
        R, S = collisions.relations(np.random.default_rng(size), BITS, 60_000, 80_000, [(b, w["R"], w["S"])])
        what = "cluster of %d%s at slot %d of %d" % (size, " (one three times)" if dup else "", w["home"], w["slots"])
        p = run_case(rhj, oracle, R, S, BITS, cap, what)
        assert int(p.bc[b]) == w["bc"] and bool(p.flip[b])
        assert (int(p.slots[b]) if table == 32 else 1 << int(p.lg[b])) == w["slots"]


# ---- (e) match counts at the stash's limits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("flagged", [False, True], ids=["unflagged", "every_second_unit_flagged"])
@pytest.mark.parametrize("table", [32, 64], ids=["lds32", "hbm64"])
def test_match_counts_at_the_stash_limits(rhj, oracle, knobs, table, flagged):
    """One bucket whose build keys come 1, 2, 16, 17, 254, 255, 256, 257 and 300 times: the count pass stashes min(c, 255) in a
    byte and the emit pass trusts the stash for c <= 1 only.  Every such key is probed eight times, from units of both kinds,
    between tuples without a match (tiled_model.stash_bucket)."""
    kn, cap = TABLES["lds32" if table == 32 else "hbm64"]
    Rk, Sk, units = tm.stash_bucket(table, 6, BITS, flagged, seed=9)
    knobs(**kn)
    p = run_case(rhj, oracle, Rk, Sk, BITS, cap, "stash limits")
    assert p.units == units and p.max_build == len(Rk)


# ---- (f) the two-pass handover, in a fresh process and a warmed one ---------------------------------------------------------------
def child_main():
    """A process's first join: 600 K x 600 K on 9 bits with one build side of FUSED_LDS_CAP + 1, default knobs — the narrow
    two-pass partition, the fused kernel's refusal, the partition again with 16-byte tuples, the refusal again, the tiled
    path.  Then the joins the docstring of test_two_pass_handover lists."""
    from pyoracle import Oracle
    oracle = Oracle()
    rhj = importlib.import_module("sigmod-2018_amd").RHJ(device=0)
    n, hot = 600_000, 77
    assert rhj.lib.rhj_sub_bits(9, n, n) == 0
    Rk, Sk = tm.hot_bucket_relations(np.random.default_rng(1), 9, n, hot, C.FUSED_LDS_CAP + 1)
    for what in ("a fresh process's first join", "the same join again"):
        p = run_case(rhj, oracle, Rk, Sk, 9, C.fused_cap, what)
        assert p.hbm_units == -(-(C.FUSED_LDS_CAP + 1) // C.BUILD_CHUNK) and int((p.mode == 2).sum()) == 1 and p.lds_buckets == 511
        assert p.table_slots == (1 << tm.tab64_lg(C.FUSED_LDS_CAP + 1)) + p.tab32_slots
    one = np.nonzero((Rk & np.uint64(511)) == np.uint64(hot))[0][0]
    Rk2 = np.delete(Rk, one)
    assert tm.plan(*tm.histograms(Rk2, Sk, 9), C.fused_cap).max_build == C.FUSED_LDS_CAP
    run_case(rhj, oracle, Rk2, Sk, 9, C.fused_cap, "the build side at FUSED_LDS_CAP", path="fused")
    for bits in (12, 14):
        m = 300_000
        Rk, Sk = tm.hot_bucket_relations(np.random.default_rng(bits), bits, m, hot, 33_000)
        R, S = make_rel(Rk), make_rel(Sk)
        S["row_id"][m // 2:m // 2 + 3] += np.uint64(1) << np.uint64(33)
        S["row_id"][m // 3] = np.uint64((1 << 32) + 1)
        p = run_case(rhj, oracle, R, S, bits, C.tiled_cap, "%d bits, planned" % bits)
        assert 33_000 > C.tiled_cap and p.hbm_units == -(-33_000 // C.BUILD_CHUNK) and int((p.mode == 2).sum()) == 1
    print("ok")


def test_two_pass_handover_in_a_fresh_process(oracle):
    """In a child process (one GPU process at a time): the 9-bit handover as the process's first join (fused refuses the narrow
    partition, RUN_WIDE, wide partition, fused refuses again, tiled: one 64-bit table of ceil((FUSED_LDS_CAP + 1) / BUILD_CHUNK)
    build units beside 511 32-bit ones), the same join now that the process has seen wide tuples, the join with that bucket at
    exactly FUSED_LDS_CAP, which the fused path keeps, and a 12- and a 14-bit join of 300 K x 300 K (tiny buckets: the tiled path
    planned behind a two-pass wide partition) with one build side of 33 000 and row ids beyond 2^32 in the middle of S."""
    code = "import sys; sys.path[:0] = ['tests', 'oracle', '.']; import test_gpu_tiled_edges as t; t.child_main()"
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0 and b"ok" in res.stdout, res.stderr.decode()[-3000:]
