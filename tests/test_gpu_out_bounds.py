"""GPU: no join path writes outside the caller's pair buffer (include/rhj.h: "*matches gets the exact match count even when it
exceeds out_capacity (then nothing beyond capacity is written and the return value is 1)").

Every case calls one raw entry point through helpers.guarded_join: the pair buffer lies between 4096 sentinel rows in front and
behind and always spans all M pair positions of the oracle's list, so a store whose `at < cap` guard is wrong lands in the test's
own tensor and is reported with its row and contents.  Asserted per call: return code, *matches, the prefix bit for bit, both
guards, the input relations, and the route the join took (stats()["path"], rhj_last_spec / rhj_last_exact, hbm_units) — a case
that ran on another path than the one it is named for fails.  Rows [M, capacity) are open by the header; every case prints
how many of them it found written.

The capacities come from the wanted list (helpers.guard_capacities): 0 with a buffer, 1, the first bucket edge and one near
the middle +- 1, a position inside the longest run of pairs of one probe tuple, M - 1, M, M + 1.  Inputs and knobs are those of
the tests that already reach each kernel (test_gpu_parity.py, test_gpu_small.py, test_gpu_split_paths.py,
test_gpu_hash_collisions.py, test_gpu_shard.py, test_gpu_devices.py), cut to the smallest size the path takes."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import test_gpu_split_paths as split_paths
from helpers import GuardedRows, guarded_join, make_rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = np.uint64(1) << np.uint64(40)

# rhj_set_* knobs and their defaults; every case restores all of them
DEFAULTS = {"spec": 1, "exact": 0, "resident": 1, "fused": 1, "small": 1, "lowradix": 1, "force_hbm_table": 0}


def restore(rhj):
    for k, v in DEFAULTS.items():
        getattr(rhj.lib, "rhj_set_" + k)(v)


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


def route(path, spec=0, exact=0, hbm=False):
    return dict(path=path, spec=spec, exact=exact, hbm=hbm)


def check_route(rhj, bits, expect, what):
    st = rhj.stats()
    got = dict(path=st["path"], spec=rhj.lib.rhj_last_spec(), exact=rhj.lib.rhj_last_exact(), hbm=st["hbm_units"] > 0)
    assert got == expect and st["radix_bits"] == bits, "%s: ran as %r on %d bits, the case is built for %r" % (what, got, st["radix_bits"], expect)


def sweep(rhj, name, R, S, bits, want, expect, entry=None, prepare=None, extra_caps=(), run=None):
    """The entry point (rhj_join_device unless `entry(dR, dS, out, cap, matches_ref)` is given) at every capacity of the wanted
    list; prepare() runs before each call (the speculation's try-or-not scores move with every outcome).  run = (lo, hi): the
    longest run of pairs of one probe tuple the input was built for (hi None: any length from lo)."""
    dR, dS = rhj.to_device(R), rhj.to_device(S)
    want_t = helpers.pairs_to_device(rhj, want)
    b, probe = helpers.pair_layout(R, S, want, bits)
    if run:
        longest = int(np.diff(np.concatenate([[0], np.nonzero(np.diff(probe))[0] + 1, [len(probe)]])).max())
        assert longest >= run[0] and (run[1] is None or longest <= run[1]), "%s: the longest run has %d pairs" % (name, longest)
    caps = sorted(set(helpers.guard_capacities(b, probe)) | set(extra_caps))
    rhj.set_bits(bits)

    def call(out, cap, m):
        if prepare:
            prepare()
        if entry:
            return entry(dR, dS, out, cap, m)
        return rhj.lib.rhj_join_device(dR.data_ptr(), len(R), dS.data_ptr(), len(S), out, cap, m)

    seen = {}
    for cap in caps:
        written = guarded_join(rhj, call, dR, dS, cap, want_t)
        check_route(rhj, bits, expect, "%s, capacity %d" % (name, cap))
        if cap > len(want):
            seen[cap - len(want)] = written
    print("%s: %d pairs, capacities %s; rows written in [M, capacity): %s" % (name, len(want), caps, seen))
    return caps


def rel(rng, n, dom):
    return make_rel(rng.integers(0, dom, size=n, dtype=np.uint64))


def widen(R, S):
    """Row ids beyond 32 bits where the partition's sample sees them (the ends); the wanted list goes through relabel()."""
    R, S = R.copy(), S.copy()
    R["row_id"][:10] += WIDE
    S["row_id"][-3:] += WIDE
    return R, S


def relabel(want, R, S):
    """The list of the same keys under other row ids: the order depends on positions alone (want: of positional row ids)."""
    out = want.copy()
    out["row_idR"], out["row_idS"] = R["row_id"][want["row_idR"]], S["row_id"][want["row_idS"]]
    return out


# ---- 1. the small path (rhj_small.hip.h) -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nR,nS,dom,bits,resident,fan", [
    ("fk", 20_000, 30_000, 0, 4, 1, 1),
    ("duplicates", 20_000, 30_000, 500, 4, 1, 17),             # ~50 matches a probe tuple on resident build sides: runs emitted output-centrically
    ("runs_of_125", 20_000, 5_000, 40, 2, 1, 17),
    ("gathered_walk", 60_000, 60_000, 600, 4, 0, 17),          # 100 a tuple on gathered build sides: beyond the stash, k_join_walk on the caller's buffer
])
def test_small_path(rhj, oracle, knobs, name, nR, nS, dom, bits, resident, fan):
    rng = np.random.default_rng(nR + dom)
    if dom:
        R, S = rel(rng, nR, dom), rel(rng, nS, dom)
    else:
        R, S = oracle.generate(nR, 0, 0, 0.0, 11), oracle.generate(nS, 1, nR, 0.0, 12)
    knobs(resident=resident)
    sweep(rhj, "small " + name, R, S, bits, oracle.join(R, S, bits), route("small"), run=(fan, None))


# ---- 2. k_join_fused, speculation off ----------------------------------------------------------------------------------
_FUSED = {}


def fused_inputs(oracle, kind):
    """9 radix bits (the two-pass partition, 12-byte tuples unless the row ids are wide): foreign keys; a few matches a tuple;
    18 a tuple on both sides (the fan-out of test_more_matches_than_the_overflow_stash_describes at a quarter of its size)."""
    if kind not in _FUSED:
        if kind == "fk":
            R, S = oracle.generate(700_000, 0, 0, 0.0, 21), oracle.generate(900_000, 1, 700_000, 0.0, 22)
        elif kind == "few":
            R, S = oracle.generate(400_000, 4, 300_000, 0.0, 23), oracle.generate(500_000, 4, 300_000, 0.0, 24)
        else:
            rng = np.random.default_rng(9 * 1000 + 57_500)
            R, S = rel(rng, 1_050_000, 57_500), rel(rng, 1_050_000, 57_500)
        _FUSED[kind] = (R, S, oracle.join(R, S, 9))
    return _FUSED[kind]


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("resident", [1, 0], ids=["resident", "gather"])
@pytest.mark.parametrize("kind", ["fk", "few", "stash"])
def test_fused_kernel(rhj, oracle, knobs, kind, resident, wide):
    """k_join_fused<resident or gathering, 12- or 16-byte tuples>: the group emit, the streaming emit with its patch list, and —
    more than 16 matches a tuple on a gathered build side — k_join_walk behind it, all on the caller's buffer."""
    R, S, want = fused_inputs(oracle, kind)
    if wide:
        R, S = widen(R, S)
        want = relabel(want, R, S)
    knobs(spec=0, resident=resident, fused=2)
    sweep(rhj, "fused %s %s %s" % (kind, "resident" if resident else "gather", "wide" if wide else "narrow"), R, S, 9, want, route("fused"),
          run=({"fk": 1, "few": 3, "stash": 17}[kind], None))


# ---- 3. and 4. k_join_spec and k_join_walk -----------------------------------------------------------------------------
def lone_tuple_in_the_last_bucket(S, bits):
    """One S tuple loses its partner and stays in the LAST bucket: the speculative kernel has written most of its pairs
    before a unit notices."""
    S2 = S.copy()
    last = np.uint64((1 << bits) - 1)
    victim = int(np.nonzero((S2["value"] & last) == last)[0][-1])
    S2["value"][victim] = last | (np.uint64(1) << np.uint64(50))
    return S2


def spec_prepare(rhj):
    return lambda: rhj.lib.rhj_set_spec(1)                   # (also resets the try-or-not score a failed try lowers)


@pytest.mark.parametrize("case", ["S_probes", "R_probes", "fails", "fails_R_probes"])
def test_speculation_on_resident_build_sides(rhj, oracle, knobs, case):
    """k_join_spec<true> (1.2M x 2.2M foreign keys on 9 bits, test_foreign_key_speculation_holds_or_hands_over): the hypothesis'
    relation given as S and as R; with capacities far below its size; and failing in the last bucket, k_join_fused taking over
    on the same buffer."""
    R = oracle.generate(1_200_000, 0, 0, 0.0, 91)
    S = oracle.generate(2_200_000, 1, 1_200_000, 0.0, 92)
    fails = case.startswith("fails")
    if fails:
        S = lone_tuple_in_the_last_bucket(S, 9)
    if case.endswith("R_probes"):
        R, S = S, R
    knobs(fused=2)
    want = oracle.join(R, S, 9)
    sweep(rhj, "spec resident " + case, R, S, 9, want, route("fused", spec=2 if fails else 1), prepare=spec_prepare(rhj),
          extra_caps=[max(len(R), len(S)) + 16])


_GATHERED = {}


def gathered_R(oracle):
    if "R" not in _GATHERED:
        _GATHERED["R"] = oracle.generate(8_000_000, 0, 0, 0.0, 191)
    return _GATHERED["R"]


@pytest.mark.parametrize("case", ["uniform", "first_quarter", "one_with_700", "fails"])
def test_speculation_on_gathered_build_sides(rhj, oracle, knobs, case):
    """k_join_spec<false> (8M x 8M on 10 bits, the inputs of test_speculation_on_gathered_build_sides_both_kinds_of_units): half of
    the buckets probed by S (pairs from the probe loop), half by R (fj_group_direct, fj_emit_records); units whose records run
    out — whole groups of tuples with four matches, one tuple with 700 — are written again by k_join_walk; one tuple without a
    partner in the last bucket hands the whole join to k_join_fused."""
    bits, n = 10, 8_000_000
    R = gathered_R(oracle)
    rng = np.random.default_rng(192)
    S = make_rel(R["value"][rng.integers(0, n, n)])
    if case == "first_quarter":
        S = make_rel(R["value"][rng.integers(0, n // 4, n)])
    elif case == "one_with_700":
        mask = np.uint64((1 << bits) - 1)
        hr = np.bincount((R["value"] & mask).astype(np.int64), minlength=1 << bits)
        hs = np.bincount((S["value"] & mask).astype(np.int64), minlength=1 << bits)
        b0 = int(np.nonzero(hr >= hs)[0][0])                          # a bucket R probes (rhjoin.c:86)
        k0 = R["value"][np.nonzero((R["value"] & mask) == np.uint64(b0))[0][7]]
        S["value"][np.nonzero((S["value"] & mask) == np.uint64(b0))[0][:700]] = k0
    elif case == "fails":
        S = lone_tuple_in_the_last_bucket(S, bits)
    knobs(fused=2)
    sweep(rhj, "spec gathered " + case, R, S, bits, oracle.join(R, S, bits), route("fused", spec=2 if case == "fails" else 1),
          prepare=spec_prepare(rhj), extra_caps=[n + 16], run=(700 if case == "one_with_700" else 1, None))


# ---- 5. k_join_exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["S_probes", "both_probe", "hands_over"])
def test_exact_kernel(rhj, oracle, knobs, case):
    """k_join_exact (rhj_set_exact(1), 10 bits, gathered build sides, 4.1 K tuples of the bigger relation a bucket, as
    test_gpu_hash_collisions.py builds them).  S_probes: build sides of 256 tuples, the hypothesis' relation probes every bucket
    (pair i of a unit at base + i).  both_probe: relations of one size, R probes half of the buckets with 0..9 matches a tuple
    (up to four from the slot's first window, the others one pair a step).  hands_over: row ids that decrease with the
    position are not this kernel's; k_join_fused does the join on the same buffer."""
    bits = 10
    nS = (4096 << bits) + 50_000
    nR = nS if case == "both_probe" else 256 << bits
    R = oracle.generate(nR, 0, 0, 0.0, 51)
    if case == "both_probe":
        S = make_rel(R["value"][np.random.default_rng(52).integers(0, nR, nS)])
    else:
        S = oracle.generate(nS, 1, nR, 0.0, 52)
    if case == "hands_over":
        R["row_id"] = R["row_id"][::-1].copy()
    knobs(resident=0, fused=2)
    took = 2 if case == "hands_over" else 1

    def prepare():
        rhj.lib.rhj_set_spec(1)
        rhj.lib.rhj_set_exact(1)
    sweep(rhj, "exact " + case, R, S, bits, oracle.join(R, S, bits), route("fused", spec=took, exact=took), prepare=prepare,
          run=(5 if case == "both_probe" else 1, None))


# ---- 6. the tiled path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fk", "fanout", "hashed_runs"])
@pytest.mark.parametrize("table", ["lds32", "hbm64"])
def test_tiled_path(rhj, oracle, knobs, kind, table):
    """k_probe<true> over 32-bit tables built in LDS and 64-bit tables in HBM: foreign keys; 20 matches a tuple (beyond the 16
    of the stash) in buckets of 5000 probe tuples (beyond one unit's PR_UNIT = 2048); and hashed 64-bit keys with three
    matches a probe tuple — units in which a foreign key's tag hit are flagged and verify every candidate again while they
    emit, the small keys of `fanout` flag none."""
    rng = np.random.default_rng(61)
    if kind == "fk":
        R, S = oracle.generate(50_000, 0, 0, 0.0, 61), oracle.generate(90_000, 1, 50_000, 0.0, 62)
    elif kind == "fanout":
        R, S = rel(rng, 60_000, 3_000), rel(rng, 80_000, 3_000)
    else:
        R = oracle.generate(90_000, 0, 0, 0.0, 63)
        S = make_rel(rng.permutation(np.repeat(R["value"][:15_000], 3)))
    knobs(fused=0, force_hbm_table=1 if table == "hbm64" else 0)
    sweep(rhj, "tiled %s %s" % (table, kind), R, S, 4, oracle.join(R, S, 4), route("tiled", hbm=table == "hbm64"),
          run={"fk": (1, None), "fanout": (17, None), "hashed_runs": (3, 3)}[kind])


# ---- 7. the reruns on the caller's buffer ------------------------------------------------------------------------------
_BIG4 = {}


def beyond_lds_on_4_bits(oracle):
    """1.2M x 0.9M foreign keys on 4 bits (test_first_call_in_fresh_process_takes_the_fallback): build sides of 56 K tuples"""
    if not _BIG4:
        R, S = oracle.generate(1_200_000, 0, 0, 0.0, 5), oracle.generate(900_000, 1, 1_200_000, 0.0, 6)
        _BIG4.update(R=R, S=S, want=oracle.join(R, S, 4))
    return _BIG4["R"], _BIG4["S"], _BIG4["want"]


@pytest.mark.parametrize("small", [1, 0], ids=["after_small", "after_fused"])
def test_tiled_path_after_the_fused_kernel_ran_on_the_buffer(rhj, oracle, knobs, small):
    """The fused kernel is launched on the caller's buffer (by the small path, or behind the partition), the plan rejects it
    (a build side beyond the LDS index) and the tiled path answers on the same buffer."""
    R, S, want = beyond_lds_on_4_bits(oracle)
    knobs(lowradix=0, small=small)
    sweep(rhj, "tiled after " + ("small" if small else "fused"), R, S, 4, want, route("tiled", hbm=True))


@pytest.mark.parametrize("bits", [9, 12])
def test_wide_rerun_on_the_buffer(rhj, oracle, knobs, bits):
    """A wide row id in the middle of a relation, where the sample does not see it: the narrow run notices in pass 1 or in the
    join and the whole chain runs again wide, on the same buffer (test_row_ids_wider_than_32_bits_in_the_two_pass_partition)."""
    nR, nS = 60_000, 90_000
    R = oracle.generate(nR, 0, 0, 0.0, 71)
    S = oracle.generate(nS, 1, nR, 0.0, 72)
    R["row_id"][nR // 2: nR // 2 + 5] += WIDE
    S["row_id"][nS // 3] += WIDE
    knobs(fused=2)
    sweep(rhj, "wide rerun", R, S, bits, oracle.join(R, S, bits), route("fused"))


# ---- 8. the low-radix and sub-bucket paths -----------------------------------------------------------------------------
def doubled(R, twice, once, seed):
    """S: R's first `twice` keys two times each and the next `once` keys one time, shuffled: runs of two pairs and single pairs"""
    keys = np.concatenate([np.repeat(R["value"][:twice], 2), R["value"][twice:twice + once]])
    np.random.default_rng(seed).shuffle(keys)
    return make_rel(keys)


def test_low_radix_path_foreign_keys(rhj, oracle, knobs):
    """Single pairs through the direct store of k_lr_emit (and, where R probes a bucket, short runs)."""
    R, S, want = beyond_lds_on_4_bits(oracle)
    assert rhj.lib.rhj_sub_bits(4, len(R), len(S)) >= 1
    sweep(rhj, "lowradix 4 bits fk", R, S, 4, want, route("lowradix"))


@pytest.mark.parametrize("bits,nR,twice,once", [(4, 1_200_000, 300_000, 300_000), (8, 9_000_000, 2_200_000, 4_400_000)])
def test_low_radix_path_copies_from_its_list(rhj, oracle, knobs, bits, nR, twice, once):
    """Probe tuples with two matches: k_lr_emit copies their pairs from the internal join's list (`at + i < cap`)."""
    R = oracle.generate(nR, 0, 0, 0.0, 81)
    S = doubled(R, twice, once, 82)
    assert rhj.lib.rhj_sub_bits(bits, len(R), len(S)) >= 1
    sweep(rhj, "lowradix %d bits doubled" % bits, R, S, bits, oracle.join(R, S, bits), route("lowradix"), run=(2, 2))


def test_low_radix_path_sixteen_matches(rhj, oracle, knobs):
    """One tuple with 16 matches in an R-probing and in an S-probing bucket (test_sixteen_matches_accepted_and_capacity): a
    capacity inside the run of 16."""
    r = 4
    R, S, _ = split_paths.match_relations(r, 16, 80 + r)
    assert rhj.lib.rhj_sub_bits(r, len(R), len(S)) == split_paths.MATCH[r][1]
    sweep(rhj, "lowradix 16 matches", R, S, r, oracle.join(R, S, r), route("lowradix"), run=(16, 16))


def test_seventeen_matches_leave_the_low_radix_path(rhj, oracle, knobs):
    """17 matches (test_seventeen_matches_refused): the internal join's unit goes to k_join_walk, the path gives up after it
    and the tiled path answers on the caller's buffer."""
    r = 4
    R, S, _ = split_paths.match_relations(r, 17, 90 + r)
    assert rhj.lib.rhj_sub_bits(r, len(R), len(S)) == split_paths.MATCH[r][1]
    sweep(rhj, "17 matches", R, S, r, oracle.join(R, S, r), route("tiled", hbm=True), run=(17, 17))


def test_sub_bucket_path(rhj, oracle, knobs):
    """9 bits on 17.5 M tuples a side (the smallest the rule splits): single pairs (the direct store of k_sb_emit) and runs of
    two (its copy from the internal join's list)."""
    R = oracle.generate(17_500_000, 0, 0, 0.0, 51)
    S = doubled(R, 4_000_000, 9_500_000, 52)
    assert rhj.lib.rhj_sub_bits(9, len(R), len(S)) >= 1
    sweep(rhj, "subbucket", R, S, 9, oracle.join(R, S, 9), route("subbucket"), run=(2, 2))


# ---- 9. shares, key columns, the selection -----------------------------------------------------------------------------
def in_buckets(rel_, bits, lo, hi):
    b = rel_["value"] & np.uint64((1 << bits) - 1)
    return rel_[(b >= np.uint64(lo)) & (b < np.uint64(hi))]


def bucket_ranks(rel_, bits):
    """Of every tuple: its position among the tuples of its bucket, in input order (= partition order)"""
    b = (rel_["value"] & np.uint64((1 << bits) - 1)).astype(np.int64)
    order = np.argsort(b, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=1 << bits))])
    rank = np.empty(len(rel_), dtype=np.int64)
    rank[order] = np.arange(len(rel_)) - start[b[order]]
    return rank


def slice_of(want, R, S, bits, lo, hi, skip, end):
    """include/rhj.h, rhj_join_device_slice: the canonical list's pairs of the buckets [lo, hi), without those of the first
    bucket's probe tuples in front of position `skip` and of the last bucket's from position `end` on (0: all).  Row ids are
    positions."""
    b, probe = helpers.pair_layout(R, S, want, bits)
    rank = np.where((probe & np.uint64(1)) == 1, bucket_ranks(R, bits)[want["row_idR"]], bucket_ranks(S, bits)[want["row_idS"]])
    keep = (b >= lo) & (b < hi) & ~((b == lo) & (rank < skip))
    if end:
        keep &= ~((b == hi - 1) & (rank >= end))
    return want[keep]


@pytest.mark.parametrize("where", ["fused", "lowradix"])
def test_range_and_slice_shares(rhj, oracle, knobs, where):
    """rhj_join_device_range and rhj_join_device_slice (a share that starts and ends inside buckets) on an input the fused
    path takes and on one the low-radix path takes (its slice is the plan's matter: the fused kernel runs on the buffer, the
    tiled path answers)."""
    if where == "fused":
        R, S, whole = fused_inputs(oracle, "fk")
        bits, lo, hi, skip, end = 9, 100, 300, 37, 500
        knobs(fused=2)
    else:
        R, S, whole = beyond_lds_on_4_bits(oracle)
        bits, lo, hi, skip, end = 4, 3, 9, 1000, 2000
    lib = rhj.lib

    def ranged(dR, dS, out, cap, m):
        return lib.rhj_join_device_range(dR.data_ptr(), len(R), dS.data_ptr(), len(S), lo, hi, out, cap, m)

    def sliced(dR, dS, out, cap, m):
        return lib.rhj_join_device_slice(dR.data_ptr(), len(R), dS.data_ptr(), len(S), lo, hi, skip, end, out, cap, m)

    share = oracle.join(in_buckets(R, bits, lo, hi), in_buckets(S, bits, lo, hi), bits)
    sweep(rhj, "range on " + where, R, S, bits, share, route(where), entry=ranged)
    want = slice_of(whole, R, S, bits, lo, hi, skip, end)
    assert 0 < len(want) < len(share)
    sweep(rhj, "slice on " + where, R, S, bits, want, route("fused") if where == "fused" else route("tiled", hbm=True), entry=sliced)


@pytest.mark.parametrize("bits,nR,nS,path", [(8, 300_000, 500_000, "small"), (12, 2_000_000, 3_000_000, "fused")])
def test_join_of_key_columns(rhj, oracle, knobs, bits, nR, nS, path):
    """rhj_join_keys_device (the sizes of test_gpu_parity.py's test of it, whose short-buffer call compares no pair)."""
    import torch
    R = oracle.generate(nR, 0, 0, 0.0, 301)
    S = oracle.generate(nS, 1, nR, 0.0, 302)
    kR = torch.from_numpy(R["value"].view(np.int64).copy()).to(rhj.dev)
    kS = torch.from_numpy(S["value"].view(np.int64).copy()).to(rhj.dev)
    keepR, keepS = kR.clone(), kS.clone()
    knobs(fused=2)

    def keys(dR, dS, out, cap, m):
        return rhj.lib.rhj_join_keys_device(kR.data_ptr(), nR, kS.data_ptr(), nS, out, cap, m)
    sweep(rhj, "key columns", R, S, bits, oracle.join(R, S, bits), route(path), entry=keys)
    assert torch.equal(kR, keepR) and torch.equal(kS, keepS)


def test_select_bucket_range_with_a_short_buffer(rhj, oracle):
    """rhj_select_bucket_range_device: k_select_write stores `dst < capacity` — the first `capacity` selected tuples are written,
    nothing else; rc 1 and the full count when they do not all fit."""
    bits, n, lo, hi = 6, 10_000, 5, 40
    rhj.set_bits(bits)
    R = oracle.generate(n, 1, 1000, 0.0, 9)
    dR = rhj.to_device(R)
    keep = dR.clone()
    want = helpers.pairs_to_device(rhj, in_buckets(R, bits, lo, hi))
    M = want.shape[0]
    assert 1000 < M < n
    for cap in (0, 1, 100, M - 1, M, M + 1):
        g = GuardedRows(rhj.torch, rhj.dev, max(M, cap))
        got = C.c_uint64(0)
        rc = rhj.lib.rhj_select_bucket_range_device(dR.data_ptr(), n, lo, hi, g.ptr, cap, C.byref(got))
        rhj.torch.cuda.synchronize()
        assert rc == (1 if M > cap else 0) and got.value == M, (cap, rc, got.value)
        g.assert_untouched(-helpers.GUARD_ROWS, 0, "select, capacity %d, in front" % cap)
        g.assert_untouched(cap, max(M, cap) + helpers.GUARD_ROWS, "select, capacity %d, behind" % cap)
        assert rhj.torch.equal(g.body(0, min(cap, M)), want[:min(cap, M)]) and rhj.torch.equal(dR, keep), cap


# ---- 10. the device set ------------------------------------------------------------------------------------------------
DEVICES_CHILD = r'''
import ctypes as C, importlib, sys
import numpy as np
sys.path.insert(0, "oracle"); sys.path.insert(0, "tests")
import helpers
from helpers import GuardedRows, GUARD_ROWS
from pyoracle import Oracle
o = Oracle()
rhj = importlib.import_module("sigmod-2018_amd").RHJ(device=0)
lib, torch = rhj.lib, rhj.torch
n, bits = 2, 8
assert lib.rhj_get_devices() == n
R = o.generate(400_000, 4, 150_000, 0.0, 11)                 # duplicates on both sides, 2.7 matches an S tuple
S = o.generate(700_000, 4, 150_000, 0.0, 12)
rhj.set_bits(bits)
want = o.join(R, S, bits)
b, _ = helpers.pair_layout(R, S, want, bits)
dR, dS = rhj.to_device(R), rhj.to_device(S)
keepR, keepS = dR.clone(), dS.clone()
lo, hi = C.c_uint32(), C.c_uint32()
wants = []
for d in range(n):
    assert lib.rhj_device_range(bits, n, d, C.byref(lo), C.byref(hi)) == 0
    wants.append(helpers.pairs_to_device(rhj, want[(b >= lo.value) & (b < hi.value)]))
Ms = [w.shape[0] for w in wants]
assert sum(Ms) == len(want) and min(Ms) > 1000
pr = (C.c_void_p * n)(*[dR.data_ptr()] * n); ps = (C.c_void_p * n)(*[dS.data_ptr()] * n)

def run(caps):
    bufs = [GuardedRows(torch, rhj.dev, max(M, c)) for M, c in zip(Ms, caps)]
    po = (C.c_void_p * n)(*[g.ptr for g in bufs]); cc = (C.c_uint64 * n)(*caps); ms = (C.c_uint64 * n)()
    rc = lib.rhj_join_devices(pr, len(R), ps, len(S), po, cc, ms)
    torch.cuda.synchronize()
    assert rc == (1 if any(M > c for M, c in zip(Ms, caps)) else 0), (caps, rc)
    assert list(ms) == Ms, (caps, list(ms))
    assert rhj.stats()["path"] == "fused", rhj.stats()
    for d, (g, w, c) in enumerate(zip(bufs, wants, caps)):
        what = "device %d, capacity %d of %d" % (d, c, Ms[d])
        g.assert_untouched(-GUARD_ROWS, 0, what + ", in front")
        g.assert_untouched(c, max(Ms[d], c) + GUARD_ROWS, what + ", behind")
        assert torch.equal(g.body(0, min(c, Ms[d])), w[:min(c, Ms[d])]), what
    assert torch.equal(dR, keepR) and torch.equal(dS, keepS)
    return bufs, po, ms

run([Ms[0] // 2, Ms[1]])                                     # one list short, the other exact
run([Ms[0], Ms[1] - 1])
bufs, po, ms = run(Ms)
# the whole list on one device: a destination one pair short is refused untouched, an exact one is filled and no more
M = len(want)
for cap in (M - 1, M):
    dst = GuardedRows(torch, rhj.dev, M)
    tot = C.c_uint64(0)
    rc = lib.rhj_gather_pairs_devices(po, ms, n - 1, dst.ptr, cap, C.byref(tot))
    torch.cuda.synchronize()
    assert rc == (1 if cap < M else 0) and tot.value == M, (cap, rc, tot.value)
    dst.assert_untouched(-GUARD_ROWS, 0 if cap == M else M, "gather, capacity %d" % cap)
    dst.assert_untouched(M, M + GUARD_ROWS, "gather, capacity %d, behind" % cap)
    if cap == M:
        assert torch.equal(dst.body(0, M), helpers.pairs_to_device(rhj, want))
lib.rhj_release()
print("ok")
'''


def test_device_set_lists_and_gather():
    """rhj_join_devices at n = 2 on one GPU (RHJ_DEVICES_SAME=1, a process of its own as in test_gpu_devices.py): one guarded
    buffer per device, one short and the other exact; rhj_gather_pairs_devices with a destination one pair short."""
    env = dict(os.environ, RHJ_DEVICES="2", RHJ_DEVICES_SAME="1")
    res = subprocess.run([sys.executable, "-c", DEVICES_CHILD], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert res.returncode == 0 and b"ok" in res.stdout, res.stderr.decode()[-3000:]


# ---- 11. the host ABI's second launch ----------------------------------------------------------------------------------
def test_host_abi_launches_the_fused_join_again_when_its_guess_was_short(rhj, oracle, knobs):
    """RadixHashJoin() on the fused path with duplicates on both sides: M = 2 M pairs against the context's own buffer of
    max(nR, nS) + 1024 = 501 K (and an eighth: a first allocation, the workspace is dropped in front), so out_grow makes
    join_fused clear its status words and launch the kernels a second time.  The list is the oracle's."""
    R = oracle.generate(400_000, 4, 100_000, 0.0, 111)
    S = oracle.generate(500_000, 4, 100_000, 0.0, 112)
    want = oracle.join(R, S, 9)
    assert len(want) > 2 * (len(S) + 1024)
    knobs(fused=2)
    rhj.set_bits(9)
    rhj.lib.rhj_release()
    got = rhj.RadixHashJoin(R, S)
    check_route(rhj, 9, route("fused"), "RadixHashJoin")
    assert len(got) == len(want) and (got == want).all()
