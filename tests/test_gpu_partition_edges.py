"""rhj_partition_device at the tile, group, strip, batch, run and scan edges of its launch plan (rhj_device.hip: run_partition,
partition_pass; rhj_partition.hip.h), and two relations of very different sizes in one launch through rhj_join_device.

The shapes come from tests/partition_model.py; tests/test_partition_model.py holds every one of them, on the CPU, to the
regime its name claims.  Every comparison is bit for bit — the partitioned tuples, h_hist and h_psum — against the oracle on
the CPU, or above 8.4 M tuples against partition_model.stable_partition on the device; never against the call under test.
Row ids are the positions (a stability error shows), keys carry random bits above the radix and above bit 32 (a tuple
misplaced inside its bucket shows), d_out lies between sentinel rows, h_hist and h_psum between guard words, and the input is
compared unchanged after every call."""
import functools
import importlib

import numpy as np
import pytest

import helpers
import partition_model as pm
from helpers import make_rel

pytestmark = pytest.mark.gpu

CONST = pm.constants()
T = CONST.PT_TILE
GUARD_WORDS = 8
HIST_GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)
PSUM_GUARD = np.int64(helpers.SENTINEL)


@pytest.fixture(scope="module")
def rhj():
    mod = importlib.import_module("sigmod-2018_amd")
    r = mod.RHJ(device=0)
    bits0 = r.lib.rhj_get_radix_bits()
    yield r
    r.lib.rhj_set_count_in_pass1(1)
    r.set_bits(bits0)


def call_partition(rhj, d_in, bits, want_t, whist, wpsum, what):
    """One rhj_partition_device call on a guarded output, compared with (want_t, whist, wpsum)."""
    torch = rhj.torch
    n, bins = d_in.shape[0], 1 << bits
    keep = d_in.clone()
    g = helpers.GuardedRows(torch, rhj.dev, n)                       # (GUARD_ROWS >= 64 sentinel tuples on each side)
    hist = np.full(bins + 2 * GUARD_WORDS, HIST_GUARD, dtype=np.uint64)
    psum = np.full(bins + 2 * GUARD_WORDS, PSUM_GUARD, dtype=np.int64)
    rhj.set_bits(bits)
    rc = rhj.lib.rhj_partition_device(d_in.data_ptr(), n, g.ptr, hist[GUARD_WORDS:].ctypes.data, psum[GUARD_WORDS:].ctypes.data)
    torch.cuda.synchronize()
    assert rc == 0, "%s: return code %d" % (what, rc)
    g.assert_untouched(-helpers.GUARD_ROWS, 0, what + ", in front of d_out")
    g.assert_untouched(n, n + helpers.GUARD_ROWS, what + ", behind d_out")
    for name, a, guard in (("h_hist", hist, HIST_GUARD), ("h_psum", psum, PSUM_GUARD)):
        assert (a[:GUARD_WORDS] == guard).all() and (a[-GUARD_WORDS:] == guard).all(), "%s: words written beside %s" % (what, name)
    h, p = hist[GUARD_WORDS:-GUARD_WORDS], psum[GUARD_WORDS:-GUARD_WORDS]
    if not np.array_equal(h, whist):
        b = int(np.nonzero(h != whist)[0][0])
        raise AssertionError("%s: h_hist[%d] is %d, expected %d" % (what, b, h[b], whist[b]))
    if not np.array_equal(p, wpsum):
        b = int(np.nonzero(p != wpsum)[0][0])
        raise AssertionError("%s: h_psum[%d] is %d, expected %d" % (what, b, p[b], wpsum[b]))
    got = g.body(0, n)
    if not torch.equal(got, want_t):
        bad = (got != want_t).any(dim=1)
        i = int(bad.nonzero()[0].item())
        raise AssertionError("%s: %d tuples differ, the first at %d: (%#x, %d), expected (%#x, %d)" % (
            what, int(bad.sum().item()), i, *got[i].tolist(), *want_t[i].tolist()))
    assert torch.equal(d_in, keep), "%s: the input was written" % what


def check(rhj, oracle, keys, bits, what, modes=(1,), row_ids=None):
    """keys (numpy) with their positions as row ids through rhj_partition_device, against the oracle; modes: the values of
    rhj_set_count_in_pass1 to run with (the expected output is the same)."""
    rel = make_rel(keys, row_ids)
    want, whist, wpsum = oracle.partition(rel, bits)
    d_in, want_t = rhj.to_device(rel), rhj.to_device(want)
    try:
        for on in modes:
            rhj.lib.rhj_set_count_in_pass1(on)
            call_partition(rhj, d_in, bits, want_t, whist, wpsum, "%s, n = %d, %d bits, count_in_pass1 = %d" % (what, len(rel), bits, on))
    finally:
        rhj.lib.rhj_set_count_in_pass1(1)


@functools.lru_cache(maxsize=2)
def a_key_set(kind, bits):
    return pm.a_keys(kind, bits, pm.a_sizes(bits)[-1])


@functools.lru_cache(maxsize=4)
def b_key_set(kind, bits):
    return pm.b_keys(kind, bits, pm.B_MAX_TILES * T)


@functools.lru_cache(maxsize=2)
def f_key_set(kind, bits):
    return pm.f_keys(kind, bits, max(pm.f_sizes()))


# ---- A: tile, group and slice edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pm.A_KINDS)
@pytest.mark.parametrize("bits", pm.A_BITS)
def test_a_tile_group_and_slice_edges(rhj, oracle, bits, kind):
    """n = 1 .. one tile, one group of pass-1 tiles to two, eight groups to nine (a slice of k_group_scan takes two groups and
    slices stay empty); up to 12 bits with pass 1's own counts and with k_hist_runs'."""
    keys = a_key_set(kind, bits)
    for n in pm.a_sizes(bits):
        check(rhj, oracle, keys[:n], bits, "A %s" % kind, modes=(1, 0) if bits <= 12 else (1,))


# ---- B: strips ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", list(pm.B_ROWS))
@pytest.mark.parametrize("bits", pm.B_BITS)
def test_b_strips(rhj, oracle, bits, regime):
    """Strips of 1, 2 and 4 tiles at 9 bits (4 strips a group, the last of 3 tiles), 10 (8, the last of 2) and 12 (15, none
    short); the relation ends with a full tile or with one tuple, inside a strip for most tile counts; the 16-bit cells reach
    strip * 4096 in the upper half of a word (equal) and 2 * 4096 in both halves (pair)."""
    for tiles, full, kind, both in pm.B_ROWS[regime]:
        n = pm.b_size(tiles, full)
        assert pm.plan(bits, n).strip == pm.B_REGIME_STRIP[regime]
        check(rhj, oracle, b_key_set(kind, bits)[:n], bits, "B %s, %d tiles, %s" % (regime, tiles, kind), modes=(1, 0) if both else (1,))


# ---- C: pass-2 batch edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", pm.C_BITS)
def test_c_pass2_batch_edges(rhj, oracle, bits):
    """One group; pass-2 tile (d*, 0) holds exactly 0, 1, a batch less one, a batch, a batch and one, ... , every tuple."""
    for dstar in pm.c_dstars(bits):
        for count in pm.c_counts(bits):
            check(rhj, oracle, pm.c_keys(bits, dstar, count), bits, "C d* = %d, %d tuples" % (dstar, count))


# ---- D: runs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", pm.D_PLACES)
@pytest.mark.parametrize("bits", pm.D_BITS)
def test_d_runs(rhj, oracle, bits, place):
    """One group at 9 bits (15 runs: the wave's scan of the run table) and 14 (120 runs: the workgroup's); the runs of one
    pass-1 digit are 1, 0, 0, 1, ... (the run search's fallback), 63, 64, 65, ... (borders on a round's ends), one whole
    tile among empty runs, and the group's very last tuple."""
    check(rhj, oracle, pm.d_keys(place, bits), bits, "D %s" % place)


# ---- E: a workgroup of k_scatter_runs with several tiles ---------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", list(pm.E_TILES))
@pytest.mark.parametrize("bits", pm.E_BITS)
def test_e_a_workgroup_with_several_tiles(rhj, oracle, bits, tiles):
    """More pass-2 tiles than workgroups: two tiles for the first workgroups (500 pass-1 tiles), three or four (1447); tiles
    of many batches among one-batch tiles, and empty tiles as a workgroup's first and as its last."""
    n = pm.e_size(tiles)
    assert pm.plan(bits, n).busiest == pm.E_TILES[tiles][1]
    for kind in pm.E_KINDS:
        check(rhj, oracle, pm.e_keys(kind, bits, n), bits, "E %d tiles, %s" % (tiles, kind))


# ---- F: one pass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pm.F_KINDS)
@pytest.mark.parametrize("bits", pm.F_BITS)
def test_f_one_pass(rhj, oracle, bits, kind):
    """1, 2, 16 | 17 tiles (one chunk, two), 1024 | 1025 (k_scan_bins carries into a second round of 64 chunks), 2048 | 2049
    (k_hist_tiles strides its grid); the last tile full and with one tuple."""
    keys = f_key_set(kind, bits)
    for n in pm.f_sizes():
        check(rhj, oracle, keys[:n], bits, "F %s" % kind)


# ---- G: large, wholly on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bits,n", pm.g_rows(), ids=["%s, %d bits" % (r[0], r[1]) for r in pm.g_rows()])
def test_g_large_on_the_device(rhj, name, bits, n):
    """8193 tiles less 5 tuples: the one-pass chunk count clamps at 512 (17 tiles a chunk, empty chunks behind the last tile,
    8 rounds of k_scan_bins, 5 grid strides of k_hist_tiles); k_group_scan<true> without shares (9, 11 bits) and with shares
    over R > 1 groups that do not divide the rows (10, 12); 15362 tiles at 14 bits: k_hist_runs with 8 digits a workgroup."""
    torch = rhj.torch
    gen = torch.Generator(device=rhj.dev)
    gen.manual_seed(1000 + bits)
    keys = torch.randint(0, 1 << pm.KEY_BITS, (n,), dtype=torch.int64, device=rhj.dev, generator=gen)
    ids = torch.arange(n, dtype=torch.int64, device=rhj.dev)
    want, hist, psum = pm.stable_partition(keys, ids, bits)
    d_in = torch.stack([keys, ids], dim=1)
    del keys, ids
    call_partition(rhj, d_in, bits, want, hist.cpu().numpy().astype(np.uint64), psum.cpu().numpy(), "G %s, n = %d, %d bits" % (name, n, bits))


# ---- H: two relations in one launch ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def h_big_keys():
    return pm.keys_uniform(np.random.default_rng(8), max(max(s) for s in pm.h_sizes()), 0)


def join_case(rhj, oracle, bits, nR, nS):
    big = h_big_keys()
    rng = np.random.default_rng(nR + 3 * nS + bits)
    small = big[rng.integers(0, len(big), size=min(nR, nS))]           # the small side's keys are drawn from the large side's
    R, S = (make_rel(small), make_rel(big)) if nR < nS else (make_rel(big), make_rel(small))
    assert (len(R), len(S)) == (nR, nS)
    want = oracle.join(R, S, bits)
    assert len(want) >= min(nR, nS)
    rhj.set_bits(bits)
    t, m = rhj.join_device(rhj.to_device(R), rhj.to_device(S), capacity=len(want) + 8)
    what = "H %d x %d, %d bits" % (nR, nS, bits)
    assert m == len(want), "%s: %d matches, expected %d" % (what, m, len(want))
    assert rhj.torch.equal(t, helpers.pairs_to_device(rhj, want)), "%s: the pairs differ" % what
    return rhj.stats()["path"]


@pytest.mark.parametrize("bits", pm.H_BITS)
def test_h_two_relations_of_very_different_sizes(rhj, oracle, bits):
    """One side has one or two tiles, the other 2050 and selects strips of four: the small side's extra workgroups of pass 1
    write zero counts and nothing else.  Every such join runs on the fused path (the build sides are the small relation's)."""
    for nR, nS in pm.h_sizes():
        assert join_case(rhj, oracle, bits, nR, nS) == "fused"


def test_h_one_pass_with_two_relations_beyond_the_small_route(rhj, oracle):
    """partition_pass with two relations beyond SMALL_TILES: the fused path on 8 bits or fewer with a relation too large for
    the small path — 2 tiles beside 2050, so k_hist_tiles strides for one relation only."""
    n = pm.h_sizes()[0][1]
    assert pm.tiles_for(n) > CONST.SMALL_TILES
    for nR, nS in ((4097, n), (n, 4097)):
        assert join_case(rhj, oracle, pm.H_ONE_PASS_BITS, nR, nS) == "fused"


# ---- B, wide row ids: last, because a process that met one launches the 16-byte kernels from then on ---------------------------------
def test_b_wide_row_ids_inside_a_strip(rhj, oracle):
    """A single row id of 2^32 or more that the sample of the first and last 2048 tuples does not see: in the first tile of a
    strip (pass 1 carries the flag across the strip's tiles) and in the last, partial tile; the partition runs again with
    16-byte intermediates."""
    bits = pm.B_WIDE_BITS
    keys = b_key_set("uniform", bits)
    for name, tiles, n, pos in pm.b_wide_rows():
        ids = np.arange(n, dtype=np.uint64)
        ids[pos] += np.uint64(pm.WIDE)
        check(rhj, oracle, keys[:n], bits, "B wide row id in the %s, %d tiles" % (name, tiles), row_ids=ids)


def test_b_narrow_row_ids_after_wide_ones(rhj, oracle):
    """The same process, narrow row ids again: both widths are launched now, the 12-byte kernels move the data."""
    bits = pm.B_WIDE_BITS
    tiles, full, kind, _ = pm.B_ROWS["strip 4"][4]
    n = pm.b_size(tiles, full)
    check(rhj, oracle, b_key_set(kind, bits)[:n], bits, "B strip 4 after wide row ids, %d tiles, %s" % (tiles, kind), modes=(1, 0))
