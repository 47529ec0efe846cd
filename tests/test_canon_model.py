"""CPU: tests/canon.py, the vectorised model of the canonical order, equals the oracle bit for bit at every radix width, on
the inputs where the order is easy to get wrong: probe-side ties and near-ties, buckets with one side empty, duplicates on
both sides, skew, and row ids that are not positions.  Both backends (numpy; torch on the CPU) are checked."""
import numpy as np
import pytest

from canon import canonical_join
from pyoracle import TUPLE

M64 = (1 << 64) - 1


def rel(keys, ids=None):
    r = np.zeros(len(keys), dtype=TUPLE)
    r["value"] = keys
    r["row_id"] = np.arange(len(keys), dtype=np.uint64) if ids is None else ids
    return r


def bucket_keys(rng, bits, buckets):
    """Random 64-bit keys with their low `bits` bits forced to the given buckets."""
    mask = np.uint64((1 << bits) - 1)
    return (rng.integers(0, M64, size=len(buckets), dtype=np.uint64, endpoint=True) & ~mask) | buckets.astype(np.uint64)


def tie_inputs(bits, seed):
    """Bucket by bucket: hR == hS, hR == hS +- 1, one side empty, and a few matches per probe tuple (S keys drawn from R's
    keys of the same bucket, some of them fresh)."""
    rng = np.random.default_rng(seed)
    nb = 1 << bits
    base = rng.integers(1, 7, size=nb)
    kind = np.arange(nb) % 5                               # 0: tie, 1: R one more, 2: S one more, 3: S empty, 4: R empty
    hR = np.where(kind == 4, 0, base + (kind == 1))
    hS = np.where(kind == 3, 0, base + (kind == 2))
    bR = np.repeat(np.arange(nb), hR)
    kR = bucket_keys(rng, bits, bR)
    dup = np.zeros(len(kR), dtype=bool)
    dup[1::3] = True
    dup &= np.concatenate([[False], bR[1:] == bR[:-1]])
    kR[dup] = kR[np.nonzero(dup)[0] - 1]                   # duplicates in R: several matches per S tuple
    offR = np.concatenate([[0], np.cumsum(hR)])
    bS = np.repeat(np.arange(nb), hS)
    pick = np.minimum(offR[bS] + (rng.random(len(bS)) * hR[bS]).astype(np.int64), max(len(kR) - 1, 0))
    drawn = (hR[bS] > 0) & (rng.random(len(bS)) < 0.8)
    kS = bucket_keys(rng, bits, bS)
    kS[drawn] = kR[pick[drawn]]
    return rel(rng.permutation(kR)), rel(rng.permutation(kS))


def inputs(oracle, kind, bits):
    if kind == "foreign_keys":
        return oracle.generate(3000, 0, 0, 0.0, 5 + bits), oracle.generate(4000, 1, 3000, 0.0, 6 + bits)
    if kind == "foreign_keys_R_bigger":
        return oracle.generate(4000, 1, 2500, 0.0, 7 + bits), oracle.generate(2500, 0, 0, 0.0, 8 + bits)
    if kind == "duplicates":
        return oracle.generate(3000, 4, 700, 0.0, 9 + bits), oracle.generate(2600, 4, 700, 0.0, 10 + bits)
    if kind == "zipf":                                    # (kind 2: Zipf ranks; a hot key holds hundreds of tuples on either side)
        return oracle.generate(3000, 2, 2000, 0.9, 11 + bits), oracle.generate(3500, 2, 2000, 0.99, 12 + bits)
    if kind == "ties":
        return tie_inputs(bits, 13 + bits)
    if kind == "arbitrary_row_ids":                       # as helpers.Golden.arbitrary_row_id_inputs
        R = oracle.generate(3000, 4, 500, 0.0, 14 + bits)
        S = oracle.generate(2000, 4, 500, 0.0, 15 + bits)
        R["row_id"] = (R["row_id"] * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0xABCDEF)
        S["row_id"] = np.uint64(M64) - S["row_id"] * np.uint64(977)
        return R, S
    raise ValueError(kind)


KINDS = ["foreign_keys", "foreign_keys_R_bigger", "duplicates", "zipf", "ties", "arbitrary_row_ids"]


def as_pairs(want):
    return np.ascontiguousarray(want).view(np.uint64).reshape(-1, 2)


@pytest.mark.parametrize("bits", range(1, 16))
@pytest.mark.parametrize("kind", KINDS)
def test_model_equals_the_oracle(oracle, kind, bits):
    R, S = inputs(oracle, kind, bits)
    want = as_pairs(oracle.join(R, S, bits))
    got = canonical_join(R["value"], R["row_id"], S["value"], S["row_id"], bits)
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert np.array_equal(got, want)


@pytest.mark.parametrize("bits", [1, 4, 9, 13])
@pytest.mark.parametrize("kind", ["ties", "arbitrary_row_ids", "zipf"])
def test_torch_backend_equals_the_numpy_backend(oracle, kind, bits):
    torch = pytest.importorskip("torch")
    R, S = inputs(oracle, kind, bits)
    t = [torch.from_numpy(np.ascontiguousarray(x).view(np.int64).copy()) for x in (R["value"], R["row_id"], S["value"], S["row_id"])]
    got = canonical_join(*t, bits)
    assert got.dtype == torch.int64
    want = as_pairs(oracle.join(R, S, bits))
    assert np.array_equal(got.numpy().view(np.uint64), want)


def test_ties_and_empty_sides_are_present():
    """The tie inputs hold what they claim at every width (else the test above would not test them)."""
    for bits in range(1, 16):
        R, S = tie_inputs(bits, 13 + bits)
        nb = 1 << bits
        mask = np.uint64(nb - 1)
        hR = np.bincount((R["value"] & mask).astype(np.int64), minlength=nb)
        hS = np.bincount((S["value"] & mask).astype(np.int64), minlength=nb)
        both = (hR > 0) & (hS > 0)
        assert (both & (hR == hS)).any() and (both & (hR == hS + 1)).any()
        if bits >= 2:
            assert (both & (hR + 1 == hS)).any() and ((hR > 0) & (hS == 0)).any()
        if bits >= 3:
            assert ((hR == 0) & (hS > 0)).any()


def test_zipf_inputs_are_skewed(oracle):
    """The Zipf inputs hold long duplicate runs on both sides (else they would only repeat the duplicates case)."""
    for bits in (1, 15):
        R, S = inputs(oracle, "zipf", bits)
        for rel_ in (R, S):
            _, counts = np.unique(rel_["value"], return_counts=True)
            assert counts.max() >= 200
