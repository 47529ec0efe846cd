"""CPU: rhj_sub_bits(), the rule that sends a canonical join on few radix bits with oversized buckets to the low-radix path
(r <= 8) or the sub-bucket path (r = 9..13) and says how many more bits it runs on internally.  Pure host logic: no
device is touched."""
import importlib
import os

import pytest

MAX_BITS = 15


@pytest.fixture(scope="module")
def rule():
    m = importlib.import_module("sigmod-2018_amd")
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m.load_library().rhj_sub_bits


# the rule as it stood for r = 1..8 before the sub-bucket path (csrc/rhj_device.hip, lowradix_sub_bits): pinned
PINNED = {
    (600_000, 900_000): [4, 3, 2, 1, 0, 0, 0, 0],
    (3_000_000, 4_000_000): [7, 6, 5, 4, 3, 2, 0, 0],
    (12_000_000, 16_000_000): [8, 8, 7, 6, 5, 4, 3, 2],
    (100_000_000, 100_000_000): [0, 0, 0, 8, 8, 7, 6, 5],
    (1_000_000_000, 100_000_000): [0, 0, 0, 8, 8, 7, 6, 5],
    (2_000_000_000, 4_000_000_000): [0] * 8,
    (4_000_000_000, 4_000_000_000): [0] * 8,
}


@pytest.mark.parametrize("sizes", sorted(PINNED))
def test_low_radix_widths_unchanged(rule, sizes):
    nR, nS = sizes
    assert [rule(r, nR, nS) for r in range(1, 9)] == PINNED[sizes]
    assert [rule(r, nS, nR) for r in range(1, 9)] == PINNED[sizes]


SIZES = [1_000, 600_000, 17_000_000, 20_000_000, 24_000_000, 40_000_000, 140_000_000, 200_000_000, 400_000_000,
         1_000_000_000, 2_000_000_000, 4_000_000_000]


@pytest.mark.parametrize("r", range(1, MAX_BITS + 1))
def test_zero_where_the_average_bucket_fits(rule, r):
    for n in SIZES:
        for m in (n, 3 * n):
            if (min(n, m) >> r) <= 33000:
                assert rule(r, n, m) == 0 and rule(r, m, n) == 0, (r, n, m)


@pytest.mark.parametrize("r", range(9, 14))
def test_sub_bucket_widths(rule, r):
    """9..13 bits: a split that brings the sub-buckets under 30 000 tuples within r + k < 15, or none at all."""
    for n in SIZES:
        for m in (n, 3 * n, n // 2 + 1):
            nmin = min(n, m)
            k = rule(r, n, m)
            assert k == rule(r, m, n)
            if (nmin >> r) <= 33000:
                assert k == 0
                continue
            fits = [j for j in range(1, MAX_BITS - r) if (nmin >> (r + j)) <= 30000]
            if not fits:
                assert k == 0, (r, n, m)
            else:
                assert k >= 1 and (nmin >> (r + k)) <= 30000 and r + k < MAX_BITS, (r, n, m, k)
                assert k == 1 or (nmin >> (r + k - 1)) > 20000               # no wider than the rule's 20 000 target needs


def test_sub_bucket_cases_of_the_workloads(rule):
    assert rule(9, 20_000_000, 24_000_000) == 1           # 39 K a bucket -> 19.5 K
    assert rule(10, 40_000_000, 40_000_000) == 1
    assert rule(12, 200_000_000, 200_000_000) == 2        # 48.8 K a bucket -> 12.2 K
    assert rule(12, 140_000_000, 140_000_000) == 1        # 34.2 K a bucket -> 17.1 K
    assert rule(12, 100_000_000, 100_000_000) == 0        # the headline workload: 24.4 K a bucket fits
    assert rule(13, 1_000_000_000, 1_000_000_000) == 0    # 122 K a bucket: even 14 bits leave 61 K


@pytest.mark.parametrize("r", [14, 15])
def test_never_at_the_widest_radix(rule, r):
    for n in SIZES:
        assert rule(r, n, n) == 0


def test_invalid_widths(rule):
    assert rule(0, 10**8, 10**8) == -1 and rule(16, 10**8, 10**8) == -1
