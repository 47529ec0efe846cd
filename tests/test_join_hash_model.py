"""The numpy restatement of the join kernels' hashes (tests/hashkeys.py) against the oracle and the kernel sources, and
the collision constructors against the properties they claim.  CPU only."""
import os
import re

import numpy as np
import pytest

import hashkeys as hk

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sigmod-2018_amd", "csrc")


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_mix64_is_the_oracle_generators():
    """oracle.generate(n, 0, ...) is mix64 of a permutation of [0, n)."""
    from pyoracle import Oracle
    n = 50000
    v = Oracle().generate(n, 0, 0, 0.0, 17)["value"]
    x = hk.unmix64(v)
    assert np.array_equal(np.sort(x), np.arange(n, dtype=np.uint64))
    assert np.array_equal(hk.mix64(x), v)


def test_inverses():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 1 << 64, size=10000, dtype=np.uint64, endpoint=False)
    assert np.array_equal(hk.unmix64(hk.mix64(x)), x)
    for bits in (1, 8, 12, 15):
        h = hk.h32(x, bits)
        k = hk.h32_keys(1, bits, h[:50])
        assert hk._bucket_ok(k, 1, bits) and np.array_equal(hk.h32(k, bits), h[:50])


def test_kernel_sources_still_hash_as_restated():
    """Drift guard: the constants and shifts the restatement uses appear in the kernel headers.  A change to a kernel
    hash fails here until tests/hashkeys.py follows it."""
    common, fused, tiled, exact = (src(n) for n in ("rhj_common.hip.h", "rhj_join_fused.hip.h", "rhj_join_tiled.hip.h",
                                                     "rhj_join_exact.hip.h"))
    flat = lambda s: re.sub(r"\s+", " ", s)
    assert "x ^= x >> 30; x *= 0x%xull;" % hk.MIX_C1 in flat(common)
    assert "x ^= x >> 27; x *= 0x%xull;" % hk.MIX_C2 in flat(common)
    assert "x ^= x >> 31;" in flat(common)
    f = flat(fused)
    assert "(uint32_t)(key >> bits) ^ __builtin_rotateleft32((uint32_t)(key >> 32) >> bits, 16)" in f
    assert "x * 0x%xu" % hk.H32_C in f and "h ^ (h >> 15)" in f
    assert "__umul24(h >> 16, hs) >> 16" in f
    assert "min(h & 0xffffu, 0x%xu) + 1u" % hk.TAG_CLAMP in f
    assert "min((uint32_t)(h >> 16) & 0xffffu, 0x%xu) + 1u" % hk.TAG_CLAMP in f
    assert "__umulhi((uint32_t)(h >> 32), hs)" in f
    t = flat(tiled)
    assert "__umulhi((uint32_t)(h >> 32), slots)" in t and "(uint32_t)(h >> 16) & 0xffffu" in t
    assert "return h >> (64 - lg);" in t and "tag(uint64_t h) const { return (uint32_t)h; }" in t
    x = flat(exact)
    assert "((key >> bits) * 0x%xull) << bits" % hk.XJ_C in x
    assert "__umulhi((uint32_t)(y >> 32) & 0xffffff00u, hs)" in x
    assert "(uint32_t)(y >> bits)" in x and "(uint32_t)(y >> (bits + 32u)) & 0xffu" in x
    assert "1u << (24u - f.radix_bits)" in x


@pytest.mark.parametrize("bits", range(1, 16))
def test_h32_clones(bits):
    b = (1 << bits) - 1
    k = hk.h32_clones(b, bits, 2000, seed=bits)
    assert hk._bucket_ok(k, b, bits) and len(np.unique(hk.h32(k, bits))) == 1
    s = hk.h32_clones(b, bits, min(300, 1 << bits), seed=bits, shared_low=True)
    assert hk._bucket_ok(s, b, bits) and len(np.unique(hk.h32(s, bits))) == 1
    assert len(np.unique(s & np.uint64(hk.M32))) == 1


def test_keys_with_hash():
    hv = [0x12340000, 0x1234FFFD, 0x1234FFFE, 0x1234FFFF]
    k = hk.keys_with_hash(3, 9, hv, hash="h32", per=40)
    assert hk._bucket_ok(k, 3, 9)
    assert np.array_equal(hk.h32(k, 9), np.repeat(np.array(hv, dtype=np.uint64), 40))
    h = hk.h32(k, 9)
    assert len(np.unique(hk.h32_slot(h, 1000))) == 1
    assert list(np.unique(hk.clamp_tag(hk.h32_raw_tag(h)))) == [1, 0xFFFE]
    k = hk.keys_with_hash(7, 10, [(100, 0xFFFD), (100, 0xFFFF), (100, 0)], hash="mix64", per=300, hs=1500)
    h = hk.mix64(k)
    assert hk._bucket_ok(k, 7, 10) and list(np.unique(hk.mix_slot(h, 1500))) == [100]
    assert list(np.unique(hk.mix_raw_tag(h))) == [0, 0xFFFD, 0xFFFF]
    k = hk.keys_with_hash(7, 6, [0, hk.M32], hash="tab64", per=500)
    h = hk.mix64(k)
    assert hk._bucket_ok(k, 7, 6) and list(np.unique(hk.tab64_tag(h))) == [0, hk.M32]
    assert len(np.unique(hk.tab64_home(h, 14))) == 1
    k = hk.mix64_keys(5, 6, 500, 0x9E3779B9, 1, 0x1234)       # one top word: one Tab32 home at any size
    h = hk.mix64(k)
    assert len(k) == 500 and hk._bucket_ok(k, 5, 6) and len(np.unique(h >> np.uint64(16))) == 1


def test_mix64_lowword_pairs():
    p = hk.mix64_lowword_pairs(9, 10, 1200, 3, seed=1)
    h = hk.mix64(p)
    assert hk._bucket_ok(p.reshape(-1), 9, 10)
    assert np.array_equal(p[:, 0] & np.uint64(hk.M32), p[:, 1] & np.uint64(hk.M32))
    assert np.array_equal(hk.mix_slot(h[:, 0], 1200), hk.mix_slot(h[:, 1], 1200))
    assert np.array_equal(hk.clamp_tag(hk.mix_raw_tag(h[:, 0])), hk.clamp_tag(hk.mix_raw_tag(h[:, 1])))


@pytest.mark.parametrize("bits", [10, 11, 12])
def test_exact_colliders(bits):
    """Kind a: equal 40 stored bits, the next slot at hs_min and the same slot at hs_min / 2 (so the index is exact only
    from hs_min on); kind b: equal ent, another ext, the same slot at hs_min."""
    hm = hk.xj_hs_min(bits)
    seeds = hk.exact_seed_keys(3, bits, 200, seed=bits)
    col = np.array([hk.exact_colliders(k, bits) for k in seeds], dtype=np.uint64)
    a, b = col[:, 0], col[:, 1]
    assert hk._bucket_ok(np.concatenate([seeds, a, b]), 3, bits)
    e, x = hk.xj_ent, hk.xj_ext
    assert np.array_equal(e(a, bits), e(seeds, bits)) and np.array_equal(x(a, bits), x(seeds, bits))
    assert np.array_equal(e(b, bits), e(seeds, bits)) and not np.any(x(b, bits) == x(seeds, bits))
    assert np.array_equal(hk.xj_slot(a, bits, hm), hk.xj_slot(seeds, bits, hm) + np.uint64(1))
    assert np.array_equal(hk.xj_slot(a, bits, hm // 2), hk.xj_slot(seeds, bits, hm // 2))
    assert np.array_equal(hk.xj_slot(b, bits, hm), hk.xj_slot(seeds, bits, hm))
    p = hk.xj_product(np.concatenate([seeds, a, b]), bits)
    assert len(np.unique(p)) == 3 * len(seeds)                # a bijection: distinct keys, distinct products


def test_extreme_keys():
    k = hk.EXTREME_KEYS
    assert len(np.unique(k)) == 5 and k.min() == 0 and k.max() == np.uint64(hk.M64)
