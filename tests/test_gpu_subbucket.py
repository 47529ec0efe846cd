"""GPU: the sub-bucket path (csrc/rhj_subbucket.hip.h) — canonical joins on 9..13 radix bits whose buckets are beyond the
LDS index run on r + k bits and are emitted in the order of the r bits: bit for bit the oracle's result on r bits, through
every entry point that reaches it; what the path refuses comes out of the tiled path, equally exact."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rhj():
    mod = importlib.import_module("sigmod-2018_amd")
    r = mod.RHJ(device=0)
    yield r
    r.lib.rhj_set_lowradix(1)


def dev_join(rhj, R, S, **kw):
    t, m = rhj.join_device(rhj.to_device(R), rhj.to_device(S), **kw)
    out = rhj.pairs_to_numpy(t)
    assert m == len(out)
    return out


def rel_of_keys(keys):
    from pyoracle import TUPLE
    rel = np.zeros(len(keys), dtype=TUPLE)
    rel["value"] = keys
    rel["row_id"] = np.arange(len(keys), dtype=np.uint64)
    return rel


@pytest.mark.parametrize("bits,nR,nS,kind", [
    (9, 20_000_000, 24_000_000, 1),       # S probes in most buckets
    (9, 24_000_000, 20_000_000, 0),       # R probes
    (10, 40_000_000, 40_000_000, 1),
])
def test_foreign_keys_match_the_oracle(rhj, oracle, bits, nR, nS, kind):
    rhj.set_bits(bits)
    dom = min(nR, nS)
    if kind == 1:
        R = oracle.generate(nR, 0, 0, 0.0, 31 + bits)
        S = oracle.generate(nS, 1, nR, 0.0, 32 + bits)
    else:                                 # the bigger R holds the foreign keys of the smaller S
        S = oracle.generate(nS, 0, 0, 0.0, 33 + bits)
        R = oracle.generate(nR, 1, nS, 0.0, 34 + bits)
    want = oracle.join(R, S, bits)
    assert rhj.lib.rhj_sub_bits(bits, nR, nS) >= 1
    got = dev_join(rhj, R, S)
    st = rhj.stats()
    assert st["path"] == "subbucket" and st["radix_bits"] == bits
    assert len(got) == len(want) and (got == want).all()


def test_duplicates_on_both_sides(rhj, oracle):
    """A few matches per probe tuple (Poisson), copied from the internal join's list."""
    rhj.set_bits(9)
    R = oracle.generate(18_000_000, 4, 14_000_000, 0.0, 41)
    S = oracle.generate(18_000_000, 4, 14_000_000, 0.0, 42)
    want = oracle.join(R, S, 9)
    got = dev_join(rhj, R, S)
    assert rhj.stats()["path"] == "subbucket"
    assert len(got) == len(want) and (got == want).all()


def test_two_matches_per_probe_tuple_and_capacity(rhj, oracle):
    """20 M unique R keys probing 18 M S tuples whose keys come in pairs: every matching R tuple has exactly two matches;
    and the capacity protocol (count only, too small a buffer) on this path."""
    rhj.set_bits(9)
    R = oracle.generate(20_000_000, 0, 0, 0.0, 51)
    keys = np.repeat(R["value"][:9_000_000], 2)
    np.random.default_rng(52).shuffle(keys)
    S = rel_of_keys(keys)
    want = oracle.join(R, S, 9)
    got = dev_join(rhj, R, S)
    assert rhj.stats()["path"] == "subbucket"
    assert len(got) == len(want) == 18_000_000 and (got == want).all()
    dR, dS = rhj.to_device(R), rhj.to_device(S)
    _, m = rhj.join_device(dR, dS, count_only=True)
    assert m == len(want) and rhj.stats()["path"] == "subbucket"
    t, m = rhj.join_device(dR, dS, capacity=1000)
    assert m == len(want) and rhj.stats()["path"] == "subbucket"
    assert (rhj.pairs_to_numpy(t) == want[:1000]).all()


def test_more_than_16_matches_is_refused(rhj, oracle):
    """One R tuple with 17 matches: the fused kernel hands its unit to the index walk, the path refuses and the tiled path
    answers in the same call."""
    rhj.set_bits(9)
    R = oracle.generate(20_000_000, 0, 0, 0.0, 61)
    keys = R["value"][:18_000_000].copy()
    keys[1:17] = keys[0]
    np.random.default_rng(62).shuffle(keys)
    S = rel_of_keys(keys)
    want = oracle.join(R, S, 9)
    got = dev_join(rhj, R, S)
    assert rhj.stats()["path"] not in ("subbucket", "lowradix")
    assert len(got) == len(want) and (got == want).all()


def test_bucket_range_shares_concatenate(rhj, oracle):
    rhj.set_bits(9)
    R = oracle.generate(20_000_000, 0, 0, 0.0, 71)
    S = oracle.generate(24_000_000, 1, 20_000_000, 0.0, 72)
    dR, dS = rhj.to_device(R), rhj.to_device(S)
    whole, m = rhj.join_device(dR, dS)
    assert rhj.stats()["path"] == "subbucket"
    parts = []
    for lo, hi in ((0, 100), (100, 101), (101, 512)):
        t, mm = rhj.join_device(dR, dS, bucket_range=(lo, hi))
        assert rhj.stats()["path"] == "subbucket", (lo, hi)
        assert mm == t.shape[0]
        parts.append(t)
    assert rhj.torch.equal(rhj.torch.cat(parts), whole)
    want = oracle.join(R, S, 9)
    assert m == len(want) and (rhj.pairs_to_numpy(whole) == want).all()


def test_host_relations(rhj, oracle):
    rhj.set_bits(9)
    R = oracle.generate(20_000_000, 0, 0, 0.0, 81)
    S = oracle.generate(24_000_000, 1, 20_000_000, 0.0, 82)
    want = oracle.join(R, S, 9)
    got = rhj.RadixHashJoin(R, S)
    assert rhj.stats()["path"] == "subbucket"
    assert len(got) == len(want) and (got == want).all()


def test_first_call_in_fresh_process(oracle):
    """The path as a fresh process's first join: every workspace buffer at its smallest."""
    code = r'''
import importlib, sys
sys.path.insert(0, "oracle"); sys.path.insert(0, "tests")
from pyoracle import Oracle
o = Oracle()
mod = importlib.import_module("sigmod-2018_amd"); rhj = mod.RHJ(device=0)
rhj.set_bits(9)
R = o.generate(18000000, 0, 0, 0.0, 91); S = o.generate(20000000, 1, 18000000, 0.0, 92)
t, m = rhj.join_device(rhj.to_device(R), rhj.to_device(S), capacity=len(S))
got = rhj.pairs_to_numpy(t); want = o.join(R, S, 9)
assert rhj.stats()["path"] == "subbucket"
assert m == len(want) and (got == want).all()
print("ok")
'''
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0 and b"ok" in res.stdout, res.stderr.decode()[-1500:]


def test_140m_at_12_bits_equals_the_tiled_path(rhj):
    """Beyond the oracle's reach: 140M x 140M uniform foreign keys at 12 bits (34 K a bucket), byte for byte the result of the
    path that takes the join without the split (rhj_set_lowradix(0); oracle-checked at smaller sizes) in the same process."""
    free, _ = rhj.torch.cuda.mem_get_info()
    if free < 40 * (1 << 30):
        pytest.skip("needs ~40 GB of device memory")
    import bench
    w = dict(nR=140_000_000, nS=140_000_000, bits=12, dist="uniform")
    rhj.set_bits(12)
    R, S = bench.make_relations(w, rhj.dev, 5)
    t, m = rhj.join_device(R, S, capacity=w["nS"])
    assert rhj.stats()["path"] == "subbucket" and m == w["nS"]
    rhj.lib.rhj_set_lowradix(0)
    try:
        t2, m2 = rhj.join_device(R, S, capacity=w["nS"])
        assert rhj.stats()["path"] in ("fused", "tiled")
    finally:
        rhj.lib.rhj_set_lowradix(1)
    assert m2 == m and rhj.torch.equal(t, t2)
