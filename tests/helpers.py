"""Shared helpers of the test-suite: golden-fixture loading and input regeneration."""
import io
import json
import lzma
import os

import numpy as np

from pyoracle import Oracle, TUPLE, PAIR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M64 = (1 << 64) - 1


def load_npz_xz(name):
    with lzma.open(os.path.join(GOLD, name), "rb") as f:
        return dict(np.load(io.BytesIO(f.read())))


def make_rel(values, row_ids=None):
    values = np.asarray(values, dtype=np.uint64)
    rel = np.zeros(len(values), dtype=TUPLE)
    rel["value"] = values
    rel["row_id"] = np.arange(len(values), dtype=np.uint64) if row_ids is None else row_ids
    return rel


def digest(o, pairs):
    pairs = np.ascontiguousarray(pairs, dtype=PAIR)
    return {
        "matches": int(len(pairs)),
        "fnv": "%016x" % o.fnv(pairs),
        "sumR": int(pairs["row_idR"].sum(dtype=np.uint64)) if len(pairs) else 0,
        "sumS": int(pairs["row_idS"].sum(dtype=np.uint64)) if len(pairs) else 0,
        "head": [[int(a), int(b)] for a, b in pairs[:8].tolist()],
        "tail": [[int(a), int(b)] for a, b in pairs[-8:].tolist()],
    }


DIGEST_KEYS = ("matches", "fnv", "sumR", "sumS", "head", "tail")


def assert_digest(o, pairs, rec, what=""):
    got = digest(o, pairs)
    for k in DIGEST_KEYS:
        assert got[k] == rec[k], "%s: %s differs: got %r, golden %r" % (what, k, got[k], rec[k])


class Golden:
    def __init__(self):
        self.o = Oracle()
        self.synthetic = json.load(open(os.path.join(GOLD, "synthetic_joins.json")))
        self.edges = json.load(open(os.path.join(GOLD, "edge_cases.json")))
        self.filters = json.load(open(os.path.join(GOLD, "filters.json")))
        self.small = json.load(open(os.path.join(GOLD, "small_boundary.json")))
        self._rels = None
        self._jin = None

    def gen(self, spec):
        return self.o.generate(spec["n"], spec["kind"], spec.get("domain", 0), spec.get("theta", 0.0), spec["seed"])

    def arbitrary_row_id_inputs(self):
        rec = self.synthetic["arbitrary_row_ids"]
        R = self.o.generate(3000, 4, 500, 0, rec["seedR"])
        S = self.o.generate(2000, 4, 500, 0, rec["seedS"])
        R["row_id"] = (R["row_id"] * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0xABCDEF)
        S["row_id"] = np.uint64(M64) - S["row_id"] * np.uint64(977)
        return R, S, rec

    def filter_inputs(self, c):
        col = self.o.generate(c["n"], 4, c["domain"], 0, c["seed"])["value"]
        sel = self.o.generate(c["n"] // 2 + 3, 4, c["n"], 0, c["seed"] + 100)["value"] if c["mode"] == "indirect" else None
        return col, sel

    @property
    def small_relations(self):
        if self._rels is None:
            self._rels = load_npz_xz("small_relations.npz.xz")
        return self._rels

    @property
    def small_join_inputs(self):
        if self._jin is None:
            self._jin = load_npz_xz("small_join_inputs.npz.xz")
        return self._jin

    def small_join(self, idx):
        j = self.small_join_inputs
        return make_rel(j["j%d_R" % idx]), make_rel(j["j%d_S" % idx])


def spec_join(R, S, bits):
    """Independent numpy statement of SURVEY.md A.1 (not a restatement of the
    reference's code): bucket ascending, probe side = R if cR >= cS else S, probe
    tuples in input order, build matches in descending input position."""
    mask = np.uint64((1 << bits) - 1)
    out = []
    bR, bS = (R["value"] & mask), (S["value"] & mask)
    oR, oS = np.argsort(bR, kind="stable"), np.argsort(bS, kind="stable")
    cR = np.bincount(bR.astype(np.int64), minlength=1 << bits)
    cS = np.bincount(bS.astype(np.int64), minlength=1 << bits)
    sR, sS = np.concatenate([[0], np.cumsum(cR)]), np.concatenate([[0], np.cumsum(cS)])
    for b in range(1 << bits):
        if cR[b] == 0 or cS[b] == 0:
            continue
        r, s = R[oR[sR[b]:sR[b + 1]]], S[oS[sS[b]:sS[b + 1]]]
        probe, build, flip = (r, s, False) if cR[b] >= cS[b] else (s, r, True)
        pos = {}
        for i in range(len(build) - 1, -1, -1):
            pos.setdefault(int(build["value"][i]), []).append(i)
        for p in probe:
            for q in pos.get(int(p["value"]), ()):
                a, c = int(p["row_id"]), int(build["row_id"][q])
                out.append((c, a) if flip else (a, c))
    return np.array(out, dtype=PAIR) if out else np.zeros(0, dtype=PAIR)


# relation_map.c:64-84 (and rhj_column_stats_device, sigmod-2018_amd/csrc/rhj_inter.hip): one flag per value of
# [l, u] below this range, folded modulo STATS_FOLD at this range or above
STATS_CAP = 50_000_000
STATS_FOLD = 5_000_000


def column_stats_model(col):
    """(l, u, d) of a u64 column as relation_map.c:53-84 computes them, in Python ints: u - l + 1 is
    never allowed to wrap, so the full range (0, 2^64 - 1) is the range 2^64 and folds like any other
    range of STATS_CAP or more (the reference's own code is undefined there)."""
    col = np.asarray(col, dtype=np.uint64)
    lo, hi = int(col.min()), int(col.max())
    x = col - np.uint64(lo)                       # in [0, hi - lo]: no wrap
    if hi - lo + 1 >= STATS_CAP:
        x = x % np.uint64(STATS_FOLD)
    return lo, hi, float(len(np.unique(x)))


# ---- pair buffers between sentinel rows (tests/test_gpu_out_bounds.py) --------------------------------------------------
GUARD_ROWS = 4096                        # 64 KiB of 16-byte rows on either side: row 0 keeps a fresh allocation's alignment
SENTINEL = -0x5A5A5A5A5A5A5A5B           # 0xA5A5A5A5A5A5A5A5 as int64: no row id or key of the tests (all below 2^48)


class GuardedRows:
    """`rows` 16-byte rows on the device (row 0 is what an entry point gets) with GUARD_ROWS rows in front of and behind them,
    every word SENTINEL: what a kernel writes outside [0, capacity) lands in this tensor and is found."""

    def __init__(self, torch, dev, rows):
        self.rows = int(rows)
        self.t = torch.full((GUARD_ROWS + self.rows + GUARD_ROWS, 2), SENTINEL, dtype=torch.int64, device=dev)

    @property
    def ptr(self):
        return self.t[GUARD_ROWS:].data_ptr()

    def body(self, lo, hi):
        return self.t[GUARD_ROWS + lo:GUARD_ROWS + hi]

    def touched(self, lo, hi):
        """rows of [lo, hi) (lo may be negative: the front guard) that no longer hold the sentinel, counted on the device"""
        return int((self.body(lo, hi) != SENTINEL).any(dim=1).sum().item())

    def assert_untouched(self, lo, hi, what):
        part = self.body(lo, hi)
        bad = part != SENTINEL
        words = int(bad.sum().item())
        if words:
            row = int(bad.any(dim=1).nonzero()[0].item())
            a, b = (int(x) for x in part[row].cpu().numpy().view(np.uint64))
            raise AssertionError("%s: %d words written outside the buffer, the first in row %d: (%d, %d)" % (what, words, lo + row, a, b))


def pairs_to_device(rhj, pairs):
    a = np.ascontiguousarray(pairs).view(np.int64).reshape(-1, 2)
    return rhj.torch.from_numpy(a.copy()).to(rhj.dev)


def guarded_join(rhj, call, dR, dS, cap, want):
    """One raw join entry point on a sentinel-guarded buffer.  call(out_ptr, cap, matches_ref) -> rc invokes it; want: the
    oracle's pairs (PAIR array or [M, 2] device tensor).  Asserts the capacity contract of include/rhj.h: rc 1 iff M > cap,
    *matches == M, rows [0, min(cap, M)) the oracle's, nothing written in front of row 0 or from row cap on, the relations
    unchanged.  The buffer spans max(M, cap) rows, so a store whose guard is wrong stays inside it.  Rows [M, cap) are left
    open by the header; returns how many of them were written."""
    import ctypes as C
    torch = rhj.torch
    want_t = want if torch.is_tensor(want) else pairs_to_device(rhj, want)
    M = want_t.shape[0]
    g = GuardedRows(torch, rhj.dev, max(M, cap))
    keepR, keepS = dR.clone(), dS.clone()
    m = C.c_uint64(0xDEAD)
    rc = call(g.ptr, cap, C.byref(m))
    torch.cuda.synchronize()
    what = "capacity %d, %d pairs" % (cap, M)
    assert rc == (1 if M > cap else 0), "%s: return code %d" % (what, rc)
    assert m.value == M, "%s: *matches = %d" % (what, m.value)
    g.assert_untouched(-GUARD_ROWS, 0, what + ", in front of the buffer")
    g.assert_untouched(cap, max(M, cap) + GUARD_ROWS, what + ", behind the capacity (row 0 = d_out)")
    n = min(cap, M)
    got = g.body(0, n)
    if not torch.equal(got, want_t[:n]):
        i = int((got != want_t[:n]).any(dim=1).nonzero()[0].item())
        raise AssertionError("%s: pair %d is %r, expected %r" % (what, i, got[i].tolist(), want_t[i].tolist()))
    assert torch.equal(dR, keepR) and torch.equal(dS, keepS), "%s: an input relation was written" % what
    return g.touched(M, cap) if cap > M else 0


def _keys_of(rel, ids):
    if np.array_equal(rel["row_id"], np.arange(len(rel), dtype=np.uint64)):
        return rel["value"][ids]
    order = np.argsort(rel["row_id"], kind="stable")
    return rel["value"][order[np.searchsorted(rel["row_id"][order], ids)]]


def pair_layout(R, S, want, bits):
    """Of every wanted pair: its bucket, and a number that names its probe tuple (R's where cR >= cS, rhjoin.c:86).
    Row ids must be unique in R."""
    mask = np.uint64((1 << bits) - 1)
    b = (_keys_of(R, want["row_idR"]) & mask).astype(np.int64)
    cR = np.bincount((R["value"] & mask).astype(np.int64), minlength=1 << bits)
    cS = np.bincount((S["value"] & mask).astype(np.int64), minlength=1 << bits)
    probe = np.where((cR >= cS)[b], want["row_idR"] * np.uint64(2) + np.uint64(1), want["row_idS"] * np.uint64(2))
    return b, probe


def guard_capacities(b, probe):
    """The capacities a guarded case runs, from the wanted list alone: 0, 1, the first bucket edge and one near the middle
    with their neighbours, a position inside the longest run of pairs of one probe tuple, M - 1, M, M + 1."""
    M = len(b)
    caps = {0, 1, M - 1, M, M + 1}
    edge = np.nonzero(np.diff(b))[0] + 1
    for e in ((edge[0], edge[len(edge) // 2]) if len(edge) else ()):
        caps |= {int(e) - 1, int(e), int(e) + 1}
    if M > 1:
        starts = np.concatenate([[0], np.nonzero(np.diff(probe))[0] + 1, [M]])
        lens = np.diff(starts)
        i = int(np.argmax(lens))
        if lens[i] > 1:
            caps.add(int(starts[i] + lens[i] // 2))
    return sorted(c for c in caps if 0 <= c <= M + 1)
