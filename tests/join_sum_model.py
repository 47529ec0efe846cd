"""What rhj_join_sum_batch_device (include/rhj_inter.h) computes, restated without the library: join_sum, a numpy model of an
item (counts per key by np.unique, Python-integer arithmetic modulo 2^64); the table rule of csrc/rhj_join_sum_batch.hip.h (hash,
size, build side) with its constants read out of the header; and keys built from that rule to collide or to wrap."""
import os
import re

import numpy as np

from source_constants import c_int, one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "sigmod-2018_amd", "csrc", "rhj_join_sum_batch.hip.h")
DEVICE = os.path.join(ROOT, "sigmod-2018_amd", "csrc", "rhj_device.hip")
M64 = (1 << 64) - 1


def join_sum(keysR, keysS, terms):
    """(matches, sums) of the join keysR[i] == keysS[j]: the number of pairs (i, j) and, per term (side, values), the sum of
    values[i] (side 0) or values[j] (side 1) over them modulo 2^64.  keys and values are u64 numpy arrays, values aligned with
    its side's keys (the caller has applied d_sel and d_src)."""
    keysR, keysS = np.asarray(keysR, dtype=np.uint64), np.asarray(keysS, dtype=np.uint64)
    uR, cR = np.unique(keysR, return_counts=True)
    uS, cS = np.unique(keysS, return_counts=True)
    cntR = dict(zip(uR.tolist(), cR.tolist()))
    cntS = dict(zip(uS.tolist(), cS.tolist()))
    matches = sum(c * cntS.get(k, 0) for k, c in cntR.items())
    assert matches < (1 << 64)
    sums = []
    for side, values in terms:
        keys, other = (keysR, cntS) if side == 0 else (keysS, cntR)
        values = np.asarray(values, dtype=np.uint64)
        assert len(values) == len(keys)
        # per distinct key the sum of its rows' values (exact Python integers), times the other side's count
        order = np.argsort(keys, kind="stable")
        sk, sv = keys[order], values[order]
        total = 0
        if len(sk):
            starts = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
            # the halves of the values summed apart: below 2^64 for fewer than 2^32 rows, so numpy's sums are exact
            hi = np.add.reduceat(sv >> np.uint64(32), starts).tolist()
            lo = np.add.reduceat(sv & np.uint64(0xFFFFFFFF), starts).tolist()
            for k, h, l in zip(sk[starts].tolist(), hi, lo):
                total += other.get(k, 0) * ((h << 32) + l)
        sums.append(total & M64)
    return matches, sums


def brute_force(keysR, keysS, terms):
    """the same by a double loop"""
    matches, sums = 0, [0] * len(terms)
    for i, a in enumerate(keysR):
        for j, b in enumerate(keysS):
            if int(a) == int(b):
                matches += 1
                for t, (side, values) in enumerate(terms):
                    sums[t] = (sums[t] + int(values[i if side == 0 else j])) & M64
    return matches, sums


# ---- the table's rule, with the header's constants ---------------------------------------------------------------------------------

def parse_constants():
    with open(HEADER) as f:
        text = f.read()
    with open(DEVICE) as f:
        dev = f.read()
    names = {}
    for m in re.finditer(r"constexpr\s+(?:int|uint32_t|uint64_t|size_t)\s+(\w+)\s*=\s*([^;,]+)[;,]", text):
        try:
            names[m.group(1)] = c_int(m.group(2), names)
        except (ValueError, NameError, SyntaxError, TypeError, ZeroDivisionError):
            pass
    who = "tests/join_sum_model.py"
    names["JSUM_HASH_MUL"] = int(one(r"JSUM_HASH_MUL = (0x[0-9A-Fa-f]+)ull;", text, "the hash constant", who).group(1), 16)
    # the rules restated below, as the code words them: a change there must be looked at here
    for pat, what in ((r"while \(\(\(uint64_t\)1 << l\) < JSUM_SLOTS_PER_ROW \* rows\) \+\+l;", "the table's size"),
                      (r"uint32_t l = 1;", "the smallest table"),
                      (r"return \(key \* JSUM_HASH_MUL\) >> \(64 - log2_slots\);", "the hash"),
                      (r"jsum_build_side\(uint64_t nR, uint64_t nS\) \{ return nS < nR \? 1 : 0; \}", "the build side"),
                      (r"s = \(s \+ 1\) & mask", "the probe step")):
        one(pat, text, what, who)
    one(r"JSUM_ARENA_BYTES = BATCH_ARENA_BUDGET;", dev, "the arena of the tables", who)
    names["JSUM_ARENA_BYTES"] = 1 << int(one(r"BATCH_ARENA_BUDGET = \(size_t\)1 << (\d+);", dev, "the arena budget", who).group(1))
    names["JSUM_MAX_ITEMS"] = int(one(r"JSUM_MAX_ITEMS = (\d+);", dev, "the items of a chunk", who).group(1))
    missing = [n for n in ("JSUM_TILE", "JSUM_EMPTY", "JSUM_SLOTS_PER_ROW", "JSUM_SLOT_BYTES") if n not in names]
    if missing:
        raise AssertionError("%s no longer finds %s in the sources" % (who, missing))
    return names


K = parse_constants()
TILE, EMPTY, MUL, ARENA_BYTES, MAX_ITEMS, SLOT_BYTES = K["JSUM_TILE"], K["JSUM_EMPTY"], K["JSUM_HASH_MUL"], K["JSUM_ARENA_BYTES"], K["JSUM_MAX_ITEMS"], K["JSUM_SLOT_BYTES"]
MUL_INV = pow(MUL, -1, 1 << 64)


def log2_slots(rows):
    l = 1
    while (1 << l) < K["JSUM_SLOTS_PER_ROW"] * rows:
        l += 1
    return l


def build_side(nR, nS):
    return 1 if nS < nR else 0


def table_log2(nR, nS):
    return log2_slots(nS if build_side(nR, nS) else nR)


def table_bytes(nR, nS):
    return SLOT_BYTES << table_log2(nR, nS)


def home(key, log2):
    return ((int(key) * MUL) & M64) >> (64 - log2)


def keys_homed_at(slot, log2, count, start=1):
    """`count` distinct keys, none of them EMPTY, whose home in a table of 2^log2 slots is `slot`: the hash is key * MUL, so the
    keys are MUL^-1 times the values whose top bits are the slot"""
    out, low = [], start
    while len(out) < count:
        k = ((((slot << (64 - log2)) | low) & M64) * MUL_INV) & M64
        low += 1
        if k != EMPTY:
            out.append(k)
    return np.array(out, dtype=np.uint64)


# ---- a query's final join as an item ------------------------------------------------------------------------------------------------

def final_join_item(cols, query):
    """(keysR, keysS, terms) of the item the query's LAST predicate is when it joins two nodes: everything before it is
    executed as query_model.trace_query does; None when the query has no predicate or its last one is an equality inside a node.
    terms are (side, values) as join_sum takes them, one per view."""
    from query_model import _match
    rels, joins, filters, views = query
    if not joins:
        return None
    ids, node = {}, list(range(len(rels)))
    for b, r in enumerate(rels):
        keep = np.ones(len(cols[r][0]), dtype=bool)
        for a, c, op, v in filters:
            if a == b:
                x, v = cols[r][c], np.uint64(int(v) & M64)
                keep &= (x < v) if op == "<" else (x > v) if op == ">" else (x == v)
        ids[b] = np.flatnonzero(keep)
    for a, ca, b, cb in joins[:-1]:
        ka, kb = cols[rels[a]][ca][ids[a]], cols[rels[b]][cb][ids[b]]
        na, nb = node[a], node[b]
        if na == nb:
            keep = np.flatnonzero(ka == kb)
            for x in range(len(rels)):
                if node[x] == na:
                    ids[x] = ids[x][keep]
        else:
            ia, ib = _match(ka, kb)
            for x in range(len(rels)):
                if node[x] == na:
                    ids[x] = ids[x][ia]
                elif node[x] == nb:
                    ids[x] = ids[x][ib]
            node = [na if x == nb else x for x in node]
    a, ca, b, cb = joins[-1]
    if node[a] == node[b]:
        return None
    terms = [(1 if node[x] == node[b] else 0, cols[rels[x]][c][ids[x]]) for x, c in views]
    return cols[rels[a]][ca][ids[a]], cols[rels[b]][cb][ids[b]], terms
