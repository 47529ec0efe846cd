"""The shapes tests/test_gpu_fold_combine.py runs and tests/test_slot_combine_model.py holds to the regime each is named for
(DESIGN.md 4.21).  A fold shape on one key is a dict: name, keysR, colS and selS (S's keys are colS[selS], or colS), weights (one
u64 array over S's positions per value), regime (slot_combine_model.regime's name for S's slots), and expect:
    "exact"   the entries are distinct: slot_adds and combined_tiles are the model's figures
    "bails"   no tile has a duplicate: combined_tiles 0, slot_adds nS x nvalues
    "bounds"  two hot slots share an entry: the winner is a race, the answers are not
Every key set in a table has homes of its own, so a key's slot is its home and the model needs no probing."""
import numpy as np

import join_sum_model as jm
import slot_combine_model as cm

M64 = (1 << 64) - 1
TILE_EDGES = (1, 255, 256, 2047, 2048, 2049, 2 * 2048 + 1)


def u64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64))


def weights(rng, n, nvalues):
    """values up to 2^64 - 1, odd: no row's value is 0 and the sums wrap"""
    return [u64(rng.integers(0, 1 << 63, size=n, dtype=np.uint64)) * np.uint64(2) + np.uint64(1) for _ in range(nvalues)]


def shape(name, keysR, keysS, w, regime, expect, selS=None, colS=None):
    return {"name": name, "keysR": u64(keysR), "colS": u64(keysS if colS is None else colS), "selS": None if selS is None else u64(selS),
            "weights": w, "regime": regime, "expect": expect}


def keys_of_S(sh):
    return sh["colS"] if sh["selS"] is None else sh["colS"][sh["selS"].astype(np.int64)]


def table_keys(sh):
    """(log2 of the table's slots, the distinct keys in it): the build side's, without the empty key"""
    kS = keys_of_S(sh)
    nR, nS = len(sh["keysR"]), len(kS)
    build = kS if jm.build_side(nR, nS) else sh["keysR"]
    return jm.table_log2(nR, nS), sorted({int(k) for k in build.tolist()} - {jm.EMPTY})


def slots_of_S(sh):
    """the slot of every row of S (None: not in the table), given that the table's keys have homes of their own"""
    log2, held = table_keys(sh)
    held = set(held)
    return [jm.home(k, log2) if k in held else None for k in keys_of_S(sh).tolist()]


def tile_edge_shapes():
    """2 keys interleaved row by row, the build side R's two rows, 1 value and 9 values"""
    rng = np.random.default_rng(421)
    a, b = cm.distinct_home_keys(2, jm.log2_slots(2))
    out = []
    for nS in TILE_EDGES:
        for nv in (1, 9):
            out.append(shape("%d rows on 2 keys, %d values" % (nS, nv), [a, b], u64([a, b])[np.arange(nS) % 2], weights(rng, nS, nv),
                             "entries distinct", "exact"))
    return out


def key_mix_shapes(nS=4096, nv=3):
    rng = np.random.default_rng(422)
    i = np.arange(nS)
    out = []

    def interleaved(count):
        keys = u64(cm.distinct_home_keys(count, jm.log2_slots(count)))
        return keys, keys[i % count]
    for count in (1, 3, 64):
        kR, kS = interleaved(count)
        out.append(shape("%d keys" % count, kR, kS, weights(rng, nS, nv), "entries distinct", "exact"))
    # 2048 keys each twice: a tile holds 1024 of them, each twice
    keys = u64(cm.distinct_home_keys(2048, jm.log2_slots(2048)))
    out.append(shape("2048 keys each twice", keys, keys[(i // cm.TILE) * 1024 + i % 1024], weights(rng, nS, nv), "entries distinct", "exact"))
    keys = u64(cm.distinct_home_keys(nS, jm.log2_slots(nS)))
    out.append(shape("all distinct", keys, keys, weights(rng, nS, nv), "no duplicates in any tile", "bails"))
    kR, kS = interleaved(3)
    kS = kS.copy()
    kS[i % 3 == 1] = jm.EMPTY
    out.append(shape("the empty key at a third of the rows", np.concatenate([kR, u64([jm.EMPTY])]), kS, weights(rng, nS, nv), "entries distinct", "exact"))
    # a third of S's rows carry keys R does not hold (R builds: they find no slot)
    held = u64(cm.distinct_home_keys(3, jm.log2_slots(3)))
    absent = jm.keys_homed_at(5, 20, 7, start=900)
    assert not set(absent.tolist()) & set(held.tolist())
    out.append(shape("a third of S's keys absent from R", held, np.where(i % 3 == 2, absent[i % 7], held[i % 3]), weights(rng, nS, nv), "entries distinct", "exact"))
    kR, kS = interleaved(3)
    w = weights(rng, nS, nv)
    w[0] = u64(np.zeros(nS))                                                  # a value that is 0 everywhere: no add at all
    w[1] = w[1] * u64(i % 4 != 0)                                             # and one that is 0 in a quarter of the rows
    out.append(shape("values that are 0", kR, kS, w, "entries distinct", "exact"))
    out.append(shape("no value", kR, kS, [], "entries distinct", "exact"))
    col = u64(rng.integers(1, 1 << 40, size=3 * nS))
    sel = u64(rng.permutation(3 * nS)[:nS])
    kR, kS = interleaved(64)
    col[sel.astype(np.int64)] = kS
    out.append(shape("d_selS given", kR, kS, weights(rng, nS, nv), "entries distinct", "exact", selS=sel, colS=col))
    # S builds: nS < nR, the add launch claims.  S's 64 keys have homes of their own in the table of S's rows; R holds them and others
    keys = u64(cm.distinct_home_keys(64, jm.log2_slots(nS), first=3, step=5))
    others = jm.keys_homed_at(9, 20, 40, start=77)
    out.append(shape("S builds", np.concatenate([keys, others, keys])[np.arange(nS + 904) % 168], keys[i % 64], weights(rng, nS, nv), "entries distinct", "exact"))
    return out


def conflict_shape(nv=3):
    """a table of 4 x COMBINE_ENTRIES slots whose two keys' slots differ by 2 x COMBINE_ENTRIES: one entry.  One tile of S holds 1500
    rows of the one and 500 of the other, three and one by turns, so that no wave's round is on one slot; the rest of S is the empty key"""
    rng = np.random.default_rng(423)
    nR = 2 * cm.ENTRIES
    log2 = jm.log2_slots(nR)
    assert 1 << log2 == 4 * cm.ENTRIES
    a = int(jm.keys_homed_at(7, log2, 1)[0])
    b = int(jm.keys_homed_at(7 + 2 * cm.ENTRIES, log2, 1, start=2)[0])
    i = np.arange(nR)
    kS = u64([a, b, jm.EMPTY])[np.where(i >= 2000, 2, i % 4 == 3)]
    return shape("two hot slots in one entry", u64([a, b])[(i == 1).astype(np.int64)], kS, weights(rng, nR, nv), "two slots in one entry", "bounds")


def sharing_shapes(count=64, nv=2):
    """one-tile items with key sets of their own, for one call"""
    rng = np.random.default_rng(424)
    out = []
    for j in range(count):
        nk = 2 + j % 3
        keys = u64(cm.distinct_home_keys(nk, jm.log2_slots(nk), start=1 + 10 * j))
        keys = keys if j % 2 == 0 else keys[::-1].copy()
        out.append(shape("item %d of a launch" % j, keys, keys[(np.arange(cm.TILE) + j) % nk], weights(rng, cm.TILE, nv), "entries distinct", "exact"))
    return out


def fold_shapes():
    return tile_edge_shapes() + key_mix_shapes() + [conflict_shape()] + sharing_shapes()


def join_sum_shapes():
    """(name, keysR, keysS): 1 key and 2 keys at 2049 and 4097 rows a side (R builds on the tie)"""
    out = []
    for n in (2049, 4097):
        for nk in (1, 2):
            log2 = jm.log2_slots(n)
            keys = u64(cm.distinct_home_keys(nk, log2, first=11, step=2048 + 17))
            i = np.arange(n)
            out.append(("%d keys at %d rows a side" % (nk, n), keys[i % nk], keys[(i + 1) % nk]))
    return out
