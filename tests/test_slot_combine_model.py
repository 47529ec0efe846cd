"""tests/slot_combine_model.py, the restatement of the combiner's entry rule (csrc/rhj_slot_combine.hip.h), held to
hand-made tiles, and every shape of tests/slot_combine_shapes.py held to the regime it is named for: conditions asserted on the
CPU, so that the GPU test's exact counts never rest on a race."""
import numpy as np

import join_sum_model as jm
import slot_combine_model as cm
import slot_combine_shapes as cs


def test_the_constants():
    assert cm.ENTRIES & (cm.ENTRIES - 1) == 0 and cm.ENTRIES >= 64
    assert 1 <= cm.MIN_RIDERS <= cm.TILE
    # LDS of a workgroup: 4-byte tags, 8-byte sums and two counters stay at or below 32 KB
    assert cm.ENTRIES * (4 + 8) + 8 <= 32 * 1024
    assert cm.entry(cm.ENTRIES + 5) == 5 and cm.tag(cm.ENTRIES + 5) == 2 and cm.tag(5) == 1
    # entry and tag together are the slot, for every slot index the batches allow (below 2^33), in 32 bits
    top = (1 << 33) - 1
    assert cm.tag(top) < (1 << 32) and (cm.tag(top) - 1) * cm.ENTRIES + cm.entry(top) == top


def test_tiles_made_by_hand():
    one = [5] * cm.TILE
    assert cm.regime(one) == "entries distinct" and cm.riders(one) == cm.TILE - 1 and cm.combines(one)
    assert cm.fold_adds(one, [[1] * cm.TILE, [0] * cm.TILE, [1 << 63] * cm.TILE]) == (1, 1)      # 2048 x 2^63 wraps to 0: no add
    assert cm.count_adds(one + [5]) == (1, 2)                                  # a second tile of one row adds by itself
    distinct = list(range(cm.TILE))
    assert cm.regime(distinct) == "no duplicates in any tile" and not cm.combines(distinct)
    assert cm.fold_adds(distinct, [[3] * cm.TILE]) == (0, cm.TILE) and cm.count_adds(distinct) == (0, cm.TILE)
    clash = [7, 7 + cm.ENTRIES] * 100
    assert cm.regime(clash) == "two slots in one entry"
    # just below the threshold the tile adds per lane; a wave's round on one slot is then one add, a mixed one an add a row
    few = [9] * cm.MIN_RIDERS + [None] * (cm.TILE - cm.MIN_RIDERS)
    assert cm.riders(few) == cm.MIN_RIDERS - 1 and cm.fold_adds(few, [[1] * cm.TILE]) == (0, cm.MIN_RIDERS // 64)
    mixed = [9, 10] * (cm.MIN_RIDERS // 2)
    assert cm.riders(mixed) == cm.MIN_RIDERS - 2 and cm.fold_adds(mixed, [[1] * len(mixed)]) == (0, cm.MIN_RIDERS)
    assert cm.fold_adds(mixed + [9, 10], [[1] * (len(mixed) + 2)]) == (1, 2)
    assert cm.fold_adds([None] * 10, [[1] * 10]) == (0, 0)


def test_every_fold_shape_is_in_its_regime():
    shapes = cs.fold_shapes()
    assert {sh["regime"] for sh in shapes} == {"entries distinct", "two slots in one entry", "no duplicates in any tile"}
    for sh in shapes:
        log2, held = cs.table_keys(sh)
        homes = [jm.home(k, log2) for k in held]
        assert len(set(homes)) == len(homes), sh["name"]                     # so a key's slot is its home
        slots = cs.slots_of_S(sh)
        # (a tile of one row is in both of the first two regimes: the shape's name says which figure it is held to)
        assert cm.entries_distinct(slots) == (sh["regime"] != "two slots in one entry"), sh["name"]
        assert cm.no_duplicates(slots) or sh["regime"] != "no duplicates in any tile", sh["name"]
        assert cm.regime(slots) == sh["regime"] or len(slots) == 1, sh["name"]
        assert (sh["expect"] == "exact") == (sh["regime"] == "entries distinct"), sh["name"]
        assert all(len(w) == len(slots) for w in sh["weights"])


def test_the_tile_edges_combine_wherever_a_tile_has_riders():
    for sh in cs.tile_edge_shapes():
        slots = cs.slots_of_S(sh)
        nS, nv = len(slots), len(sh["weights"])
        combined, adds = cm.fold_adds(slots, [w.tolist() for w in sh["weights"]])
        tiles = cm.tiles(slots)
        assert combined == sum(len(t) > cm.MIN_RIDERS + 1 for t in tiles), sh["name"]
        # two adds a value and combining tile, one for a last tile of a single row
        assert adds == nv * sum(2 if len(t) > 1 else 1 for t in tiles), sh["name"]
        if nS > 1:
            assert adds * 16 <= nS * nv, sh["name"]


def test_the_mixes_and_the_conflict():
    by = {sh["name"]: sh for sh in cs.key_mix_shapes() + [cs.conflict_shape()]}
    sh = by["all distinct"]
    assert cm.fold_adds(cs.slots_of_S(sh), [w.tolist() for w in sh["weights"]]) == (0, 4096 * len(sh["weights"]))
    sh = by["2048 keys each twice"]
    assert cm.fold_adds(cs.slots_of_S(sh), [w.tolist() for w in sh["weights"]]) == (2, 2048 * len(sh["weights"]))
    sh = by["values that are 0"]
    assert cm.fold_adds(cs.slots_of_S(sh), [w.tolist() for w in sh["weights"]]) == (2, 2 * 3 * (len(sh["weights"]) - 1))
    sh = by["the empty key at a third of the rows"]
    assert sum(s is None for s in cs.slots_of_S(sh)) in (1365, 1366)
    sh = by["a third of S's keys absent from R"]
    assert sum(s is None for s in cs.slots_of_S(sh)) == 1365
    sh = by["S builds"]
    assert jm.build_side(len(sh["keysR"]), len(sh["colS"])) == 1
    sh = by["two hot slots in one entry"]
    slots = cs.slots_of_S(sh)
    a, b = sorted(set(slots) - {None})
    assert cm.entry(a) == cm.entry(b) and 1 << jm.table_log2(len(sh["keysR"]), len(slots)) >= 4 * cm.ENTRIES
    assert (slots.count(a), slots.count(b)) == (1500, 500) and all(s is None for s in slots[cm.TILE:])
    for at in range(0, 2000, 64):                                              # no wave's round is on one slot
        assert len(set(slots[at:at + 64]) - {None}) == 2


def test_the_join_sum_shapes():
    for name, kR, kS in cs.join_sum_shapes():
        log2 = jm.table_log2(len(kR), len(kS))
        assert jm.build_side(len(kR), len(kS)) == 0
        held = sorted(set(kR.tolist()))
        assert len({jm.home(k, log2) for k in held}) == len(held), name
        for keys in (kR, kS):
            slots = cm.homes(keys, log2)
            assert cm.regime(slots) == "entries distinct", name
            combined, adds = cm.count_adds(slots)
            assert combined == len(keys) // cm.TILE and adds == combined * len(held) + 1, name
