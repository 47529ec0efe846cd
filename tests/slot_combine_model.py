"""The entry rule of csrc/rhj_slot_combine.hip.h restated without the library, with its constants read out of the
source: which LDS entry a table slot takes, which rows of a 2048-row tile own, ride or bypass, whether the tile combines, and how
many device-scope adds into table slots an add launch then issues (rhj_table_batch_last_combine_info's slot_adds).

The figures are exact where the outcome is no race: every distinct slot of a tile has an entry of its own ("entries distinct").
Where two slots of a tile share an entry the first compare-and-swap wins it and the other slot's rows bypass; the model then
gives the bounds.  A side is a list of slots, one a row, None for a row without a slot in the table (the empty key, a key the
table does not hold).  For a key set whose homes are all distinct no probe sequence moves on, so a key's slot is its home
(join_sum_model.home, join_foldk_model.home)."""
import os

from source_constants import c_int, one

import join_sum_model as jm

HEADER = os.path.join(jm.ROOT, "sigmod-2018_amd", "csrc", "rhj_slot_combine.hip.h")
M64 = (1 << 64) - 1
WAVE, THREADS = 64, 256


def parse_constants():
    with open(HEADER) as f:
        text = f.read()
    who = "tests/slot_combine_model.py"
    names = {}
    for name in ("COMBINE_ROWS", "COMBINE_LOG2_ENTRIES", "COMBINE_ENTRIES", "COMBINE_MIN_RIDERS"):
        m = one(r"constexpr\s+(?:int|uint32_t)\s+%s\s*=\s*([^;]+);" % name, text, name, who)
        names[name] = c_int(m.group(1), names)
    # the rules restated below, as the code words them: a change there must be looked at here
    for pat, what in ((r"return \(uint32_t\)slot & \(COMBINE_ENTRIES - 1\);", "a slot's entry"),
                      (r"\(uint32_t\)\(slot\[k\] >> COMBINE_LOG2_ENTRIES\) \+ 1u;", "a slot's tag"),
                      (r"role = seen == mine \? COMBINE_RIDER : COMBINE_BYPASS;", "the roles"),
                      (r"return L\.riders >= COMBINE_MIN_RIDERS;", "the bail-out")):
        one(pat, text, what, who)
    return names


K = parse_constants()
ENTRIES, LOG2_ENTRIES, MIN_RIDERS, TILE = K["COMBINE_ENTRIES"], K["COMBINE_LOG2_ENTRIES"], K["COMBINE_MIN_RIDERS"], jm.TILE
assert ENTRIES == 1 << LOG2_ENTRIES and K["COMBINE_ROWS"] * THREADS == TILE


def entry(slot):
    return slot & (ENTRIES - 1)


def tag(slot):
    return (slot >> LOG2_ENTRIES) + 1


def tiles(rows):
    """the 2048-row tiles of a side"""
    return [rows[a:a + TILE] for a in range(0, len(rows), TILE)]


def tile_slots(tile):
    """the distinct slots of a tile's rows"""
    return sorted({s for s in tile if s is not None})


def entries_distinct(slots):
    """whether, in every tile, every distinct slot has an entry of its own: no bypass, no race"""
    return all(len({entry(s) for s in tile_slots(t)}) == len(tile_slots(t)) for t in tiles(slots))


def no_duplicates(slots):
    """whether no tile has two rows of one slot: no rider anywhere"""
    return all(len(tile_slots(t)) == sum(s is not None for s in t) for t in tiles(slots))


def regime(slots):
    """the regime a shape is named for"""
    if not entries_distinct(slots):
        return "two slots in one entry"
    return "no duplicates in any tile" if no_duplicates(slots) else "entries distinct"


def riders(tile):
    """a tile's riders where its entries are distinct: the rows with a slot beyond the first of each slot"""
    assert entries_distinct(tile)
    return sum(s is not None for s in tile) - len(tile_slots(tile))


def combines(tile):
    return riders(tile) >= MIN_RIDERS


def _plain_adds(tile, v):
    """the adds of a tile that adds per lane, for one value: one a row with a slot and a non-zero value; but where all the rows
    of a wave's round that have a slot (two or more) have the same one, one add of their non-zero sum.  A wave's round is 64
    consecutive rows: thread t has rows t, t + 256, ..."""
    adds = 0
    for a in range(0, len(tile), WAVE):
        rows = [(s, x) for s, x in zip(tile[a:a + WAVE], v[a:a + WAVE]) if s is not None]
        if len(rows) >= 2 and len({s for s, _ in rows}) == 1:
            adds += (sum(x for _, x in rows) & M64) != 0
        else:
            adds += sum(1 for _, x in rows if x != 0)
    return adds


def fold_adds(slots, values):
    """(combined tiles, slot adds) of a fold's add launch over a side whose entries are distinct: values[c][j] the value c of row j
    as Python integers.  A combining tile issues one add per distinct slot whose rows' values sum to non-zero modulo 2^64."""
    assert entries_distinct(slots)
    combined = adds = 0
    for t, tile in enumerate(tiles(slots)):
        vals = [v[t * TILE:t * TILE + len(tile)] for v in values]
        if combines(tile):
            combined += 1
            for v in vals:
                sums = {}
                for s, x in zip(tile, v):
                    if s is not None:
                        sums[s] = (sums.get(s, 0) + x) & M64
                adds += sum(1 for x in sums.values() if x)
        else:
            adds += sum(_plain_adds(tile, v) for v in vals)
    return combined, adds


def count_adds(slots):
    """(combined tiles, slot adds) of one count launch of the join sums over a side whose entries are distinct: one add a distinct
    slot in a combining tile, one a row with a slot in any other"""
    assert entries_distinct(slots)
    combined = adds = 0
    for tile in tiles(slots):
        if combines(tile):
            combined += 1
            adds += len(tile_slots(tile))
        else:
            adds += sum(s is not None for s in tile)
    return combined, adds


def homes(keys, log2):
    """the slots of a side's keys in a table of 2^log2 slots when the table's keys all have homes of their own; jm.EMPTY has none"""
    return [None if int(k) == jm.EMPTY else jm.home(k, log2) for k in keys]


def distinct_home_keys(count, log2, first=0, step=1, start=1):
    """`count` keys with the homes first, first + step, ... in a table of 2^log2 slots: distinct homes, so slot = home (`start`
    chooses among the keys of a home)"""
    assert first + step * (count - 1) < (1 << log2)
    return [int(jm.keys_homed_at(first + step * k, log2, 1, start=start + k)[0]) for k in range(count)]
