"""The resident form of rhj_join_foldk_batch_device and rhj_join_foldn_batch_device (include/rhj_inter.h,
csrc/rhj_fold_keys_lds.hip.h) restated without the library: resident(nR, nS, nvalues), which items one workgroup folds in LDS
while rhj_set_fold_resident_keys is on, with the constants read from the sources; path(), what such an item reports; and the
edges of the rule as a list of sizes.  The number of key columns does not enter: a slot holds an owner, not a key."""
import os

import join_sum_model as jm
from source_constants import c_int, one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "sigmod-2018_amd", "csrc", "rhj_fold_keys_lds.hip.h")
WORDS_HEADER = os.path.join(ROOT, "sigmod-2018_amd", "csrc", "rhj_fold_lds.hip.h")
WHO = "tests/fold_resident_keys_model.py"
MAX_VALUES = 9
PATH_FOLDK, PATH_FOLDN, PATH_RESIDENT = 14, 16, 19


def parse_constants():
    names = {"JSUM_SLOTS_PER_ROW": jm.K["JSUM_SLOTS_PER_ROW"], "JSUM_TILE": jm.K["JSUM_TILE"]}
    with open(WORDS_HEADER) as f:
        text = f.read()
    names["FOLD_LDS_WORDS"] = c_int(one(r"constexpr uint64_t FOLD_LDS_WORDS = ([^;]+);", text, "FOLD_LDS_WORDS", WHO).group(1), names)
    with open(HEADER) as f:
        text = f.read()
    names["FOLDK_LDS_MAX_ROWS"] = c_int(one(r"constexpr uint64_t FOLDK_LDS_MAX_ROWS = ([^;]+);", text, "FOLDK_LDS_MAX_ROWS", WHO).group(1), names)
    # the rule restated below, as the code words it: a change there must be looked at here
    for pat, what in ((r"constexpr int fold_keys_resident_rule\(uint64_t nR, uint64_t nS, int nvalues\)", "the rule's arguments: no nkeys"),
                      (r"if \(nR == 0 \|\| nS == 0 \|\| nvalues < 0 \|\| nvalues > RHJ_FOLD_MAX_VALUES\) return 0;", "both sides have rows, 0..9 values"),
                      (r"const int build = jsum_build_side\(nR, nS\);", "the build side"),
                      (r"return jsum_slots\(nb\) \* \(uint64_t\)\(1 \+ nvalues\) <= FOLD_LDS_WORDS && no <= FOLDK_LDS_MAX_ROWS;", "the two limits")):
        one(pat, text, what, WHO)
    return names


K = parse_constants()
WORDS, MAX_ROWS, TILE = K["FOLD_LDS_WORDS"], K["FOLDK_LDS_MAX_ROWS"], K["JSUM_TILE"]


def slots(rows):
    return 1 << jm.log2_slots(rows)


def resident(nR, nS, nvalues):
    """whether an item of these sizes runs resident while the switch is on"""
    if nR == 0 or nS == 0 or not 0 <= nvalues <= MAX_VALUES:
        return False
    build, other = (nS, nR) if jm.build_side(nR, nS) else (nR, nS)
    return slots(build) * (1 + nvalues) <= WORDS and other <= MAX_ROWS


def path(nR, nS, nvalues, on=True, table=PATH_FOLDK):
    """what the item reports: 0 with an empty side, 19 resident, else the table form's 14 (foldk) or 16 (foldn)"""
    if nR == 0 or nS == 0:
        return 0
    return PATH_RESIDENT if on and resident(nR, nS, nvalues) else table


def build_cap(nvalues):
    """the most rows of a build side whose table of 1 + nvalues words a slot fits: the slots are a power of two"""
    s = 2
    while 2 * s * (1 + nvalues) <= WORDS:
        s *= 2
    return s // K["JSUM_SLOTS_PER_ROW"]


def edges():
    """(nR, nS, nvalues) at every edge of the rule"""
    out = []
    for v in (0, 1, 3, 9):
        cap = build_cap(v)
        for rows in (cap, cap + 1):
            out += [(rows, rows, v), (rows, rows + 1, v), (rows + 1, rows, v), (rows, MAX_ROWS, v), (MAX_ROWS, rows, v)]
        out += [(cap, MAX_ROWS + 1, v), (MAX_ROWS + 1, cap, v), (1, MAX_ROWS, v), (1, MAX_ROWS + 1, v), (MAX_ROWS + 1, 1, v)]
        out += [(0, 5, v), (5, 0, v), (0, 0, v), (1, 1, v)]
    return out
