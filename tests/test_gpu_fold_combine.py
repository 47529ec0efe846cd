"""rhj_set_fold_combine (include/rhj_inter.h, csrc/rhj_slot_combine.hip.h): the add launches of the four table
batches combine a tile's adds to one slot in LDS.  Every shape of tests/slot_combine_shapes.py runs under both settings of the
switch, which the tests set themselves: every output vector and total is compared bit for bit between the two and with the numpy
models, and rhj_table_batch_last_combine_info with the figures of tests/slot_combine_model.py, exact wherever the shape's entries
are distinct (asserted on the CPU by tests/test_slot_combine_model.py)."""
import importlib

import numpy as np
import pytest

import fold_exact as fe
import join_fold_model as fm
import join_foldk_model as km
import join_foldn_model as nm
import join_sum_model as jm
import slot_combine_model as cm
import slot_combine_shapes as cs

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
ONES = (None, None, None)
ZERO = {"tiles": 0, "combined_tiles": 0, "slot_adds": 0}
EDGES = {sh["name"]: sh for sh in cs.tile_edge_shapes()}
MIXES = {sh["name"]: sh for sh in cs.key_mix_shapes()}


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def rhj(mod):
    r = mod.RHJ(device=0)
    was = r.lib.rhj_get_fold_combine()
    r.lib.rhj_set_timing(0)
    r.set_bits(4)
    yield r
    r.set_fold_combine(was)
    r.lib.rhj_set_timing(2)


def dev(rhj, a):
    return None if a is None else rhj.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


def host(t):
    return t.cpu().numpy().view(np.uint64)


def both(rhj, call):
    """call() under the switch off and on: [(its result, the combine info)] in that order"""
    out = []
    for on in (False, True):
        rhj.set_fold_combine(on)
        res = call()
        out.append((res, rhj.table_batch_last_combine_info()))
    return out


def fold_parts(sh):
    """(values, outs) of a shape as the model takes them: every weight vector a value, every value an output with a vector, the
    last one under an odd weight over R (a bijection of the u64 values, so it hides no difference)"""
    values = [(w, None, None) for w in sh["weights"]]
    outs = [(c, ONES) for c in range(len(values))]
    if values:
        outs[-1] = (len(values) - 1, ((sh["keysR"] * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1), None, None))
    return values, outs


def fold_args(rhj, sh):
    values, outs = fold_parts(sh)
    return (dev(rhj, sh["keysR"]), None, dev(rhj, sh["colS"]), dev(rhj, sh["selS"]), [(dev(rhj, w), None, None) for w, _, _ in values],
            [(c, (dev(rhj, p[0]), None, None), True) for c, p in outs])


def fold_answers(res):
    """[(vector as a numpy array, total)] per output of every item"""
    return [[(host(vec), total) for vec, total in item] for item in res]


def same_answers(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(t == u and (v == w).all() for (v, t), (w, u) in zip(x, y)) for x, y in zip(a, b))


def fold_model(sh):
    values, outs = fold_parts(sh)
    return [(np.asarray(vec, dtype=np.uint64), total) for vec, total in fm.fold_item_np(sh["keysR"], cs.keys_of_S(sh), values, outs)]


def run_folds(rhj, shapes):
    """the shapes as one rhj_join_fold_batch_device call under both settings; the answers checked between the two and with the
    model; returns the info with the switch on"""
    args = [fold_args(rhj, sh) for sh in shapes]
    (off, info_off), (on, info_on) = both(rhj, lambda: fold_answers(rhj.join_fold_batch_device(args)))
    assert same_answers(off, on)
    assert same_answers(on, [fold_model(sh) for sh in shapes])
    assert info_off == ZERO
    return info_on


def model_info(shapes):
    tiles = combined = adds = 0
    for sh in shapes:
        slots = cs.slots_of_S(sh)
        c, a = cm.fold_adds(slots, [w.tolist() for w in sh["weights"]])
        tiles, combined, adds = tiles + len(cm.tiles(slots)), combined + c, adds + a
    return {"tiles": tiles, "combined_tiles": combined, "slot_adds": adds}


@pytest.mark.parametrize("name", list(EDGES))
def test_tile_edges(rhj, name):
    sh = EDGES[name]
    info = run_folds(rhj, [sh])
    nS, nv = len(sh["colS"]), len(sh["weights"])
    print(name, info)
    assert info == model_info([sh])
    if nS > 1:                                            # (a single row has nobody to combine with: its one add a value stays)
        assert info["slot_adds"] * 16 <= nS * nv
    else:
        assert info["slot_adds"] == nv


@pytest.mark.parametrize("name", list(MIXES))
def test_key_mixes(rhj, name):
    sh = MIXES[name]
    info = run_folds(rhj, [sh])
    nS, nv = len(cs.keys_of_S(sh)), len(sh["weights"])
    print(name, info)
    assert info == model_info([sh])
    if sh["expect"] == "bails":
        assert info["combined_tiles"] == 0 and info["slot_adds"] == nS * nv
    else:
        assert info["combined_tiles"] == info["tiles"] == 2
        assert nv == 0 or info["slot_adds"] < nS * nv


def test_two_hot_slots_in_one_entry(rhj):
    """the entry goes to whichever slot's row comes first; the other slot's rows add by themselves.  The answers do not depend on it."""
    sh = cs.conflict_shape()
    info = run_folds(rhj, [sh])
    nv = len(sh["weights"])
    print(info)
    assert info["tiles"] == 2 and info["combined_tiles"] == 1 and info["slot_adds"] % nv == 0
    assert 1 + 500 <= info["slot_adds"] // nv <= 1 + 1500


def test_items_sharing_a_launch(rhj):
    shapes = cs.sharing_shapes()
    assert len(shapes) == 64 and all(len(sh["colS"]) == cm.TILE for sh in shapes)
    info = run_folds(rhj, shapes)
    assert info == model_info(shapes) and info["combined_tiles"] == 64
    assert info["slot_adds"] == sum(len(set(sh["keysR"].tolist())) * len(sh["weights"]) for sh in shapes)


def tuple_shape():
    """4097 rows on two hot tuples that differ in their second word alone, R's two rows the table"""
    rng = np.random.default_rng(425)
    log2 = jm.log2_slots(2)
    second = [x for x in range(1, 40) if km.home((7, x), log2) != km.home((7, 1), log2)][0]
    tuples = [(7, 1), (7, second)]
    i = np.arange(4097)
    kR = [cs.u64([7, 7]), cs.u64([1, second])]
    kS = [cs.u64(np.full(4097, 7)), cs.u64(np.where(i % 2 == 0, 1, second))]
    slots = [km.home(tuples[k % 2], log2) for k in range(4097)]
    assert cm.regime(slots) == "entries distinct"
    return kR, kS, cs.weights(rng, 4097, 2), slots


def tuple_checks(rhj, call, want, slots, w):
    (off, info_off), (on, info_on) = both(rhj, lambda: fold_answers(call()))
    assert same_answers(off, on) and same_answers(on, [[(np.asarray(v, dtype=np.uint64), t) for v, t in want]])
    combined, adds = cm.fold_adds(slots, [x.tolist() for x in w])
    assert info_off == ZERO and info_on == {"tiles": 3, "combined_tiles": combined, "slot_adds": adds}
    assert combined == 2 and adds == 2 * (2 * 2 + 1)


def test_tuple_keys(rhj):
    kR, kS, w, slots = tuple_shape()
    values = [(x, None, None) for x in w]
    outs = [(0, ONES), (1, ONES)]
    item = ([dev(rhj, c) for c in kR], None, [dev(rhj, c) for c in kS], None, [(dev(rhj, x), None, None) for x in w], [(c, ONES, True) for c, _ in outs])
    tuple_checks(rhj, lambda: rhj.join_foldk_batch_device([item]), km.foldk_item_np(kR, kS, values, outs), slots, w)


def test_tuple_keys_with_a_vector_a_word(rhj):
    kR, kS, w, slots = tuple_shape()
    rng = np.random.default_rng(426)
    values = [(x, None, None) for x in w]
    outs = [(0, ONES), (1, ONES)]
    # S's words through a permutation each, R's second word through a vector: col[t][sel[t][p]] is the shape's word
    sels = [cs.u64(rng.permutation(4097)) for _ in range(2)]
    cols = []
    for word, sel in zip(kS, sels):
        col = np.zeros(4097, dtype=np.uint64)
        col[sel.astype(np.int64)] = word
        cols.append(col)
    R = (kR[:1] + [kR[1][::-1].copy()], [None, cs.u64([1, 0])], 2)
    S = (cols, sels, 4097)
    assert all((a == b).all() for a, b in zip(nm.words(*S), kS)) and all((a == b).all() for a, b in zip(nm.words(*R), kR))
    item = ([dev(rhj, c) for c in R[0]], [dev(rhj, s) for s in R[1]], [dev(rhj, c) for c in S[0]], [dev(rhj, s) for s in S[1]],
            [(dev(rhj, x), None, None) for x in w], [(c, ONES, True) for c, _ in outs])
    tuple_checks(rhj, lambda: rhj.join_foldn_batch_device([item]), nm.foldn_item_np(R, S, values, outs), slots, w)


def test_join_sums(rhj):
    rng = np.random.default_rng(427)
    shapes = cs.join_sum_shapes()
    items, want, model = [], [], dict(ZERO)
    for name, kR, kS in shapes:
        tR, tS = cs.weights(rng, len(kR), 1)[0], cs.weights(rng, len(kS), 1)[0]
        items.append((dev(rhj, kR), None, dev(rhj, kS), None, [(0, None, dev(rhj, tR)), (1, None, dev(rhj, tS))]))
        want.append(jm.join_sum(kR, kS, [(0, tR), (1, tS)]))
        log2 = jm.table_log2(len(kR), len(kS))
        for keys in (kR, kS):                             # the insert launch over R, which builds, and the count launch over S
            slots = cm.homes(keys, log2)
            c, a = cm.count_adds(slots)
            model = {"tiles": model["tiles"] + len(cm.tiles(slots)), "combined_tiles": model["combined_tiles"] + c, "slot_adds": model["slot_adds"] + a}
    for k in range(len(items)):                           # each item alone, then all in one call
        (off, info_off), (on, info_on) = both(rhj, lambda: [(m, list(s)) for m, s in rhj.join_sum_batch_device(items[k:k + 1])])
        assert off == on == [(want[k][0], list(want[k][1]))], shapes[k][0]
        assert info_off == ZERO and info_on["combined_tiles"] == 2 * (len(shapes[k][1]) // cm.TILE)
    (off, info_off), (on, info_on) = both(rhj, lambda: [(m, list(s)) for m, s in rhj.join_sum_batch_device(items)])
    assert off == on == [(m, list(s)) for m, s in want]
    assert info_off == ZERO and info_on == model
    assert info_on["slot_adds"] * 16 <= sum(len(kR) + len(kS) for _, kR, kS in shapes)


def fold_switches(rhj, on, one_wait=False):
    rhj.set_query_fold(on)
    rhj.set_query_fold_keys(on)
    rhj.set_query_fold_self(on)
    rhj.set_query_fold_nodes(on)
    rhj.set_query_fold_one_wait(on and one_wait)
    rhj.set_query_fold_one_wait_rows(65536 if on and one_wait else 4096)


@pytest.mark.parametrize("one_wait", (False, True))
def test_a_query_batch_on_the_fold_route(rhj, one_wait):
    """a star of two bindings: 5000 rows on 3 distinct join values against a 3-row binding, two views, in both binding orders, so
    that one of the two folds the large binding into the small one"""
    rng = np.random.default_rng(428)
    keys = cs.u64([11, 22, 33])
    small = [keys, cs.u64(rng.integers(0, 1 << 64, size=3, dtype=np.uint64))]
    big = [keys[rng.integers(0, 3, size=5000)], cs.u64(rng.integers(0, 1 << 64, size=5000, dtype=np.uint64))]
    relations = [small, big]
    queries = [([0, 1], [(0, 0, 1, 0)], [], [(1, 1), (0, 1)]), ([1, 0], [(0, 0, 1, 0)], [], [(0, 1), (1, 1)])]
    want = [fe.modulo(fe.exact_tree(relations, q)) for q in queries]
    assert want[0][1] == want[1][1] == 5000
    cols = [[dev(rhj, c) for c in rel] for rel in relations]
    fold_switches(rhj, True, one_wait)
    try:
        (off, info_off), (on, info_on) = both(rhj, lambda: [(list(s), r) for s, r in rhj.query_batch_device(cols, queries)])
    finally:
        fold_switches(rhj, False)
    assert off == on == [(list(s), r) for s, r in want]
    assert info_off == ZERO
    assert info_on["combined_tiles"] > 0 and info_on["tiles"] >= 3 and 0 < info_on["slot_adds"] < 5000
