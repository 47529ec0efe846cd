"""rhj_fold_pred_batch_device (include/rhj_inter.h) on the GPU: ONE scrambled batch of 4100 items, 4099 of them with rows, so that a
chunk is cut after the 4096th launched item and three items with written outputs and guard words make up the second chunk.  The
sides have every size at which the kernel's tiles, waves and rounds change; every operator stands alone against 0 and 2^64 - 1
over a column with values at and above 2^63; 0..4 constant terms are crossed with 0..4 equalities, direct and through row-id
vectors; 0..9 outputs in every form of the factor, written and not, with guard words between and behind all output vectors; items
whose every row is masked; an item without rows in the middle.  Every output word, every guard word and every total is compared
with tests/fold_pred_model.py; every comparison is an integer equality."""
import importlib

import numpy as np
import pytest

import fold_pred_model as pm
import join_folds_model as sm

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
B63 = 1 << 63
GUARD = 0xA5A5A5A5A5A5A5A5
SIZES = (1, 255, 256, 257, 2047, 2048, 2049, 4097)
L = 4200                                                 # rows of every shared column and vector
ITEMS = 4100                                             # 4099 with rows: one chunk of 4096 and one of 3
TAIL = 3                                                 # the items placed behind the scrambled ones: the second chunk


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def rhj(mod):
    r = mod.RHJ(device=0)
    r.lib.rhj_set_timing(2)
    yield r
    r.lib.rhj_set_timing(2)


def dev(rhj, a):
    return rhj.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(rhj.dev)


def build_pool():
    """name -> u64 host array: `big` over values on both sides of 2^63, key columns of a few values, row-id vectors, weights"""
    rng = np.random.default_rng(20191)
    pool = {"big": rng.choice(np.array([0, 1, 7, B63 - 1, B63, B63 + 1, M64 - 1, M64], dtype=np.uint64), size=L)}
    for k in range(4):
        pool["k%d" % k] = rng.integers(0, 2 + k % 3, size=L).astype(np.uint64)
    for k in range(3):
        pool["v%d" % k] = rng.integers(0, L, size=L).astype(np.uint64)
    pool["ramp"] = np.arange(L, dtype=np.uint64) + np.uint64(B63)          # row i holds 2^63 + i: a threshold picks a prefix or a suffix
    pool["w"] = rng.integers(0, 1 << 63, size=L).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    return pool


FACTORS = ((None, None, None), ("w", None, None), (None, None, "big"), (None, "v1", "big"), ("w", "v2", "big"), ("w", None, "big"), ("big", "v0", "k0"))
OPS = "<>="


def build_items():
    """[(n, consts, eqs, outs)]: a constant term is (column, vector, op, value), an equality four names of the pool (a vector may
    be None), an output (factor of names, whether it is written)."""
    rng = np.random.default_rng(20192)
    some_outs = lambda k: [(FACTORS[(k + o) % len(FACTORS)], (k + o) % 3 != 1) for o in range(k % 10)]
    consts_of = lambda nc, k, vec: [("big" if (k + c) % 2 else "k%d" % (c % 4), ("v%d" % ((k + c) % 3) if vec else None), OPS[(k + c) % 3],
                                     (0, 1, B63, M64, 2, B63 + 1)[(k + c) % 6]) for c in range(nc)]
    eqs_of = lambda ne, k, vec: [("k%d" % ((k + t) % 4), ("v%d" % (t % 3) if vec else None), "k%d" % ((k + t + 1) % 4), ("v%d" % ((t + 1) % 3) if vec == 2 else None))
                                 for t in range(ne)]
    items = []
    for s, n in enumerate(SIZES):
        # every operator alone against 0 and 2^64 - 1, direct and through a vector, one output written and the plain count
        for op in OPS:
            for value in (0, M64):
                for vec in (None, "v0"):
                    items.append((n, [("big", vec, op, value)], [], [(FACTORS[0], True), (FACTORS[4], False)]))
        # 0..4 constant terms x 0..4 equalities, direct (0), every column through a vector (1), two vectors an equality (2)
        for nc in range(5):
            for ne in range(5):
                k = s * 25 + nc * 5 + ne
                items.append((n, consts_of(nc, k, k % 3 != 0), eqs_of(ne, k, k % 3), some_outs(k + 1)))
        # the rows that pass: a prefix, a suffix, the last row alone, none at all (every output word written as 0)
        items.append((n, [("ramp", None, "<", B63 + n // 2)], [], [(FACTORS[1], True), (FACTORS[0], False)]))
        items.append((n, [("ramp", None, ">", B63 + n // 2)], [], [(FACTORS[1], True), (FACTORS[0], False)]))
        items.append((n, [("ramp", None, "=", B63 + n - 1)], [], [(FACTORS[0], True), (FACTORS[4], True)]))
        items.append((n, [("ramp", None, "<", B63)], [], [(FACTORS[0], True), (FACTORS[1], True), (FACTORS[3], False)]))
        items.append((n, [("ramp", None, ">", 0), ("ramp", None, "=", 5)], [("k0", None, "k0", None)], [(FACTORS[4], True)]))
        # nine outputs, all written; nine, none written
        items.append((n, [("big", "v2", ">", 7)], [("k0", "v2", "k1", None)], [(FACTORS[o % len(FACTORS)], True) for o in range(9)]))
        items.append((n, [("big", None, "<", M64)], [("k0", None, "k1", "v2")], [(FACTORS[o % len(FACTORS)], False) for o in range(9)]))
    k = 0
    while len(items) < ITEMS - 1 - TAIL:
        n = 1 + k % 5
        items.append((n, consts_of(k % 5, k, k % 2), eqs_of((k // 5) % 5, k, k % 3), some_outs(k)))
        k += 1
    order = rng.permutation(len(items))
    items = [items[i] for i in order]
    items.insert(ITEMS // 2, (0, [("big", "v0", "<", 9)], [("k0", "v0", "k1", None)], [(FACTORS[0], True), (FACTORS[1], True)]))      # no row: nothing launched, nothing written
    # the second chunk: its descriptors, tile starts and words begin anew, and its outputs are written and guarded like the others
    items.append((257, [("big", "v0", ">", B63)], [("k0", None, "k0", None)], [(FACTORS[4], True), (FACTORS[0], False), (FACTORS[3], True)]))
    items.append((2049, [("ramp", None, "=", B63 + 2048)], [], [(FACTORS[0], True), (FACTORS[6], True)]))
    items.append((3, [], [], [(FACTORS[o % len(FACTORS)], o % 2 == 0) for o in range(9)]))
    assert len(items) == ITEMS and sum(1 for x in items if x[0]) == ITEMS - 1 > 4096
    assert all(x[0] for x in items[4097:]) and sum(1 for x in items[:4097] if x[0]) == 4096      # the cut falls in front of the TAIL items
    return items


@pytest.fixture(scope="module")
def batch(rhj):
    pool = build_pool()
    on_dev = {k: dev(rhj, v) for k, v in pool.items()}
    items = build_items()
    h = lambda name: None if name is None else pool[name]
    d = lambda name: None if name is None else on_dev[name]
    words = sum(max(n, 1) + 1 for n, _, _, outs in items for _, written in outs if written) + 1
    guard = rhj.torch.full((words,), GUARD - (1 << 64), dtype=rhj.torch.int64, device=rhj.dev)
    want_words = np.full(words, GUARD, dtype=np.uint64)
    call, want_totals, at = [], [], 1
    for n, consts, eqs, outs in items:
        model = pm.pred_item_np(n, [(h(c), h(s), op, v) for c, s, op, v in consts], [tuple(h(x) for x in t) for t in eqs], [tuple(h(x) for x in f) for f, _ in outs])
        want_totals.append([t for _, t in model])
        mine = []
        for (f, written), (vecw, _) in zip(outs, model):
            if written:
                room = max(n, 1)                         # (the item without rows keeps a word that must stay as it was)
                mine.append((tuple(d(x) for x in f), guard[at:at + room]))
                want_words[at:at + n] = vecw
                at += room + 1
            else:
                mine.append((tuple(d(x) for x in f), None))
        call.append((n, [(d(c), d(s), op, v) for c, s, op, v in consts], [tuple(d(x) for x in t) for t in eqs], mine))
    assert at == words
    res, paths = rhj.fold_pred_batch_device(call, with_info=True)
    stats = rhj.stats()
    rhj.torch.cuda.synchronize()
    return {"items": items, "pool": pool, "dev": on_dev, "res": res, "paths": paths, "stats": stats,
            "words": guard.cpu().numpy().view(np.uint64), "want_words": want_words, "want_totals": want_totals}


def test_every_total(batch):
    got = [[t for _, t in item] for item in batch["res"]]
    for k, (g, w) in enumerate(zip(got, batch["want_totals"])):
        assert g == w, (k, batch["items"][k][:3])
    assert sum(1 for n, consts, eqs, _ in batch["items"] if n >= 255 and consts and eqs) >= 100


def test_every_output_word_and_every_guard_word(batch):
    assert np.array_equal(batch["words"], batch["want_words"])
    assert int((batch["want_words"] == np.uint64(GUARD)).sum()) >= sum(1 for _, _, _, outs in batch["items"] for _, w in outs if w)
    assert int((batch["want_words"] == 0).sum()) >= 4097  # masked rows are written as 0


def test_the_built_cases_are_what_they_say(batch):
    """(of the model: the rows that pass each built item)"""
    pool = batch["pool"]
    one = [(None, None, None)]
    count = lambda n, consts: pm.pred_item_np(n, consts, [], one)[0]
    for n in SIZES:
        assert count(n, [(pool["ramp"], None, "<", B63 + n // 2)])[1] == n // 2
        assert count(n, [(pool["ramp"], None, ">", B63 + n // 2)])[1] == n - 1 - n // 2
        assert count(n, [(pool["ramp"], None, "=", B63 + n - 1)])[0].tolist() == [0] * (n - 1) + [1]
        assert count(n, [(pool["ramp"], None, "<", B63)])[1] == 0 == count(n, [(pool["ramp"], None, ">", 0), (pool["ramp"], None, "=", 5)])[1]
        # nothing is below 0, nothing above 2^64 - 1; a signed comparison would differ on `big`
        assert count(n, [(pool["big"], None, "<", 0)])[1] == 0 == count(n, [(pool["big"], None, ">", M64)])[1]
    big = pool["big"][:4097]
    assert count(4097, [(pool["big"], None, ">", B63 - 1)])[1] == int((big >= np.uint64(B63)).sum()) > 1000
    assert int((big.view(np.int64) > np.int64(B63 - 1)).sum()) == 0


def test_paths_and_statistics(batch):
    assert batch["paths"] == [17 if x[0] else 0 for x in batch["items"]]
    st = batch["stats"]
    assert st["path"] == "fold_pred_batch" and st["units"] == ITEMS - 1 > 4096 and st["n_r"] == sum(x[0] for x in batch["items"])


def test_without_constant_terms_it_is_the_fold_self_batch(rhj, batch):
    d, pool = batch["dev"], batch["pool"]
    for n in (1, 2049, 4097):
        eqs = [(d["k0"], d["v0"], d["k1"], None), (d["k2"], None, d["k2"], None)]
        outs = [((None, None, None), True), ((d["w"], d["v2"], d["big"]), True), ((None, d["v1"], d["big"]), None)]
        a = rhj.fold_pred_batch_device([(n, [], eqs, outs)])[0]
        b = rhj.fold_self_batch_device([(n, eqs, outs)])[0]
        assert [t for _, t in a] == [t for _, t in b]
        for (va, _), (vb, _) in zip(a[:2], b[:2]):
            assert rhj.torch.equal(va, vb)


def test_a_count_is_the_filter_batch_s_hits(rhj, batch):
    d, pool = batch["dev"], batch["pool"]
    for n in (1, 2049, 4097):
        terms = [("big", ">", 7), ("k1", "<", 2)]
        total = rhj.fold_pred_batch_device([(n, [(d[c], None, op, v) for c, op, v in terms], [], [((None, None, None), None)])])[0][0][1]
        keep = np.ones(n, dtype=bool)
        for c, op, v in terms:
            keep &= (pool[c][:n] < np.uint64(v)) if op == "<" else (pool[c][:n] > np.uint64(v))
        assert total == int(keep.sum())
        ids, hits = rhj.filter_batch_device([([(d[c][:n], op, v) for c, op, v in terms], None)])[0]
        assert hits == total and np.array_equal(ids.cpu().numpy(), np.flatnonzero(keep))


def test_the_other_batches_still_agree_afterwards(rhj, batch):
    d, pool = batch["dev"], batch["pool"]
    ones = (None, None, None)
    again = rhj.fold_self_batch_device([(4097, [(d["k0"], d["v0"], d["k1"], None)], [(ones, True)])])[0][0]
    model = sm.self_item_np(4097, [(pool["k0"], pool["v0"], pool["k1"], None)], [ones])[0]
    assert again[1] == model[1] and np.array_equal(again[0].cpu().numpy().view(np.uint64), model[0])
    once_more = rhj.fold_pred_batch_device([(4097, [(d["big"], d["v0"], ">", B63)], [(d["k0"], d["v0"], d["k1"], None)], [(ones, True)])])[0][0]
    model = pm.pred_item_np(4097, [(pool["big"], pool["v0"], ">", B63)], [(pool["k0"], pool["v0"], pool["k1"], None)], [ones])[0]
    assert once_more[1] == model[1] and np.array_equal(once_more[0].cpu().numpy().view(np.uint64), model[0])
