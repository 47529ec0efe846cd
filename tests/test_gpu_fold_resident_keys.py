"""rhj_join_foldk_batch_device and rhj_join_foldn_batch_device with rhj_set_fold_resident_keys on (include/rhj_inter.h,
csrc/rhj_fold_keys_lds.hip.h): the items of tests/fold_resident_keys_shapes.py in ONE batch each, resident and table items
alternating in call order on shared inputs, every d_out between sentinel words.  A batch runs with the switch on, off, and on
again; every run is compared bit for bit - every word of the output buffer, every total - with the model of join_foldk_model.py
and with the run with the switch off, every item's path with the model of fold_resident_keys_model.py (19 resident, 14 or 16 in
the table form, 0 with an empty side), and the resident info with the model's counts."""
import importlib

import numpy as np
import pytest

import fold_resident_keys_model as rk
import fold_resident_keys_shapes as shapes
import join_sum_model as jm

pytestmark = pytest.mark.gpu

SENTINEL = 0x5E5E5E5E5E5E5E5E

ZERO = {"resident_items": 0, "resident_launches": 0, "table_items": 0}
BATCHES = {"foldk": ("join_foldk_batch_device", rk.PATH_FOLDK), "foldn": ("join_foldn_batch_device", rk.PATH_FOLDN)}


@pytest.fixture(scope="module")
def rhj():
    mod = importlib.import_module("sigmod-2018_amd")
    r = mod.RHJ(device=0)
    was, old = r.lib.rhj_get_fold_resident_keys(), r.lib.rhj_get_fold_resident()
    r.lib.rhj_set_timing(0)
    yield r
    r.lib.rhj_set_fold_resident_keys(was)
    r.lib.rhj_set_fold_resident(old)
    r.lib.rhj_set_timing(2)


class Device:
    """numpy arrays on the device, every root array uploaded once: what items share on the host they share on the device"""
    def __init__(self, rhj):
        self.rhj, self.roots = rhj, {}

    def __call__(self, a):
        if a is None:
            return None
        root = a.base if a.base is not None else a
        assert root.dtype == np.uint64 and root.ndim == 1 and root.flags.c_contiguous and (len(a) == 0 or a.strides == (8,))
        if id(root) not in self.roots:
            self.roots[id(root)] = (root, self.rhj.torch.from_numpy(root.view(np.int64)).to(self.rhj.dev))
        off = (a.__array_interface__["data"][0] - root.__array_interface__["data"][0]) // 8
        return self.roots[id(root)][1][off:off + len(a)]


class Outputs:
    """one device buffer of sentinels; every d_out is a slice of it with a sentinel word before and behind"""
    def __init__(self, rhj, items, kind):
        self.kind, self.entry = kind, getattr(rhj, BATCHES[kind][0])
        self.places, at = [], 1
        for it in items:
            nR = shapes.sizes(it)[0]
            mine = []
            for _, _, given in it["outs"]:
                mine.append(at if given else None)
                if given:
                    at += nR + 1
            self.places.append(mine)
        self.words = at
        self.buf = rhj.torch.full((at,), SENTINEL, dtype=rhj.torch.int64, device=rhj.dev)

    def args(self, dev, items):
        out = []
        for it, mine in zip(items, self.places):
            nR = shapes.sizes(it)[0]
            outs = [(c, tuple(dev(x) for x in p), None if a is None else self.buf[a:a + nR]) for (c, p, _), a in zip(it["outs"], mine)]
            values = [tuple(dev(x) for x in f) for f in it["values"]]
            cR, cS = [dev(c) for c in it["R"][0]], [dev(c) for c in it["S"][0]]
            if self.kind == "foldk":
                out.append((cR, dev(it["R"][1]), cS, dev(it["S"][1]), values, outs))
            else:
                out.append((cR, [dev(s) for s in shapes.vectors(it, "R")], cS, [dev(s) for s in shapes.vectors(it, "S")], values, outs))
        return out

    def expected(self, items, want):
        """the whole buffer as the model has it: the vectors, zeros written where a tuple is absent, sentinels everywhere else"""
        expect = np.full(self.words, SENTINEL, dtype=np.uint64)
        for it, mine, w in zip(items, self.places, want):
            nR, nS, _ = shapes.sizes(it)
            if nR and nS:
                for a, (vec, _) in zip(mine, w):
                    if a is not None:
                        expect[a:a + nR] = vec
        return expect

    def run(self, rhj, args):
        """(every word of the buffer, the totals, the paths, the infos) of one call"""
        self.buf.fill_(SENTINEL)
        got, paths = self.entry(args, with_info=True)
        return {"words": self.buf.cpu().numpy().view(np.uint64), "totals": [[t for _, t in g] for g in got], "paths": paths,
                "resident": rhj.table_batch_last_resident_keys_info(), "one_key": rhj.table_batch_last_resident_info(),
                "combine": rhj.table_batch_last_combine_info(), "reserved": rhj.lib.rhj_last_stats().contents.reserved}


@pytest.fixture(scope="module")
def shared(rhj):
    items = shapes.build_items()
    return {"items": items, "want": [shapes.model(it) for it in items], "dev": Device(rhj)}     # computed once, shared, left unchanged


@pytest.fixture(scope="module", params=("foldk", "foldn"))
def batch(rhj, shared, request):
    kind = request.param
    which = [k for k, it in enumerate(shared["items"]) if kind == "foldn" or "nR" not in it]       # (a vector per word: the foldn batch only)
    items, want = [shared["items"][k] for k in which], [shared["want"][k] for k in which]
    outputs = Outputs(rhj, items, kind)
    args = outputs.args(shared["dev"], items)
    rhj.set_fold_resident(0)
    runs = []
    for on in (1, 0, 1):
        rhj.set_fold_resident_keys(on)
        runs.append(outputs.run(rhj, args))
    rhj.set_fold_resident_keys(0)
    rhj.set_fold_resident(1)                             # the switch of the folds on one key alone: nothing here is resident
    old = outputs.run(rhj, args)
    rhj.set_fold_resident(0)
    return {"kind": kind, "table": BATCHES[kind][1], "items": items, "want": want, "expect": outputs.expected(items, want), "on": runs[0], "off": runs[1],
            "again": runs[2], "old": old, "dev": shared["dev"]}


def names(batch):
    return [it["name"] for it in batch["items"]]


def differing(batch, run, totals):
    return [n for n, a, b in zip(names(batch), run["totals"], totals) if a != b][:8]


@pytest.mark.parametrize("which", ("on", "off", "again", "old"))
def test_every_word_and_every_total_equals_the_model(batch, which):
    run = batch[which]
    assert differing(batch, run, [[t for _, t in w] for w in batch["want"]]) == []
    wrong = np.flatnonzero(run["words"] != batch["expect"])
    assert len(wrong) == 0, "output words %s differ from the model" % wrong[:8].tolist()


@pytest.mark.parametrize("which", ("on", "again"))
def test_every_word_and_every_total_equals_the_run_with_the_switch_off(batch, which):
    run, off = batch[which], batch["off"]
    assert differing(batch, run, off["totals"]) == []
    assert (run["words"] == off["words"]).all()


def test_the_paths_follow_the_rule(batch):
    sizes = [shapes.sizes(it) for it in batch["items"]]
    table = batch["table"]
    for which, on in (("on", True), ("off", False), ("again", True), ("old", False)):
        want = [rk.path(nR, nS, v, on, table) for nR, nS, v in sizes]
        assert [n for n, p, w in zip(names(batch), batch[which]["paths"], want) if p != w] == []
        assert batch[which]["reserved"] == table
    paths = batch["on"]["paths"]
    assert paths.count(19) > jm.MAX_ITEMS and paths.count(table) >= 9 and paths.count(0) == 2
    # the head of the batch alternates the two forms in call order
    assert paths[0:18:2].count(table) == 0 and paths[1:18:2] == [table] * 9
    # the switch of the folds on one key alone leaves every item here on the table path
    assert set(batch["old"]["paths"]) == {0, table}


def test_the_infos_count_each_form(batch):
    sizes = [shapes.sizes(it) for it in batch["items"]]
    resident = sum(rk.path(*s) == 19 for s in sizes)
    table = sum(rk.path(*s) == 14 for s in sizes)
    launched = sum(1 for nR, nS, _ in sizes if nR and nS)
    tiles = lambda on: sum(-(-nS // rk.TILE) for nR, nS, v in sizes if rk.path(nR, nS, v, on) == 14)
    for which in ("on", "again"):
        info = batch[which]["resident"]
        assert info["resident_items"] == resident and info["table_items"] == table and resident + table == launched
        # one launch per chunk that has a resident item; the batch is cut at 4096 items (its tables and tiles are far below the
        # other cuts), and the table items all stand in the first chunk, which has resident ones too
        assert info["resident_launches"] == -(-launched // jm.MAX_ITEMS) == 2
        assert batch[which]["combine"]["tiles"] == tiles(True)       # the table items' add tiles only
        assert batch[which]["one_key"] == ZERO            # the info of the folds on one key does not move
    for which in ("off", "old"):
        assert batch[which]["resident"] == ZERO and batch[which]["one_key"] == ZERO
        assert batch[which]["combine"]["tiles"] == tiles(False) > tiles(True)


def test_resident_items_alone_and_a_chunk_of_them(rhj, batch):
    """a call of resident items only issues no table launch (the combine info has no tile), and an item alone gives what it
    gives in the batch"""
    items = batch["items"]
    which = [k for k, it in enumerate(items) if it["regime"] == shapes.RESIDENT and not it["name"].startswith("1x1 #")]
    mine = [items[k] for k in which]
    outputs = Outputs(rhj, mine, batch["kind"])
    args = outputs.args(batch["dev"], mine)
    want = [batch["want"][k] for k in which]
    try:
        rhj.set_fold_resident_keys(1)
        run = outputs.run(rhj, args)
        assert run["paths"] == [19] * len(mine)
        assert run["resident"] == {"resident_items": len(mine), "resident_launches": 1, "table_items": 0}
        assert run["combine"] == {"tiles": 0, "combined_tiles": 0, "slot_adds": 0}
        assert run["totals"] == [[t for _, t in w] for w in want]
        assert (run["words"] == outputs.expected(mine, want)).all()
        for k in (0, len(mine) // 2, len(mine) - 1):
            one = Outputs(rhj, mine[k:k + 1], batch["kind"])
            alone = one.run(rhj, one.args(batch["dev"], mine[k:k + 1]))
            assert alone["paths"] == [19] and alone["totals"] == [run["totals"][k]] and (alone["words"] == one.expected(mine[k:k + 1], want[k:k + 1])).all()
    finally:
        rhj.set_fold_resident_keys(0)


def test_both_batches_agree_where_every_vector_of_a_side_is_the_same(rhj, shared):
    """an item whose words all read through one vector is the same item in both batches: the same totals, bit for bit"""
    items = [it for it in shared["items"] if "nR" not in it and not it["name"].startswith("1x1 #")]
    got = {}
    try:
        rhj.set_fold_resident_keys(1)
        for kind in BATCHES:
            outputs = Outputs(rhj, items, kind)
            got[kind] = outputs.run(rhj, outputs.args(shared["dev"], items))
    finally:
        rhj.set_fold_resident_keys(0)
    assert got["foldk"]["totals"] == got["foldn"]["totals"] and (got["foldk"]["words"] == got["foldn"]["words"]).all()
    assert [p if p != 14 else 16 for p in got["foldk"]["paths"]] == got["foldn"]["paths"]


def test_the_new_switch_alone_leaves_an_item_on_one_key_on_path_13(rhj):
    torch = rhj.torch
    col = torch.arange(1, 101, dtype=torch.int64, device=rhj.dev)
    item = (col, None, col, None, [(None, None, None)], [(0, (None, None, None), True)])
    try:
        rhj.set_fold_resident(0)
        rhj.set_fold_resident_keys(1)
        got, paths = rhj.join_fold_batch_device([item], with_info=True)
        assert paths == [13] and got[0][0][1] == 100
        assert rhj.table_batch_last_resident_info() == ZERO and rhj.table_batch_last_resident_keys_info() == ZERO
    finally:
        rhj.set_fold_resident_keys(0)
