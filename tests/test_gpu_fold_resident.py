"""rhj_join_fold_batch_device with rhj_set_fold_resident on (include/rhj_inter.h, csrc/rhj_fold_lds.hip.h): the items of
tests/fold_resident_shapes.py in ONE batch, resident and table items alternating in call order on shared inputs, every d_out
between sentinel words.  The batch runs with the switch on, off, and on again; every run is compared bit for bit - every word of
the output buffer, every total, rc - with the model of join_fold_model.py and with the run with the switch off, and every item's
path with the model of fold_resident_model.py: 18 resident, 13 in the table form, 0 with an empty side."""
import importlib

import numpy as np
import pytest

import fold_resident_model as rm
import fold_resident_shapes as shapes
import join_sum_model as jm

pytestmark = pytest.mark.gpu

SENTINEL = 0x5E5E5E5E5E5E5E5E


@pytest.fixture(scope="module")
def rhj():
    mod = importlib.import_module("sigmod-2018_amd")
    r = mod.RHJ(device=0)
    was = r.lib.rhj_get_fold_resident()
    r.lib.rhj_set_timing(0)
    yield r
    r.lib.rhj_set_fold_resident(was)
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
    def __init__(self, rhj, items):
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
            out.append((dev(it["R"][0]), dev(it["R"][1]), dev(it["S"][0]), dev(it["S"][1]), [tuple(dev(x) for x in f) for f in it["values"]], outs))
        return out

    def expected(self, items, want):
        """the whole buffer as the model has it: the vectors, zeros written where a key is absent, sentinels everywhere else"""
        expect = np.full(self.words, SENTINEL, dtype=np.uint64)
        for it, mine, w in zip(items, self.places, want):
            nR, nS, _ = shapes.sizes(it)
            if nR and nS:
                for a, (vec, _) in zip(mine, w):
                    if a is not None:
                        expect[a:a + nR] = vec
        return expect

    def run(self, rhj, args):
        """(every word of the buffer, the totals, the paths, the resident info, the combine info) of one call"""
        self.buf.fill_(SENTINEL)
        got, paths = rhj.join_fold_batch_device(args, with_info=True)
        return {"words": self.buf.cpu().numpy().view(np.uint64), "totals": [[t for _, t in g] for g in got], "paths": paths,
                "resident": rhj.table_batch_last_resident_info(), "combine": rhj.table_batch_last_combine_info(),
                "reserved": rhj.lib.rhj_last_stats().contents.reserved}


@pytest.fixture(scope="module")
def batch(rhj):
    items = shapes.build_items()
    dev = Device(rhj)
    outputs = Outputs(rhj, items)
    args = outputs.args(dev, items)
    want = [shapes.model(it) for it in items]            # computed once, shared, left unchanged
    runs = []
    for on in (1, 0, 1):
        rhj.set_fold_resident(on)
        runs.append(outputs.run(rhj, args))
    rhj.set_fold_resident(0)
    return {"items": items, "want": want, "expect": outputs.expected(items, want), "on": runs[0], "off": runs[1], "again": runs[2], "dev": dev}


def names(batch):
    return [it["name"] for it in batch["items"]]


def differing(batch, run, totals):
    return [n for n, a, b in zip(names(batch), run["totals"], totals) if a != b][:8]


@pytest.mark.parametrize("which", ("on", "off", "again"))
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
    for which, on in (("on", True), ("off", False), ("again", True)):
        want = [rm.path(nR, nS, v, on) for nR, nS, v in sizes]
        assert [n for n, p, w in zip(names(batch), batch[which]["paths"], want) if p != w] == []
        assert batch[which]["reserved"] == 13
    paths = batch["on"]["paths"]
    assert paths.count(18) > jm.MAX_ITEMS and paths.count(13) >= 8 and paths.count(0) == 2
    # the head of the batch alternates the two forms in call order
    assert paths[0:16:2].count(13) == 0 and paths[1:16:2] == [13] * 8


def test_the_infos_count_each_form(batch):
    sizes = [shapes.sizes(it) for it in batch["items"]]
    resident = sum(rm.path(*s) == 18 for s in sizes)
    table = sum(rm.path(*s) == 13 for s in sizes)
    tiles = lambda on: sum(-(-nS // rm.TILE) for nR, nS, v in sizes if rm.path(nR, nS, v, on) == 13)
    for which in ("on", "again"):
        info = batch[which]["resident"]
        assert info["resident_items"] == resident and info["table_items"] == table
        assert 2 <= info["resident_launches"] <= 3       # more resident items than one chunk holds: at least two chunks
        assert batch[which]["combine"]["tiles"] == tiles(True)       # the table items' add tiles only
    assert batch["off"]["resident"] == {"resident_items": 0, "resident_launches": 0, "table_items": 0}
    assert batch["off"]["combine"]["tiles"] == tiles(False) > tiles(True)


def test_resident_items_alone_and_a_chunk_of_them(rhj, batch):
    """a call of resident items only issues no table launch (the combine info has no tile), and an item alone gives what it
    gives in the batch"""
    items = batch["items"]
    which = [k for k, it in enumerate(items) if it["regime"] == shapes.RESIDENT and not it["name"].startswith("1x1 #")]
    mine = [items[k] for k in which]
    outputs = Outputs(rhj, mine)
    args = outputs.args(batch["dev"], mine)
    want = [batch["want"][k] for k in which]
    try:
        rhj.set_fold_resident(1)
        run = outputs.run(rhj, args)
        assert run["paths"] == [18] * len(mine)
        assert run["resident"] == {"resident_items": len(mine), "resident_launches": 1, "table_items": 0}
        assert run["combine"] == {"tiles": 0, "combined_tiles": 0, "slot_adds": 0}
        assert run["totals"] == [[t for _, t in w] for w in want]
        assert (run["words"] == outputs.expected(mine, want)).all()
        for k in (0, len(mine) // 2, len(mine) - 1):
            one = Outputs(rhj, mine[k:k + 1])
            alone = one.run(rhj, one.args(batch["dev"], mine[k:k + 1]))
            assert alone["paths"] == [18] and alone["totals"] == [run["totals"][k]] and (alone["words"] == one.expected(mine[k:k + 1], want[k:k + 1])).all()
    finally:
        rhj.set_fold_resident(0)
