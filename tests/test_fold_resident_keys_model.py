"""tests/fold_resident_keys_model.py, the restatement of the rule of csrc/rhj_fold_keys_lds.hip.h, at every edge of the rule; the
shape table of tests/fold_resident_keys_shapes.py, each shape held to the regime it is named for; and the numpy model the GPU
tests compare with against a double loop, on the shapes of at most a few hundred rows.  No device."""
import pytest

import fold_resident_keys_model as rk
import fold_resident_keys_shapes as shapes
import join_foldk_model as km
import join_sum_model as jm


@pytest.fixture(scope="module")
def items():
    return shapes.build_items()


def test_the_constants_are_read_from_the_sources():
    assert rk.WORDS * 8 == 128 * 1024 and rk.TILE == 2048 and rk.K["JSUM_SLOTS_PER_ROW"] == 2
    assert rk.MAX_ROWS >= rk.TILE and rk.MAX_ROWS & (rk.MAX_ROWS - 1) == 0        # a power of two


@pytest.mark.parametrize("nvalues", (0, 1, 3, 9))
def test_the_build_side_at_the_cap_and_beyond(nvalues):
    cap = rk.build_cap(nvalues)
    assert rk.slots(cap) * (1 + nvalues) <= rk.WORDS < rk.slots(cap + 1) * (1 + nvalues)
    assert cap == {0: 8192, 1: 4096, 3: 2048, 9: 512}[nvalues]
    for other in (cap, cap + 1, rk.MAX_ROWS):             # R builds (the tie too), then S builds
        assert rk.resident(cap, other, nvalues) == rk.resident(other, cap, nvalues) == (cap <= other <= rk.MAX_ROWS)
    assert not rk.resident(cap + 1, cap + 1, nvalues) and not rk.resident(cap + 1, cap + 2, nvalues) and not rk.resident(cap + 2, cap + 1, nvalues)
    assert rk.resident(cap, cap + 1, nvalues) == rk.resident(cap + 1, cap, nvalues) == (cap + 1 <= rk.MAX_ROWS)      # the smaller side builds


@pytest.mark.parametrize("nvalues", (0, 1, 3, 9))
def test_the_other_side_at_the_limit_and_beyond(nvalues):
    for build in (1, 100, min(rk.build_cap(nvalues), rk.MAX_ROWS)):
        assert rk.resident(build, rk.MAX_ROWS, nvalues) and rk.resident(rk.MAX_ROWS, build, nvalues)
        assert not rk.resident(build, rk.MAX_ROWS + 1, nvalues) and not rk.resident(rk.MAX_ROWS + 1, build, nvalues)


def test_an_empty_side_is_never_resident():
    for v in (0, 1, 9):
        assert not rk.resident(0, 5, v) and not rk.resident(5, 0, v) and not rk.resident(0, 0, v)
        assert rk.path(0, 5, v) == rk.path(5, 0, v) == 0


def test_the_value_count_is_bounded():
    assert not rk.resident(5, 5, -1) and not rk.resident(5, 5, 10) and rk.resident(5, 5, 0) and rk.resident(5, 5, 9)


def test_the_path_follows_the_switch_and_the_batch():
    assert rk.path(1, 1, 1) == 19 and rk.path(1, 1, 1, on=False) == 14 and rk.path(1, 1, 1, on=False, table=rk.PATH_FOLDN) == 16
    assert rk.path(5000, 5000, 1) == 14 and rk.path(5000, 5000, 1, table=rk.PATH_FOLDN) == 16
    assert rk.path(4096, 4096, 1) == 19 and rk.path(4096, 4096, 2) == 14 and rk.path(4096, 4096, 1, table=rk.PATH_FOLDN) == 19


def test_the_edge_list_holds_both_answers_for_every_value_count():
    for v in (0, 1, 3, 9):
        mine = [rk.resident(nR, nS, nv) for nR, nS, nv in rk.edges() if nv == v]
        assert True in mine and False in mine


def test_every_shape_is_in_the_regime_it_is_named_for(items):
    wrong = [(it["name"], shapes.sizes(it)) for it in items if shapes.regime_of(it) != it["regime"]]
    assert wrong == []
    named = [it for it in items if not it["name"].startswith("1x1 #")]
    assert sum(it["regime"] == shapes.TABLE for it in named) >= 9 and sum(it["regime"] == shapes.RESIDENT for it in named) >= 90
    assert sum(it["regime"] == shapes.EMPTY_SIDE for it in named) == 2
    assert len(items) - len(named) == jm.MAX_ITEMS + 1
    # resident and table items alternate at the head of the batch
    head = [it["regime"] for it in items[:18]]
    assert all(a != shapes.TABLE for a in head[0::2]) and all(b == shapes.TABLE for b in head[1::2])
    # the sizes the workgroup's loops turn on are there, on either side and on both, and every key count on every build side
    rows = {shapes.sizes(it)[:2] for it in items}
    for n in (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2 * rk.TILE + 1):
        assert (n, 3000) in rows and (3000, n) in rows and (n, n) in rows
    assert any(s == rk.MAX_ROWS for _, s in rows) and any(s == rk.MAX_ROWS + 1 for _, s in rows)
    assert any(r == rk.MAX_ROWS for r, _ in rows) and any(r == rk.MAX_ROWS + 1 for r, _ in rows)
    for nk in (1, 2, 3, 4):
        mine = [shapes.sizes(it)[:2] for it in named if len(it["R"][0]) == nk and it["regime"] == shapes.RESIDENT]
        assert any(r < s for r, s in mine) and any(r > s for r, s in mine) and any(r == s for r, s in mine), nk
    for v in (1, 3, 9):
        cap = rk.build_cap(v)
        other = min(cap + 50, rk.MAX_ROWS)
        pairs = [(cap + 1, cap + 51), (cap + 51, cap + 1)] + [(cap, other)] * (cap <= rk.MAX_ROWS) + [(other, cap)] * (cap < rk.MAX_ROWS)
        for pair in pairs:
            assert any(shapes.sizes(it) == pair + (v,) for it in named), (pair, v)
    assert sum(rk.build_cap(v) < rk.MAX_ROWS for v in (1, 3, 9)) >= 2                     # the cap is met from both build sides at two value counts at least


def test_the_pairs_with_one_hash_have_one_home_and_one_tag(items):
    """the shapes named for it hold distinct tuples whose 64-bit hashes are equal, one of each pair absent from the build side"""
    mine = [it for it in items if it["name"].startswith("two tuples a hash")]
    assert len(mine) == 4
    for it in mine:
        nR, nS, _ = shapes.sizes(it)
        build, other = ("S", "R") if jm.build_side(nR, nS) else ("R", "S")
        b, o = set(km.tuples_of(shapes.side_words(it, build))), set(km.tuples_of(shapes.side_words(it, other)))
        by_hash = {}
        for t in o:
            by_hash.setdefault(km.tuple_hash(t), set()).add(t)
        assert len(by_hash) == 64 and all(len(v) == 2 and len(v & b) == 1 for v in by_hash.values())


def test_the_wrapping_run_wraps(items):
    for it in items:
        if not it["name"].startswith("a run that wraps"):
            continue
        nR, nS, _ = shapes.sizes(it)
        build = "S" if jm.build_side(nR, nS) else "R"
        log2 = jm.log2_slots(min(nR, nS))
        homes = sorted({km.home(t, log2) for t in km.tuples_of(shapes.side_words(it, build))})
        assert homes == [(1 << log2) - 3, (1 << log2) - 2, (1 << log2) - 1]       # 18 tuples from the last three slots on: the run passes slot 0


def test_the_numpy_model_equals_the_double_loop_on_the_small_shapes(items):
    small = [it for it in items if not it["name"].startswith("1x1 #") and 0 < shapes.sizes(it)[0] * shapes.sizes(it)[1] <= 400 * 400]
    assert len(small) >= 30
    for it in small + [it for it in items if it["name"].startswith("1x1 #")][:14]:
        outs = [(c, p) for c, p, _ in it["outs"]]
        got = shapes.model(it)
        want = km.brute_force(shapes.side_words(it, "R"), shapes.side_words(it, "S"), it["values"], outs)
        assert [(list(map(int, v)), int(t)) for v, t in got] == [(list(map(int, v)), int(t)) for v, t in want], it["name"]
