"""tests/fold_resident_model.py, the restatement of the rule of csrc/rhj_fold_lds.hip.h, at every edge of the rule, and the
shape table of tests/fold_resident_shapes.py, each shape held to the regime it is named for.  No device."""
import pytest

import fold_resident_model as rm
import fold_resident_shapes as shapes
import join_sum_model as jm


def test_the_constants_are_read_from_the_sources():
    assert rm.WORDS * 8 == 128 * 1024 and rm.TILE == 2048 and rm.K["JSUM_SLOTS_PER_ROW"] == 2
    assert rm.MAX_ROWS >= rm.TILE and rm.MAX_ROWS & (rm.MAX_ROWS - 1) == 0        # a power of two


@pytest.mark.parametrize("nvalues", (0, 1, 3, 9))
def test_the_build_side_at_the_cap_and_beyond(nvalues):
    cap = rm.build_cap(nvalues)
    assert rm.slots(cap) * (1 + nvalues) <= rm.WORDS < rm.slots(cap + 1) * (1 + nvalues)
    assert cap == {0: 8192, 1: 4096, 3: 2048, 9: 512}[nvalues]
    for other in (cap, cap + 1, rm.MAX_ROWS):             # R builds (the tie too), then S builds
        assert rm.resident(cap, other, nvalues) and rm.resident(other, cap, nvalues)
    assert not rm.resident(cap + 1, cap + 1, nvalues) and not rm.resident(cap + 1, cap + 2, nvalues) and not rm.resident(cap + 2, cap + 1, nvalues)
    assert rm.resident(cap, cap + 1, nvalues) and rm.resident(cap + 1, cap, nvalues)          # the smaller side builds


def test_the_tie_builds_from_R():
    cap = rm.build_cap(1)
    assert jm.build_side(cap, cap) == 0 and rm.resident(cap, cap, 1)
    assert jm.build_side(cap + 1, cap + 1) == 0 and not rm.resident(cap + 1, cap + 1, 1)


@pytest.mark.parametrize("nvalues", (0, 1, 3, 9))
def test_the_other_side_at_the_limit_and_beyond(nvalues):
    for build in (1, 100, rm.build_cap(nvalues)):
        assert rm.resident(build, rm.MAX_ROWS, nvalues) and rm.resident(rm.MAX_ROWS, build, nvalues)
        assert not rm.resident(build, rm.MAX_ROWS + 1, nvalues) and not rm.resident(rm.MAX_ROWS + 1, build, nvalues)


def test_an_empty_side_is_never_resident():
    for v in (0, 1, 9):
        assert not rm.resident(0, 5, v) and not rm.resident(5, 0, v) and not rm.resident(0, 0, v)
        assert rm.path(0, 5, v) == rm.path(5, 0, v) == 0


def test_the_path_follows_the_switch():
    assert rm.path(1, 1, 1) == 18 and rm.path(1, 1, 1, on=False) == 13
    assert rm.path(5000, 5000, 1) == 13 and rm.path(4096, 4096, 1) == 18 and rm.path(4096, 4096, 2) == 13


def test_the_edge_list_holds_both_answers_for_every_value_count():
    for v in (0, 1, 3, 9):
        mine = [rm.resident(nR, nS, nv) for nR, nS, nv in rm.edges() if nv == v]
        assert True in mine and False in mine


def test_every_shape_is_in_the_regime_it_is_named_for():
    items = shapes.build_items()
    wrong = [(it["name"], shapes.sizes(it)) for it in items if shapes.regime_of(it) != it["regime"]]
    assert wrong == []
    named = [it for it in items if not it["name"].startswith("1x1 #")]
    assert sum(it["regime"] == shapes.TABLE for it in named) >= 8 and sum(it["regime"] == shapes.RESIDENT for it in named) >= 50
    assert len(items) - len(named) == jm.MAX_ITEMS + 1
    # resident and table items alternate at the head of the batch
    head = [it["regime"] for it in items[:16]]
    assert all(a != shapes.TABLE for a in head[0::2]) and all(b == shapes.TABLE for b in head[1::2])
    # the sizes the workgroup's loops turn on are there, on either side
    rows = {shapes.sizes(it)[:2] for it in items}
    for n in (255, 256, 257, 2047, 2048, 2049, 4096):
        assert (n, 100) in rows and (100, n) in rows and (n, n) in rows
    assert (1, 1) in rows and any(s == rm.MAX_ROWS for _, s in rows) and any(s == rm.MAX_ROWS + 1 for _, s in rows)
