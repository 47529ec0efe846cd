"""The fused join (sigmod-2018_amd/csrc/rhj_join_fused.hip.h, fj_body) at its overflow, patch, run, unit and record edges.

Every case is a shape of tests/fused_shapes.py — one planted bucket that puts a unit on a capacity constant of the kernel, in a
thin random background — which tests/test_fused_model.py holds in its regime on the CPU.  Here the device's pair list is
compared with the oracle's bit for bit, order included, and every case asserts the path it meant to reach: stats()["path"],
rhj_last_spec() and rhj_last_walk_units() against the number of units tests/fused_model.py routes to k_join_walk.

Kernel variants (fused_shapes.VARIANTS): the small path at 8 bits (fj_body<MAYRES, N32 = false>: resident and rhj_set_resident(0)),
the two-pass fused path at 9 bits with rhj_set_small(0) and rhj_set_fused(2) (N32 = true), and the same with one row id beyond
2^32 (the join runs again on 16-byte tuples: N32 = false behind the two-pass partition).  The families that need a gather unit
(a, b and the second half of d) run on the gather variants only: a resident unit has neither an overflow buffer nor a patch list;
the resident runs (d) on the resident variants only; b's MAYRES case needs residency on.  c and e run on all six.  At 4 bits
(e) only the small path exists below the split paths' sizes.  f and g are two-pass (and batched) by their nature: 12-byte tuples.
"""
import importlib

import numpy as np
import pytest

import fused_model as fm
import fused_shapes as fs
from pyoracle import PAIR

pytestmark = pytest.mark.gpu

C = fm.constants()

# rhj_set_* knobs and their defaults; every case restores all of them
DEFAULTS = {"spec": 1, "exact": 0, "resident": 1, "fused": 1, "small": 1, "lowradix": 1, "force_hbm_table": 0, "walk_count": 0}


def restore(rhj):
    for k, v in DEFAULTS.items():
        getattr(rhj.lib, "rhj_set_" + k)(v)


@pytest.fixture(scope="module")
def rhj():
    mod = importlib.import_module("sigmod-2018_amd")
    r = mod.RHJ(device=0)
    restore(r)
    yield r
    restore(r)


@pytest.fixture
def knobs(rhj):
    def set_(**kw):
        for k, v in kw.items():
            getattr(rhj.lib, "rhj_set_" + k)(v)
    try:
        yield set_
    finally:
        restore(rhj)


def same(got, want, what):
    want = np.ascontiguousarray(want, dtype=PAIR)
    assert len(got) == len(want), "%s: %d pairs, oracle %d" % (what, len(got), len(want))
    assert np.array_equal(got["row_idR"], want["row_idR"]) and np.array_equal(got["row_idS"], want["row_idS"]), what


def run(rhj, oracle, knobs, s, path):
    """One shape on the device: the oracle's pairs, the path, the speculation's outcome, the walked units."""
    knobs(walk_count=1, **s.knobs)                         # (rhj_set_spec(1) also resets the try-or-not score)
    rhj.set_bits(s.bits)
    m = fm.model(s.R, s.S, s.bits, s.knobs)
    want = oracle.join(s.R, s.S, s.bits)
    assert len(m.pairs) == len(want) and np.array_equal(m.pairs[:, 0], want["row_idR"]) and np.array_equal(m.pairs[:, 1], want["row_idS"])
    t, n = rhj.join_device(rhj.to_device(s.R), rhj.to_device(s.S), capacity=len(want) + 8)
    got = rhj.pairs_to_numpy(t)
    assert n == len(got)
    same(got, want, s.name)
    assert rhj.stats()["path"] == path == m.path, (s.name, rhj.stats()["path"])
    assert rhj.lib.rhj_last_spec() == m.last_spec, (s.name, rhj.lib.rhj_last_spec(), m.last_spec)
    assert rhj.lib.rhj_last_walk_units() == m.walk_units, (s.name, rhj.lib.rhj_last_walk_units(), m.walk_units)
    return m


@pytest.mark.parametrize("case", list(fs.CASES))
def test_edge(rhj, oracle, knobs, case):
    """Families a (overflow buffer), b (patch list), c (index build), d (resident runs, count byte) and e (units and groups):
    see the builders' docstrings in tests/fused_shapes.py for each shape's regime."""
    s = fs.build(case)
    m = run(rhj, oracle, knobs, s, "small" if s.bits <= C.PT_MAX_BITS else "fused")
    assert m.last_spec == 0
    if s.walk is not None:
        assert sum(u.route == "walk" for u in m.units_of(s.b)) == s.walk


def test_walk_count_knob_off(rhj, oracle, knobs):
    """rhj_set_walk_count(0): the two-pass fused path does not fetch the number (no speculation tried: -1), the small path has
    it anyway; a join on another path says -1."""
    s = fs.gather_many("two_gather", 17)
    knobs(**s.knobs)
    rhj.set_bits(s.bits)
    want = oracle.join(s.R, s.S, s.bits)
    dR, dS = rhj.to_device(s.R), rhj.to_device(s.S)
    t, n = rhj.join_device(dR, dS, capacity=len(want) + 8)
    same(rhj.pairs_to_numpy(t), want, "knob off")
    assert rhj.stats()["path"] == "fused" and rhj.lib.rhj_last_walk_units() == -1
    knobs(walk_count=1)
    t, n = rhj.join_device(dR, dS, capacity=len(want) + 8)
    same(rhj.pairs_to_numpy(t), want, "knob on")
    assert rhj.lib.rhj_last_walk_units() == 1
    assert rhj.join_device(dR, dS, count_only=True)[1] == len(want) and rhj.lib.rhj_last_walk_units() == -1    # nothing is walked without a buffer
    s = fs.gather_many("small_gather", 17)
    restore(rhj)
    knobs(**s.knobs)
    rhj.set_bits(s.bits)
    want = oracle.join(s.R, s.S, s.bits)
    t, n = rhj.join_device(rhj.to_device(s.R), rhj.to_device(s.S), capacity=len(want) + 8)
    same(rhj.pairs_to_numpy(t), want, "small path")
    assert rhj.stats()["path"] == "small" and rhj.lib.rhj_last_walk_units() == 1
    knobs(fused=0)
    rhj.join_device(rhj.to_device(s.R), rhj.to_device(s.S), capacity=len(want) + 8)
    assert rhj.stats()["path"] == "tiled" and rhj.lib.rhj_last_walk_units() == -1


# ---- f. deferred emit and the double buffer ---------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [0, 1])
def test_deferred_emit(rhj, oracle, knobs, resident):
    """10 bits, two-pass, every bucket populated with at most ~300 tuples a side and a kind drawn per bucket (no match, foreign
    key, overflow entries, irregular tuple, 17 matches, resident duplicates, one side empty): 256 workgroups take about four
    units each, so a deferred emit reads its half of the double buffer while the next unit fills the other, and a third unit
    reuses the first one's."""
    s = fs.deferred(resident)
    m = run(rhj, oracle, knobs, s, "fused")
    assert m.walk_units > 50 and m.last_spec == 0


@pytest.mark.parametrize("resident", [0, 1])
def test_deferred_emit_batch(rhj, oracle, knobs, resident):
    """The same mix on 8 bits through rhj_join_batch_device: BJ_WGS workgroups a join take every unit in turn, and the drawn
    kinds have every ordered pair at every distance 1..BJ_WGS in the unit order (asserted in tests/test_fused_model.py)."""
    joins = fs.deferred_batch(resident)
    every = {(a, b) for a in fs.KINDS[:-1] for b in fs.KINDS[:-1]}         # ("empty" makes no unit)
    for _, _, kinds in joins:
        assert all(fs.pairs_at(kinds, d) == every for d in range(1, C.BJ_WGS + 1))
    knobs(resident=resident)
    rhj.set_bits(8)
    wants = [oracle.join(R, S, 8) for R, S, _ in joins]
    walk = sum(fm.model(R, S, 8, {"resident": resident}, batch=True, with_pairs=False).walk_units for R, S, _ in joins)
    dev = [(rhj.to_device(R), rhj.to_device(S)) for R, S, _ in joins]
    res, paths = rhj.join_batch_device(dev, capacities=[len(w) + 8 for w in wants], with_info=True)
    assert paths == [6] * len(joins)
    for (t, n), w in zip(res, wants):
        assert n == len(w)
        same(rhj.pairs_to_numpy(t), w, "batch")
    assert rhj.stats()["path"] == "batch"
    assert walk > 60 and rhj.lib.rhj_last_walk_units() == walk


# ---- g. the speculation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [0, 1], ids=["spec_false", "spec_true"])
@pytest.mark.parametrize("kind", fs.SPEC_KINDS)
def test_speculation(rhj, oracle, knobs, kind, resident):
    """k_join_spec<false> (rhj_set_resident(0)) and <true> on a foreign-key join of 1.2 M x 2.2 M tuples at 9 bits with one bucket
    that R, the other relation, probes:
      rec511 / rec512 / rec513  one 256-tuple group of R with that many second-and-later matches.  <false>: the speculation
                                holds and k_join_walk takes 0, 0, 1 units (flag 8).  <true>: a MAYRES kernel keeps the stash for
                                such units, the unit is resident and goes through fj_emit_res: held, no unit walked
      lookback                  a unit of 133 groups, every one with records.  <false>: fj_group_direct, and fj_group_lookback's
                                second step of 64 groups.  <true>: that code is never entered — the kernel keeps the stash for
                                other-side units, and this one (30 133 build tuples: a gather unit of a MAYRES kernel) goes
                                through fj_count_batch and fj_emit_stream<true> at the predicted base; held, nothing walked
      split                     R's side beyond the span: two units, the speculation fails (2), the ordinary kernel's pairs
      totals                    one S tuple with two partners and one with none: the unit's total agrees, the speculation
                                holds (1) — and the pairs are still the oracle's, since the unit itself is joined as usual"""
    s = fs.spec(kind, resident)
    m = run(rhj, oracle, knobs, s, "fused")
    assert m.last_spec == s.extra["last_spec"] and m.walk_units == s.walk
