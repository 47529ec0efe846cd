"""The four plan functions of the fold route, rhj_query_fold_plan, rhj_query_foldk_plan, rhj_query_folds_plan and
rhj_query_foldn_plan (pure functions, no device), each held to its own Python model on one seeded random sample of queries:
accept or refuse, and every field of what they return.  The library derives the four from one planner; the models
(tests/join_fold*_model.py) are four independent statements of the rules.  Then the containments include/rhj_inter.h states: what
rhj_query_fold_plan accepts rhj_query_foldk_plan plans the same way with one key a step, what that accepts rhj_query_folds_plan
plans the same way unless it drops an implied predicate, and rhj_query_foldn_plan at levels 0 is rhj_query_folds_plan's.

A query has 1..5 bindings, columns 0..2 and 0..7 predicates that connect all its bindings: a random spanning tree and extras drawn
by kind (a literal repeat, a repeat written the other way round, x.c = x.c, a predicate on one binding, a parallel predicate, an
implied one, any predicate at all), in random order.  The sample must hold every kind and true cycles, and every rule must accept
and refuse some dozens of it, or the test fails for having exercised nothing."""
import ctypes as C
import importlib

import numpy as np
import pytest

import join_fold_model as fm
import join_foldk_model as km
import join_foldn_model as nm
import join_folds_model as sm

SEED, COUNT = 20188, 1500
MAX_BINDINGS, COLUMNS, MAX_PREDICATES = 5, 3, 7
KINDS = ("literal repeat", "flipped repeat", "x.c = x.c", "one binding", "parallel", "implied", "any")
FEATURES = KINDS[:6] + ("true cycle",)
AT_LEAST = 36                                            # of the sample: queries with each feature; accepted and refused by each rule


def random_queries(count=COUNT, seed=SEED):
    """[(relations, joins, filters, views)], all valid (rhj_query_levels accepts them: the bindings end in one node)"""
    rng = np.random.default_rng(seed)
    col = lambda: int(rng.integers(0, COLUMNS))
    queries = []
    while len(queries) < count:
        nb = int(rng.integers(1, MAX_BINDINGS + 1))
        order = [int(x) for x in rng.permutation(nb)]
        joins = []
        for k in range(1, nb):                           # a spanning tree: every binding hangs off one drawn before it
            p = (order[int(rng.integers(0, k))], col(), order[k], col())
            joins.append(p if rng.integers(0, 2) else (p[2], p[3], p[0], p[1]))
        for _ in range(int(rng.integers(0, MAX_PREDICATES - len(joins) + 1))):
            kind = KINDS[int(rng.integers(0, len(KINDS)))]
            e = joins[int(rng.integers(0, len(joins)))] if joins else None
            x = int(rng.integers(0, nb))
            if kind == "literal repeat" and e:
                p = e
            elif kind == "flipped repeat" and e:
                p = (e[2], e[3], e[0], e[1])
            elif kind == "x.c = x.c":
                c = col()
                p = (x, c, x, c)
            elif kind == "one binding":
                c = col()
                p = (x, c, x, (c + 1 + int(rng.integers(0, COLUMNS - 1))) % COLUMNS)
            elif kind == "parallel" and e:
                p = (e[0], col(), e[2], col())
            elif kind == "implied" and e:                # two predicates that share a term say a third between their other terms
                meets = [(m, far) for m in joins if m != e for near, far in (((m[0], m[1]), (m[2], m[3])), ((m[2], m[3]), (m[0], m[1]))) if near == (e[2], e[3])]
                p = (e[0], e[1]) + meets[int(rng.integers(0, len(meets)))][1] if meets else (x, col(), int(rng.integers(0, nb)), col())
            else:
                p = (x, col(), int(rng.integers(0, nb)), col())
            joins.append(p)
        joins = [joins[int(k)] for k in rng.permutation(len(joins))]
        queries.append(([int(r) for r in rng.integers(0, 3, size=nb)], joins, [], [(int(rng.integers(0, nb)), col())]))
    return queries


def features(query):
    """which of FEATURES a query shows, by a reading of its predicates that belongs to this test alone"""
    rels, joins, _, _ = query
    seen, up, kept = set(), {}, []

    def find(t):
        up.setdefault(t, t)
        while up[t] != t:
            t = up[t]
        return t

    for l, (a, ca, b, cb) in enumerate(joins):
        literal, flipped = (a, ca, b, cb) in joins[:l], (b, cb, a, ca) in joins[:l]
        x, y = find((a, ca)), find((b, cb))
        if literal:
            seen.add("literal repeat")
        if flipped and (a, ca) != (b, cb):
            seen.add("flipped repeat")
        if (a, ca) == (b, cb):
            seen.add("x.c = x.c")
        elif a == b:
            seen.add("one binding")
        if x == y and not literal and not flipped and (a, ca) != (b, cb):
            seen.add("implied")
        if x != y:
            up[y] = x
            if a != b:
                kept.append((min(a, b), max(a, b)))
    if len(kept) > len(set(kept)):
        seen.add("parallel")
    if len(set(kept)) > len(rels) - 1:
        seen.add("true cycle")
    return seen


@pytest.fixture(scope="module")
def mod():
    return importlib.import_module("sigmod-2018_amd")


@pytest.fixture(scope="module")
def lib(mod):
    return mod.load_library()


def step_fields(s, keys=True):
    return (s.child, s.parent, s.round) + ((s.nkeys, tuple(s.joins)) if keys else ())


def library_plans(mod, lib, query, nrel=3):
    """the four functions on one query: per rule (return value, every field of everything it wrote).  root starts at -1: a refusal
    leaves it alone."""
    arr, keep = mod.query_descs([query])
    q = C.byref(arr[0])
    root, steps = C.c_int(-1), (mod.FoldStep * (mod.QUERY_MAX_RELS - 1))()
    n = lib.rhj_query_fold_plan(q, nrel, None, C.byref(root), steps)
    fold = (n, root.value, [step_fields(s, False) for s in steps[:max(n, 0)]])
    root, steps = C.c_int(-1), (mod.FoldKStep * (mod.QUERY_MAX_RELS - 1))()
    n = lib.rhj_query_foldk_plan(q, nrel, None, C.byref(root), steps)
    foldk = (n, root.value, [step_fields(s) for s in steps[:max(n, 0)]])
    plan = mod.FoldsPlan()
    n = lib.rhj_query_folds_plan(q, nrel, None, C.byref(plan))
    folds = (n, plan.root, plan.nsteps, plan.nself, [step_fields(s) for s in plan.steps], list(plan.self))
    plan = mod.FoldNPlan()
    n = lib.rhj_query_foldn_plan(q, nrel, None, C.byref(plan))
    foldn = (n, plan.levels, plan.root, plan.nsteps, plan.nself, list(plan.node), [step_fields(s) for s in plan.steps], list(plan.self))
    del keep
    return fold, foldk, folds, foldn


def whole_steps(steps):
    """a model's [(child, parent, round, [predicate indices])] as every field of the structure's seven steps: zero where unused"""
    pad = lambda x, n: tuple(x) + (0,) * (n - len(x))
    return [(c, p, r, len(idx), pad(idx, km.MAX_KEYS)) for c, p, r, idx in steps] + [(0, 0, 0, 0, (0,) * km.MAX_KEYS)] * (7 - len(steps))


def test_the_four_plans_against_their_models_and_each_other(mod, lib):
    assert (mod.FOLD_MAX_KEYS, mod.FOLD_SELF_MAX_TERMS, mod.QUERY_MAX_RELS) == (km.MAX_KEYS, sm.MAX_TERMS, 8)
    queries = random_queries()
    shown = dict.fromkeys(FEATURES, 0)
    accepted = dict.fromkeys(("fold", "foldk", "folds", "foldn at levels 0"), 0)
    nself_words = mod.QUERY_MAX_RELS * mod.FOLD_SELF_MAX_TERMS
    pad = lambda x, n: list(x) + [0] * (n - len(x))
    for query in queries:
        assert sm.valid(query), query
        nb = len(query[0])
        for f in features(query):
            shown[f] += 1
        fold, foldk, folds, foldn = library_plans(mod, lib, query)
        # each against its model
        want = fm.fold_plan(query)
        assert fold == ((0, -1, []) if want is None else (nb - 1, want[0], [tuple(s) for s in want[1]])), query
        want = km.foldk_plan(query)
        assert foldk == ((0, -1, []) if want is None else (nb - 1, want[0], whole_steps(want[1])[:nb - 1])), query
        want = sm.folds_plan(query)
        empty = mod.FoldsPlan()
        if want is None:                                 # refused: the structure is as it was handed in
            assert folds == (0, 0, 0, 0, [step_fields(s) for s in empty.steps], list(empty.self)), query
        else:
            assert folds == (1, want[0], len(want[1]), len(want[2]), whole_steps(want[1]), pad(want[2], nself_words)), query
        L, node, root, steps, selfs = nm.foldn_plan(query)
        assert foldn == (1, L, root, len(steps), len(selfs), pad(node, mod.QUERY_MAX_RELS), whole_steps(steps), pad(selfs, nself_words)), query
        # the containments
        accepted["fold"] += fold[0] > 0
        accepted["foldk"] += foldk[0] > 0
        accepted["folds"] += folds[0] == 1
        accepted["foldn at levels 0"] += foldn[1] == 0
        if fold[0] > 0:
            assert foldk[:2] == fold[:2] and [(s[:3], s[3]) for s in foldk[2]] == [(s, 1) for s in fold[2]], query
        if foldk[0] > 0:
            assert folds[0] == 1 and folds[1:4] == (foldk[1], foldk[0], 0), query
            assert [s[:3] for s in folds[4][:nb - 1]] == [s[:3] for s in foldk[2]], query
            if "implied" not in features(query):
                assert folds[4][:nb - 1] == foldk[2], query
            else:                                        # that plan keeps an implied predicate as a key word, this one does not
                assert all(set(a[4][:a[3]]) <= set(b[4][:b[3]]) for a, b in zip(folds[4], foldk[2])), query
        assert (foldn[1] == 0) == (folds[0] == 1), query
        if folds[0] == 1:
            assert foldn[2:5] == folds[1:4] and foldn[5][:nb] == list(range(nb)) and foldn[6:] == folds[4:], query
    print("of %d queries:" % len(queries), ", ".join("%s %d" % kv for kv in shown.items()))
    print("accepted / refused:", ", ".join("%s %d / %d" % (k, v, len(queries) - v) for k, v in accepted.items()))
    assert all(n >= AT_LEAST for n in shown.values()), shown
    assert all(AT_LEAST <= n <= len(queries) - AT_LEAST for n in accepted.values()), accepted
