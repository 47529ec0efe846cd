"""tests/fold_pred_model.py against a per-row Python loop: the numpy restatement of rhj_fold_pred_batch_device's item is what the GPU
tests compare with, so it is held to account here, without a device.  Values at and above 2^63 pin the unsigned comparison."""
import numpy as np
import pytest

import fold_pred_model as pm

M64 = pm.M64
B63 = 1 << 63


def pool(n=97, seed=1917):
    rng = np.random.default_rng(seed)
    vals = np.array([0, 1, 5, B63 - 1, B63, B63 + 1, M64 - 1, M64], dtype=np.uint64)
    return {"a": rng.choice(vals, size=n), "b": rng.choice(vals, size=n), "k": rng.integers(0, 3, size=n).astype(np.uint64),
            "l": rng.integers(0, 3, size=n).astype(np.uint64), "v": rng.integers(0, n, size=n).astype(np.uint64),
            "w": rng.integers(0, 1 << 63, size=n).astype(np.uint64) * np.uint64(2) + np.uint64(1)}


OUTS = [(None, None, None), ("w", None, None), (None, "v", "a"), ("w", None, "b")]


def named(p, t):
    return tuple(p[x] if isinstance(x, str) and x in p else x for x in t)


@pytest.mark.parametrize("n", (1, 2, 64, 97))
@pytest.mark.parametrize("nconst", range(5))
@pytest.mark.parametrize("neq", range(5))
def test_the_model_is_the_loop(n, nconst, neq):
    p = pool()
    ops = ("<", ">", "=", "<")
    values = (B63, 1, 5, M64)
    consts = [named(p, ("ab"[c % 2], "v" if c % 2 else None, ops[c], values[c])) for c in range(nconst)]
    eqs = [named(p, ("k", "v" if t % 2 else None, "l", None if t < 2 else "v")) for t in range(neq)]
    outs = [named(p, f) for f in OUTS]
    got, want = pm.pred_item_np(n, consts, eqs, outs), pm.pred_item_loop(n, consts, eqs, outs)
    assert [(v.tolist(), t) for v, t in got] == want


@pytest.mark.parametrize("op", "<>=")
@pytest.mark.parametrize("value", (0, 1, B63 - 1, B63, B63 + 1, M64))
def test_the_comparison_is_unsigned(op, value):
    col = np.array([0, 1, B63 - 1, B63, B63 + 1, M64], dtype=np.uint64)
    vec, total = pm.pred_item_np(len(col), [(col, None, op, value)], [], [(None, None, None)])[0]
    want = [int(x < value if op == "<" else x > value if op == ">" else x == value) for x in col.tolist()]
    assert vec.tolist() == want and total == sum(want)
    assert pm.pred_item_loop(len(col), [(col, None, op, value)], [], [(None, None, None)])[0] == (want, sum(want))


def test_nothing_is_below_0_and_nothing_above_the_largest_value():
    col = np.array([0, B63, M64], dtype=np.uint64)
    one = [(None, None, None)]
    assert pm.pred_item_np(3, [(col, None, "<", 0)], [], one)[0][1] == 0
    assert pm.pred_item_np(3, [(col, None, ">", M64)], [], one)[0][1] == 0
    assert pm.pred_item_np(3, [(col, None, ">", 0)], [], one)[0][0].tolist() == [0, 1, 1]
    assert pm.pred_item_np(3, [(col, None, "<", M64)], [], one)[0][0].tolist() == [1, 1, 0]
    # a signed comparison would call 2^63 negative
    assert pm.pred_item_np(3, [(col, None, ">", B63 - 1)], [], one)[0][0].tolist() == [0, 1, 1]


def test_no_term_and_no_row():
    p = pool()
    assert pm.pred_item_np(5, [], [], [(p["w"], None, None)])[0][0].tolist() == p["w"][:5].tolist()
    assert pm.pred_item_np(0, [(p["a"], None, "<", 3)], [], [(None, None, None)])[0][1] == 0
    assert pm.pred_item_np(5, [], [], []) == []


def test_totals_wrap():
    col = np.full(4, B63, dtype=np.uint64)
    vec, total = pm.pred_item_np(4, [(col, None, "=", B63)], [], [(None, None, col)])[0]
    assert vec.tolist() == [B63] * 4 and total == 0
