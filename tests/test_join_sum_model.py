"""tests/join_sum_model.py held to account without a device: join_sum against a double loop and against the numpy executor of
query_model.py on the final joins of the `small` workload; the restated table rule and the keys built from it."""
import numpy as np

import join_sum_model as jm
from query_model import parse_work, run_query, track_kinds


def test_join_sum_against_a_double_loop():
    rng = np.random.default_rng(20181)
    big = [0, 1, (1 << 63), (1 << 64) - 1, (1 << 64) - 2, 12345]
    for case in range(12):
        nR, nS = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        pool = rng.choice(np.array([0, 1, 2, 3, (1 << 64) - 1, 1 << 63, 77], dtype=np.uint64), size=int(rng.integers(1, 6)), replace=False)
        kR, kS = rng.choice(pool, size=nR), rng.choice(pool, size=nS)
        terms = []
        for t in range(case % 9):
            side = int(rng.integers(0, 2))
            terms.append((side, rng.choice(np.array(big, dtype=np.uint64), size=nR if side == 0 else nS)))
        assert jm.join_sum(kR, kS, terms) == jm.brute_force(kR, kS, terms), case
    # no match at all, and an empty side
    assert jm.join_sum([1, 2, 3], [4, 5], [(0, [9, 9, 9]), (1, [7, 7])]) == (0, [0, 0])
    assert jm.join_sum([], [4, 5], [(1, [7, 7])]) == (0, [0])
    # a product that wraps: 3 pairs of 2^63 is 2^63 modulo 2^64
    assert jm.join_sum([5], [5, 5, 5], [(0, [1 << 63])]) == (3, [1 << 63])


def test_join_sum_against_the_numpy_executor_on_the_small_workload(golden):
    rels = golden.small_relations
    cols = [[np.asarray(c, dtype=np.uint64) for c in rels["r%d" % r]] for r in range(len(rels))]
    queries = parse_work(golden.small["work_lines"])
    assert len(queries) == 50
    items = 0
    for q in queries:
        item = jm.final_join_item(cols, q)
        kinds = track_kinds(q)
        assert (item is None) == (not kinds or kinds[-1] == 1), q
        if item is None:
            continue
        items += 1
        sums, rows = run_query(cols, q)
        matches, got = jm.join_sum(*item)
        assert (got, matches) == (list(sums), rows), q
    assert items >= 40                                   # (six predicates of the workload are equalities, not all of them last)


def test_the_table_rule():
    assert jm.TILE == 2048 and jm.SLOT_BYTES == 16 and jm.MUL % 2 == 1 and (jm.MUL * jm.MUL_INV) & jm.M64 == 1
    assert [jm.log2_slots(n) for n in (1, 2, 3, 1023, 1024, 1025, 2048, 2049)] == [1, 2, 3, 11, 11, 12, 12, 13]
    for n in (1, 5, 1023, 1024, 1025, 70000):
        assert (1 << jm.log2_slots(n)) >= 2 * n and ((1 << jm.log2_slots(n)) < 4 * n or n == 1)
    assert (jm.build_side(5, 5), jm.build_side(4, 5), jm.build_side(5, 4)) == (0, 0, 1)
    assert jm.table_bytes(5000, 1) == 32 and jm.table_bytes(1, 5000) == 32 and jm.table_bytes(1024, 4000) == 2048 * 16


def test_colliding_keys_home_to_one_slot():
    log2 = jm.log2_slots(600)
    keys = jm.keys_homed_at(5, log2, 600)
    assert len(set(keys.tolist())) == 600 and jm.EMPTY not in keys.tolist()
    assert {jm.home(k, log2) for k in keys.tolist()} == {5}


def test_keys_homed_in_the_last_slots():
    log2 = jm.log2_slots(40)
    last = (1 << log2) - 1
    keys = np.concatenate([jm.keys_homed_at(s, log2, 6, start=1 + 10 * k) for k, s in enumerate((last - 2, last - 1, last))])
    assert len(set(keys.tolist())) == 18
    assert sorted({jm.home(k, log2) for k in keys.tolist()}) == [last - 2, last - 1, last]      # 18 keys from there on: the run wraps to slot 0
