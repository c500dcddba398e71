"""Pins tests/adaptive_ref.py (the numpy model of the adaptive-embedding
contract) on cases worked by hand.  No GPU."""
import numpy as np

import adaptive_ref as ref

D = 2


def table(n):
    """Row h = [10 h + 1, 10 h + 2]."""
    h = np.arange(n, dtype=np.float32)
    return np.stack([10 * h + 1, 10 * h + 2], 1).astype(np.float32)


def one_per_bag(n):
    return np.stack([np.arange(n), np.zeros(n, np.int64)], 1).astype(np.int64)


def test_first_position_of_a_repeated_id_decides_its_mask(orc):
    H = table(5)
    ids = np.array([7, 3, 7, 3], np.int64)
    mask = np.array([0, 1, 1, 0])            # 7: positions 0 (0) and 2 (1); 3: 1 (1) and 3 (0)
    uids, idx, counts, m_u, h_u, bad = ref.per_id(orc, ids, mask, 5)
    assert uids.tolist() == [7, 3] and idx.tolist() == [0, 1, 0, 1] and counts.tolist() == [2, 2]
    assert m_u.tolist() == [False, True]     # the smallest k of each id
    assert h_u.tolist() == [2, 3] and not bad
    ev = ref.DictEV(D)
    out, s = ref.lookup_sparse(orc, H, ev, one_per_bag(4), ids, 4, mask, combiner="sum")
    assert s["ev_keys"].tolist() == [3] and s["ev_src"].tolist() == [1]
    assert sorted(ev.rows) == [3]            # 7 never touches the EV
    # both positions of 7 serve the hash row, both of 3 the EV row (= hash row 3 at creation)
    assert out.tolist() == [[21, 22], [31, 32], [21, 22], [31, 32]]
    # supplied bucket rows follow the same rule: the first position's row
    _, _, _, _, h_u, bad = ref.per_id(orc, ids, mask, 5, hash_rows=[4, 0, 1, 2])
    assert h_u.tolist() == [4, 0] and not bad
    _, _, _, _, h_u, bad = ref.per_id(orc, ids, mask, 5, hash_rows=[5, -1, 1, 2])
    assert h_u.tolist() == [0, 0] and bad    # out of range: row 0, flagged


def test_negative_and_large_ids_take_the_floor_mod(orc):
    assert ref.bucket([-7, -5, -1, 0, 4, 5, (1 << 40) + 3], 5).tolist() == \
        [3, 0, 4, 0, 4, 0, ((1 << 40) + 3) % 5]
    assert -7 % 5 == 3 and ((1 << 40) + 3) % 5 == 4
    H = table(5)
    ids = np.array([-7, (1 << 40) + 3], np.int64)
    out, s = ref.lookup_sparse(orc, H, ref.DictEV(D), one_per_bag(2), ids, 2, [0, 0],
                               combiner="sum")
    assert s["h_u"].tolist() == [3, 4]
    assert out.tolist() == [[31, 32], [41, 42]]


def test_two_ids_sharing_a_bucket_share_row_and_gradient(orc):
    H = table(5)
    ids = np.array([2, 7, 12], np.int64)     # all bucket 2; 12 lives in the EV
    mask = np.array([0, 0, 1])
    ev = ref.DictEV(D)
    ind = np.array([[0, 0], [0, 1], [0, 2]], np.int64)      # one bag of three
    out, s = ref.lookup_sparse(orc, H, ev, ind, ids, 1, mask, combiner="sum")
    assert out.tolist() == [[63, 66]]        # 3 x [21, 22]: 12 starts from the shared row
    g = np.array([[1.0, 2.0]], np.float32)
    gu, ek, evv, hi, hv = ref.lookup_sparse_grad(orc, s, ind, 1, g, combiner="sum")
    assert gu.tolist() == [[1, 2]] * 3
    assert ek.tolist() == [12] and evv.tolist() == [[1, 2]]
    assert hi.tolist() == [2, 2, -1]         # the two hash ids name one row; the EV id is skipped
    assert hv is gu or np.array_equal(hv, gu)
    # the initial value carries no gradient into the hash table: row 2 gets 2 x g, not 3 x g
    keep = hi >= 0
    assert gu[keep].sum(0).tolist() == [2, 4]


def test_counter_filter_key_starts_from_the_hash_row_of_the_step_that_admits_it(orc):
    """filter_freq = 3, the id twice per lookup (count 2): freq is compared
    BEFORE the add, so sight 1 (0 -> 2) and sight 2 (2 -> 4) serve the hash
    row and sight 3 (4 >= 3) creates the EV row -- from the hash row as it
    stands at sight 3, not at sight 1."""
    H = table(5)
    ev = ref.DictEV(D, filter_freq=3)
    ids = np.array([8, 8], np.int64)
    ind = np.array([[0, 0], [0, 1]], np.int64)
    mask = [1, 1]
    out, _ = ref.lookup_sparse(orc, H, ev, ind, ids, 1, mask, combiner="mean")
    assert out.tolist() == [[31, 32]] and ev.freq == {8: 2} and not ev.rows
    H[3] = [5, 6]                                            # the hash row trains on
    out, _ = ref.lookup_sparse(orc, H, ev, ind, ids, 1, mask, combiner="mean")
    assert out.tolist() == [[5, 6]] and ev.freq == {8: 4} and not ev.rows
    H[3] = [7, 9]
    out, _ = ref.lookup_sparse(orc, H, ev, ind, ids, 1, mask, combiner="mean")
    assert out.tolist() == [[7, 9]] and ev.rows[8].tolist() == [7, 9] and ev.freq == {8: 4}
    H[3] = [100, 100]                                        # from now on the EV row is its own
    out, _ = ref.lookup_sparse(orc, H, ev, ind, ids, 1, mask, combiner="mean")
    assert out.tolist() == [[7, 9]]
    # read-only: an admitted key with a row serves it, anything else its hash row; no change
    out, _ = ref.lookup_sparse(orc, H, ev, one_per_bag(2), np.array([8, 13], np.int64), 2,
                               [1, 1], combiner="sum", read_only=True)
    assert out.tolist() == [[7, 9], [100, 100]] and sorted(ev.rows) == [8] and ev.freq == {8: 4}
    # with one occurrence per lookup the third sight only brings freq to 3: row at sight 4
    ev1 = ref.DictEV(D, filter_freq=3)
    seen = []
    for step in range(4):
        _, s = ref.lookup_sparse(orc, H, ev1, one_per_bag(1), np.array([8], np.int64), 1, [1])
        seen.append(8 in ev1.rows)
    assert seen == [False, False, False, True] and ev1.freq == {8: 3}


def test_mask_zero_never_touches_the_ev_and_compaction_is_stable(orc):
    H = table(7)
    ev = ref.DictEV(D, filter_freq=2)
    ids = np.array([9, 4, 9, 1, 30, 4], np.int64)
    mask = np.array([1, 0, 0, 1, 1, 1])
    s = ref.served(orc, H, ev, ids, mask)
    assert s["uids"].tolist() == [9, 4, 1, 30] and s["m_u"].tolist() == [True, False, True, True]
    assert s["ev_keys"].tolist() == [9, 1, 30] and s["ev_src"].tolist() == [0, 2, 3]
    assert ev.freq == {9: 2, 1: 1, 30: 1} and 4 not in ev.freq     # occurrence counts go along
    assert np.array_equal(s["emb"], H[[2, 4, 1, 2]])
