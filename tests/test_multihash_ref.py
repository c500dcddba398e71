"""tests/multihash_ref.py, the reference of the multi-hash GPU tests, against
vectors worked out by hand: Q = 3 rows, R = 2 rows, D = 2, ids 0..8 (every
(q, r) pair that occurs), the three operations, one bag of 9 and one of 10
with mean, the gradient split and one SGD step with repeated slice indices.
All values are small integers, so every sum is exact in fp32 whatever its
order; only the mean's single division rounds."""
import numpy as np
import pytest

import multihash_ref as ref
from deeprec_amd import get_multihash_variable  # noqa: F401  (the feature under test)

QT = np.array([[1, 2], [3, 4], [5, 6]], np.float32)
RT = np.array([[10, 20], [30, 40]], np.float32)
IDS = np.arange(9, dtype=np.int64)
# id:        0  1  2  3  4  5  6  7  8
Q_OF = [0, 0, 0, 1, 1, 1, 2, 2, 2]          # id // 3
R_OF = [0, 1, 0, 1, 0, 1, 0, 1, 0]          # id % 2
ADD = [[11, 22], [31, 42], [11, 22], [33, 44], [13, 24], [33, 44], [15, 26], [35, 46], [15, 26]]
MUL = [[10, 40], [30, 80], [10, 40], [90, 160], [30, 80], [90, 160], [50, 120], [150, 240],
       [50, 120]]
CAT = [[1, 2, 10, 20], [1, 2, 30, 40], [1, 2, 10, 20], [3, 4, 30, 40], [3, 4, 10, 20],
       [3, 4, 30, 40], [5, 6, 10, 20], [5, 6, 30, 40], [5, 6, 10, 20]]
HAND = {"add": ADD, "mul": MUL, "concat": CAT}


def test_index_rule():
    q, r, ok = ref.index(IDS, 3, 2)
    assert q.tolist() == Q_OF and r.tolist() == R_OF and ok.all()
    # the quotient's divisor is the Q table's row count, floor semantics
    q, r, ok = ref.index([9, -1, -3, -4], 3, 2)
    assert q.tolist() == [3, -1, -1, -2] and r.tolist() == [1, 1, 1, 0]
    assert ok.tolist() == [False] * 4


@pytest.mark.parametrize("op", ref.OPS)
def test_rows_by_hand(orc, op):
    got = ref.rows(orc, QT, RT, op, IDS)
    assert got.dtype == np.float32 and got.tolist() == HAND[op]
    assert ref.lookup(orc, QT, RT, op, IDS.reshape(3, 3)).tolist() == \
        np.array(HAND[op], np.float32).reshape(3, 3, -1).tolist()
    # out of range: a zero row
    assert ref.rows(orc, QT, RT, op, [9, 4, -1]).tolist() == \
        [[0.0] * len(HAND[op][0]), HAND[op][4], [0.0] * len(HAND[op][0])]
    assert ref.materialize(orc, QT, RT, op, 9).tolist() == HAND[op]


@pytest.mark.parametrize("op", ref.OPS)
def test_bags_of_9_and_10_with_mean(orc, op):
    # bag 0: ids 0..8 (9 rows: one first chunk of 9, divided at once);
    # bag 1: ids 0..8 and 0 again (10 rows: a chunk of 2, a chunk of 8, then / 10)
    values = np.concatenate([IDS, IDS, [0]]).astype(np.int64)
    seg = np.array([0] * 9 + [1] * 10, np.int64)
    indices = np.stack([seg, np.concatenate([np.arange(9), np.arange(10)])], 1)
    got = ref.lookup_sparse(orc, QT, RT, op, indices, values, 2, combiner="mean")
    h = np.array(HAND[op], np.float32)
    s9 = h.sum(0)                      # exact: small integers
    s10 = s9 + h[0]
    want = np.stack([s9 / np.float32(9), s10 / np.float32(10)])
    assert {"add": [197, 296], "mul": [510, 1040], "concat": [27, 36, 170, 260]}[op] == s9.tolist()
    assert got.dtype == np.float32 and np.array_equal(got, want)
    got = ref.lookup_sparse(orc, QT, RT, op, indices, values, 2, combiner="sum")
    assert np.array_equal(got, np.stack([s9, s10]))


def test_gradient_split_by_hand(orc):
    gu = np.array([[i + 1, -(i + 1)] for i in range(9)], np.float32)
    qi, qv, ri, rv = ref.split(QT, RT, "add", IDS, gu)
    assert qi.tolist() == Q_OF and ri.tolist() == R_OF
    assert np.array_equal(qv, gu) and np.array_equal(rv, gu)
    qi, qv, ri, rv = ref.split(QT, RT, "mul", IDS, gu)
    assert qi.tolist() == Q_OF and ri.tolist() == R_OF
    # id 3: q = 1, r = 1, g = [4, -4]:  dQ[1] gets g * R[1], dR[1] gets g * Q[1]
    assert qv[3].tolist() == [120, -160] and rv[3].tolist() == [12, -16]
    assert qv[8].tolist() == [90, -180] and rv[8].tolist() == [45, -54]
    g4 = np.arange(36, dtype=np.float32).reshape(9, 4)
    qi, qv, ri, rv = ref.split(QT, RT, "concat", IDS, g4)
    assert np.array_equal(qv, g4[:, :2]) and np.array_equal(rv, g4[:, 2:])
    # out of range: index -1 and zero rows in both slices
    qi, qv, ri, rv = ref.split(QT, RT, "mul", np.array([9, 4]), gu[:2])
    assert qi.tolist() == [-1, 1] and ri.tolist() == [-1, 0]
    assert qv.tolist() == [[0, 0], [20, -40]] and rv.tolist() == [[0, 0], [6, -8]]


def test_backward_of_a_sum_bag_and_one_sgd_step(orc):
    # one bag [0, 3, 0], sum, top gradient [1, 2]: unique ids [0, 3], gu = [[2, 4], [1, 2]]
    values = np.array([0, 3, 0], np.int64)
    indices = np.array([[0, 0], [0, 1], [0, 2]], np.int64)
    uids, gu, qi, qv, ri, rv = ref.lookup_sparse_grad(
        orc, QT, RT, "add", indices, values, 1, np.array([[1, 2]], np.float32), combiner="sum")
    assert uids.tolist() == [0, 3] and gu.tolist() == [[2, 4], [1, 2]]
    assert qi.tolist() == [0, 1] and ri.tolist() == [0, 1]
    # repeated slice indices are summed first, then applied: R row 0 hit twice
    table = RT.copy()
    ref.apply_sgd(orc, table, 0.5, np.array([0, 1, 0, -1]),
                  np.array([[2, 4], [1, 2], [4, 8], [100, 100]], np.float32))
    assert table.tolist() == [[10 - 3, 20 - 6], [30 - 0.5, 40 - 1]]
    acc = np.full_like(RT, 1.0)
    table = RT.copy()
    ref.apply_adagrad(orc, table, acc, 1.0, np.array([1, 1]), np.array([[1, 2], [2, 0]], np.float32))
    assert acc.tolist() == [[1, 1], [10, 5]]
    assert np.array_equal(table[0], RT[0])
    assert np.array_equal(table[1], RT[1] - np.float32([3, 2]) *
                          (np.float32(1) / np.sqrt(np.float32([10, 5]))))
