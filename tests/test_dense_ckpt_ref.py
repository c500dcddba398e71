"""The numpy model of the dense checkpoint entries (tests/dense_ckpt_ref.py),
pinned on cases worked by hand: the bit layout, what a mark skips, the export
order and overflow, the upsert's skip-and-latch, and the names and contents of
the tensors of a full save and of a delta."""
import numpy as np

import dense_ckpt_ref as ref


def test_words_and_masks():
    assert [ref.words(r) for r in (0, 1, 31, 32, 33, 64, 65, 1 << 31)] == \
        [0, 1, 1, 1, 2, 2, 3, 1 << 26]
    assert ref.tail_mask(1) == 1
    assert ref.tail_mask(31) == 0x7FFFFFFF
    assert ref.tail_mask(32) == 0xFFFFFFFF
    assert ref.tail_mask(33) == 1
    assert ref.valid_mask(0, 33) == 0xFFFFFFFF and ref.valid_mask(1, 33) == 1
    assert ref.valid_mask(2, 33) == 0 and ref.valid_mask(-1, 33) == 0


def test_mark_by_hand():
    bits = ref.new_bits(40)
    assert bits.dtype == np.uint32 and bits.tolist() == [0, 0]
    # rows 0, 3, 31 -> word 0 = 1 + 8 + 2^31; row 32 -> word 1 bit 0; 39 -> bit 7
    got = ref.mark(bits, 40, [3, 0, 31, 3, 32, 39])
    assert got.tolist() == [0x80000009, 0x81]
    assert bits.tolist() == [0, 0]                  # the input is left alone
    # -1, 40 (== rows), 2^40 are skipped
    assert ref.mark(bits, 40, [-1, 40, 1 << 40, 5]).tolist() == [0x20, 0]
    # the device count cuts the list; what lies past it is never read as a row
    assert ref.mark(bits, 40, [1, 2, 1 << 40, -9], n_dev=2).tolist() == [6, 0]
    assert ref.mark(bits, 40, [1, 2], n_dev=0).tolist() == [0, 0]
    assert ref.mark(bits, 40, [1, 2], n_dev=37).tolist() == [6, 0]
    assert ref.mark(bits, 40, [1, 2], n_dev=-3).tolist() == [0, 0]
    assert ref.mark(bits, 40, []).tolist() == [0, 0]


def test_mark_all_count_and_tail():
    assert ref.mark_all(33).tolist() == [0xFFFFFFFF, 1]
    assert ref.mark_all(64).tolist() == [0xFFFFFFFF, 0xFFFFFFFF]
    assert ref.mark_all(1).tolist() == [1]
    assert ref.count(ref.mark_all(33), 33) == 33
    # hand-set tail bits (rows 33 .. 63 of a 33-row table) are ignored
    bits = np.array([0x5, 0xFFFFFFFE], np.uint32)
    assert ref.count(bits, 33) == 2
    assert ref.marked_rows(bits, 33).tolist() == [0, 2]
    bits[1] = 0xFFFFFFFF
    assert ref.marked_rows(bits, 33).tolist() == [0, 2, 32]


def test_export_by_hand():
    w = np.arange(40 * 2, dtype=np.float32).reshape(40, 2)
    acc = -w
    bits = ref.mark(ref.new_bits(40), 40, [39, 3, 32, 0])
    m, rows, (vw, va) = ref.export(bits, 40, [w, acc], 10)
    assert m == 4 and rows.tolist() == [0, 3, 32, 39] and rows.dtype == np.int64
    assert vw.tolist() == [[0, 1], [6, 7], [64, 65], [78, 79]]
    assert va.tolist() == [[0, -1], [-6, -7], [-64, -65], [-78, -79]]
    # a capacity below m: the first `capacity` rows, and m still the full count
    m, rows, (vw,) = ref.export(bits, 40, [w], 2)
    assert m == 4 and rows.tolist() == [0, 3] and vw.shape == (2, 2)
    m, rows, cols = ref.export(bits, 40, [], 4)
    assert m == 4 and rows.tolist() == [0, 3, 32, 39] and cols == []
    m, rows, _ = ref.export(ref.new_bits(40), 40, [w], 4)
    assert m == 0 and rows.size == 0


def test_upsert_by_hand():
    w = np.zeros((5, 2), np.float32)
    acc = np.ones((5, 2), np.float32)
    v = np.array([[1, 2], [3, 4], [5, 6]], np.float32)
    (w2, a2), latched = ref.upsert([w, acc], 5, [4, 0, 2], [v, 10 * v])
    assert not latched
    assert w2.tolist() == [[3, 4], [0, 0], [5, 6], [0, 0], [1, 2]]
    assert a2.tolist() == [[30, 40], [1, 1], [50, 60], [1, 1], [10, 20]]
    assert w.tolist() == [[0, 0]] * 5
    # out of range: skipped and latched; past the count: not looked at
    (w2,), latched = ref.upsert([w], 5, [5, 1, -1], [v])
    assert latched and w2.tolist() == [[0, 0], [3, 4], [0, 0], [0, 0], [0, 0]]
    (w2,), latched = ref.upsert([w], 5, [1, 1 << 40], [v[:2]], n_dev=1)
    assert not latched and w2[1].tolist() == [1, 2]


def test_full_and_delta_tensors():
    w = np.arange(6, dtype=np.float32).reshape(3, 2)
    acc = w + 100
    cnt = np.array([7, 8, 9], np.int64)
    full = ref.full_tensors("t", w, [("AdagradDecay", acc), ("AdagradDecay_1", cnt)])
    assert sorted(full) == ["t", "t/AdagradDecay", "t/AdagradDecay_1"]
    assert full["t"].shape == (3, 2) and full["t/AdagradDecay_1"].tolist() == [7, 8, 9]
    bits = ref.mark(ref.new_bits(3), 3, [2, 0])
    d = ref.delta_tensors("t", bits, w, [("AdagradDecay", acc), ("AdagradDecay_1", cnt)])
    assert sorted(d) == ["t-sparse_incr_keys", "t-sparse_incr_values",
                         "t/AdagradDecay-sparse_incr_keys", "t/AdagradDecay-sparse_incr_values",
                         "t/AdagradDecay_1-sparse_incr_keys",
                         "t/AdagradDecay_1-sparse_incr_values"]
    for k in d:
        if k.endswith("keys"):
            assert d[k].tolist() == [0, 2] and d[k].dtype == np.int64
    assert d["t-sparse_incr_values"].tolist() == [[0, 1], [4, 5]]
    assert d["t/AdagradDecay-sparse_incr_values"].tolist() == [[100, 101], [104, 105]]
    assert d["t/AdagradDecay_1-sparse_incr_values"].tolist() == [7, 9]
