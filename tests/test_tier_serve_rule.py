"""tier_rows_served (kv_variable_ops), the one rule by which a read-only lookup
serves a row out of the host tier -- sparse_read(read_only=True) and the pooled
lookups of read_only_lookups(serve_tier=True) both call it -- against a dict
model, numpy only: the primary's and the column's first-touch bit in the
stored colmask, bit 16 (DR_TIER_UPDATED) and every other bit ignored, and for
a Counter EV the stored freq >= filter_freq."""
import numpy as np
import pytest

from deeprec_amd.kv_variable_ops import tier_rows_served

UPDATED = 1 << 16


def model(entry, col, filter_freq):
    """entry: {"touched": set of columns, "freq": int, "updated": bool}."""
    if 0 not in entry["touched"] or col not in entry["touched"]:
        return False
    return not filter_freq or entry["freq"] >= filter_freq


def pack(entries):
    cm = np.array([sum(1 << c for c in e["touched"]) | (UPDATED if e["updated"] else 0)
                   for e in entries], np.uint32)
    return cm, np.array([e["freq"] for e in entries], np.int64)


@pytest.mark.parametrize("col", [0, 1, 2, 15])
@pytest.mark.parametrize("filter_freq", [0, 2, 5])
def test_rule_matches_the_dict_model(col, filter_freq):
    entries = []
    for touched in (set(), {0}, {col}, {0, col}, {0, 1}, {0, 1, 2}, {1, 2}, set(range(16)),
                    set(range(1, 16)), set(range(16)) - {col}):
        for freq in (0, 1, filter_freq - 1, filter_freq, filter_freq + 1, 1 << 40):
            for updated in (False, True):
                entries.append({"touched": touched, "freq": max(freq, 0), "updated": updated})
    cm, fr = pack(entries)
    got = tier_rows_served(cm, fr, col, filter_freq)
    assert got.dtype == np.bool_ and got.shape == (len(entries),)
    want = np.array([model(e, col, filter_freq) for e in entries])
    assert np.array_equal(got, want)
    assert want.any() and not want.all()


def test_primary_and_slot_bits():
    cm = np.array([0b00, 0b01, 0b10, 0b11], np.uint32)
    fr = np.zeros(4, np.int64)
    assert tier_rows_served(cm, fr, 0, 0).tolist() == [False, True, False, True]
    # a slot column: its own bit AND the primary's
    assert tier_rows_served(cm, fr, 1, 0).tolist() == [False, False, False, True]


def test_updated_bit_is_ignored():
    cm = np.array([UPDATED, UPDATED | 1, 1, UPDATED | 0b11, UPDATED | 0b10], np.uint32)
    fr = np.full(5, 9, np.int64)
    assert tier_rows_served(cm, fr, 0, 0).tolist() == [False, True, True, True, False]
    assert tier_rows_served(cm, fr, 1, 3).tolist() == [False, False, False, True, False]


def test_counter_threshold():
    cm = np.full(4, 1, np.uint32)
    fr = np.array([0, 1, 2, 3], np.int64)           # filter_freq - 2 .. filter_freq + 1
    assert tier_rows_served(cm, fr, 0, 2).tolist() == [False, False, True, True]
    assert tier_rows_served(cm, fr, 0, 0).tolist() == [True] * 4       # no filter: freq unread
    assert tier_rows_served(cm, np.array([4, 5, 4, 5], np.int64), 0, 5).tolist() == \
        [False, True, False, True]
    # empty input
    assert tier_rows_served(np.empty(0, np.uint32), np.empty(0, np.int64), 0, 2).shape == (0,)
