"""The tiered walk is not vacuous (CPU, numpy only): over the seeds of
tests/test_gpu_host_tier.py::test_tiered_walk_equals_twin a dict model of an
LRU-budgeted, tiered key space promotes at least 200 keys, and promotes in at
least half of the steps after the first demotion.  The GPU test asserts the
same on the real EVs; this one says so before any GPU time is spent."""
import numpy as np
import pytest

import host_tier_walk as W


@pytest.mark.parametrize("seed", [21, 22, 23, 24, 25])
def test_walk_promotes(seed):
    promoted, first = W.lru_model(seed)
    assert first is not None and first < 8
    after = promoted[first + 1:]
    assert sum(promoted) >= 200, sum(promoted)
    assert sum(1 for p in after if p) * 2 >= len(after)
    b = W.batches(seed)
    assert len(b) == W.STEPS and all(k.size <= 400 for k in b)
    assert any(np.unique(k).size < k.size for k in b)       # duplicates inside a batch
