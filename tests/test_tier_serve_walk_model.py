"""The serving walk of tests/tier_serve_walk.py is not vacuous (CPU, numpy only):
on the dict model alone, every seed of tests/test_gpu_tier_serve.py's walk
serves at least 200 ids out of the tier, at least 20 ids the tier holds but
the Counter rule keeps at the default, and at least 20 ids nobody has seen --
conditions on the inputs, stated before any GPU time is spent."""
import numpy as np
import pytest

import tier_serve_walk as S


@pytest.mark.parametrize("seed", S.SEEDS)
def test_walk_serves_from_the_tier(seed):
    ops, counts = S.walk(seed)
    assert counts[S.SERVED] >= 200, counts
    assert counts[S.FILTERED] >= 20, counts
    assert counts[S.NEVER] >= 20, counts
    assert counts[S.HBM] >= 20, counts
    serves = [o for o in ops if o["op"] == "serve"]
    assert len(serves) == 4 * S.ROUNDS
    assert {o["kind"] for o in serves} == {"onehot", "bags"}
    assert {o["combiner"] for o in serves if o["kind"] == "bags"} == set(S.COMBINERS)
    for o in serves:
        assert o["values"].dtype == np.int64 and o["values"].size == o["indices"].shape[0]
        # every serving batch has ids of the tier, and duplicates
        assert (o["classes"] == S.SERVED).sum() >= 10
        assert np.unique(o["values"]).size < o["values"].size or o["kind"] == "onehot"
        if o["kind"] == "bags":
            lens = np.bincount(o["indices"][:, 0], minlength=S.BAGS)
            assert lens.min() == 0 and lens.max() == 5
    # the four special keys are served out of the tier at least once
    special = set(S.SPECIAL.tolist())
    hit = set()
    for o in serves:
        hit |= {k for k, c in zip(o["values"].tolist(), o["classes"].tolist())
                if k in special and c == S.SERVED}
    assert hit == special
    # the same seed gives the same walk
    again, _ = S.walk(seed)
    assert all(np.array_equal(a.get("values", a.get("keys", 0)), b.get("values", b.get("keys", 0)))
               for a, b in zip(ops, again))
