"""The walk of tests/test_gpu_host_tier.py::test_tiered_walk_equals_twin and a
dict model of what an LRU-budgeted, tiered key space does with it.

Not a test module and numpy only: tests/test_host_tier_walk_model.py checks on
the CPU that the walk promotes often enough to prove anything, the GPU test
runs the same batches on a tiered EV and its untiered, unbudgeted twin.
"""
import numpy as np

import ev_lifecycle as L

STEPS = 48
BUDGET = 600            # demote_to(BUDGET) ...
DEMOTE_EVERY = 4        # ... after every 4th step
SHRINK_EVERY = 16       # shrink(step) after every 16th
STEPS_TO_LIVE = 20
HOT = 250               # keys that come back all the time
INSERT_AT, REMOVE_AT = 21, 30
I64MAX = np.iinfo(np.int64).max


def batches(seed):
    """48 batches of <= 400 keys, duplicates included: half of a batch from
    the HOT keys, half from the whole universe (about 2 500 keys, the four
    special ones, the clustered groups), so that keys demoted long ago
    return; every few steps a whole clustered group, groups[0] first."""
    uni = L.universe(seed)
    rng = np.random.default_rng([seed, 7])
    hot = rng.choice(uni.keys, HOT, replace=False)
    out = []
    for step in range(STEPS):
        n = int(rng.integers(200, 361))
        parts = [rng.choice(hot, n // 2), rng.choice(uni.keys, n - n // 2)]
        if step % 5 == 0:
            parts.append(uni.groups[(step // 5) % len(uni.groups)])
        if step % 7 == 0:
            parts.append(np.array([-1, 0, L.I64MIN, L.I64MAX], np.int64))
        keys = rng.permutation(np.concatenate(parts))[:L.MAX_BATCH]
        out.append(keys.astype(np.int64))
    return out


def grads(seed, step, n):
    """Integer gradients: with LR 0.5 every value stays a multiple of 0.5 and
    within +-48 of the default over 48 steps, exact in bf16 too."""
    rng = np.random.default_rng([seed, 8, step])
    return rng.integers(-2, 3, (n, L.DIM)).astype(np.float32)


def lru_model(seed):
    """Replays the walk on (version per key, which tier holds it): a lookup
    promotes the batch's keys the tier holds and creates the absent ones
    (version 0), the apply stamps version = step, demote_to(BUDGET) moves the
    first N - BUDGET keys by (version, key) to the tier, shrink(step) drops
    step - version > STEPS_TO_LIVE from both tiers.  Returns the promotions
    per step and the step of the first demotion."""
    hbm, tier = {}, {}
    promoted, first = [], None
    for step, keys in enumerate(batches(seed)):
        p = 0
        for k in np.unique(keys).tolist():
            if k in tier:
                hbm[k] = tier.pop(k)
                p += 1
            hbm[k] = step       # created, then stamped by the apply
        promoted.append(p)
        if (step + 1) % DEMOTE_EVERY == 0 and len(hbm) > BUDGET:
            order = sorted(hbm, key=lambda k: (hbm[k], k))
            for k in order[:len(hbm) - BUDGET]:
                tier[k] = hbm.pop(k)
            first = step if first is None else first
        if (step + 1) % SHRINK_EVERY == 0:
            for d in (hbm, tier):
                for k in [k for k, v in d.items() if step - v > STEPS_TO_LIVE]:
                    del d[k]
    return promoted, first
