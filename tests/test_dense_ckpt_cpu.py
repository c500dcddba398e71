"""Full save and restore of the dense kinds on CPU tensors (no GPU): a
DenseTable, a MultiHashVariable with device="cpu", their optimizer slots and
Adam's scalars go into one bundle, are read back with BundleReader (keys,
dtypes, shapes, values), restore into fresh objects, and the refusals of
restore leave every target untouched.  An EV-free call; the EV paths and the
marks need the GPU (tests/test_gpu_dense_ckpt.py)."""
import numpy as np
import pytest
import torch

import dense_ckpt_ref as ref


@pytest.fixture(scope="module")
def dr():
    import deeprec_amd as dr
    dr.load()
    return dr


def _model(dr, seed, name):
    g = torch.Generator().manual_seed(seed)
    table = dr.DenseTable(torch.randn(37, 6, generator=g), name=name + "/bucket")
    mhv = dr.get_multihash_variable(
        name + "/mh", [[5, 4], [7, 4]],
        initializer=[torch.randn(5, 4, generator=g), torch.randn(7, 4, generator=g)],
        device="cpu")
    return {"bucket": table, "mh": mhv}


def _state(variables, opt):
    out = dict(variables)
    out.update(opt.checkpoint_variables(variables))
    return out


def _arrays(dr, state):
    """{tensor key: numpy} of everything a state dict names."""
    from deeprec_amd import checkpoint as ck
    out = {}
    for k, v in ck.expand_variables(state).items():
        out[k] = np.float32(v.get()) if hasattr(v, "get") else v.weight.numpy().copy()
    return out


def test_expand_variables(dr):
    from deeprec_amd import checkpoint as ck
    m = _model(dr, 1, "a")
    e = ck.expand_variables(m)
    assert list(e) == ["bucket", "mh/Q", "mh/R"]
    assert e["mh/Q"] is m["mh"].val_list[0] and e["mh/R"] is m["mh"].val_list[1]
    assert e["mh/Q"].name == "a/mh/Q"
    with pytest.raises(TypeError):
        ck.expand_variables({"x": torch.zeros(2, 2)})
    with pytest.raises(dr.InvalidArgumentError):
        ck.expand_variables({"mh": m["mh"], "mh/Q": m["bucket"]})
    assert dr.DenseTable(torch.zeros(2, 2)).name is None
    assert dr.DenseTable(torch.zeros(2, 2), "n").name == "n"


def test_checkpoint_variables_names_and_initial_values(dr):
    m = _model(dr, 2, "b")
    want = {
        dr.GradientDescentOptimizer(0.1): [],
        dr.AdagradOptimizer(0.1, initial_accumulator_value=0.25): ["Adagrad"],
        dr.AdamOptimizer(0.1): ["Adam", "Adam_1"],
        dr.FtrlOptimizer(0.1, initial_accumulator_value=0.5): ["Ftrl", "Ftrl_1"],
        dr.AdamAsyncOptimizer(0.1): ["AdamAsync", "AdamAsync_1"],
        dr.AdagradDecayOptimizer(0.1, global_step=0): ["AdagradDecay", "AdagradDecay_1"],
    }
    for opt, slots in want.items():
        st = opt.checkpoint_variables(m)
        keys = ["%s/%s" % (k, s) for k in ("bucket", "mh/Q", "mh/R") for s in slots]
        if isinstance(opt, dr.AdamOptimizer):
            keys += ["beta1_power", "beta2_power"]
        if isinstance(opt, dr.AdamAsyncOptimizer):
            keys += ["%s/beta%d_power" % (k, i) for k in ("bucket", "mh/Q", "mh/R")
                     for i in (1, 2)]
        assert sorted(st) == sorted(keys), type(opt).__name__
        # the same objects on a second call: the state is created once
        again = opt.checkpoint_variables(m)
        for k in st:
            if hasattr(st[k], "weight"):
                assert st[k].weight is again[k].weight, k
    st = dr.AdagradOptimizer(0.1, initial_accumulator_value=0.25).checkpoint_variables(m)
    assert st["bucket/Adagrad"].table is m["bucket"]
    assert torch.equal(st["bucket/Adagrad"].weight, torch.full((37, 6), 0.25))
    st = dr.AdagradDecayOptimizer(0.1, global_step=0).checkpoint_variables(m)
    assert st["mh/R/AdagradDecay_1"].weight.dtype == torch.int64
    assert tuple(st["mh/R/AdagradDecay_1"].weight.shape) == (7,)
    st = dr.AdamOptimizer(0.1, beta1=0.75, beta2=0.5).checkpoint_variables(m)
    assert st["beta1_power"].get() == 0.75 and st["beta2_power"].get() == 0.5
    st = dr.AdamAsyncOptimizer(0.1, beta1=0.75, beta2=0.5).checkpoint_variables(m)
    assert st["mh/Q/beta1_power"].get() == 0.75 and st["mh/Q/beta2_power"].get() == 0.5


def test_full_save_round_trip(dr, tmp_path):
    from deeprec_amd import checkpoint as ck
    m = _model(dr, 3, "c")
    opt = dr.AdamOptimizer(0.01)
    state = _state(m, opt)
    # a state that is not the initial one
    g = torch.Generator().manual_seed(9)
    for k, v in opt.checkpoint_variables(m).items():
        if hasattr(v, "weight"):
            v.weight.copy_(torch.randn(v.weight.shape, generator=g))
    opt._finish()
    opt._finish()
    b1p, b2p = opt.b1p, opt.b2p
    assert b1p == float(np.float32(0.9) * np.float32(0.9) * np.float32(0.9))
    before = _arrays(dr, state)
    prefix = ck.save(str(tmp_path / "full"), state)

    r = ck.BundleReader(prefix)
    want = {}
    for key in ("bucket", "mh/Q", "mh/R"):
        want.update(ref.full_tensors(key, before[key], [(s, before[key + "/" + s])
                                                        for s in ("Adam", "Adam_1")]))
    want["beta1_power"], want["beta2_power"] = np.float32(b1p), np.float32(b2p)
    assert r.keys() == sorted(want)
    for k, a in want.items():
        assert r.dtype_and_shape(k) == (np.dtype(np.float32), tuple(np.shape(a))), k
        assert r.entries[k]["slices"] == 0, k
        np.testing.assert_array_equal(r.lookup(k), a, err_msg=k)
    assert r.dtype_and_shape("beta1_power")[1] == ()
    assert r.dtype_and_shape("mh/R/Adam_1")[1] == (7, 4)

    m2 = _model(dr, 4, "d")
    opt2 = dr.AdamOptimizer(0.01)
    state2 = _state(m2, opt2)
    ck.restore(prefix, state2)
    after = _arrays(dr, state2)
    assert sorted(after) == sorted(before)
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    assert (opt2.b1p, opt2.b2p) == (b1p, b2p)
    # the source is left as it was
    for k, a in _arrays(dr, state).items():
        np.testing.assert_array_equal(a, before[k], err_msg=k)


def test_int64_slot_round_trip(dr, tmp_path):
    from deeprec_amd import checkpoint as ck
    m = {"bucket": _model(dr, 5, "e")["bucket"]}
    opt = dr.AdagradDecayOptimizer(0.1, global_step=0)
    st = _state(m, opt)
    st["bucket/AdagradDecay_1"].weight.copy_(torch.arange(37))
    prefix = ck.save(str(tmp_path / "dec"), st)
    r = ck.BundleReader(prefix)
    assert r.dtype_and_shape("bucket/AdagradDecay_1") == (np.dtype(np.int64), (37,))
    m2 = {"bucket": _model(dr, 6, "f")["bucket"]}
    opt2 = dr.AdagradDecayOptimizer(0.1, global_step=0)
    st2 = _state(m2, opt2)
    ck.restore(prefix, st2)
    assert torch.equal(st2["bucket/AdagradDecay_1"].weight, torch.arange(37))
    assert torch.equal(st2["bucket/AdagradDecay"].weight, st["bucket/AdagradDecay"].weight)
    assert torch.equal(m2["bucket"].weight, m["bucket"].weight)


def test_restore_refusals_leave_the_targets_untouched(dr, tmp_path):
    from deeprec_amd import _lib as L
    from deeprec_amd import checkpoint as ck
    m = _model(dr, 7, "g")
    opt = dr.AdamOptimizer(0.01)
    prefix = ck.save(str(tmp_path / "src"), _state(m, opt))

    def fresh(bucket_shape=(37, 6)):
        g = torch.Generator().manual_seed(11)
        v = {"mh": _model(dr, 8, "h")["mh"],
             "bucket": dr.DenseTable(torch.randn(*bucket_shape, generator=g))}
        o = dr.AdamOptimizer(0.01)
        o.b1p = 0.125
        return v, o

    def untouched(fn, state, o):
        before = _arrays(dr, state)
        with pytest.raises(L.DeepRecError) as e:
            fn()
        after = _arrays(dr, state)
        for k in before:
            np.testing.assert_array_equal(after[k], before[k], err_msg=k)
        assert o.b1p == 0.125
        return e.value

    # a shape mismatch on the LAST-named variable: the earlier ones stay as they were
    v, o = fresh((37, 8))
    st = _state(v, o)
    err = untouched(lambda: ck.restore(prefix, st), st, o)
    assert isinstance(err, dr.InvalidArgumentError) and "bucket" in str(err)
    v, o = fresh((36, 6))
    st = _state(v, o)
    assert isinstance(untouched(lambda: ck.restore(prefix, st), st, o), dr.InvalidArgumentError)
    # a dtype mismatch: the float table's entry offered to an int64 slot
    v, o = fresh()
    st = _state(v, o)
    st["bucket"] = type(st["bucket/Adam"])(v["bucket"], torch.zeros(37, 6, dtype=torch.int64))
    err = untouched(lambda: ck.restore(prefix, st), st, o)
    assert isinstance(err, dr.InvalidArgumentError)
    # a missing key: NOT_FOUND
    v, o = fresh()
    st = _state(v, o)
    st["other"] = dr.DenseTable(torch.ones(3, 2))
    err = untouched(lambda: ck.restore(prefix, st), st, o)
    assert err.code == L.NOT_FOUND and "other" in str(err)
    # a scalar missing from the bundle (saved without the optimizer's state)
    bare = ck.save(str(tmp_path / "bare"), m)
    v, o = fresh()
    st = _state(v, o)
    assert untouched(lambda: ck.restore(bare, st), st, o).code == L.NOT_FOUND
    # and the matching call goes through
    v, o = fresh()
    st = _state(v, o)
    ck.restore(prefix, st)
    assert torch.equal(v["bucket"].weight, m["bucket"].weight) and o.b1p == opt.b1p


def test_tracking_is_refused_with_the_reason(dr):
    t = dr.DenseTable(torch.zeros(4, 4), name="cold")
    assert not t.tracking_updates()
    with pytest.raises(dr.InvalidArgumentError, match="cold.*cpu"):
        t.track_updates()
    t.track_updates(False)          # turning it off is always allowed
    assert not t.tracking_updates()
    from deeprec_amd import checkpoint as ck
    with pytest.raises(dr.InvalidArgumentError, match="cold.*not tracking"):
        ck.save_incremental("/nonexistent/never-written", {"k": t})
