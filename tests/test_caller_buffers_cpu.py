"""CPU: the tools of tests/test_gpu_caller_buffers.py (tests/device_views.py) do what they say -- the alignments asked for, a band check that
sees one flipped element -- and THE POISON HAS TEETH: for every model and every cut point of the GPU test, the oracle's prediction on the rows a
kernel would see that read the first 8 poison pairs behind the arrays' end differs from the clean one (the poison ids hit weighted features of the
beam's parents), and so does a dense row read one element early or late.  No case is skipped: one that stops differing has to be replaced."""
import os

import numpy as np
import pytest
import scipy.sparse as smat

import device_views as V
from conftest import GOLDEN, load_X

MODELS = ("s_eurlex", "s_deep", "s_wide", "s_flat", "odd_d")
ODD_D = dict(D=601, L=300, w_nnz=[100, 60, 12], seed=47, shape=[4, 24, 300])     # D % 4 == 1, D % 64 != 0


def model_case(name, tmp_root):
    """(model folder, golden X or seeded queries) of a model of the caller-buffer tests."""
    import xrl_synth
    if name != "odd_d":
        return os.path.join(GOLDEN, "synth", name), load_X(os.path.join(GOLDEN, "synth", name + "__X.npz"))
    folder = os.path.join(str(tmp_root), "odd_d")
    if not os.path.isdir(folder):
        xrl_synth.make_model(folder, ODD_D["D"], ODD_D["L"], ODD_D["w_nnz"], seed=ODD_D["seed"], shape=ODD_D["shape"])
    X = xrl_synth.make_queries(40, ODD_D["D"], 30, seed=48).astype(np.float32)
    X.sort_indices()
    return folder, X


@pytest.mark.parametrize("dtype,per16", [(np.float32, 4), (np.int32, 4), (np.int64, 2)])
def test_banded_gives_the_requested_alignment(dtype, per16):
    import torch
    a = (np.arange(37) + 3).astype(dtype)
    for off in range(2 * per16 + 1):
        for band in (0, 1, 5, 64):
            whole, pay = V.banded(a, off, band, dtype(9))
            assert pay.data_ptr() % 16 == (a.itemsize * off) % 16 and V.addr(pay) == pay.data_ptr()
            sl = V.payload_slice(whole, pay)
            assert sl.start >= band and whole.numel() - sl.stop == band and sl.stop - sl.start == a.size
            assert np.array_equal(whole[sl].numpy(), a) and np.array_equal(pay.numpy(), a)
            assert bool((whole[: sl.start] == 9).all()) and bool((whole[sl.stop:] == 9).all())
    # a 2-D array keeps its shape; a tensor goes in as it is; an empty payload is a valid view
    whole, pay = V.banded(np.arange(12, dtype=np.float32).reshape(3, 4), 3, 8, V.poison_like("value"))
    assert pay.shape == (3, 4) and pay.is_contiguous() and bool(torch.isnan(whole[:8]).all()) and bool(torch.isnan(whole[-8:]).all())
    whole, pay = V.banded(torch.zeros(0, dtype=torch.int32), 1, 4, V.poison_like("index", 3))
    assert pay.numel() == 0 and V.addr(pay) % 16 == 4 and whole[-4:].tolist() == [0, 1, 2, 0]


def test_poison_fills():
    D = 7
    whole, pay = V.banded(np.array([5, 6], np.int32), 2, 10, V.poison_like("index", D))
    sl = V.payload_slice(whole, pay)
    assert whole[sl.stop:].tolist() == [i % D for i in range(10)]                # the back band starts the cycle: the first pairs past the end are ids 0, 1, ...
    assert int(whole.min()) >= 0 and int(whole.max()) < D                       # never an id outside the model
    assert np.isnan(V.poison_like("value")) and (np.float32(V.poison_like("value")).view(np.uint32) & 0x7FC00000) == 0x7FC00000   # quiet
    assert V.poison_like("rowptr") == 0


def test_band_check_catches_one_flipped_element():
    for a, fill in ((np.arange(20, dtype=np.float32), V.poison_like("value")), (np.arange(20, dtype=np.int32), V.poison_like("index", 11)),
                    (np.arange(20, dtype=np.int64), V.poison_like("rowptr")), (np.arange(20, dtype=np.float32), np.float32(V.SENT_VAL))):
        whole, pay = V.banded(a, 1, 16, fill)
        V.assert_bands_intact(whole, pay, fill)
        V.assert_bands_intact(whole, V.payload_slice(whole, pay), fill)
        pay += 1                                                                 # the payload may change
        V.assert_bands_intact(whole, pay, fill)
        sl = V.payload_slice(whole, pay)
        for pos in (0, sl.start - 1, sl.stop, whole.numel() - 1):
            keep = whole[pos].clone()
            if a.dtype == np.float32:                                            # one bit of the element: NaN payload bits count too
                whole[pos: pos + 1].view(__import__("torch").int32)[0] ^= 1
            else:
                whole[pos] += 1
            with pytest.raises(AssertionError, match="band"):
                V.assert_bands_intact(whole, pay, fill)
            whole[pos] = keep
            V.assert_bands_intact(whole, pay, fill)


@pytest.mark.parametrize("model", MODELS)
def test_the_poison_has_teeth(model, oracle_mod, tmp_path):
    folder, X = model_case(model, tmp_path)
    om = oracle_mod.OracleModel.load(folder)
    Xt, cuts = V.with_tails(X)
    assert [int(n) for n in np.diff(Xt.indptr)[-8:]] == list(V.TAIL_LENGTHS) and len(cuts) == 8
    kw = dict(beam_size=10, only_topk=10)
    clean = om.predict(Xt, **kw)
    for R in cuts:
        bad = om.predict(V.poisoned_rows(Xt, R), **kw)
        assert not V.differs(bad[: R - 1], clean[: R - 1])                       # (the rows before it are what they were)
        assert V.differs(bad[R - 1: R], clean[R - 1: R]), f"{model}: cut {R}: 8 poison pairs behind row {R - 1} leave its prediction as it is"
    # dense X: the last row read one element early / late (an address rounded to 16 bytes, a row stride off by one) takes a NaN in
    Xd = np.ascontiguousarray(Xt.toarray())
    cd = om.predict(Xd, **kw)
    r = Xd.shape[0] - 1
    for by in (-1, 1, 3):
        Xb = Xd.copy(); Xb[r] = V.shifted_dense_row(Xd[r], by)
        assert V.differs(om.predict(Xb, **kw)[r: r + 1], cd[r: r + 1]), f"{model}: dense row {r} shifted by {by}"
