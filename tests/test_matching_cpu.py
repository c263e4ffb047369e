"""Matcher-aware negatives without a GPU: the numpy statement of the union rule against scipy's M += binarized(...); the chain loop of
tests/matching_rule.py over the live reference (where oracle/_ref is built) against tests/golden/man_training_ref.npz; the preconditions
of that fixture; every refusal of xrl_smat_pattern_union_device and xrl_single_layer_predict_device that needs no GPU; the Python
surface."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as smat

import matching_rule as mr
import ranker_training_rule as rr
from conftest import GOLDEN

RECORDED = np.load(os.path.join(GOLDEN, "man_training_ref.npz"))
TFN = np.load(os.path.join(GOLDEN, "ranker_training_ref.npz"))
CONFIGS = [(s, p) for s in mr.SCHEMES for p in mr.POST]


# ------------------------------------------------------------------------------------------------ the union
@pytest.mark.parametrize("name", sorted(mr.union_cases()))
def test_numpy_union_equals_scipys_sum_of_binarized(name):
    mats = mr.union_cases()[name]
    got = mr.union(mats)
    M = smat.csc_matrix(mats[0].shape, dtype=np.float32)
    for A in mats:
        B = smat.csr_matrix(A.shape, dtype=np.float32)                    # binarized(A): the stored entries, explicit zeros and NaN included, as ones
        B.indptr, B.indices, B.data = A.indptr.copy(), A.indices.copy(), np.ones(len(A.indices), np.float32)
        M += smat.csc_matrix(B)
    M = smat.csr_matrix(M)
    M.sort_indices()
    assert mr.same_pattern(got, M), name
    assert np.all(got.data.view(np.uint32) == np.float32(1).view(np.uint32))
    for r in range(got.shape[0]):
        assert np.all(np.diff(got.indices[got.indptr[r]:got.indptr[r + 1]]) > 0), "a row is not strictly ascending"


def test_union_cases_hold_what_they_promise():
    dup = mr.duplicates_case()[0]
    r1 = dup.indices[dup.indptr[1]:dup.indptr[2]]
    assert (r1 == 11).sum() == 66 and np.isnan(dup.data).any() and (dup.data == 0).any() and (dup.data < 0).any()
    a, b = mr.interleaved_case()
    u = mr.union([a, b])
    assert u.nnz == 201 and 63 in b.indices and 64 in b.indices
    tot = mr.totals_case(3)
    assert [int(sum(A.indptr[r + 1] - A.indptr[r] for A in tot)) for r in range(len(mr.TOTALS))] == list(mr.TOTALS)


# ------------------------------------------------------------------------------------------------ the fixture
def test_fixture_preconditions():
    depth = int(RECORDED["depth"][0])
    assert depth == 3 and [c.shape for c in mr.recorded_chain(RECORDED)] == [(2, 1), (8, 2), (64, 8)]
    X, Y, C = rr.e2e_problem()
    chain = mr.recorded_chain(RECORDED)
    Ys = [smat.csc_matrix(Y)]
    for Cm in reversed(chain[1:]):
        Ys.append(smat.csc_matrix(Ys[-1].tocsr() * Cm.tocsr()))
    Ys.reverse()
    for post in mr.POST:
        both, man = mr.recorded_config(RECORDED, "tfn+man", post), mr.recorded_config(RECORDED, "man", post)
        assert both["M"][0] is None and both["M_pred"][0] is None
        outside = 0
        for t in (1, 2):
            tfn = mr.union([smat.csr_matrix(Ys[t - 1])])
            assert smat.csr_matrix(both["M"][t]).nnz > tfn.nnz, "man adds no entry to M"
            assert mr.same_pattern(smat.csr_matrix(man["M"][t]), mr.union([smat.csr_matrix(man["M_pred"][t])])), "man alone: M is the prediction"
            # a positive outside its M column: an instance of a label whose cluster the prediction does not list for it
            # (layer 1's prediction lists both clusters for every instance: the beam is as wide as the layer; layer 2's does not)
            Yt, Ct, Mt = Ys[t].tocsc(), chain[t].tocsc(), man["M"][t].tocsc()
            for k in range(Ct.shape[1]):
                listed = set(Mt.indices[Mt.indptr[k]:Mt.indptr[k + 1]])
                for lab in Ct.indices[Ct.indptr[k]:Ct.indptr[k + 1]]:
                    outside += sum(1 for i in Yt.indices[Yt.indptr[lab]:Yt.indptr[lab + 1]] if i not in listed)
            recorded_tfn = smat.csc_matrix((TFN[f"e2e__{t}__W__data"], TFN[f"e2e__{t}__W__indices"], TFN[f"e2e__{t}__W__indptr"]), shape=tuple(TFN[f"e2e__{t}__W__shape"]))
            if post == "l3-hinge":
                assert not mr.same_bits(both["W"][t], recorded_tfn), "man does not change the layer's weights"
        assert outside > 0, "under man alone no job has a positive outside its M column"
        W0 = smat.csc_matrix((TFN["e2e__0__W__data"], TFN["e2e__0__W__indices"], TFN["e2e__0__W__indptr"]), shape=tuple(TFN["e2e__0__W__shape"]))
        assert mr.same_bits(both["W"][0], W0), "layer 0 is unchanged by man"
    # the per-layer list trains layer 1 as tfn does
    per = mr.recorded_config(RECORDED, "perlayer", "l3-hinge")
    W1 = smat.csc_matrix((TFN["e2e__1__W__data"], TFN["e2e__1__W__indices"], TFN["e2e__1__W__indptr"]), shape=tuple(TFN["e2e__1__W__shape"]))
    assert mr.same_bits(per["W"][1], W1)
    assert os.path.getsize(os.path.join(GOLDEN, "man_training_ref.npz")) < 512 * 1024


@pytest.mark.parametrize("threads", [1, 8])
@pytest.mark.parametrize("scheme,post", CONFIGS)
def test_chain_loop_over_the_live_reference_equals_the_recording(scheme, post, threads):
    if not mr.refpy_available():
        pytest.skip("oracle/_ref (the compiled reference and its python package) is not built")
    X, Y, _ = rr.e2e_problem()
    predict_layer, train_layer = mr.reference_backend(threads)
    names = mr.SCHEMES[scheme]
    schemes = names if isinstance(names, list) else [names] * 3
    got = mr.chain_loop(X, Y, mr.recorded_chain(RECORDED), schemes, predict_layer, train_layer, mr.layer_pred_params(post),
                        matching_chain=mr.usn_chain() if "usn" in scheme else None)
    want = mr.recorded_config(RECORDED, scheme, post)
    for t in range(3):
        assert mr.same_bits(got["W"][t], want["W"][t]), f"layer {t}: W"
        assert (got["M"][t] is None) == (want["M"][t] is None) and (want["M"][t] is None or mr.same_pattern(got["M"][t], want["M"][t])), f"layer {t}: M"
        assert (got["M_pred"][t] is None) == (want["M_pred"][t] is None)
        if want["M_pred"][t] is not None:
            assert mr.same_bits(smat.csr_matrix(got["M_pred"][t]), want["M_pred"][t]), f"layer {t}: M_pred"


# ------------------------------------------------------------------------------------------------ refusals that need no GPU
def _fake(lib, device, rows, cols, nnz=3):
    """A wrapped handle around addresses that are never read: the refusals under test come before any data is touched."""
    lib.xrl_smat_from_device_csr.restype = ctypes.c_void_p
    lib.xrl_smat_from_device_csr.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    h = lib.xrl_smat_from_device_csr(device, rows, cols, 0x1000, 0x1000, 0x1000, nnz)
    assert h
    return h


def test_union_refusals_need_no_gpu():
    lib = rr.load(rr.OURS)
    fn = lib.xrl_smat_pattern_union_device
    fn.restype, fn.argtypes = ctypes.c_void_p, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_void_p]
    lib.xrl_smat_free.argtypes = [ctypes.c_void_p]
    start = "xrl_smat_pattern_union_device: "
    made = [_fake(lib, 0, 5, 7), _fake(lib, 0, 5, 8), _fake(lib, 0, 6, 7), _fake(lib, 1, 5, 7)]

    def refusal(handles, n=None):
        arr = (ctypes.c_void_p * max(1, len(handles)))(*handles)
        assert fn(arr, len(handles) if n is None else n, None) is None
        return rr.last_error(lib)

    try:
        assert refusal([], 0).startswith(start + "no operands")
        assert fn(None, 2, None) is None and rr.last_error(lib).startswith(start + "no operands")
        assert refusal([made[0], None]) == start + "null matrix handle (operand 1)"
        assert refusal([made[0], made[1]]) == start + "operand 1 has shape 5 x 8, operand 0 has 5 x 7"
        assert refusal([made[0], made[0], made[2]]) == start + "operand 2 has shape 6 x 7, operand 0 has 5 x 7"
        assert refusal([made[0], made[3]]).startswith(start + "the operands are on devices 0 and 1")
    finally:
        for h in made:
            lib.xrl_smat_free(h)


def test_predict_refusals_need_no_gpu():
    lib = rr.load(rr.OURS)
    fn = lib.xrl_single_layer_predict_device
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_float] + [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_void_p]
    lib.xrl_smat_free.argtypes = [ctypes.c_void_p]
    N, d, L, K = 30, 12, 6, 2
    x, wt, ct = _fake(lib, 0, N, d), _fake(lib, 0, L, d + 1), _fake(lib, 0, K, L)
    made = [x, wt, ct]
    start = "xrl_single_layer_predict_device: "
    buf = 0x1000                                                               # never written: every call below is refused first

    def refusal(X=x, Wt=wt, Ct=ct, codes=(None, None, None), c_stride=0, pp=b"l3-hinge", topk=5, bias=1.0, out=(buf, buf, buf), stride=5):
        assert fn(X, Wt, Ct, *codes, c_stride, pp, topk, bias, *out, stride, None) == -1
        return rr.last_error(lib)

    try:
        assert refusal(X=None) == start + "null matrix handle (X)"
        assert refusal(Wt=None) == start + "null matrix handle (Wt)"
        assert refusal(topk=0) == start + "only_topk must be positive"
        assert refusal(stride=4) == start + "out_stride (4) is smaller than only_topk (5)"
        assert refusal(out=(buf, None, buf)) == start + "null output buffer"
        assert refusal(codes=(buf, None, buf), c_stride=3).startswith(start + "csr_codes: labels, scores and counts come together")
        assert refusal(codes=(buf, buf, buf), c_stride=0) == start + "csr_codes: a stride of 0"
        wide, off, far = _fake(lib, 0, L, d + 2), _fake(lib, 0, K, L + 1), _fake(lib, 1, L, d + 1)
        made.extend((wide, off, far))
        assert refusal(Wt=wide).startswith(start + "Feature dimension of query and W do not match")
        assert refusal(bias=0.0).startswith(start + "Feature dimension of query and W do not match")
        assert refusal(Ct=off) == start + "Label dimension of C and W do not match (7 != 6)"
        assert refusal(Wt=far).startswith(start + "the operands are on devices 0 and 1")
    finally:
        for h in made:
            lib.xrl_smat_free(h)


def test_match_forms_needs_an_array():
    lib = rr.load(rr.OURS)
    lib.xrl_debug_match_forms.restype, lib.xrl_debug_match_forms.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]
    assert lib.xrl_debug_match_forms(None, 5) == -1 and rr.last_error(lib) == "xrl_debug_match_forms: null argument"
    out = (ctypes.c_uint64 * 5)()
    assert lib.xrl_debug_match_forms(out, 5) == 0


# ------------------------------------------------------------------------------------------------ the Python surface
def test_new_symbols_are_exported_and_bound():
    import pecos_amd
    from pecos_amd import DeviceMatrix, HierarchicalMLModel, MLModel, XLinearModel, clib
    for name in ("train_chain_device", "single_layer_predict_device"):
        assert name in pecos_amd.__all__ and callable(getattr(pecos_amd, name))
    assert callable(DeviceMatrix.pattern_union) and callable(HierarchicalMLModel.train_device) and callable(XLinearModel.train_device) and callable(MLModel.predict)
    for name in ("xrl_smat_pattern_union_device", "xrl_single_layer_predict_device", "xrl_debug_match_forms"):
        assert getattr(clib.clib_float32, name).argtypes is not None
    assert clib.MATCH_FORMS == ("lds_rows", "big_rows", "read", "written", "last_bound")
    header = open(os.path.join(rr.REPO, "include", "xrl_abi.h")).read()
    assert "void* xrl_smat_pattern_union_device(void* const* mats, uint32_t n, void* hip_stream);" in header
    assert "int xrl_debug_match_forms(uint64_t* out, uint32_t n);" in header


def _small():
    X, Y, C, M = rr.problem(30, 12, 6, 2, 3, 4, 3)
    return X, Y, C, M


def test_train_device_refuses_what_train_refuses_in_the_same_words():
    from pecos_amd import HierarchicalMLModel, XLinearModel
    from pecos_amd.xlinear import MLProblem
    X, Y, C, M = _small()
    for kw in (dict(mode="matcher"), dict(mode="ranker"), dict(rel_mode="induce"), dict(user_supplied_negatives={0: M})):
        with pytest.raises(NotImplementedError) as a:
            XLinearModel.train(X, Y, C=C, **kw)
        with pytest.raises(NotImplementedError) as b:
            XLinearModel.train_device(X, Y, C=C, **kw)
        assert str(a.value) == str(b.value) and "is not served on the device" in str(b.value)
    with pytest.raises(ValueError, match="the bottom clustering matrix has 6 rows, the problem 5 labels"):
        HierarchicalMLModel.train_device(MLProblem(X, Y[:, :5]), clustering=[smat.csc_matrix(np.ones((2, 1), dtype=np.float32)), C], negative_sampling_scheme="tfn+man")
    with pytest.raises(ValueError, match=r"len\(neg_mining_chain\)=3 != 2"):
        HierarchicalMLModel.train_device(MLProblem(X, Y), clustering=[smat.csc_matrix(np.ones((2, 1), dtype=np.float32)), C],
                                         train_params=dict(neg_mining_chain=["tfn", "man", "man"], model_chain=dict()))
    for features in (X, np.ascontiguousarray(X.toarray())):            # (dense X is served like sparse X: it meets the same refusals, none of its own)
        with pytest.raises(ValueError, match="pred_params is not valid"):
            HierarchicalMLModel.train_device(MLProblem(features, Y), clustering=[smat.csc_matrix(np.ones((2, 1), dtype=np.float32)), C], pred_kwargs=dict(post_processor="nope"))


def test_a_single_cluster_of_the_problems_own_that_is_not_everything_is_refused():
    """Without a clustering a problem's one cluster must hold every label and its M every instance: that is the pure form the loop trains."""
    from pecos_amd import HierarchicalMLModel
    from pecos_amd.xlinear import MLProblem
    X, Y, C, M = _small()
    part = smat.csc_matrix((np.ones(5, dtype=np.float32), np.arange(5), np.array([0, 5])), shape=(6, 1))
    some = smat.csc_matrix((np.ones(29, dtype=np.float32), np.arange(29), np.array([0, 29])), shape=(30, 1))
    for kw in (dict(C=part), dict(M=some)):
        for train in (HierarchicalMLModel.train, HierarchicalMLModel.train_device):
            with pytest.raises(NotImplementedError, match="whose single cluster leaves out a label, or whose M leaves out an instance"):
                train(MLProblem(X, Y, **kw))


def test_mlmodel_predict_refuses_a_wrong_feature_count():
    from pecos_amd import MLModel
    X, Y, C, M = _small()
    W = smat.csc_matrix(np.ones((13, 6), dtype=np.float32))
    layer = MLModel(W=W, C=C, bias=1.0)
    assert (layer.nr_features, layer.nr_labels, layer.nr_codes) == (12, 6, 2)
    with pytest.raises(ValueError, match="Feature dimension of query matrix does not match weight matrix"):
        layer.predict(X[:, :11])
    with pytest.raises(ValueError, match="pred_params is not valid"):
        layer.predict(X, post_processor="nope")
    assert layer.get_pred_params() == MLModel.PredParams() and layer.get_pred_params() is not layer.pred_params
