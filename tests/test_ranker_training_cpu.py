"""Ranker training (K13), the half that needs no GPU: the numpy statement of the rule (tests/ranker_training_rule.py) against the compiled
reference -- as recorded in tests/golden/ranker_training_ref.npz and, where oracle/_ref is built, live at 1 and 8 threads -- bit for
bit; the two wrong variants; the shuffle restatement against permutations recorded from std::shuffle; every refusal that needs no data
on the device; the Python surface."""
import ctypes
import os
import sys

import numpy as np
import pytest
import scipy.sparse as smat

import clustering_rule as cr
import ranker_training_rule as rr
from conftest import GOLDEN

REPO = rr.REPO
CASES = rr.cases()
RECORDED = np.load(os.path.join(GOLDEN, "ranker_training_ref.npz"))
HAVE_REF = os.path.exists(rr.REF)
_truth = {}


def truth(name):
    if name not in _truth:
        X, Y, C, M, R, kw = CASES[name]
        _truth[name] = rr.statement(X, Y, C, M, R, **kw)
    return _truth[name]


def recorded(name):
    return RECORDED[f"case__{name}__rows"].astype(np.uint64), RECORDED[f"case__{name}__cols"].astype(np.uint64), RECORDED[f"case__{name}__vals"]


def pinned_order(kw):
    """The order inside a label is pinned unless max_nonzeros_per_label leaves it to std::nth_element."""
    return not kw.get("max_nonzeros")


@pytest.mark.parametrize("name", sorted(CASES))
def test_statement_equals_the_recorded_reference(name):
    kw = CASES[name][5]
    assert rr.same_coo(truth(name), recorded(name), canon=not pinned_order(kw))


@pytest.mark.parametrize("name", sorted(CASES))
def test_statement_equals_the_live_reference_at_1_and_8_threads(name):
    if not HAVE_REF:
        pytest.skip("oracle/_ref not built")
    X, Y, C, M, R, kw = CASES[name]
    assert rr.same_coo(truth(name), rr.reference(X, Y, C, M, R, threads=1, **kw), canon=not pinned_order(kw))
    assert rr.same_coo(truth(name), rr.reference(X, Y, C, M, R, threads=8, **kw), canon=True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_statement_equals_the_reference_recorded_at_8_threads(name):
    """The reference at 8 threads returns the same weights in another order: its canonical COO, recorded as a digest, is the statement's."""
    assert rr.digest(truth(name)) == str(RECORDED[f"digest8__{name}"])


@pytest.mark.parametrize("variant", sorted(rr.VARIANT_CASES))
def test_wrong_variants_differ_from_the_reference(variant):
    """Otherwise the suite could not tell a pairwise dot, or an alpha kept in fp64, from the rule."""
    for name in rr.VARIANT_CASES[variant]:
        X, Y, C, M, R, kw = CASES[name]
        assert not rr.same_coo(rr.statement(X, Y, C, M, R, variant=variant, **kw), recorded(name), canon=True), f"{variant} shows no difference on {name}"


def test_cases_cover_what_they_claim():
    """Preconditions on the statement's own counters: a case that stops exercising its path fails here."""
    c = truth("shrink_l1")["counters"]
    assert c["shrinks"] > 0 and c["reactivations"] > 0 and c["clipped"] > 0 and c["max_iter_stops"] > 0
    assert truth("shrink_l2")["counters"]["shrinks"] > 0 and truth("shrink_l2")["counters"]["clipped"] == 0
    assert truth("stop_l1")["counters"]["max_iter_stops"] == 6 and truth("stop_l1")["counters"]["iters"] == 12
    assert truth("coded_l1")["counters"]["reactivations"] > 0 and truth("coded_l1")["counters"]["max_iter_stops"] == 0
    assert truth("iter0_l1")["counters"]["iters"] == 0
    assert sorted(n for _, _, n in truth("job_sizes_l1")["per_job"]) == [0, 1, 2, 3, 4, 5, 63, 64, 65, 1000]
    X = CASES["row_lengths_l1"][0]
    assert sorted(set(np.diff(X.indptr).tolist())) == [0, 1, 63, 64, 65, 127, 128, 129, 1000]
    # layouts: a label without positives, one whose positives are its whole M column, one whose positives lie outside it, one in no column
    X, Y, C, M, _, _ = CASES["layouts_l1"]
    col = lambda A, j: set(A.indices[A.indptr[j]:A.indptr[j + 1]].tolist())
    assert not col(Y, 1) and col(Y, 2) == col(M, 1) and not (col(Y, 3) & col(M, 2)) and 5 not in set(C.indices.tolist())
    assert list(C.indices[C.indptr[2]:C.indptr[3]]) == [6, 4, 3] and 0.0 in Y.data and 5.0 in Y.data and 0.0 in M.data
    assert sorted(l for l, _, _ in truth("layouts_l1")["per_job"]) == [0, 1, 2, 3, 4, 6]
    # emission: threshold 0 emits every entry, zeros included; one above every weight emits nothing; ties and the displaced feature
    d, L = CASES["thr_all_l1"][0].shape[1], 24
    assert len(truth("thr_all_l1")["vals"]) == (d + 1) * L and (truth("thr_all_l1")["vals"] == 0).any() and len(truth("thr_none_l1")["vals"]) == 0
    t = truth("ties_maxnz5_l1")
    assert len(set(np.abs(t["vals"]).tolist())) < len(t["vals"])
    tb, d = truth("ties_bias_l1"), CASES["ties_bias_l1"][0].shape[1]
    assert (tb["rows"] == d).sum() == 2 and len(tb["vals"]) == 4, "the bias displaces the least kept feature in both labels"
    assert (truth("ties_maxnz1_l1")["rows"] == d).sum() < 2, "with bias 1 a feature wins in at least one label"
    # bias: the row count of the result
    for b in (1.0, 0.5, 0.0, -1.0):
        assert ((truth(f"bias{b}_l2")["rows"] == 120).any()) == (b > 0), "the bias row exists exactly when bias > 0"


@pytest.mark.parametrize("n", list(range(0, 71)) + [65535, 65536, 65537])
def test_shuffle_restatement_matches_std_shuffle(n):
    a = list(range(n))
    g = cr.Mt19937(0)
    cr.shuffle(g, a)
    assert np.array_equal(np.array(a, dtype=np.uint64), RECORDED[f"shuffle__{n}__perm"].astype(np.uint64))
    assert g() == int(RECORDED[f"shuffle__{n}__next"][0])


# ------------------------------------------------------------------------------------------------ refusals
def _small():
    X, Y, C, M = rr.problem(30, 12, 6, 2, 3, 4, 3)
    return X, Y, C, M


def _refusal(*a, **kw):
    got, err = rr.run_library(rr.OURS, *a, **kw)
    assert got is None and err is not None
    return err


@pytest.mark.parametrize("entry", ["csr", "drm"])
def test_refused_solvers(entry):
    X, Y, C, M = _small()
    Xe = X if entry == "csr" else np.ascontiguousarray(X.toarray())
    start = f"xrl_single_layer_train_{entry}_f32: "
    err = _refusal(Xe, Y, C, M, solver=rr.LR_DUAL)
    assert err.startswith(start) and "L2R_LR_DUAL" in err
    err = _refusal(Xe, Y, C, M, solver=rr.L2_PRIMAL)
    assert err.startswith(start) and "L2R_L2LOSS_SVC_PRIMAL" in err
    assert "unknown solver_type 4" in _refusal(Xe, Y, C, M, solver=4)


def test_refused_shapes_and_patterns():
    X, Y, C, M = _small()
    start = "xrl_single_layer_train_csr_f32: "
    assert _refusal(X[:20], Y, C, M).startswith(start + "Y.rows != X.rows (30 != 20)")
    assert _refusal(X, Y, smat.csc_matrix(C[:5]), M).startswith(start + "C.rows != Y.cols (5 != 6)")
    assert _refusal(X, Y, C, smat.csc_matrix(M[:20])).startswith(start + "M.rows != X.rows (20 != 30)")
    assert _refusal(X, Y, C, smat.csc_matrix(M[:, :1])).startswith(start + "M.cols != C.cols (1 != 2)")
    twice = rr.raw_csc((6, 2), [([0, 1, 2], [1, 1, 1]), ([2, 3, 4, 5], [1, 1, 1, 1])])
    assert "listed under two columns of C" in _refusal(X, Y, twice, M)
    R = rr.relevance(Y, 1)
    assert "R's shape differs" in _refusal(X, Y, C, M, smat.csc_matrix(R[:, :5]))
    other = R.copy()
    other.indices = other.indices.copy()
    other.indices[0] = (other.indices[0] + 7) % 30
    assert "R does not share Y's pattern" in _refusal(X, Y, C, M, other)


def test_refused_null_arguments():
    lib = rr.load(rr.OURS)
    for sfx in ("csr", "drm"):
        fn = getattr(lib, f"xrl_single_layer_train_{sfx}_f32")
        fn.restype = None
        fn.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_double, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_size_t, ctypes.c_double,
                       ctypes.c_double, ctypes.c_int]
        fn(None, None, None, None, None, None, 0.1, 0, 1, 1.0, 1.0, 10, 0.1, 1.0, 1)
        assert rr.last_error(lib) == f"xrl_single_layer_train_{sfx}_f32: null X"


def test_refused_sizes_before_any_array_is_read():
    """2^31 rows and 2^32 - 1 jobs through the host entry points: the views name sizes whose arrays do not exist, so a refusal that came
    after a read would fault instead."""
    lib = rr.load(rr.OURS)
    argtypes = [ctypes.c_void_p] * 5 + [rr._COO_ALLOC, ctypes.c_double, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_size_t,
                ctypes.c_double, ctypes.c_double, ctypes.c_int]
    solver_args = (0.1, 0, 1, 1.0, 1.0, 10, 0.1, 1.0, 1)
    alloc = rr._COO_ALLOC(lambda *a: None)
    ptr = np.zeros(2, np.uint64)
    for sfx, view in (("csr", cr.CsrView(1 << 31, 5, ptr.ctypes.data, 0, 0)), ("drm", cr.DrmView(1 << 31, 5, 0))):
        fn = getattr(lib, f"xrl_single_layer_train_{sfx}_f32")
        fn.restype, fn.argtypes = None, argtypes
        fn(ctypes.byref(view), None, None, None, None, alloc, *solver_args)
        assert rr.last_error(lib) == f"xrl_single_layer_train_{sfx}_f32: 2^31 rows or more"
    X, Y, _, _ = _small()
    keep = []
    xp, xi, xv = X.indptr.astype(np.uint64), X.indices.astype(np.uint32), X.data.astype(np.float32)
    xview = cr.CsrView(X.shape[0], X.shape[1], xp.ctypes.data, xi.ctypes.data, xv.ctypes.data)
    yview = rr._csc_view(Y, keep)
    mview = rr._csc_view(smat.csc_matrix(np.ones((X.shape[0], 1), dtype=np.float32)), keep)
    cptr = np.array([0, (1 << 32) - 1], np.uint64)
    cview = rr.CscView(Y.shape[1], 1, cptr.ctypes.data, 0x1000, 0)                 # its row ids are never read
    fn = lib.xrl_single_layer_train_csr_f32
    fn.restype, fn.argtypes = None, argtypes
    fn(ctypes.byref(xview), ctypes.byref(yview), ctypes.byref(cview), ctypes.byref(mview), None, alloc, *solver_args)
    assert rr.last_error(lib) == "xrl_single_layer_train_csr_f32: 2^32 - 1 jobs or more"


def _fake_handle(lib, device, rows, cols, nnz=3):
    """A matrix handle over addresses that are never read: the resident form's refusals come before any GPU call."""
    lib.xrl_smat_from_device_csr.restype = ctypes.c_void_p
    lib.xrl_smat_from_device_csr.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    h = lib.xrl_smat_from_device_csr(device, rows, cols, 0x1000, 0x1000, 0x1000, nnz)
    assert h
    return h


def test_resident_form_refusals_need_no_gpu():
    lib = rr.load(rr.OURS)
    fn = lib.xrl_train_layer_device
    fn.restype = ctypes.c_void_p
    fn.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_double, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_uint64, ctypes.c_double, ctypes.c_double,
                   ctypes.c_void_p]
    lib.xrl_smat_free.argtypes = [ctypes.c_void_p]
    N, d, L, K = 30, 12, 6, 2
    x, yt, ct, mt = _fake_handle(lib, 0, N, d), _fake_handle(lib, 0, L, N), _fake_handle(lib, 0, K, L), _fake_handle(lib, 0, K, N)
    made = [x, yt, ct, mt]

    def refusal(*handles, solver=1):
        assert fn(*handles, 0.1, 0, solver, 1.0, 1.0, 10, 0.1, 1.0, None) is None
        return rr.last_error(lib)

    try:
        start = "xrl_train_layer_device: "
        assert "L2R_LR_DUAL" in refusal(x, yt, ct, mt, None, solver=7) and "L2R_L2LOSS_SVC_PRIMAL" in refusal(x, yt, ct, mt, None, solver=2)
        assert refusal(None, yt, ct, mt, None) == start + "null matrix handle (X)"
        assert refusal(x, None, ct, mt, None) == start + "null matrix handle (Yt)"
        assert refusal(x, yt, ct, None, None) == start + "Ct comes without Mt"
        for bad, msg in (((_fake_handle(lib, 0, L, N + 1), ct, mt, None), "Yt.cols != X.rows (31 != 30)"),
                         ((yt, _fake_handle(lib, 0, K, L + 1), mt, None), "Ct.cols != Yt.rows (7 != 6)"),
                         ((yt, ct, _fake_handle(lib, 0, K, N + 1), None), "Mt.cols != X.rows (31 != 30)"),
                         ((yt, ct, _fake_handle(lib, 0, K + 1, N), None), "Mt.rows != Ct.rows (3 != 2)"),
                         ((yt, ct, mt, _fake_handle(lib, 0, L, N, nnz=4)), "Rt does not share Yt's pattern"),
                         ((yt, _fake_handle(lib, 1, K, L), mt, None), "the operands are on devices 0 and 1")):
            made.extend(h for h in bad if h and h not in made)
            assert refusal(x, *bad).startswith(start + msg), msg
        big = [_fake_handle(lib, 0, 1 << 31, d), _fake_handle(lib, 0, L, 1 << 31)]          # positions of instances are 32-bit with a spare bit
        made.extend(big)
        assert refusal(big[0], big[1], None, None, None) == start + "2^31 rows or more"
        many = [_fake_handle(lib, 0, K, L, nnz=(1 << 32) - 1), _fake_handle(lib, 0, L, N, nnz=3)]     # a job per stored entry of Ct: job ids are 32-bit
        made.extend(many)
        assert refusal(x, yt, many[0], mt, None) == start + "2^32 - 1 jobs or more"
        wide = [_fake_handle(lib, 0, N, d), _fake_handle(lib, 0, (1 << 32) - 1, N)]                    # pure multi-label: a job per label
        made.extend(wide)
        assert refusal(wide[0], wide[1], None, None, None) == start + "2^32 - 1 jobs or more"
    finally:
        for h in made:
            lib.xrl_smat_free(h)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_wrapper_dispatch_and_defaults(monkeypatch):
    """clib.xlinear_single_layer_train picks the entry point by the view's type, passes the reference's defaults and its solver table."""
    import inspect
    from pecos_amd import clib
    from pecos_amd.core import XLINEAR_SOLVERS, ScipyCscF32, ScipyCsrF32, ScipyDrmF32
    assert XLINEAR_SOLVERS == {"L2R_L2LOSS_SVC_DUAL": 1, "L2R_L1LOSS_SVC_DUAL": 3, "L2R_LR_DUAL": 7, "L2R_L2LOSS_SVC_PRIMAL": 2}
    sig = inspect.signature(clib.xlinear_single_layer_train)
    assert list(sig.parameters)[:5] == ["pX", "pY", "pC", "pM", "pR"]
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == dict(
        threshold=0.1, max_nonzeros_per_label=None, solver_type="L2R_L2LOSS_SVC_DUAL", Cp=1.0, Cn=1.0, max_iter=1000, eps=0.1, bias=1.0, threads=-1, verbose=0)
    X, Y, C, M = _small()
    calls = []

    class Lib:
        def __getattr__(self, name):
            def fn(*a):
                calls.append((name, a))
                if name.startswith("xrl_single_layer_train"):
                    a[5](13, 6, 0, *(ctypes.byref(ctypes.c_uint64()) for _ in range(3)))
            return fn

    monkeypatch.setattr(type(clib), "clib_float32", property(lambda self: Lib()))
    monkeypatch.setattr(type(clib), "_check", lambda self: None)
    W = clib.xlinear_single_layer_train(ScipyCsrF32(X), ScipyCscF32(Y), ScipyCscF32(C), ScipyCscF32(M), None)
    assert isinstance(W, smat.csc_matrix) and W.shape == (13, 6) and W.dtype == np.float32
    assert calls[-1][0] == "xrl_single_layer_train_csr_f32" and calls[-1][1][4] is None and calls[-1][1][6:] == (0.1, 0, 1, 1.0, 1.0, 1000, 0.1, 1.0, -1)
    clib.xlinear_single_layer_train(ScipyDrmF32(np.ascontiguousarray(X.toarray())), ScipyCscF32(Y), None, None, None, solver_type="L2R_L1LOSS_SVC_DUAL",
                                    max_nonzeros_per_label=7)
    assert calls[-1][0] == "xrl_single_layer_train_drm_f32" and calls[-1][1][2] is None and calls[-1][1][7:9] == (7, 3)
    with pytest.raises(NotImplementedError):
        clib.xlinear_single_layer_train(X, ScipyCscF32(Y), None, None, None)
    with pytest.raises(ValueError, match="unknown solver_type"):
        clib.xlinear_single_layer_train(ScipyCsrF32(X), ScipyCscF32(Y), None, None, None, solver_type="NO_SUCH")


def test_train_params_defaults_and_names():
    import dataclasses as dc
    from pecos_amd import HierarchicalMLModel, MLModel, XLinearModel
    assert {f.name: f.default for f in dc.fields(MLModel.TrainParams)} == dict(
        threshold=0.1, max_nonzeros_per_label=None, solver_type="L2R_L2LOSS_SVC_DUAL", Cp=1.0, Cn=1.0, max_iter=100, eps=0.1, bias=1.0, threads=-1, verbose=0,
        newton_eps=0.01)
    tp = MLModel.TrainParams.from_dict(dict(threshold=0.2, Cp=3.0, nr_splits=4))
    assert (tp.threshold, tp.Cp, tp.max_iter) == (0.2, 3.0, 100)
    h = HierarchicalMLModel.TrainParams.from_dict(dict(neg_mining_chain=["tfn", "usn"], model_chain=[dict(Cp=2.0), dict(eps=0.5)]))
    assert h.neg_mining_chain == ["tfn", "usn"] and h.model_chain[0].Cp == 2.0 and h.model_chain[1].eps == 0.5
    x = XLinearModel.TrainParams.from_dict(dict(nr_splits=4, min_codes=4, threshold=0.2))
    assert (x.mode, x.nr_splits, x.min_codes, x.rel_mode, x.shallow) == ("full-model", 4, 4, "disable", False)


def test_mlproblem(monkeypatch):
    from pecos_amd import clib
    from pecos_amd.core import ScipyCscF32, ScipyCsrF32, ScipyDrmF32
    from pecos_amd.xlinear import MLProblem
    X, Y, C, M = _small()
    p = MLProblem(X, Y.tocsr())
    assert isinstance(p.pX, ScipyCsrF32) and isinstance(p.pY, ScipyCscF32) and p.pR is None and p.nr_labels == 6
    assert p.C.shape == (6, 1) and p.C.nnz == 6 and p.M.shape == (30, 1) and p.M.nnz == 30, "no C: one all-ones column each"
    assert isinstance(MLProblem(np.ascontiguousarray(X.toarray()), Y).pX, ScipyDrmF32)
    products = []
    monkeypatch.setattr(type(clib), "sparse_matmul", lambda self, A, B, **kw: products.append((A.shape, B.shape)) or (A.tocsr() * B.tocsr()).tocsc())
    p = MLProblem(X, Y, C=C)
    assert products == [((30, 6), (6, 2))], "M = Y * C through clib.sparse_matmul when M is not given"
    assert p.M.shape == (30, 2) and p.M.has_sorted_indices and np.array_equal(p.M.indices, M.indices) and np.array_equal(p.M.indptr, M.indptr)
    assert MLProblem(X, Y, C=C, M=M.tocsr()).M.nnz == M.nnz and len(products) == 1
    R = rr.relevance(Y, 2)
    assert np.array_equal(MLProblem(X, Y, R=R).R.data, R.data)
    bad = R.copy()
    bad.data = -bad.data
    with pytest.raises(ValueError, match="got value < 0"):
        MLProblem(X, Y, R=bad)
    with pytest.raises(ValueError, match="Y.indptr != R.indptr"):
        MLProblem(X, Y, R=smat.csc_matrix(R[:, ::-1]))
    with pytest.raises(NotImplementedError):
        MLProblem(X.tocsc(), Y)


def test_matcher_aware_negatives_are_refused_by_name():
    from pecos_amd import HierarchicalMLModel, XLinearModel
    from pecos_amd.xlinear import MLProblem
    X, Y, C, M = _small()
    chain = [smat.csc_matrix(np.ones((2, 1), dtype=np.float32)), C]
    for scheme in ("man", "tfn+man"):
        with pytest.raises(NotImplementedError, match=scheme.replace("+", r"\+")):
            HierarchicalMLModel.train(MLProblem(X, Y), clustering=chain, negative_sampling_scheme=scheme)
    with pytest.raises(NotImplementedError, match="mode = 'matcher'"):
        XLinearModel.train(X, Y, C=C, mode="matcher")
    with pytest.raises(NotImplementedError, match="rel_mode"):
        XLinearModel.train(X, Y, C=C, rel_mode="induce")


def test_a_loaded_model_cannot_be_saved(tmp_path):
    from pecos_amd import HierarchicalMLModel
    m = HierarchicalMLModel.__new__(HierarchicalMLModel)
    m.model_chain = None
    with pytest.raises(Exception, match="predict only"):
        m.save(str(tmp_path / "m"))


def test_reference_binding_drives_both_entry_points_under_their_names_here():
    """The reference's own prototypes (link_xlinear_methods) and its own xlinear_single_layer_train fit xrl_single_layer_train_{csr,drm}_f32:
    one rename binds them.  The reference's names themselves are NOT exported here, so a binding that takes this library first and the
    reference otherwise keeps the reference's trainer and all its solvers (tests/test_reference_binding.py holds that)."""
    refpy = os.path.join(REPO, "oracle", "_ref", "refpy")
    if not os.path.isdir(os.path.join(refpy, "pecos")):
        pytest.skip("oracle/_ref/refpy (the reference's python package) is not built")
    if refpy not in sys.path:
        sys.path.insert(0, refpy)
    import pecos.core.base as pcb
    ours = ctypes.CDLL(rr.OURS)
    assert not hasattr(ours, "c_xlinear_single_layer_train_csr_f32") and not hasattr(ours, "c_xlinear_single_layer_train_drm_f32")

    class Renamed:
        def __getattr__(self, name):
            return getattr(ours, name.replace("c_xlinear_single_layer_train_", "xrl_single_layer_train_"))

    lib = pcb.corelib.__new__(pcb.corelib)
    lib.clib_float32 = Renamed()
    lib.link_xlinear_methods()
    for sfx in ("csr", "drm"):
        fn = getattr(ours, f"xrl_single_layer_train_{sfx}_f32")
        assert len(fn.argtypes) == 15 and fn.argtypes[5] is pcb.ScipyCoordinateSparseAllocator.CFUNCTYPE
    # a refusal travels through the reference's own binding and structures
    X, Y, C, M = _small()
    with pytest.raises(Exception):
        lib.xlinear_single_layer_train(pcb.ScipyCsrF32.init_from(X), pcb.ScipyCscF32.init_from(Y), pcb.ScipyCscF32.init_from(C), pcb.ScipyCscF32.init_from(M), None,
                                       solver_type="L2R_LR_DUAL")
    assert "L2R_LR_DUAL" in rr.last_error(ours)
