"""Primal L2-loss SVC training (K16), the half that needs no GPU: the numpy statement of the rule (tests/primal_training_rule.py) against
the compiled reference -- as recorded in tests/golden/primal_training_ref.npz and, where oracle/_ref is built, live at 1 and 8 threads --
bit for bit; the compressed form against the dense reference in a matrix ten times wider; three wrong variants, each shown to differ;
what every case claims to meet, asserted from the statement's trace; every refusal of the new entry points that needs no data on the
device; the Python dispatch by solver number.

Exits the seeded search (primal_training_rule.search_cases, at most 3000 problems of up to 13 rows and 6 features) does NOT reach: the
1000-iteration cap of the Newton loop (the line search fails or the reduction becomes too small long before), and f < -1e32 (the
objective is a sum of squares).  Neither is forced."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as smat

import clustering_rule as cr
import primal_training_rule as pr
import ranker_training_rule as rr

CASES = pr.cases()
SEARCH = pr.search_cases()
ALL = dict(CASES, **{"search_" + k: v for k, v in SEARCH.items()})
RECORDED = pr.recorded()
HAVE_REF = os.path.exists(pr.REF)
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref not built")
_truth = {}


def truth(name):
    if name not in _truth:
        X, Y, C, M, R, kw = ALL[name]
        _truth[name] = pr.statement(X, Y, C, M, R, **kw)
    return _truth[name]


def canon(kw):
    """The order inside a label is pinned unless max_nonzeros_per_label leaves it to std::nth_element."""
    return bool(kw.get("max_nonzeros"))


@pytest.mark.parametrize("name", sorted(ALL))
def test_statement_equals_the_recorded_reference(name):
    assert pr.same_coo(truth(name), pr.recorded_case(RECORDED, name), canon=canon(ALL[name][5]))
    assert not any(t["nonfinite"] for t in truth(name)["trace"]), "the compressed form covers finite step lengths only"


@needs_ref
@pytest.mark.parametrize("name", sorted(ALL))
def test_statement_equals_the_live_reference_at_1_and_8_threads(name):
    X, Y, C, M, R, kw = ALL[name]
    assert pr.same_coo(truth(name), pr.reference(X, Y, C, M, R, threads=1, **kw), canon=canon(kw))
    assert pr.same_coo(truth(name), pr.reference(X, Y, C, M, R, threads=8, **kw), canon=True)


def _mapped(coo, d, mult=37, add=5, width=None):
    """A COO over d features (+ the bias row d) with its rows renumbered as primal_training_rule.renumbered does."""
    rows = np.where(coo["rows"] == d, width, coo["rows"].astype(np.int64) * mult + add).astype(np.uint64)
    return rows, coo["cols"], coo["vals"]


@needs_ref
@pytest.mark.parametrize("seed", range(12))
def test_compressed_form_equals_the_dense_reference_in_a_wider_matrix(seed):
    """Feature f moved to 37 f + 5 inside a matrix at least ten times wider: every weight bit of the DENSE reference stays, and every
    feature no instance stores is emitted as +0 at threshold 0.  The CG step cap, max(d + (bias > 0), 5), grows with the matrix, so the
    problems are ones whose trace shows that no run reaches it."""
    rs = np.random.RandomState(700 + seed)
    N, d, L = int(rs.randint(20, 60)), int(rs.randint(6, 30)), int(rs.randint(2, 5))
    X, Y, C, M = pr.problem(N, d, L, 2, 4, 6, 800 + seed, scale=float(rs.choice([0.3, 1.0, 5.0])))
    kw = dict(eps=float(rs.choice([0.1, 1e-3])), bias=float(rs.choice([1.0, 0.0])), Cp=float(rs.choice([1.0, 4.0])), threshold=0.0)
    st = pr.statement(X, Y, C, M, **kw)
    assert all("cap" not in t["cg_exits"] and not t["nonfinite"] for t in st["trace"])
    Z = pr.renumbered(X)
    assert Z.shape[1] >= 10 * d
    narrow, wide = pr.reference(X, Y, C, M, **kw), pr.reference(Z, Y, C, M, **kw)
    assert pr.same_coo(st, narrow)
    touched = {(int(r), int(c)) for r, c in zip(*_mapped(narrow, d, width=Z.shape[1])[:2])}
    keep = np.array([(int(r), int(c)) in touched for r, c in zip(wide["rows"], wide["cols"])])
    assert pr.same_coo(_mapped(narrow, d, width=Z.shape[1]), (wide["rows"][keep], wide["cols"][keep], wide["vals"][keep]), canon=True)
    assert len(wide["vals"]) == (Z.shape[1] + (kw["bias"] > 0)) * len(st["trace"]) and not wide["vals"][~keep].view(np.uint32).any(), "an untouched feature is +0"
    assert pr.same_coo(pr.statement(Z, Y, C, M, **kw), wide), "the statement itself, over the wide matrix"


VARIANT_CASES = {"no_alias": lambda: CASES["alias"], "dot64": lambda: CASES["order"], "cg_touched": pr.cg_cap_wide_problem}


@needs_ref
@pytest.mark.parametrize("variant", sorted(VARIANT_CASES))
def test_wrong_variants_differ_from_the_reference(variant):
    """Otherwise the suite could not tell a grad that compacts into its own array, an fp64 dot, or a step cap from the touched count from
    the rule.  The rule itself equals the reference on the same input."""
    X, Y, C, M, R, kw = VARIANT_CASES[variant]()
    ref = pr.reference(X, Y, C, M, R, **kw)
    assert pr.same_coo(pr.statement(X, Y, C, M, R, **kw), ref)
    assert not pr.same_coo(pr.statement(X, Y, C, M, R, variant=variant, **kw), ref, canon=True), f"{variant} shows no difference"


@needs_ref
def test_the_alias_changes_the_weights():
    """M = {10, 20, 30} and the positive at row 1: moving that row's data to row 39 gives other weight bits (from the reference alone)."""
    a, b = (pr.reference(*pr.alias_problem(r), **CASES["alias"][5]) for r in (1, 39))
    assert np.array_equal(a["rows"], b["rows"]) and not np.array_equal(a["vals"].view(np.uint32), b["vals"].view(np.uint32))


def test_cases_cover_what_they_claim():
    """Preconditions on the statement's own trace: a case that stops exercising its path fails here."""
    one = lambda name: truth(name)["trace"][0]          # noqa: E731
    assert one("alias")["alias_overwrites"] > 0 and one("alias")["instances"] == 4, "the appended positive overwrites a live compacted slot"
    assert one("alias_twin")["alias_overwrites"] == 0 and one("alias_twin")["instances"] == 4
    assert all(t["alias_overwrites"] == 0 for t in truth("pure")["trace"]), "index is the identity in the pure form"
    # the exits: every job of eps = 0 ends otherwise than by the gradient test; the search's cases end as their names say
    assert {t["newton_exit"] for t in truth("eps0")["trace"]} == {"linesearch"} and {t["newton_exit"] for t in truth("eps0.0001")["trace"]} == {"gradient"}
    assert {t["newton_exit"] for t in truth("coded")["trace"]} == {"gradient"} and truth("coded")["counters"]["cg_q"] == truth("coded")["counters"]["newton_iters"]
    assert one("search_linesearch")["newton_exit"] == "linesearch" and one("search_linesearch")["halvings"][-1] == pr.MAX_HALVINGS
    assert one("search_actred")["newton_exit"] == "actred"
    assert "dhd" in one("search_dhd")["cg_exits"] and "positive" in one("search_positive")["cg_exits"]
    t = one("search_cg_cap")
    assert "cap" in t["cg_exits"] and t["max_cg_iter"] == 5 and max(t["cg_iters"]) == 5, "a run that takes all of max(d + (bias > 0), 5) steps"
    t = one("search_halving")
    assert 0 < max(t["halvings"]) < pr.MAX_HALVINGS and t["newton_exit"] != "linesearch", "a halved step that is then accepted"
    assert sorted(SEARCH) == ["actred", "cg_cap", "dhd", "halving", "linesearch", "positive"]
    assert truth("job_sizes")["counters"]["end_before_first"] == 1, "the job without instances: gnorm0 = 0"
    # small d: the step cap on both sides of max(d + (bias > 0), 5)
    for d, b, cap in ((1, 1.0, 5), (3, 1.0, 5), (4, 0.0, 5), (4, 1.0, 5), (5, 0.0, 5), (5, 1.0, 6)):
        assert {t["max_cg_iter"] for t in truth(f"d{d}_bias{b}")["trace"]} == {cap}
    assert {t["max_cg_iter"] for t in truth("wide_nobias")["trace"]} == {120} and not (truth("wide_nobias")["rows"] == 120).any()
    # sizes
    assert sorted(t["instances"] for t in truth("job_sizes")["trace"]) == [0, 1, 2, 5, 63, 64, 65, 1000]
    assert sorted(t["touched"] for t in truth("touched")["trace"]) == [1, 63, 64, 65, 129, 1000]
    assert sorted(set(np.diff(CASES["row_lengths"][0].indptr).tolist())) == [0, 1, 63, 64, 65, 127, 128, 129, 1000]
    c = truth("row_lengths")["counters"]
    assert c["lane_rows"] == 3 * 6 and c["wave_rows"] == 3 * 12, "rows of 64 entries and more are summed by the wavefront"
    # layouts (ranker_training_rule.layouts): a label without positives, only positives, positives outside M, one in no column of C
    assert sorted(t["label"] for t in truth("layouts")["trace"]) == [0, 1, 2, 3, 4, 6]
    # repeated ids: a job lists more positions than it has distinct rows
    X, Y, C, M, _, _ = CASES["dups"]
    assert any(t["instances"] > len(set(M.indices.tolist()) | set(Y.indices[Y.indptr[t["label"]]:Y.indptr[t["label"] + 1]].tolist())) for t in truth("dups_R0")["trace"])
    # emission
    d, L = CASES["thr_all"][0].shape[1], 24
    assert len(truth("thr_all")["vals"]) == (d + 1) * L and (truth("thr_all")["vals"].view(np.uint32) == 0).any() and len(truth("thr_none")["vals"]) == 0
    t = truth("ties_maxnz5")
    assert len(set(np.abs(t["vals"]).tolist())) < len(t["vals"])
    tb, d = truth("ties_bias"), CASES["ties_bias"][0].shape[1]
    assert (tb["rows"] == d).sum() == 2 and len(tb["vals"]) == 4, "the bias displaces the least kept feature in both labels"
    for b in (1.0, 0.5, 0.0, -1.0):
        assert ((truth(f"bias{b}")["rows"] == 120).any()) == (b > 0), "the bias row exists exactly when bias > 0"
    X, Y = pr.nonfinite_problem()[:2]
    t = pr.statement(X, Y, **pr.nonfinite_problem()[5])["trace"][0]
    assert t["nonfinite"] == "alpha" and np.isfinite(X.data).all() and t["touched"] < X.shape[1]


@needs_ref
def test_max_iter_is_not_used():
    X, Y, C, M, R, kw = CASES["coded"]
    a, b = pr.reference(X, Y, C, M, R, max_iter=1, **kw), pr.reference(X, Y, C, M, R, max_iter=1000, **kw)
    assert len(a["vals"]) > 0 and pr.same_coo(a, b) and pr.same_coo(pr.statement(X, Y, C, M, R, max_iter=1, **kw), a)


# ------------------------------------------------------------------------------------------------ refusals
def _small():
    return pr.problem(30, 12, 6, 2, 3, 4, 3)


def _refusal(*a, **kw):
    got, err = pr.run_newton(pr.OURS, *a, **kw)
    assert got is None and err is not None
    return err


@pytest.mark.parametrize("entry", ["csr", "drm"])
def test_refused_solvers(entry):
    X, Y, C, M = _small()
    Xe = X if entry == "csr" else np.ascontiguousarray(X.toarray())
    start = f"xrl_single_layer_train_newton_{entry}_f32: "
    for solver, name in ((rr.L2_DUAL, "L2R_L2LOSS_SVC_DUAL"), (rr.L1_DUAL, "L2R_L1LOSS_SVC_DUAL")):
        err = _refusal(Xe, Y, C, M, solver=solver)
        assert err.startswith(start + "solver " + name) and "xrl_single_layer_train_{csr,drm}_f32" in err and "xrl_train_layer_device" in err
    err = _refusal(Xe, Y, C, M, solver=rr.LR_DUAL)
    assert err.startswith(start + "solver L2R_LR_DUAL") and "log in fp64" in err
    assert _refusal(Xe, Y, C, M, solver=4).startswith(start + "unknown solver_type 4")


def test_refused_shapes_and_patterns():
    X, Y, C, M = _small()
    start = "xrl_single_layer_train_newton_csr_f32: "
    assert _refusal(X[:20], Y, C, M).startswith(start + "Y.rows != X.rows (30 != 20)")
    assert _refusal(X, Y, smat.csc_matrix(C[:5]), M).startswith(start + "C.rows != Y.cols (5 != 6)")
    assert _refusal(X, Y, C, smat.csc_matrix(M[:20])).startswith(start + "M.rows != X.rows (20 != 30)")
    assert _refusal(X, Y, C, smat.csc_matrix(M[:, :1])).startswith(start + "M.cols != C.cols (1 != 2)")
    twice = pr.raw_csc((6, 2), [([0, 1, 2], [1, 1, 1]), ([2, 3, 4, 5], [1, 1, 1, 1])])
    assert _refusal(X, Y, twice, M).startswith(start + "a label is listed under two columns of C")
    R = pr.relevance(Y, 1)
    assert _refusal(X, Y, C, M, smat.csc_matrix(R[:, :5])).startswith(start + "R's shape differs")
    other = R.copy()
    other.indices = other.indices.copy()
    other.indices[0] = (other.indices[0] + 7) % 30
    assert _refusal(X, Y, C, M, other).startswith(start + "R does not share Y's pattern")


_HOST_ARGS = [ctypes.c_void_p] * 5 + [rr._COO_ALLOC, ctypes.c_double, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_size_t,
                                      ctypes.c_double, ctypes.c_double, ctypes.c_int]
_SOLVER_ARGS = (0.1, 0, 2, 1.0, 1.0, 10, 0.1, 1.0, 1)


def test_refused_null_arguments_and_sizes_before_any_array_is_read():
    lib = cr.load(pr.OURS)
    alloc = rr._COO_ALLOC(lambda *a: None)
    ptr = np.zeros(2, np.uint64)
    for sfx, view in (("csr", cr.CsrView(1 << 31, 5, ptr.ctypes.data, 0, 0)), ("drm", cr.DrmView(1 << 31, 5, 0))):
        fn = getattr(lib, f"xrl_single_layer_train_newton_{sfx}_f32")
        fn.restype, fn.argtypes = None, _HOST_ARGS
        fn(None, None, None, None, None, alloc, *_SOLVER_ARGS)
        assert cr.last_error(lib) == f"xrl_single_layer_train_newton_{sfx}_f32: null X"
        fn(ctypes.byref(view), None, None, None, None, alloc, *_SOLVER_ARGS)
        assert cr.last_error(lib) == f"xrl_single_layer_train_newton_{sfx}_f32: 2^31 rows or more"
    X, Y, _, _ = _small()
    keep = []
    xp, xi, xv = X.indptr.astype(np.uint64), X.indices.astype(np.uint32), X.data.astype(np.float32)
    xview = cr.CsrView(X.shape[0], X.shape[1], xp.ctypes.data, xi.ctypes.data, xv.ctypes.data)
    yview = rr._csc_view(Y, keep)
    fn = lib.xrl_single_layer_train_newton_csr_f32
    fn(ctypes.byref(xview), None, None, None, None, alloc, *_SOLVER_ARGS)
    assert cr.last_error(lib) == "xrl_single_layer_train_newton_csr_f32: null Y"
    fn.argtypes = [ctypes.c_void_p] * 6 + _HOST_ARGS[6:]
    fn(ctypes.byref(xview), ctypes.byref(yview), None, None, None, None, *_SOLVER_ARGS)
    assert cr.last_error(lib) == "xrl_single_layer_train_newton_csr_f32: null allocator"
    fn.argtypes = _HOST_ARGS
    mview = rr._csc_view(smat.csc_matrix(np.ones((X.shape[0], 1), dtype=np.float32)), keep)
    cptr = np.array([0, (1 << 32) - 1], np.uint64)
    cview = rr.CscView(Y.shape[1], 1, cptr.ctypes.data, 0x1000, 0)                 # its row ids are never read
    fn(ctypes.byref(xview), ctypes.byref(yview), ctypes.byref(cview), ctypes.byref(mview), None, alloc, *_SOLVER_ARGS)
    assert cr.last_error(lib) == "xrl_single_layer_train_newton_csr_f32: 2^32 - 1 jobs or more"


def _fake_handle(lib, device, rows, cols, nnz=3):
    """A matrix handle over addresses that are never read: the resident form's refusals come before any GPU call."""
    lib.xrl_smat_from_device_csr.restype = ctypes.c_void_p
    lib.xrl_smat_from_device_csr.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    h = lib.xrl_smat_from_device_csr(device, rows, cols, 0x1000, 0x1000, 0x1000, nnz)
    assert h
    return h


def test_resident_form_refusals_need_no_gpu():
    lib = cr.load(pr.OURS)
    fn = lib.xrl_train_layer_newton_device
    fn.restype = ctypes.c_void_p
    fn.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_double, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_uint64, ctypes.c_double, ctypes.c_double,
                   ctypes.c_void_p]
    lib.xrl_smat_free.argtypes = [ctypes.c_void_p]
    N, d, L, K = 30, 12, 6, 2
    x, yt, ct, mt = _fake_handle(lib, 0, N, d), _fake_handle(lib, 0, L, N), _fake_handle(lib, 0, K, L), _fake_handle(lib, 0, K, N)
    made = [x, yt, ct, mt]

    def refusal(*handles, solver=2):
        assert fn(*handles, 0.1, 0, solver, 1.0, 1.0, 10, 0.1, 1.0, None) is None
        return cr.last_error(lib)

    try:
        start = "xrl_train_layer_newton_device: "
        assert refusal(x, yt, ct, mt, None, solver=1).startswith(start + "solver L2R_L2LOSS_SVC_DUAL is served by") and "xrl_train_layer_device" in refusal(x, yt, ct, mt, None, solver=3)
        assert refusal(x, yt, ct, mt, None, solver=7).startswith(start + "solver L2R_LR_DUAL") and "log in fp64" in refusal(x, yt, ct, mt, None, solver=7)
        assert refusal(x, yt, ct, mt, None, solver=0).startswith(start + "unknown solver_type 0")
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
        big = [_fake_handle(lib, 0, 1 << 31, d), _fake_handle(lib, 0, L, 1 << 31)]
        made.extend(big)
        assert refusal(big[0], big[1], None, None, None) == start + "2^31 rows or more"
        many = [_fake_handle(lib, 0, K, L, nnz=(1 << 32) - 1)]
        made.extend(many)
        assert refusal(x, yt, many[0], mt, None) == start + "2^32 - 1 jobs or more"
        wide = [_fake_handle(lib, 0, (1 << 32) - 1, N)]
        made.extend(wide)
        assert refusal(x, wide[0], None, None, None) == start + "2^32 - 1 jobs or more"
    finally:
        for h in made:
            lib.xrl_smat_free(h)


def test_counters_entry_point():
    lib = cr.load(pr.OURS)
    lib.xrl_debug_newton_counters.restype, lib.xrl_debug_newton_counters.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]
    assert lib.xrl_debug_newton_counters(None, 20) == -1 and cr.last_error(lib) == "xrl_debug_newton_counters: null argument"
    assert len(pr.COUNTERS) == 20 and set(pr.counters()) == set(pr.COUNTERS)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_dispatch_by_solver_number(monkeypatch):
    """clib.xlinear_single_layer_train and clib.train_layer_device take K16's symbols for L2R_L2LOSS_SVC_PRIMAL (by name or number) and
    K13's for every other solver, L2R_LR_DUAL included (whose refusal through the Python surface is pinned)."""
    from pecos_amd import clib
    from pecos_amd.core import ScipyCscF32, ScipyCsrF32, ScipyDrmF32
    assert clib.NEWTON_COUNTERS == pr.COUNTERS
    X, Y, C, M = _small()
    calls = []

    class Lib:
        def __getattr__(self, name):
            def fn(*a):
                calls.append((name, a))
                if name.startswith("xrl_single_layer_train"):
                    a[5](13, 6, 0, *(ctypes.byref(ctypes.c_uint64()) for _ in range(3)))
                return 1
            return fn

    monkeypatch.setattr(type(clib), "clib_float32", property(lambda self: Lib()))
    monkeypatch.setattr(type(clib), "_check", lambda self: None)
    views = (ScipyCscF32(Y), ScipyCscF32(C), ScipyCscF32(M), None)
    for solver, number, infix in (("L2R_L2LOSS_SVC_PRIMAL", 2, "_newton"), (2, 2, "_newton"), ("L2R_L2LOSS_SVC_DUAL", 1, ""), ("L2R_L1LOSS_SVC_DUAL", 3, ""), (3, 3, ""),
                                  ("L2R_LR_DUAL", 7, "")):
        clib.xlinear_single_layer_train(ScipyCsrF32(X), *views, solver_type=solver)
        assert calls[-1][0] == f"xrl_single_layer_train{infix}_csr_f32" and calls[-1][1][8] == number
        clib.xlinear_single_layer_train(ScipyDrmF32(np.ascontiguousarray(X.toarray())), *views, solver_type=solver)
        assert calls[-1][0] == f"xrl_single_layer_train{infix}_drm_f32" and calls[-1][1][8] == number
        clib.train_layer_device(1, 2, 3, 4, None, solver_type=solver)
        assert calls[-1][0] == f"xrl_train_layer{infix}_device" and calls[-1][1][7] == number


def test_the_primal_solver_stops_at_newton_eps():
    """pecos/xmc/base.py:868-870: MLModel.train replaces eps by newton_eps (0.01) for the primal solver; so does the layer loop."""
    from pecos_amd import MLModel
    from pecos_amd.training import _params_dict
    assert _params_dict(MLModel.TrainParams(solver_type="L2R_L2LOSS_SVC_PRIMAL", eps=0.3))["eps"] == 0.01
    assert _params_dict(dict(solver_type="L2R_L2LOSS_SVC_PRIMAL", eps=0.3, newton_eps=0.5))["eps"] == 0.5
    assert _params_dict(dict(solver_type="L2R_L2LOSS_SVC_PRIMAL"))["eps"] == 0.01
    assert _params_dict(MLModel.TrainParams(solver_type="L2R_L1LOSS_SVC_DUAL", eps=0.3))["eps"] == 0.3 and "eps" not in _params_dict(dict(threshold=0.1))
