"""Primal L2-loss SVC training on the device (K16): xrl_single_layer_train_newton_csr_f32 / _drm_f32, xrl_train_layer_newton_device and
xrl_debug_newton_counters against the numpy statement of the rule (tests/primal_training_rule.py), the compiled reference as recorded
in tests/golden/primal_training_ref.npz and, where oracle/_ref is built, the live reference library -- rows, cols and value bits, and
what ran against the statement's own counters; then the Python surface end to end against the recorded reference.

The tolerance is zero and it is derived: both sides run IEEE-correct + - * / sqrt on fp32 and fp64 values in one fixed order, with no
libm call.  If a case differs, an order or a rounding is wrong, and the statement's trace says where to look.

Exits no case reaches (see tests/test_primal_training_cpu.py): the 1000-iteration cap of the Newton loop, and f < -1e32."""
import os

import numpy as np
import pytest
import scipy.sparse as smat

import device_views as dv
import matching_rule as mr
import primal_training_rule as pr
import ranker_training_rule as rr

pytestmark = pytest.mark.gpu

CASES = pr.cases()
ALL = dict(CASES, **{"search_" + k: v for k, v in pr.search_cases().items()})
RECORDED = pr.recorded()
HAVE_REF = os.path.exists(pr.REF)
DENSE = ("coded", "coded_costs", "pure", "bias0.0", "bias0.5", "layouts_R", "maxnz5", "thr_all", "ties_bias", "d3_bias1.0", "alias", "dups_R0")
_truth = {}


def truth(name, dense=False):
    """The statement's answer for a case, computed once."""
    key = (name, dense)
    if key not in _truth:
        X, Y, C, M, R, kw = ALL[name]
        _truth[key] = pr.statement(X.toarray() if dense else X, Y, C, M, R, **kw)
    return _truth[key]


def same_counters(got, want, what):
    assert {k: got[k] for k in want} == want, f"{what}: the counters differ from the statement's"


def check(name, got, err, X, dense=False):
    _, Y, C, M, R, kw = ALL[name]
    canon = bool(kw.get("max_nonzeros"))                       # there the order inside a label is std::nth_element's: the set is the contract
    assert err is None, err
    assert got["shape"] == (X.shape[1] + (kw.get("bias", 1.0) > 0), Y.shape[1])
    assert pr.same_coo(got, truth(name, dense), canon=canon), f"{name}: differs from the statement"
    if not dense:
        assert pr.same_coo(got, pr.recorded_case(RECORDED, name), canon=canon), f"{name}: differs from the recorded reference"
    if HAVE_REF:
        assert pr.same_coo(got, pr.reference(X, Y, C, M, R, **kw), canon=canon), f"{name}: differs from the live reference"
    c = pr.counters()
    same_counters(c, truth(name, dense)["counters"], name)
    assert c["jobs"] == len(truth(name, dense)["trace"]) and c["nonfinite_jobs"] == 0
    return c


@pytest.mark.parametrize("name", sorted(ALL))
def test_csr_entry_point(name):
    X, Y, C, M, R, kw = ALL[name]
    got, err = pr.run_newton(pr.OURS, X, Y, C, M, R, **kw)
    check(name, got, err, X)


@pytest.mark.parametrize("name", sorted(ALL))
def test_resident_form(name):
    X, Y, C, M, R, kw = ALL[name]
    Wt, c = pr.resident(X, Y, C, M, R, kw)
    assert Wt.shape == (Y.shape[1], X.shape[1] + (kw.get("bias", 1.0) > 0))
    assert all((np.diff(Wt.indices[Wt.indptr[l]:Wt.indptr[l + 1]]) > 0).all() for l in range(Wt.shape[0])), "a label's features ascend"
    assert pr.same_coo(pr.wt_as_coo(Wt), truth(name), canon=True), f"{name}: differs from the statement"
    assert pr.same_coo(pr.wt_as_coo(Wt), pr.recorded_case(RECORDED, name), canon=True), f"{name}: differs from the recorded reference"
    same_counters(c, truth(name)["counters"], name)
    if name.startswith("layouts"):
        assert Wt.indptr[5] == Wt.indptr[6], "a label in no column of C has an empty row"


@pytest.mark.parametrize("name", DENSE)
def test_drm_entry_point(name):
    X, Y, C, M, R, kw = ALL[name]
    assert rr.dense_ok(X)
    D = np.ascontiguousarray(X.toarray())
    got, err = pr.run_newton(pr.OURS, D, Y, C, M, R, **kw)
    check(name, got, err, D, dense=True)


def test_drm_entry_point_with_a_row_and_a_column_of_zeros():
    X, Y, C, M, R, kw = CASES["coded"]
    D = np.ascontiguousarray(X[:90, :40].toarray())
    D[7, :] = 0.0
    D[:, 11] = 0.0
    Y2, M2 = smat.csc_matrix(Y[:90]), smat.csc_matrix(M[:90])
    kw = dict(kw, threshold=0.0)
    got, err = pr.run_newton(pr.OURS, D, Y2, C, M2, **kw)
    want = pr.statement(D, Y2, C, M2, **kw)
    assert err is None and pr.same_coo(got, want) and all(t["touched"] == 40 for t in want["trace"] if t["instances"]), "a dense row stores every column"
    if HAVE_REF:
        assert pr.same_coo(got, pr.reference(D, Y2, C, M2, **kw))
    same_counters(pr.counters(), want["counters"], "dense with zeros")


def test_which_chain_form_serves_which_row():
    """Feature rows of 0, 1 and 63 entries are summed one row per lane, of 64, 65, 127 to 129 and 1000 entries by the wavefront."""
    X, Y, C, M, R, kw = CASES["row_lengths"]
    got, err = pr.run_newton(pr.OURS, X, Y, C, M, R, **kw)
    assert err is None and pr.same_coo(got, truth("row_lengths"))
    c = pr.counters()
    lens = np.diff(X.indptr)
    jobs = Y.shape[1]                                                   # pure multi-label: every job lists every row
    assert (c["lane_rows"], c["wave_rows"]) == (jobs * int((lens < 64).sum()), jobs * int((lens >= 64).sum())) == (18, 36)


def test_counters_show_every_exit():
    """Each CG exit and Newton exit the search reaches, and the halvings, ran on the device as often as in the statement."""
    seen = dict.fromkeys(pr.COUNTERS[4:], 0)
    for name in sorted(n for n in ALL if n.startswith("search_")) + ["eps0", "job_sizes", "coded"]:
        X, Y, C, M, R, kw = ALL[name]
        got, err = pr.run_newton(pr.OURS, X, Y, C, M, R, **kw)
        assert err is None and pr.same_coo(got, truth(name))
        c = pr.counters()
        same_counters(c, truth(name)["counters"], name)
        assert c["batches"] == 1 and c["hv_calls"] == c["cg_iters"] and c["newton_iters"] == c["cg_dhd"] + c["cg_q"] + c["cg_positive"] + c["cg_cap"]
        for k in seen:
            seen[k] += c[k]
    for k in ("newton_iters", "cg_iters", "halvings", "end_before_first", "end_gradient", "end_linesearch", "end_actred", "cg_dhd", "cg_q", "cg_positive", "cg_cap"):
        assert seen[k] > 0, k
    assert seen["end_cap"] == 0 and seen["nonfinite_jobs"] == 0


def test_budget_knob_one_slot_three_batches(monkeypatch):
    name = "coded_costs"
    X, Y, C, M, R, kw = CASES[name]
    got, err = pr.run_newton(pr.OURS, X, Y, C, M, R, **kw)
    assert err is None
    c = pr.counters()
    assert (c["jobs"], c["batches"]) == (24, 1) and c["slots"] > 1
    monkeypatch.setenv("XRL_TRAIN_SCRATCH_BYTES", str(8 * c["stride"] * 8))            # staging for 8 jobs; less than two slots
    got, err = pr.run_newton(pr.OURS, X, Y, C, M, R, **kw)
    c = check(name, got, err, X)
    assert (c["slots"], c["batches"]) == (1, 3)
    Wt, c = pr.resident(X, Y, C, M, R, kw)
    assert pr.same_coo(pr.wt_as_coo(Wt), truth(name), canon=True) and (c["slots"], c["batches"]) == (1, 3)


def test_caller_buffers_at_odd_offsets_between_poison_on_a_side_stream():
    import torch
    from pecos_amd import DeviceMatrix, train_layer_device
    name = "coded_costs"
    X, Y, C, M, R, kw = CASES[name]
    held = []

    def wrap(A, off):
        A = smat.csr_matrix(A)
        A.sort_indices()
        parts = []
        for arr, dtype, kind, o in ((A.indptr, np.int64, "rowptr", off), (A.indices, np.int32, "index", off + 1), (A.data, np.float32, "value", off + 2)):
            fill = dv.poison_like(kind, A.shape[1])
            whole, payload = dv.banded(np.ascontiguousarray(arr, dtype=dtype), o, dv.BAND, fill, "cuda")
            held.append((whole, payload, fill, payload.clone()))
            parts.append(payload)
        return DeviceMatrix.from_torch(parts[0], parts[1], parts[2], A.shape)

    ops = [wrap(A, off) for A, off in ((X, 1), (Y, 3), (C, 1), (M, 3), (R, 1))]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    Wt = train_layer_device(*ops, threshold=kw["threshold"], solver_type="L2R_L2LOSS_SVC_PRIMAL", Cp=kw["Cp"], Cn=kw["Cn"], stream=side.cuda_stream).download()
    assert pr.same_coo(pr.wt_as_coo(Wt), truth(name), canon=True)
    for whole, payload, fill, before in held:
        dv.assert_bands_intact(whole, payload, fill, name)
        assert torch.equal(payload.view(torch.int32), before.view(torch.int32)), "an operand changed"


# ------------------------------------------------------------------------------------------------ refusals that need the device
def test_non_finite_x_is_refused_by_the_check():
    from pecos_amd import DeviceMatrix, clib
    X, Y, C, M, R, kw = CASES["coded"]
    bad = rr.set_entries(X, {(3, 1): float("nan"), (40, 0): float("inf")})
    before = bad.data.copy()
    got, err = pr.run_newton(pr.OURS, bad, Y, C, M, **kw)
    assert got is None and err.startswith("xrl_single_layer_train_newton_csr_f32: X stores a value that is not finite")
    assert np.array_equal(bad.data.view(np.uint32), before.view(np.uint32))
    D = np.ascontiguousarray(X[:40, :30].toarray())
    D[2, 2] = -np.inf
    got, err = pr.run_newton(pr.OURS, D, smat.csc_matrix(Y[:40]), **kw)
    assert got is None and err.startswith("xrl_single_layer_train_newton_drm_f32: X stores a value that is not finite")
    x = DeviceMatrix.upload(bad)
    hs = [DeviceMatrix.upload(pr.as_stored_transpose(A)) for A in (Y, C, M)]
    with pytest.raises(Exception, match="xrl_train_layer_newton_device: X stores a value that is not finite"):
        clib.train_layer_device(x.handle, *(h.handle for h in hs), solver_type=2)
    back = x.download()
    assert np.array_equal(back.data.view(np.uint32), before.view(np.uint32)) and np.array_equal(back.indices, bad.indices), "the matrix is unchanged"
    # the same values through K13 are served (pinned by its own tests): the refusal is this solver's
    got, err = rr.run_library(rr.OURS, bad, Y, C, M, solver=rr.L2_DUAL, max_iter=3)
    assert err is None and got is not None


def test_a_non_finite_step_length_is_refused_naming_the_label():
    """A finite X whose values are huge: the statement's trace shows zTr / dHd = inf / inf in pcg.  The reference goes on with NaNs in the
    features no instance stores; the compressed form does not cover that, so the call fails and names the label -- here label 2 of three,
    beside two labels that train."""
    X, Y, _, _, _, kw = pr.nonfinite_problem()
    t = pr.statement(X, Y, **kw)["trace"][0]
    assert t["nonfinite"] == "alpha" and np.isfinite(X.data).all()
    N = X.shape[0]
    Y3 = pr.raw_csc((N, 3), [([0], [1]), ([], []), (Y.indices.tolist(), [1] * Y.nnz)])
    tr3 = pr.statement(X, Y3, **kw)["trace"]
    assert tr3[2]["nonfinite"]
    first = [t["label"] for t in tr3 if t["nonfinite"]][0]
    got, err = pr.run_newton(pr.OURS, X, Y3, **kw)
    assert got is None and err.startswith(f"xrl_single_layer_train_newton_csr_f32: label {first}: the conjugate-gradient steps met a step length that is not finite")
    from pecos_amd import DeviceMatrix, clib
    hs = [DeviceMatrix.upload(X), DeviceMatrix.upload(pr.as_stored_transpose(Y3))]
    with pytest.raises(Exception, match=f"xrl_train_layer_newton_device: label {first}: "):
        clib.train_layer_device(hs[0].handle, hs[1].handle, solver_type="L2R_L2LOSS_SVC_PRIMAL", threshold=0.0, eps=kw["eps"], bias=kw["bias"], Cp=kw["Cp"])


# ------------------------------------------------------------------------------------------------ end to end
def sorted_csc(W):
    W = smat.csc_matrix(W, dtype=np.float32, copy=True)
    W.sort_indices()
    return W


def recorded_weights(name):
    return [mr.get_sparse(RECORDED, f"e2e__{name}__W{t}", smat.csc_matrix) for t in range(int(RECORDED[f"e2e__{name}__depth"][0]))]


def test_resident_chain_against_the_host_steps():
    """label_embedding_device -> run_clustering_device -> train_chain_device with the primal solver, nothing but the weights leaving HBM,
    against the scipy loop over this library's host entry points (and through them K16's host form)."""
    import pecos_amd
    from pecos_amd import DeviceMatrix
    from pecos_amd.indexer import chain_from_partial
    X, Y, _, _ = pr.problem(300, 100, 32, 4, 8, 10, 17)
    Ycsr = smat.csr_matrix(Y)
    depth, L = 3, Y.shape[1]
    x, y = DeviceMatrix.upload(X), DeviceMatrix.upload(Ycsr)
    E = pecos_amd.label_embedding_device(y, x)
    codes = pecos_amd.run_clustering_device(E, depth, seed=2).cpu().numpy().view(np.uint32)
    C = smat.csc_matrix((np.ones(L, np.float32), (np.arange(L), codes.astype(np.int64))), shape=(L, 1 << depth))
    chain = chain_from_partial(C, min_codes=2, nr_splits=2)
    kw = dict(threshold=0.05, solver_type="L2R_L2LOSS_SVC_PRIMAL")
    weights = pecos_amd.train_chain_device(X, Ycsr, chain, "tfn", train_params=kw)
    c = pecos_amd.clib.newton_counters()
    assert c["jobs"] == L and c["newton_iters"] > 0, "the last layer trained is the leaves', by K16"
    want = mr.chain_loop(X, Y, chain, ["tfn"] * len(chain), *mr.ours_host_backend(dict(kw, eps=0.01)), [("l3-hinge", 4)] * len(chain))["W"]
    assert len(weights) == len(chain) >= 3
    for t, w in enumerate(weights):
        W = mr.wt_to_w(w.download())
        assert W.nnz > 0 and mr.same_bits(W, want[t]), f"layer {t}"
    if HAVE_REF:
        Ch = smat.csc_matrix(chain[-1], dtype=np.float32)
        Mh = smat.csc_matrix(Ycsr * smat.csr_matrix(Ch), dtype=np.float32)
        Mh.sort_indices()
        ref = pr.reference(X, Y, Ch, Mh, threshold=0.05, eps=0.01)
        assert pr.same_coo(pr.wt_as_coo(weights[-1].download()), ref, canon=True)


def test_train_device_with_matcher_aware_negatives_against_the_recorded_reference(tmp_path):
    """XLinearModel.train_device(solver_type = primal, tfn+man) -> save -> load -> predict: per-layer weights and predictions."""
    from pecos_amd import XLinearModel
    X, Y, C, R, kw = pr.e2e_kwargs("man", ours=True)
    model = XLinearModel.train_device(X, Y, C=C, **kw)
    want = recorded_weights("man")
    assert model.depth == len(want) == 3
    for t, layer in enumerate(model.model.layers):
        assert mr.same_bits(sorted_csc(layer.W), want[t]), f"layer {t}: the weights differ from the reference's"
    model.save(str(tmp_path / "m"))
    P = XLinearModel.load(str(tmp_path / "m")).predict(X[:pr.E2E_QUERIES], **pr.E2E_PREDICT_KW).tocsr()
    P.sort_indices()
    assert mr.same_bits(P, mr.get_sparse(RECORDED, "e2e__man__pred", smat.csr_matrix)), "the predictions differ from the reference's"


def test_train_ext_with_induced_relevance_against_the_recorded_reference():
    from pecos_amd import XLinearModel
    X, Y, C, R, kw = pr.e2e_kwargs("induce", ours=True)
    model = XLinearModel.train_ext(X, Y, C=C, R=R, **kw)
    want = recorded_weights("induce")
    assert model.depth == len(want)
    for t, layer in enumerate(model.model.layers):
        assert mr.same_bits(sorted_csc(layer.W), want[t]), f"layer {t}"


def test_a_solver_per_layer_against_the_recorded_reference():
    """L2R_L2LOSS_SVC_DUAL on top, L2R_L1LOSS_SVC_DUAL below, the primal solver at the leaves: train and train_ext."""
    from pecos_amd import XLinearModel
    X, Y, C, R, kw = pr.e2e_kwargs("mixed", ours=True)
    want = recorded_weights("mixed")
    for train in (XLinearModel.train, XLinearModel.train_ext):
        model = train(X, Y, C=C, **kw)
        assert model.depth == len(want) == 3
        for t, layer in enumerate(model.model.layers):
            assert mr.same_bits(sorted_csc(layer.W), want[t]), f"{train.__name__}: layer {t}"


def test_mlmodel_train_stops_at_newton_eps():
    """One layer through MLModel.train (the host entry point): eps = newton_eps = 0.01, as the reference's MLModel.train sets it."""
    from pecos_amd import MLModel
    from pecos_amd.xlinear import MLProblem
    X, Y, C, M, _, _ = CASES["coded"]
    layer = MLModel.train(MLProblem(X, Y, C=C, M=M), threshold=0.1, solver_type="L2R_L2LOSS_SVC_PRIMAL", eps=0.5)
    W = sorted_csc(layer.W)
    want = pr.statement(X, Y, C, M, threshold=0.1, eps=0.01)
    assert pr.same_coo((W.indices.astype(np.uint64), np.repeat(np.arange(W.shape[1]), np.diff(W.indptr)).astype(np.uint64), W.data), want, canon=True)
