"""Ranker training on the device (K13): xrl_single_layer_train_csr_f32, xrl_single_layer_train_drm_f32 and
xrl_train_layer_device against the numpy statement of the rule (tests/ranker_training_rule.py), the compiled reference as recorded in
tests/golden/ranker_training_ref.npz and, where oracle/_ref is built, the live reference library -- rows, cols and value bits; what
ran, from the counters, against the statement's own counters."""
import os

import numpy as np
import pytest
import scipy.sparse as smat

import ranker_training_rule as rr
from conftest import GOLDEN
from ranker_training_rule import as_stored_transpose, resident, wt_as_coo

pytestmark = pytest.mark.gpu

CASES = rr.cases()
RECORDED = np.load(os.path.join(GOLDEN, "ranker_training_ref.npz"))
HAVE_REF = os.path.exists(rr.REF)
DENSE = ("coded_l1", "coded_l2_costs", "pure_l2", "bias0.0_l1", "bias0.5_l2", "layouts_l1_R", "layouts_l2", "maxnz5_l2", "thr_all_l2", "ties_bias_l1")
SOLVER_NAMES = {rr.L1_DUAL: "L2R_L1LOSS_SVC_DUAL", rr.L2_DUAL: "L2R_L2LOSS_SVC_DUAL"}
_truth = {}


def truth(name, dense=False):
    """The statement's answer for a case, computed once."""
    key = (name, dense)
    if key not in _truth:
        X, Y, C, M, R, kw = CASES[name]
        _truth[key] = rr.statement(X.toarray() if dense else X, Y, C, M, R, **kw)
    return _truth[key]


def recorded(name):
    return RECORDED[f"case__{name}__rows"].astype(np.uint64), RECORDED[f"case__{name}__cols"].astype(np.uint64), RECORDED[f"case__{name}__vals"]


def same_counters(name, dense=False):
    got, want = rr.counters(), truth(name, dense)["counters"]
    assert {k: got[k] for k in want} == want, f"{name}: the counters differ from the statement's"
    return got


def check(name, got, err, X, dense=False):
    _, Y, C, M, R, kw = CASES[name]
    canon = bool(kw.get("max_nonzeros"))                       # there the order inside a label is std::nth_element's: the set is the contract
    assert err is None, err
    assert got["shape"] == (X.shape[1] + (kw.get("bias", 1.0) > 0), Y.shape[1])
    assert rr.same_coo(got, truth(name, dense), canon=canon), f"{name}: differs from the statement"
    if not dense:
        assert rr.same_coo(got, recorded(name), canon=canon), f"{name}: differs from the recorded reference"
    if HAVE_REF:
        assert rr.same_coo(got, rr.reference(X, Y, C, M, R, **kw), canon=canon), f"{name}: differs from the live reference"
    same_counters(name, dense)


@pytest.mark.parametrize("name", sorted(CASES))
def test_csr_entry_point(name):
    X, Y, C, M, R, kw = CASES[name]
    got, err = rr.run_library(rr.OURS, X, Y, C, M, R, **kw)
    check(name, got, err, X)


@pytest.mark.parametrize("name", DENSE)
def test_drm_entry_point(name):
    X, Y, C, M, R, kw = CASES[name]
    assert rr.dense_ok(X)
    D = np.ascontiguousarray(X.toarray())
    got, err = rr.run_library(rr.OURS, D, Y, C, M, R, **kw)
    check(name, got, err, D, dense=True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_resident_form(name):
    X, Y, C, M, R, kw = CASES[name]
    Wt, _ = resident(X, Y, C, M, R, kw)
    assert Wt.shape == (Y.shape[1], X.shape[1] + (kw.get("bias", 1.0) > 0))
    assert all((np.diff(Wt.indices[Wt.indptr[l]:Wt.indptr[l + 1]]) > 0).all() for l in range(Wt.shape[0])), "a label's features ascend"
    # W^T by label is the canonical order of the COO; a label in no column of C has an empty row
    assert rr.same_coo(wt_as_coo(Wt), truth(name), canon=True), f"{name}: differs from the statement"
    assert rr.same_coo(wt_as_coo(Wt), recorded(name), canon=True), f"{name}: differs from the recorded reference"
    same_counters(name)
    if name.startswith("layouts"):
        assert Wt.indptr[5] == Wt.indptr[6]


@pytest.mark.parametrize("shape", [(0, 5, 2), (4, 5, 0), (4, 0, 2)], ids=["no_rows", "no_labels", "no_features"])
def test_empty_shapes(shape):
    """No instances (every job emits its zero bias under threshold 0), no labels (no job), no features (the bias alone is trained)."""
    N, d, L = shape
    X = smat.csr_matrix((N, d), dtype=np.float32)
    Y = rr.raw_csc((N, L), [(list(range(0, N, 2)), [1.0] * len(range(0, N, 2)))] * L)
    for kw in (dict(threshold=0.0, max_iter=5), dict(threshold=0.1, max_iter=5, solver=rr.L2_DUAL)):
        got, err = rr.run_library(rr.OURS, X, Y, **kw)
        assert err is None, err
        assert got["shape"] == (d + 1, L) and rr.same_coo(got, rr.statement(X, Y, **kw))
        if HAVE_REF:
            assert rr.same_coo(got, rr.reference(X, Y, **kw))
        Wt, _ = resident(X, Y, None, None, None, kw)
        assert Wt.shape == (L, d + 1) and rr.same_coo(wt_as_coo(Wt), got, canon=True)


def test_which_chain_form_serves_which_row():
    """x'x of rows of 0, 1 and 63 entries is summed one row per lane, of 64, 65, 127 to 129 and 1000 entries by the wavefront."""
    name = "row_lengths_l2"
    X, Y, C, M, R, kw = CASES[name]
    got, err = rr.run_library(rr.OURS, X, Y, C, M, R, **kw)
    assert err is None and rr.same_coo(got, truth(name))
    c = rr.counters()
    lens = np.diff(X.indptr)
    jobs = Y.shape[1]                                                   # pure multi-label: every job lists every row
    assert (c["lane_rows"], c["wave_rows"]) == (jobs * int((lens < 64).sum()), jobs * int((lens >= 64).sum())) == (18, 36)


def test_counters_show_every_path():
    """Shrinking, re-activation, clipping at C under the L1 loss and a stop by max_iter ran on the device as often as in the statement."""
    for name in ("shrink_l1", "shrink_l2", "stop_l1"):
        X, Y, C, M, R, kw = CASES[name]
        got, err = rr.run_library(rr.OURS, X, Y, C, M, R, **kw)
        assert err is None and rr.same_coo(got, truth(name))
        c = same_counters(name)
        if name == "shrink_l1":
            assert c["shrinks"] > 0 and c["reactivations"] > 0 and c["clipped"] > 0 and c["max_iter_stops"] > 0
        assert c["extensions"] == 0 and c["batches"] == 1


def test_budget_knob_one_slot_three_batches(monkeypatch):
    name = "coded_l2_costs"
    X, Y, C, M, R, kw = CASES[name]
    got, err = rr.run_library(rr.OURS, X, Y, C, M, R, **kw)
    assert err is None
    c = rr.counters()
    assert (c["jobs"], c["batches"]) == (24, 1) and c["slots"] > 1
    monkeypatch.setenv("XRL_TRAIN_SCRATCH_BYTES", str(8 * c["stride"] * 8))            # staging for 8 jobs; less than two slots
    got, err = rr.run_library(rr.OURS, X, Y, C, M, R, **kw)
    check(name, got, err, X)
    c = rr.counters()
    assert (c["slots"], c["batches"]) == (1, 3)
    Wt, c = resident(X, Y, C, M, R, kw)
    assert rr.same_coo(wt_as_coo(Wt), truth(name), canon=True) and (c["slots"], c["batches"]) == (1, 3)


def test_table_knob_jobs_cross_the_tables_end(monkeypatch):
    name = "coded_l1"
    X, Y, C, M, R, kw = CASES[name]
    monkeypatch.setenv("XRL_TRAIN_RANDOM_WORDS", "64")
    got, err = rr.run_library(rr.OURS, X, Y, C, M, R, **kw)
    check(name, got, err, X)
    c = rr.counters()
    assert c["extensions"] >= 2 and c["reruns"] >= c["extensions"]


@pytest.mark.parametrize("n", rr.BIG_JOBS)
def test_jobs_around_the_shuffles_switch(n):
    """65 535 instances are shuffled two positions per draw, 65 536 and more one per draw."""
    X, Y, kw = rr.big_job(n)
    got, err = rr.run_library(rr.OURS, X, Y, **kw)
    assert err is None, err
    assert rr.digest(got) == str(RECORDED[f"digest__big{n}"])
    if HAVE_REF:
        assert rr.same_coo(got, rr.reference(X, Y, **kw))
    c = rr.counters()
    assert (c["jobs"], c["iters"], c["lane_rows"]) == (1, 2, n)


def test_scale_against_the_reference():
    X, Y, C, M, kw = rr.scale_problem()
    got, err = rr.run_library(rr.OURS, X, Y, C, M, **kw)
    assert err is None, err
    assert rr.counters()["jobs"] == 2000
    assert rr.digest(got) == str(RECORDED["digest__scale"])
    if HAVE_REF:
        assert rr.same_coo(got, rr.reference(X, Y, C, M, **kw))


def test_caller_buffers_at_odd_offsets_on_a_side_stream():
    import torch
    from pecos_amd import DeviceMatrix, train_layer_device
    name = "coded_l1_costs"
    X, Y, C, M, R, kw = CASES[name]
    poison = 0x5EADBEEF

    def embed(arr, dtype, off):
        """arr inside a poisoned buffer at element offset off -> (view, whole buffer)"""
        whole = torch.full((len(arr) + 2 * off + 5,), poison, dtype=torch.int64, device="cuda").to(dtype) if dtype != torch.float32 else \
            torch.full((len(arr) + 2 * off + 5,), float("nan"), dtype=torch.float32, device="cuda")
        whole[off:off + len(arr)] = torch.from_numpy(np.ascontiguousarray(arr)).to(dtype).cuda()
        return whole[off:off + len(arr)], whole

    held = []

    def wrap(A, off):
        A = smat.csr_matrix(A)
        A.sort_indices()
        parts = [embed(A.indptr, torch.int64, off), embed(A.indices, torch.int32, off + 1), embed(A.data.astype(np.float32), torch.float32, off + 2)]
        held.extend((v.clone(), w, w.clone()) for v, w in parts)
        return DeviceMatrix.from_torch(parts[0][0], parts[1][0], parts[2][0], A.shape)

    ops = [wrap(A, off) for A, off in ((X, 1), (Y, 3), (C, 5), (M, 7), (R, 9))]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    Wt = train_layer_device(*ops, threshold=kw["threshold"], solver_type=SOLVER_NAMES[kw["solver"]], Cp=kw["Cp"], Cn=kw["Cn"], max_iter=kw["max_iter"],
                            stream=side.cuda_stream).download()
    assert rr.same_coo(wt_as_coo(Wt), truth(name), canon=True)
    for _, whole, before in held:
        assert torch.equal(whole.view(torch.int32), before.view(torch.int32)), "an operand or the poison around it changed"


def test_resident_chain_against_the_host_path():
    """label_embedding_device -> run_clustering_device -> train_layer_device, nothing but the weights leaving HBM, against the host entry
    points fed the same way."""
    import torch
    import pecos_amd
    from pecos_amd import DeviceMatrix, clib
    from pecos_amd.core import ScipyCscF32, ScipyCsrF32
    X, Y, _, _ = rr.problem(400, 150, 48, 4, 8, 10, 17)
    Ycsr = smat.csr_matrix(Y)
    depth, L = 3, Y.shape[1]
    x, y = DeviceMatrix.upload(X), DeviceMatrix.upload(Ycsr)
    E = pecos_amd.label_embedding_device(y, x)
    codes = pecos_amd.run_clustering_device(E, depth, seed=2)
    dev = codes.device
    Cdev = DeviceMatrix.from_torch(torch.arange(L + 1, dtype=torch.int64, device=dev), codes.contiguous(), torch.ones(L, dtype=torch.float32, device=dev), (L, 1 << depth))
    Wt = pecos_amd.train_layer_device(x, y, Cdev, threshold=0.05, solver_type="L2R_L1LOSS_SVC_DUAL", max_iter=30).download()
    # the host path
    Eh = pecos_amd.LabelEmbeddingFactory.create(Ycsr, X, method="pifa")
    ch, err = __import__("clustering_rule").run_library(rr.OURS, Eh, depth, seed=2)
    assert err is None and np.array_equal(ch, codes.cpu().numpy().view(np.uint32))
    Ch = smat.csc_matrix((np.ones(L, dtype=np.float32), (np.arange(L), ch.astype(np.int64))), shape=(L, 1 << depth))
    Mh = clib.sparse_matmul(smat.csc_matrix(Y), Ch).tocsc()
    Mh.sort_indices()
    W = clib.xlinear_single_layer_train(ScipyCsrF32(X), ScipyCscF32(smat.csc_matrix(Y)), ScipyCscF32(Ch), ScipyCscF32(Mh), None, threshold=0.05,
                                        solver_type="L2R_L1LOSS_SVC_DUAL", max_iter=30)
    W.sort_indices()
    Wd = smat.csc_matrix((Wt.data, Wt.indices, Wt.indptr), shape=W.shape)
    assert np.array_equal(W.indptr, Wd.indptr) and np.array_equal(W.indices, Wd.indices) and np.array_equal(W.data.view(np.uint32), Wd.data.view(np.uint32))
    assert W.nnz > 0
    if HAVE_REF:
        ref = rr.reference(X, Y, Ch, Mh, threshold=0.05, solver=rr.L1_DUAL, max_iter=30)
        assert rr.same_coo(wt_as_coo(Wt), ref, canon=True)


def test_python_form_computes_m_and_transposes():
    """pecos_amd.train_layer_device from scipy operands, M left to the device sparse product."""
    import pecos_amd
    name = "coded_l2"
    X, Y, C, M, R, kw = CASES[name]
    Wt = pecos_amd.train_layer_device(X, smat.csr_matrix(Y), smat.csr_matrix(C), threshold=kw["threshold"], solver_type=SOLVER_NAMES[kw["solver"]],
                                      max_iter=kw["max_iter"]).download()
    assert rr.same_coo(wt_as_coo(Wt), truth(name), canon=True)
    name = "pure_l1"
    X, Y, C, M, R, kw = CASES[name]
    Wt = pecos_amd.train_layer_device(X, smat.csr_matrix(Y), threshold=kw["threshold"], solver_type=SOLVER_NAMES[kw["solver"]], max_iter=kw["max_iter"]).download()
    assert rr.same_coo(wt_as_coo(Wt), truth(name), canon=True)


def _recorded_layers():
    def mat(d, tag):
        return smat.csc_matrix((RECORDED[f"e2e__{d}__{tag}__data"], RECORDED[f"e2e__{d}__{tag}__indices"], RECORDED[f"e2e__{d}__{tag}__indptr"]),
                               shape=tuple(RECORDED[f"e2e__{d}__{tag}__shape"]))
    return [(mat(d, "W"), mat(d, "C")) for d in range(int(RECORDED["e2e__depth"][0]))]


def test_end_to_end_train_save_load_predict(tmp_path):
    """XLinearModel.train -> save -> load -> predict; per-layer W equals the reference's recorded weights, and the predictions equal those
    of the recorded weights written as a folder and loaded by this library."""
    from pecos_amd import HierarchicalMLModel, MLModel, XLinearModel
    X, Y, C = rr.e2e_problem()
    model = XLinearModel.train(X, Y, C=C, **rr.E2E_KW)
    want = _recorded_layers()
    assert model.depth == len(want) == 3
    for layer, (W, Cm) in zip(model.model.layers, want):
        got = layer.W.tocsc()
        got.sort_indices()
        assert got.shape == W.shape and np.array_equal(got.indptr, W.indptr) and np.array_equal(got.indices, W.indices)
        assert np.array_equal(got.data.view(np.uint32), W.data.view(np.uint32)), "a layer's weights differ from the reference's"
        assert (smat.csc_matrix(layer.C) != Cm).nnz == 0
    model.save(str(tmp_path / "ours"))
    loaded = XLinearModel.load(str(tmp_path / "ours"))
    assert (loaded.depth, loaded.nr_features, loaded.nr_labels) == (3, 200, 64)
    pp = MLModel.PredParams(only_topk=rr.E2E_KW["beam_size"], post_processor=rr.E2E_KW["post_processor"])
    last = MLModel.PredParams(only_topk=rr.E2E_KW["only_topk"], post_processor=rr.E2E_KW["post_processor"])
    ref_layers = [MLModel(W=W, C=Cm, bias=1.0, pred_params=last if d == 2 else pp) for d, (W, Cm) in enumerate(want)]
    ref_model = XLinearModel(HierarchicalMLModel._from_layers(ref_layers, HierarchicalMLModel.PredParams(model_chain=[pp, pp, last])))
    ref_model.save(str(tmp_path / "ref"))
    recorded_model = XLinearModel.load(str(tmp_path / "ref"))
    Xq = X[:100]
    a, b, c = loaded.predict(Xq), recorded_model.predict(Xq), model.predict(Xq)
    assert a.nnz == 100 * rr.E2E_KW["only_topk"]
    for other in (b, c):
        assert np.array_equal(a.indptr, other.indptr) and np.array_equal(a.indices, other.indices) and np.array_equal(a.data.view(np.uint32), other.data.view(np.uint32))


def test_refusals_by_the_check_kernels():
    X, Y, C, M = rr.problem(30, 12, 6, 2, 3, 4, 3)
    start = "xrl_single_layer_train_csr_f32: "
    U = X.copy()
    b = int(np.flatnonzero(np.diff(U.indptr) >= 2)[0])
    U.indices = U.indices.copy()
    U.indices[U.indptr[b]], U.indices[U.indptr[b] + 1] = U.indices[U.indptr[b] + 1], U.indices[U.indptr[b]]
    got, err = rr.run_library(rr.OURS, U, Y, C, M)
    assert got is None and err == start + "X has a row whose column ids are not strictly ascending"
    U.indices[U.indptr[b]] = U.indices[U.indptr[b] + 1]                  # a duplicated column
    assert rr.run_library(rr.OURS, U, Y, C, M)[1] == start + "X has a row whose column ids are not strictly ascending"
    U.indices[U.indptr[b]] = 12
    assert rr.run_library(rr.OURS, U, Y, C, M)[1] == start + "X holds an id that is not below 12"
    for name, pos in (("Y", 1), ("M", 3)):
        ops = [X, Y.copy(), C, M.copy()]
        ops[pos].indices = ops[pos].indices.copy()
        ops[pos].indices[0] = 30
        assert rr.run_library(rr.OURS, *ops)[1] == start + f"{name} holds an id that is not below 30"
    # the resident form finds a label listed twice, and an R with another pattern, on the device
    twice = rr.raw_csc((6, 2), [([0, 1, 2], [1, 1, 1]), ([2, 3, 4, 5], [1, 1, 1, 1])])
    with pytest.raises(RuntimeError, match="xrl_train_layer_device: a label is listed under two columns of C"):
        resident(X, Y, twice, M, None, {})
    R = rr.relevance(Y, 1)
    R.indices = R.indices.copy()
    R.indices[0] = (R.indices[0] + 7) % 30
    with pytest.raises(RuntimeError, match="xrl_train_layer_device: Rt does not share Yt's pattern"):
        resident(X, Y, C, M, R, {})
    # a handle that claims one stored entry more than its row pointer covers would run one job more under the last cluster
    import torch
    from pecos_amd import DeviceMatrix, clib
    Ct = as_stored_transpose(C)
    long_ct = DeviceMatrix.from_torch(torch.from_numpy(Ct.indptr.astype(np.int64)).cuda(), torch.from_numpy(np.append(Ct.indices, 0).astype(np.int32)).cuda(),
                                      torch.ones(Ct.nnz + 1, dtype=torch.float32, device="cuda"), Ct.shape)
    hs = [DeviceMatrix.upload(X), DeviceMatrix.upload(as_stored_transpose(Y)), long_ct, DeviceMatrix.upload(as_stored_transpose(M))]
    with pytest.raises(RuntimeError, match="xrl_train_layer_device: C's row pointer does not ascend from 0 to its count of stored entries"):
        clib.train_layer_device(*(h.handle for h in hs))
