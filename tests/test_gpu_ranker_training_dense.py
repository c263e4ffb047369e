"""Ranker training over dense features on the device (K13D): xrl_train_layer_dense_device through pecos_amd.train_layer_device on CUDA
tensors, against the numpy statement of the rule on the same ndarray (tests/ranker_training_rule.py: the CSR of all rows * cols entries) --
rows, columns and value bits, the seven solver counters, and which form served the jobs (xrl_debug_train_dense_forms)."""
import numpy as np
import pytest
import scipy.sparse as smat

import ranker_training_rule as rr
from ranker_training_rule import as_stored_transpose, wt_as_coo

pytestmark = pytest.mark.gpu

N, L, K = 24, 4, 2
COLS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1300)     # a lane's block, a step, every STEPS, the register / LDS switch, a ragged LDS row
SOLVERS = {rr.L1_DUAL: "L2R_L1LOSS_SVC_DUAL", rr.L2_DUAL: "L2R_L2LOSS_SVC_DUAL"}
_, Y, C, M = rr.problem(N, 8, L, K, 3, 6, 11)
_truth = {}


def features(cols):
    """N x cols, a third of the entries zero, dots of order one at every width."""
    rs = np.random.RandomState(cols)
    D = (rs.standard_normal((N, cols)) * (2.0 / np.sqrt(cols))).astype(np.float32)
    D[rs.rand(N, cols) < 0.33] = 0.0
    return D


def truth(key, D, Y, C, M, kw):
    """The statement's answer, computed once per key."""
    if key not in _truth:
        _truth[key] = rr.statement(D, Y, C, M, **kw)
    return _truth[key]


def on_device(D, layout):
    """D in HBM -> (the view the trainer gets, the whole buffer): contiguous; rows padded to a 16-byte multiple with NaNs in the gap; the base
    moved by one float with a row stride of cols + 3 and NaNs in the gap."""
    import torch
    rows, cols = D.shape
    stride, off = {"contiguous": (cols, 0), "padded": ((cols + 3) // 4 * 4 + 4, 0), "offset": (cols + 3, 1)}[layout]
    whole = torch.full((rows * stride + off + 4,), float("nan"), dtype=torch.float32, device="cuda")
    view = whole[off:off + rows * stride].view(rows, stride)[:, :cols]
    view.copy_(torch.from_numpy(D))
    return view, whole


def train(view, Y, C, M, kw, R=None, stream=None):
    """pecos_amd.train_layer_device on the tensor -> (W^T's COO, the solver counters, jobs by form)."""
    import pecos_amd
    from pecos_amd import clib
    before = clib.debug_train_dense_forms()
    Wt = pecos_amd.train_layer_device(view, smat.csr_matrix(Y), None if C is None else smat.csr_matrix(C), None if M is None else smat.csr_matrix(M),
                                      None if R is None else smat.csr_matrix(R), threshold=kw.get("threshold", 0.0), max_nonzeros_per_label=kw.get("max_nonzeros"),
                                      solver_type=SOLVERS[kw["solver"]], Cp=kw.get("Cp", 1.0), Cn=kw.get("Cn", 1.0), max_iter=kw["max_iter"], eps=kw.get("eps", 0.1),
                                      bias=kw.get("bias", 1.0), stream=stream).download()
    after = clib.debug_train_dense_forms()
    return wt_as_coo(Wt), clib.debug_train_counters(), (after["reg_jobs"] - before["reg_jobs"], after["lds_jobs"] - before["lds_jobs"])


def check(got, want, cols, jobs):
    coo, counters, forms = got
    assert rr.same_coo(coo, want, canon=True), "W differs from the statement"
    assert {k: counters[k] for k in want["counters"]} == want["counters"], "the counters differ from the statement's"
    assert forms == ((jobs, 0) if cols <= 1024 else (0, jobs))


@pytest.mark.parametrize("coded", [True, False], ids=["coded", "pure"])
@pytest.mark.parametrize("bias", [1.0, 0.0])
@pytest.mark.parametrize("solver", sorted(SOLVERS))
@pytest.mark.parametrize("layout", ["contiguous", "padded", "offset"])
@pytest.mark.parametrize("cols", COLS)
def test_against_the_statement(cols, layout, solver, bias, coded):
    import torch
    D = features(cols)
    kw = dict(solver=solver, bias=bias, threshold=0.01 if coded else 0.0, max_iter=6, eps=0.01)
    c, m = (C, M) if coded else (None, None)
    want = truth((cols, solver, bias, coded), D, Y, c, m, kw)
    view, whole = on_device(D, layout)
    before = whole.clone()
    check(train(view, Y, c, m, kw), want, cols, L)
    assert len(want["vals"]) > 0 and torch.equal(whole.view(torch.int32), before.view(torch.int32)), "X or the poison around it changed"


@pytest.mark.parametrize("cols", [70, 1100])
def test_a_job_without_instances(cols):
    """Label 3 has no positive and is alone under a code whose M column is empty: its job lists nothing and, under threshold 0, emits zeros."""
    Ye = rr.raw_csc((N, L), [(Y.indices[Y.indptr[l]:Y.indptr[l + 1]], np.ones(Y.indptr[l + 1] - Y.indptr[l])) for l in range(3)] + [([], [])])
    Ce = rr.raw_csc((L, K), [([0, 1, 2], [1, 1, 1]), ([3], [1])])
    Me = rr.raw_csc((N, K), [(list(range(0, N, 2)), [1] * (N // 2)), ([], [])])
    D, kw = features(cols), dict(solver=rr.L2_DUAL, threshold=0.0, max_iter=5)
    want = truth(("empty", cols), D, Ye, Ce, Me, kw)
    assert want["per_job"][-1] == (3, 1, 0)
    check(train(on_device(D, "contiguous")[0], Ye, Ce, Me, kw), want, cols, L)


@pytest.mark.parametrize("cols", [70, 1100])
def test_non_finite_entries_meet_stored_zeros(cols):
    """Row 2 holds an inf in a column where every other row stores 0 (0 * NaN in every other row's dot), row 7 a NaN."""
    D = features(cols)
    D[:, 5] = 0.0
    D[2, 5], D[7, cols - 1] = np.inf, np.nan
    for solver in sorted(SOLVERS):
        kw = dict(solver=solver, threshold=0.0, max_iter=5)
        want = truth(("nonfinite", cols, solver), D, Y, None, None, kw)
        assert want["trace"]["nan_w_setup"] >= 2 * L and want["trace"]["dot_nonfinite"] > 0
        check(train(on_device(D, "offset")[0], Y, None, None, kw), want, cols, L)


def test_max_nonzeros_with_the_bias_competing():
    """The hand-off to the shared emission: duplicated columns tie in |w| and the bias displaces the least kept feature."""
    Xt, _ = rr.ties_problem()
    D = np.ascontiguousarray(Xt.toarray())
    rare = rr.raw_csc((D.shape[0], 2), [([3, 17, 40], [1, 1, 1]), ([3], [1])])
    for k in (1, 2, 5):
        kw = dict(solver=rr.L1_DUAL, max_nonzeros=k, threshold=0.0, max_iter=10)
        want = truth(("maxnz", k), D, rare, None, None, kw)
        check(train(on_device(D, "contiguous")[0], rare, None, None, kw), want, D.shape[1], 2)
    assert (want["rows"] == D.shape[1]).any(), "the bias is kept"


def test_on_a_side_stream_with_costs():
    import torch
    D, R = features(300), rr.relevance(Y, 5)
    kw = dict(solver=rr.L2_DUAL, Cp=2.0, Cn=0.5, threshold=0.01, max_iter=6)
    want = rr.statement(D, Y, C, M, R, **kw)
    view, whole = on_device(D, "offset")
    before = whole.clone()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    check(train(view, Y, C, M, kw, R=R, stream=side.cuda_stream), want, 300, L)
    assert torch.equal(whole.view(torch.int32), before.view(torch.int32))


def test_refusals_by_the_check_kernels():
    import torch
    from pecos_amd import DeviceMatrix, clib
    X = torch.from_numpy(features(20)).cuda()
    args = (0, X.data_ptr(), N, 20, 20)
    hs = {k: DeviceMatrix.upload(as_stored_transpose(A)) for k, A in (("Y", Y), ("C", C), ("M", M))}
    twice = DeviceMatrix.upload(as_stored_transpose(rr.raw_csc((L, K), [([0, 1, 2], [1, 1, 1]), ([2, 3], [1, 1])])))
    with pytest.raises(RuntimeError, match="xrl_train_layer_dense_device: a label is listed under two columns of C"):
        clib.train_layer_dense_device(*args, hs["Y"].handle, twice.handle, hs["M"].handle)
    R = rr.relevance(Y, 1)
    R.indices = R.indices.copy()
    R.indices[0] = (R.indices[0] + 7) % N
    rt = DeviceMatrix.upload(as_stored_transpose(R))
    with pytest.raises(RuntimeError, match="xrl_train_layer_dense_device: Rt does not share Yt's pattern"):
        clib.train_layer_dense_device(*args, hs["Y"].handle, hs["C"].handle, hs["M"].handle, rt.handle)
    bad = Y.copy()
    bad.indices = bad.indices.copy()
    bad.indices[0] = N
    yt = DeviceMatrix.upload(as_stored_transpose(bad))
    with pytest.raises(RuntimeError, match=f"xrl_train_layer_dense_device: Y holds an id that is not below {N}"):
        clib.train_layer_dense_device(*args, yt.handle)


def test_resident_chain_against_the_host_path():
    """label_embedding_dense_device -> run_clustering_device -> train_layer_device, all on tensors, against the same steps through the host
    entry points."""
    import torch
    import clustering_rule as cr
    import pecos_amd
    from pecos_amd import DeviceMatrix, clib
    from pecos_amd.core import ScipyCscF32, ScipyDrmF32
    from pecos_amd.embedding import LabelEmbeddingFactory
    _, Yc, _, _ = rr.problem(300, 8, 40, 4, 3, 9, 23)
    D = np.random.RandomState(3).standard_normal((300, 96)).astype(np.float32)
    Ycsr, depth, labels = smat.csr_matrix(Yc), 3, Yc.shape[1]
    Xd = torch.from_numpy(D).cuda()
    E = pecos_amd.label_embedding_dense_device(Ycsr, Xd)
    codes = pecos_amd.run_clustering_device(E, depth, seed=2)
    Cdev = DeviceMatrix.from_torch(torch.arange(labels + 1, dtype=torch.int64, device="cuda"), codes.contiguous(), torch.ones(labels, dtype=torch.float32, device="cuda"),
                                   (labels, 1 << depth))
    Wt = pecos_amd.train_layer_device(Xd, Ycsr, Cdev, threshold=0.05, solver_type="L2R_L1LOSS_SVC_DUAL", max_iter=10).download()
    Eh = LabelEmbeddingFactory.create(Ycsr, D, method="pifa")
    ch, err = cr.run_library(rr.OURS, Eh, depth, seed=2)
    assert err is None and np.array_equal(ch, codes.cpu().numpy().view(np.uint32))
    Ch = smat.csc_matrix((np.ones(labels, dtype=np.float32), (np.arange(labels), ch.astype(np.int64))), shape=(labels, 1 << depth))
    Mh = clib.sparse_matmul(smat.csc_matrix(Yc), Ch).tocsc()
    Mh.sort_indices()
    W = clib.xlinear_single_layer_train(ScipyDrmF32.init_from(D), ScipyCscF32(smat.csc_matrix(Yc)), ScipyCscF32(Ch), ScipyCscF32(Mh), None, threshold=0.05,
                                        solver_type="L2R_L1LOSS_SVC_DUAL", max_iter=10)
    W.sort_indices()
    Wd = smat.csc_matrix((Wt.data, Wt.indices, Wt.indptr), shape=W.shape)
    assert W.nnz > 0 and np.array_equal(W.indptr, Wd.indptr) and np.array_equal(W.indices, Wd.indices) and np.array_equal(W.data.view(np.uint32), Wd.data.view(np.uint32))
