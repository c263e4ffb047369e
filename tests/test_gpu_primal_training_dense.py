"""Primal L2-loss SVC training over dense features on the device (K16D): xrl_train_layer_newton_dense_device through
pecos_amd.train_layer_device on CUDA tensors, against the numpy statement of the rule on the same ndarray (tests/primal_training_rule.py:
the CSR of all rows * cols entries) -- rows, columns and value bits, the solver's counters, and which form served the jobs
(xrl_debug_newton_dense_forms).  Every comparison is bit equality or an exact count: both sides run IEEE-correct + - * / sqrt on fp32 and
fp64 values in one fixed order, so no tolerance is needed."""
import numpy as np
import pytest
import scipy.sparse as smat

import primal_training_rule as pr
import ranker_training_rule as rr
from ranker_training_rule import as_stored_transpose, wt_as_coo

pytestmark = pytest.mark.gpu

N, L, K = 40, 6, 2
PRIMAL = "L2R_L2LOSS_SVC_PRIMAL"
COLS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025)          # a lane's float4, the 32-column panel, the 256-column step; "lds" / "scratch": the switch
MODES = {"coded_bias": dict(bias=1.0, threshold=0.01), "pure_nobias": dict(bias=0.0, threshold=0.0)}
_, Y, C, M = rr.problem(N, 8, L, K, 3, 6, 11)
_truth = {}


def features(rows, cols):
    """rows x cols, a third of the entries zero, dots of order one at every width."""
    rs = np.random.RandomState(cols)
    D = (rs.standard_normal((rows, cols)) * (2.0 / np.sqrt(cols))).astype(np.float32)
    D[rs.rand(rows, cols) < 0.33] = 0.0
    return D


def truth(key, D, Y, C, M, R, kw):
    """The statement's answer, computed once per key."""
    if key not in _truth:
        _truth[key] = pr.statement(D, Y, C, M, R, **kw)
    return _truth[key]


def on_device(D, layout="contiguous"):
    """D in HBM -> (the view the trainer gets, the whole buffer), NaNs around it: contiguous; a row stride of cols + 3 (rows not 16-byte
    aligned); a row window that starts one float into a buffer whose row stride is a multiple of four."""
    import torch
    rows, cols = D.shape
    stride, off = {"contiguous": (cols, 0), "strided": (cols + 3, 0), "window": ((cols + 3) // 4 * 4 + 4, 1)}[layout]
    whole = torch.full((rows * stride + off + 4,), float("nan"), dtype=torch.float32, device="cuda")
    view = whole[off:off + rows * stride].view(rows, stride)[:, :cols]
    view.copy_(torch.from_numpy(D))
    return view, whole


def train(view, Y, C, M, R, kw):
    """pecos_amd.train_layer_device on the tensor -> (W^T's COO, the solver's counters, jobs by form)."""
    import pecos_amd
    from pecos_amd import clib
    before = clib.debug_newton_dense_forms()
    csr = lambda A: None if A is None else smat.csr_matrix(A)
    Wt = pecos_amd.train_layer_device(view, csr(Y), csr(C), csr(M), csr(R), threshold=kw.get("threshold", 0.0), max_nonzeros_per_label=kw.get("max_nonzeros"),
                                      solver_type=PRIMAL, Cp=kw.get("Cp", 1.0), Cn=kw.get("Cn", 1.0), eps=kw.get("eps", 0.1), bias=kw.get("bias", 1.0)).download()
    after = clib.debug_newton_dense_forms()
    return wt_as_coo(Wt), clib.newton_counters(), (after["lds_jobs"] - before["lds_jobs"], after["scratch_jobs"] - before["scratch_jobs"])


def check(got, want, cols):
    from pecos_amd import clib
    coo, counters, forms = got
    jobs = len(want["trace"])
    assert rr.same_coo(coo, want, canon=True), "W differs from the statement"
    assert pr.same_counters(counters, want["counters"]) and counters["jobs"] == jobs, "the counters differ from the statement's"
    assert forms == ((jobs, 0) if cols <= clib.debug_newton_dense_forms()["lds_cols"] else (0, jobs))


def iterates(want):
    """By the statement's own trace, a job runs two Newton iterations and a CG run two steps."""
    return any(t["newton_iters"] >= 2 for t in want["trace"]) and any(max(t["cg_iters"], default=0) >= 2 for t in want["trace"])


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("layout", ["contiguous", "strided", "window"])
@pytest.mark.parametrize("cols", COLS + ("lds", "scratch"))
def test_against_the_statement(cols, layout, mode):
    import torch
    from pecos_amd import clib
    if isinstance(cols, str):
        cols = clib.debug_newton_dense_forms()["lds_cols"] + (cols == "scratch")
    D, kw = features(N, cols), dict(MODES[mode], eps=0.01)
    c, m = (C, M) if mode == "coded_bias" else (None, None)
    want = truth((cols, mode), D, Y, c, m, None, kw)
    assert cols == 1 or iterates(want)                         # (one feature: the first Newton step is the last)
    view, whole = on_device(D, layout)
    before = whole.clone()
    check(train(view, Y, c, m, None, kw), want, cols)
    assert len(want["vals"]) > 0 and torch.equal(whole.view(torch.int32), before.view(torch.int32)), "X or the poison around it changed"


def test_instances_per_job_at_the_row_tile():
    """One code and one label per size: the code's M column lists that many rows and every third of them is positive."""
    sizes = (0, 1, 63, 64, 65, 130)
    rows = [list(range(k, k + n)) for k, n in enumerate(sizes)]
    Ys = rr.raw_csc((140, len(sizes)), [(r[::3], [1] * len(r[::3])) for r in rows])
    Cs = rr.raw_csc((len(sizes), len(sizes)), [([k], [1]) for k in range(len(sizes))])
    Ms = rr.raw_csc((140, len(sizes)), [(r, [1] * len(r)) for r in rows])
    D, kw = features(140, 70), dict(eps=0.01, threshold=0.0)
    want = truth("sizes", D, Ys, Cs, Ms, None, kw)
    assert tuple(t["instances"] for t in want["trace"]) == sizes and iterates(want)
    check(train(on_device(D)[0], Ys, Cs, Ms, None, kw), want, 70)


@pytest.mark.parametrize("case", ["alias", "zeros_costs"])
def test_aliasing_and_zeros(case):
    """grad's compaction into tmp overwritten by a later instance; a row and a column of zeros under Cp != Cn with R."""
    if case == "alias":
        X, Ya, Ca, Ma = pr.alias_problem()
        D, ops, kw = np.ascontiguousarray(X.toarray()), (Ya, Ca, Ma, None), dict(eps=0.01, threshold=0.0)
    else:
        D = features(N, 70)
        D[7, :] = 0.0
        D[:, 11] = 0.0
        ops, kw = (Y, C, M, rr.relevance(Y, 5)), dict(eps=0.01, threshold=0.0, Cp=2.0, Cn=0.5)
    want = truth(case, D, *ops, kw)
    assert want["trace"][0]["alias_overwrites"] > 0 if case == "alias" else iterates(want)
    check(train(on_device(D, "strided")[0], *ops, kw), want, D.shape[1])


def test_refusals():
    import torch
    import pecos_amd
    from pecos_amd import DeviceMatrix, clib
    D = features(N, 70)
    D[N - 1, 69] = np.inf
    view, whole = on_device(D, "window")
    before = whole.clone()
    with pytest.raises(RuntimeError, match="xrl_train_layer_newton_dense_device: X stores a value that is not finite"):
        pecos_amd.train_layer_device(view, smat.csr_matrix(Y), solver_type=PRIMAL)
    assert torch.equal(whole.view(torch.int32), before.view(torch.int32))
    with pytest.raises(RuntimeError, match="xrl_train_layer_newton_dense_device: 16385 columns: a dense X is served up to 16384"):
        pecos_amd.train_layer_device(torch.zeros((N, 16385), device="cuda"), smat.csr_matrix(Y), solver_type=PRIMAL)
    yt = DeviceMatrix.upload(as_stored_transpose(Y))
    with pytest.raises(RuntimeError, match="xrl_train_layer_newton_dense_device: solver L2R_L2LOSS_SVC_DUAL is served by .*xrl_train_layer_dense_device"):
        clib.train_layer_newton_dense_device(0, view.data_ptr(), N, 70, view.stride(0), yt.handle, solver_type=1)


def test_the_host_entry_point_takes_the_same_route():
    from pecos_amd import clib
    D, kw = features(N, 300), dict(eps=0.01, threshold=0.01)
    coo, _, _ = train(on_device(D)[0], Y, C, M, None, kw)
    before = clib.debug_newton_dense_forms()["lds_jobs"]
    got, err = pr.run_newton(pr.OURS, D, Y, C, M, **kw)
    assert err is None and rr.same_coo(got, coo, canon=True) and len(coo[2]) > 0
    assert clib.debug_newton_dense_forms()["lds_jobs"] - before == C.nnz, "K16D served the host entry point's jobs"
