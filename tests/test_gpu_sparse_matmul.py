"""Sparse matrix products on the device (K10): every result is compared bit for bit -- row pointer, indices, value bits -- with the numpy
restatement of the rule (tests/sparse_matmul_rule.py) and, where oracle/_ref is built and can hold the case, with the live reference."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as smat

import device_views as dv
import sparse_matmul_rule as R
from conftest import GOLDEN, load_X
from oracle import xrl_oracle

pytestmark = pytest.mark.gpu
CASES = R.cpu_cases()
_WANT = {}


def want(name, ez, si):
    """the restatement's whole-buffer answer, computed once per (case, setting)"""
    key = (name, ez, si)
    if key not in _WANT:
        _WANT[key] = R.rule(*CASES[name], ez, si)
    return _WANT[key]


@pytest.fixture(scope="module")
def ref():
    return R.ref_lib() if xrl_oracle.ref_available() else None


@pytest.fixture(scope="module")
def clib():
    from pecos_amd import clib
    return clib


def to_dev(M, device="cuda:0"):
    """Csr -> (crow int64, col int32, val float32, shape) CUDA tensors holding the same bits"""
    import torch
    return (torch.from_numpy(M.indptr.view(np.int64).copy()).to(device), torch.from_numpy(M.indices.view(np.int32).copy()).to(device),
            torch.from_numpy(M.data.copy()).to(device), M.shape)


def to_host(t):
    crow, col, val = t[:3]
    return crow.cpu().numpy().view(np.uint64), col.cpu().numpy().view(np.uint32), val.cpu().numpy()


def device_product(A, B, ez, si, stream=None):
    from pecos_amd.features import sparse_matmul_device
    return to_host(sparse_matmul_device(to_dev(A), to_dev(B), eliminate_zeros=ez, sorted_indices=si, stream=stream))


# --------------------------------------------------------------------------------------------------------- the rule, case by case
@pytest.mark.parametrize("ez,si", R.SETTINGS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_product_equals_the_rule(ref, name, ez, si):
    # row product counts 0 .. CAP + 1 and 20 000 (counted_rows), all products in one column / all distinct at 65, CAP, CAP + 1, runs around
    # every 64-product step, shuffled left rows, duplicates on both sides, the numeric edges, the shapes -- under all four settings
    A, B = CASES[name]
    got = device_product(A, B, ez, si)
    assert R.same(got, R.logical(want(name, ez, si))), (name, ez, si)
    if ref is not None and R.reference_can_run(A, B):
        live, _ = R.native_matmul(ref, A, B, "csr", ez, si, threads=8)
        assert R.same(got, R.logical(live)), (name, ez, si, "live reference")


def test_forms_by_row_product_count(clib):
    cap = clib.debug_spgemm_forms()["cap"]
    assert cap == 1024
    counts = R.product_counts(cap)
    A, B, counts = R.counted_rows(counts)
    n_big = sum(f > cap for f in counts)
    assert n_big == 2 and cap in counts and cap + 1 in counts and cap - 1 in counts
    before = clib.debug_spgemm_forms()
    got = device_product(A, B, False, True)
    after = clib.debug_spgemm_forms()
    assert R.same(got, R.logical(want("counted_rows", False, True)))
    # a mixed batch: the rows up to CAP (the empty one included) by the LDS form, CAP + 1 and 20 000 by the big form in one batch
    assert (after["lds_rows"] - before["lds_rows"], after["big_rows"] - before["big_rows"]) == (len(counts) - n_big, n_big)
    assert after["batches"] - before["batches"] == 1 and after["calls"] - before["calls"] == 1
    # each row alone: the form follows from its own count
    for i, f in enumerate(counts):
        Ai = R.csr([0, A.indptr[i + 1] - A.indptr[i]], A.indices[int(A.indptr[i]):int(A.indptr[i + 1])], A.data[int(A.indptr[i]):int(A.indptr[i + 1])], (1, A.shape[1]))
        before = clib.debug_spgemm_forms()
        one = device_product(Ai, B, False, False)
        after = clib.debug_spgemm_forms()
        assert R.same(one, R.logical(R.rule(Ai, B, False, False))), f
        assert after["big_rows"] - before["big_rows"] == (1 if f > cap else 0), f


def test_big_form_in_several_batches(clib, monkeypatch):
    # a scratch budget of 5 000 products: the rows of CAP + 1 and of 20 000 products go in two batches (a row above the budget is its own)
    monkeypatch.setenv("XRL_SPGEMM_SCRATCH_PRODUCTS", "5000")
    A, B = CASES["counted_rows"]
    for ez, si in R.SETTINGS:
        before = clib.debug_spgemm_forms()
        got = device_product(A, B, ez, si)
        after = clib.debug_spgemm_forms()
        assert R.same(got, R.logical(want("counted_rows", ez, si))), (ez, si)
        assert after["batches"] - before["batches"] == 2


def test_left_row_order_is_the_summation_order():
    # (the CPU half shows that the reference's own values change with the order): both orders, each its own answer
    A, B = R.shuffled_pair()
    As = R.sort_left_rows(A)
    a, b = device_product(A, B, False, True), device_product(As, B, False, True)
    assert R.same(a, R.logical(R.rule(A, B))) and R.same(b, R.logical(R.rule(As, B)))
    assert (R.bits(a[2]) != R.bits(b[2])).any()


# ------------------------------------------------------------------------------------------------------------- host entry points
@pytest.mark.parametrize("name", ["numeric_edges", "shuffled", "counted_rows", "duplicates", "shape_no_rows", "shape_empty_right", "shape_widest_columns"])
def test_host_entry_points_fill_the_whole_allocator_buffer(ref, clib, name):
    raw = C.CDLL(clib.so_path)
    A, B = CASES[name]
    for ez, si in R.SETTINGS:
        w = want(name, ez, si)
        for fmt, X, Y, call in (("csr", A, B, (False, A.shape[0], B.shape[1], len(w[1]))),
                                ("csc", R.transpose_view(B), R.transpose_view(A), (True, B.shape[1], A.shape[0], len(w[1])))):
            got, calls = R.native_matmul(raw, X, Y, fmt, ez, si, threads=3)
            assert clib.clib_float32.xrl_last_error() is None
            assert calls == [call], (name, fmt, calls)                    # once, with the count before elimination
            assert R.same(got, w), (name, fmt, ez, si)                     # the stale tail past indptr[-1] included
            if ref is not None and R.reference_can_run(A, B):
                live, live_calls = R.native_matmul(ref, X, Y, fmt, ez, si, threads=3)
                assert R.same(got, live) and calls == live_calls, (name, fmt, ez, si, "live reference")


def test_host_entry_point_refuses_an_entry_outside_the_right_operand(clib):
    raw = C.CDLL(clib.so_path)
    A = R.from_rows([[(0, 1.0)], [(5, 1.0)]], 3)                          # column 5 of a 3-column left operand
    B = R.from_rows([[(0, 1.0)], [], []], 2)
    got, calls = R.native_matmul(raw, A, B)
    assert calls == [] and got[0] is None
    err = clib.clib_float32.xrl_last_error().decode()
    clib.clib_float32.xrl_clear_error()
    assert "names a row the right operand does not have" in err


def test_python_wrapper_on_the_four_operand_type_combinations(clib):
    z = np.load(os.path.join(R.GOLDEN_DIR, "wrapper.npz"))
    for tag in ("left_larger", "right_larger"):
        X, Y = (smat.csr_matrix((z[f"{tag}__{n}_data"], z[f"{tag}__{n}_indices"], z[f"{tag}__{n}_indptr"]), shape=tuple(z[f"{tag}__{n}_shape"])) for n in "XY")
        for fx, fy in R.WRAPPER_COMBOS:
            for ez, si in R.SETTINGS:
                Z = clib.sparse_matmul(X.asformat(fx), Y.asformat(fy), eliminate_zeros=ez, sorted_indices=si, threads=2)
                key = f"{tag}__{fx}_{fy}__{int(ez)}{int(si)}"
                n = int(z[key + "__indptr"][-1])
                assert Z.format == str(z[key + "__format"]) and Z.shape == (X.shape[0], Y.shape[1]) and Z.nnz == n, key
                assert np.array_equal(Z.indptr, z[key + "__indptr"]) and np.array_equal(Z.indices[:n], z[key + "__indices"][:n]), key
                assert np.array_equal(R.bits(Z.data[:n]), R.bits(z[key + "__data"][:n])), key


# ------------------------------------------------------------------------------------------------------- results as left operands
@pytest.mark.parametrize("stride", [1, 10, 64, 65, 1024])
def test_fixed_stride_result_to_csr(stride):
    import torch
    from pecos_amd.features import result_to_csr_device
    rng = np.random.default_rng(stride)
    rows = 9
    idx = rng.integers(0, 5000, (rows, stride)).astype(np.int32)          # best-first order is whatever the row holds: not sorted, kept
    val = rng.standard_normal((rows, stride)).astype(np.float32)
    cnt = np.minimum(rng.integers(0, stride + 1, rows), stride).astype(np.int32)
    cnt[0], cnt[1], cnt[2] = 0, stride + 7, stride                       # empty, above the stride (read as the stride), full
    t = [torch.from_numpy(a).cuda() for a in (idx, val, cnt)]
    for counts in (cnt, None):
        n = np.full(rows, stride) if counts is None else np.minimum(counts, stride)
        crow, col, v = to_host(result_to_csr_device((t[0], t[1], None if counts is None else t[2]), n_cols=5000))
        assert np.array_equal(crow, np.concatenate([[0], np.cumsum(n)]).astype(np.uint64))
        assert np.array_equal(col, np.concatenate([idx[r, :n[r]] for r in range(rows)]).view(np.uint32))
        assert np.array_equal(R.bits(v), R.bits(np.concatenate([val[r, :n[r]] for r in range(rows)])))


def test_result_triple_as_left_operand(ref):
    # a fixed-stride result with a label twice in a row (two beams under one cluster) times a wider right operand
    import torch
    from pecos_amd.features import sparse_matmul_device
    rng = np.random.default_rng(2)
    rows, stride, inner = 70, 10, 40
    idx = rng.integers(0, inner, (rows, stride)).astype(np.int32)
    val = rng.standard_normal((rows, stride)).astype(np.float32)
    cnt = rng.integers(0, stride + 1, rows).astype(np.int32)
    B = R.rand_csr(rng, inner, 300, 40, sort=True)
    A = R.from_rows([list(zip(idx[r, :cnt[r]].tolist(), val[r, :cnt[r]].tolist())) for r in range(rows)], inner)
    res = tuple(torch.from_numpy(a).cuda() for a in (idx, val, cnt))
    for ez, si in R.SETTINGS:
        got = to_host(sparse_matmul_device(res, to_dev(B), eliminate_zeros=ez, sorted_indices=si))
        assert R.same(got, R.logical(R.rule(A, B, ez, si))), (ez, si)


# ------------------------------------------------------------------------------------------------ caller-owned buffers, side stream
def test_caller_owned_buffers_at_odd_offsets_on_a_side_stream(clib):
    import torch
    from pecos_amd.features import DeviceMatrix
    A, B = R.shuffled_pair()
    side = torch.cuda.Stream()
    ops = []
    for M, offs in ((A, (1, 3, 2)), (B, (1, 1, 3))):
        # poison that can never give an out-of-range address: row pointers 0, column ids 0 (a valid row / column), values NaN
        bands = [dv.banded(M.indptr.view(np.int64), offs[0], dv.BAND, np.int64(0), "cuda"), dv.banded(M.indices.view(np.int32), offs[1], dv.BAND, np.int32(0), "cuda"),
                 dv.banded(M.data, offs[2], dv.BAND, np.float32(np.nan), "cuda")]
        assert bands[0][1].data_ptr() % 16 == 8 and bands[1][1].data_ptr() % 16 in (4, 12) and bands[2][1].data_ptr() % 16 in (8, 12)
        ops.append((bands, DeviceMatrix.from_torch(bands[0][1], bands[1][1], bands[2][1], M.shape)))
    torch.cuda.synchronize()                                             # the operands are complete before the side stream reads them
    for ez, si in R.SETTINGS:
        with torch.cuda.stream(side):
            Z = ops[0][1].multiply(ops[1][1], ez, si, stream=side.cuda_stream)
            got = to_host(Z.to_torch(stream=side.cuda_stream))
        assert R.same(got, R.logical(R.rule(A, B, ez, si))), (ez, si)
    for bands, _ in ops:
        for (whole, payload), fill in zip(bands, (np.int64(0), np.int32(0), np.float32(np.nan))):
            dv.assert_bands_intact(whole, payload, fill, "operand")
    info = ops[0][1].info
    assert (info["rows"], info["cols"], info["nnz"], info["device"]) == (A.shape[0], A.shape[1], len(A.data), 0)
    assert info["row_ptr"] == ops[0][0][0][1].data_ptr() and info["val"] == ops[0][0][2][1].data_ptr()     # wrapped, not copied


def test_upload_download_and_chained_products(ref, clib):
    from pecos_amd.features import DeviceMatrix
    A, B = CASES["duplicates"]
    As = smat.csr_matrix((12, 20), dtype=np.float32)
    As.indptr, As.indices, As.data = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data       # assigned directly: order and duplicates stay
    a, b = DeviceMatrix.upload(As), DeviceMatrix.from_torch(*to_dev(B))
    Z = a.multiply(b)
    back = Z.download()
    w = R.rule(A, B)
    assert R.same((back.indptr, back.indices, back.data), R.logical(w)) and back.shape == (12, 16) == Z.shape
    # the product is an operand again: (A B) B^T-shaped second factor
    Cm = R.rand_csr(np.random.default_rng(4), 16, 9, 9)
    Z2 = Z.multiply(DeviceMatrix.from_torch(*to_dev(Cm)), eliminate_zeros=True)
    AB = R.csr(*R.logical(w), (12, 16))
    assert R.same(to_host(Z2.to_torch()), R.logical(R.rule(AB, Cm, True, True)))


# ------------------------------------------------------- the shared scan, row copy and handle bodies at their smallest shapes
def test_tiny_result_with_an_empty_and_an_overfull_row():
    import torch
    from pecos_amd.features import DeviceMatrix
    idx = np.arange(12, dtype=np.int32).reshape(3, 4)
    val = (np.arange(12, dtype=np.float32) + 0.5).reshape(3, 4)
    t = [torch.from_numpy(a).cuda() for a in (idx, val, np.array([0, 4, 9], dtype=np.int32))]
    for counts, ptr in ((t[2], [0, 0, 4, 8]), (None, [0, 4, 8, 12])):     # the 9 is read as 4
        back = DeviceMatrix.from_result((t[0], t[1], counts), n_cols=12).download()
        first = 12 - ptr[-1]
        assert back.shape == (3, 12) and np.array_equal(back.indptr, ptr)
        assert np.array_equal(back.indices, idx.ravel()[first:]) and np.array_equal(R.bits(back.data), R.bits(val.ravel()[first:]))


def test_upload_download_of_matrices_without_rows_columns_or_entries():
    from pecos_amd.features import DeviceMatrix
    zeros = smat.csr_matrix((2, 3), dtype=np.float32)                     # an explicit zero, an empty row
    zeros.indptr, zeros.indices, zeros.data = np.array([0, 2, 2]), np.array([2, 0]), np.array([0.0, -0.0], dtype=np.float32)
    mats = [smat.csr_matrix((0, 5), dtype=np.float32), smat.csr_matrix((5, 0), dtype=np.float32), smat.csr_matrix((3, 3), dtype=np.float32), zeros]
    held = [DeviceMatrix.upload(M) for M in mats]                         # no rows next to no entries: all alive at once
    for M, h in zip(mats, held):
        back = h.download()
        assert back.shape == M.shape == h.shape and h.info["nnz"] == len(M.data)
        assert np.array_equal(back.indptr, M.indptr) and np.array_equal(back.indices, M.indices) and np.array_equal(R.bits(back.data), R.bits(M.data))


def test_left_rows_of_1_64_and_65_entries():
    rng = np.random.default_rng(65)
    B = R.rand_csr(rng, 65, 30, 6, sort=True)
    A = R.from_rows([list(zip(rng.permutation(65)[:n].tolist(), rng.standard_normal(n).astype(np.float32).tolist())) for n in (1, 64, 65)], 65)
    for si in (True, False):
        assert R.same(device_product(A, B, False, si), R.logical(R.rule(A, B, False, si))), si


# --------------------------------------------------------------------------------------------------- end to end on a golden model
@pytest.fixture(scope="module")
def eurlex():
    import torch
    from pecos_amd import XLinearModel
    from pecos_amd.features import predict_from_torch
    m = XLinearModel.load(os.path.join(GOLDEN, "synth", "s_eurlex"))
    X = load_X(os.path.join(GOLDEN, "synth", "s_eurlex__X.npz"))
    Cl = smat.load_npz(os.path.join(GOLDEN, "synth", "s_eurlex", "ranker", "2.model", "C.npz")).tocsr().astype(np.float32)     # labels x clusters
    Cl.sort_indices()
    dev = torch.device("cuda", 0)
    xt = (torch.from_numpy(X.indptr.astype(np.int64)).to(dev), torch.from_numpy(X.indices.astype(np.int32)).to(dev), torch.from_numpy(X.data.astype(np.float32)).to(dev))
    res = predict_from_torch(m, *xt, X.shape[1], beam_size=10, only_topk=10)
    return m, X, xt, Cl, res


def _result_rows(res, n_cols):
    idx, val, cnt = (t.cpu().numpy() for t in res)
    return R.from_rows([list(zip(idx[r, :cnt[r]].astype(np.uint32).tolist(), val[r, :cnt[r]].tolist())) for r in range(idx.shape[0])], n_cols)


def test_label_result_rolled_up_to_clusters(ref, eurlex):
    # Y_pred * C: the scores of a query's labels summed per cluster, in the result's best-first order
    from pecos_amd.features import sparse_matmul_device
    m, X, xt, Cl, res = eurlex
    Cr = R.from_scipy(Cl)
    Y = _result_rows(res, Cl.shape[0])
    assert len(Y.data) > 0
    for ez, si in R.SETTINGS:
        got = to_host(sparse_matmul_device(res, Cl, eliminate_zeros=ez, sorted_indices=si))
        assert R.same(got, R.logical(R.rule(Y, Cr, ez, si))), (ez, si)
        if ref is not None:
            assert R.same(got, R.logical(R.native_matmul(ref, Y, Cr, "csr", ez, si, threads=4)[0])), (ez, si, "live reference")


def test_cluster_result_descends_through_c_transposed(ref, eurlex):
    # XR-Transformer's csr_codes_next = sparse_matmul(csr_codes, C.T) (matcher.py:723): the matcher's fixed-stride result over the clusters
    # -- here every label's parent with the label's score, so a row names a cluster more than once -- times C^T
    import torch
    from pecos_amd.features import sparse_matmul_device
    m, X, xt, Cl, res = eurlex
    parent = torch.from_numpy(Cl.indices.astype(np.int32)).cuda()         # one stored entry per row of C: the label's cluster
    assert np.array_equal(np.diff(Cl.indptr), np.ones(Cl.shape[0]))
    codes = (parent[res[0].long()], res[1], res[2])
    Ct = Cl.T.tocsr()
    Ct.sort_indices()
    codes_host, Ct_raw = _result_rows(codes, Cl.shape[1]), R.from_scipy(Ct)
    got = to_host(sparse_matmul_device(codes, Ct))
    assert R.same(got, R.logical(R.rule(codes_host, Ct_raw)))
    if ref is not None:
        assert R.same(got, R.logical(R.native_matmul(ref, codes_host, Ct_raw, "csr", False, True, threads=4)[0]))


def test_a_product_wrapped_as_queries_predicts_like_its_download(eurlex):
    # Z = S X on the device (sorted indices, as queries must be) -> xrl_queries_from_device_csr -> beam search, against predict on Z's host copy
    from pecos_amd.features import DeviceMatrix, predict_from_torch
    m, X, xt, Cl, res = eurlex
    rng = np.random.default_rng(6)
    S = smat.random(24, X.shape[0], density=0.05, format="csr", dtype=np.float32, random_state=np.random.RandomState(3))
    S.data = (rng.uniform(0.2, 1.0, S.nnz)).astype(np.float32)
    Z = DeviceMatrix.upload(S).multiply(DeviceMatrix.from_torch(*xt, X.shape), eliminate_zeros=True, sorted_indices=True)
    crow, col, val, shape = Z.to_torch()
    assert shape == (24, X.shape[1]) and val.numel() > 0
    idx, sc, cnt = (t.cpu().numpy() for t in predict_from_torch(m, crow, col, val, shape[1], beam_size=10, only_topk=10))
    Zh = Z.download()
    Zh.sort_indices()
    P = m.predict(Zh, beam_size=10, only_topk=10)
    for r in range(24):
        lo, hi = P.indptr[r], P.indptr[r + 1]
        assert cnt[r] == hi - lo and np.array_equal(idx[r, :cnt[r]], P.indices[lo:hi]) and np.array_equal(R.bits(sc[r, :cnt[r]]), R.bits(P.data[lo:hi])), r
