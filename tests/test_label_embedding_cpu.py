"""Label embeddings (K12) without a GPU: the numpy statements of R1 - R5 (tests/label_embedding_rule.py) against sklearn and scipy live
and against the recorded reference, bit for bit; the wrong variants on the cases built to catch them; the refusals that come before a
GPU is required; the Python wrappers' argument handling."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as smat

import label_embedding_rule as ler
from conftest import GOLDEN

RECORDED = np.load(os.path.join(GOLDEN, "label_embedding_ref.npz"))

NORMALIZE_CASES = {
    "order": ler.order_rows, "order_reversed": lambda: ler.order_rows(True), "special": ler.special_rows,
    **{f"scale_{s:g}": (lambda s=s: ler.random_rows(scale=s)) for s in (1.0, 1e-3, 1e10, 1e-21, 1e-25, 1e25)},
}
TRANSPOSE_CASES = {
    "counted": ler.counted_columns, "sorted": lambda: ler.counted_columns(unsorted=False), "golden_Y": lambda: ler.from_scipy(ler.golden_inputs()[0]),
    "no_rows": lambda: ler.from_rows([], 5), "one_row": lambda: ler.from_rows([[(4, 1.0), (0, 2.0), (4, 3.0)]], 5), "no_entries": lambda: ler.from_rows([[], [], []], 4),
}


def entry_bits(M, row, k):
    return int(ler.bits(M.data)[int(M.indptr[row]) + k])


# ------------------------------------------------------------------------------------------------ the statements against sklearn / scipy
@pytest.mark.parametrize("name", sorted(NORMALIZE_CASES))
def test_normalize_statement_equals_sklearn(name):
    """normalize() itself where it takes the case, and the routine under it (normalize refuses NaN and inf before it gets there)."""
    sk = pytest.importorskip("sklearn.preprocessing")
    fast = pytest.importorskip("sklearn.utils.sparsefuncs_fast")
    M = NORMALIZE_CASES[name]()
    S = ler.to_scipy(M)
    S.indptr, S.indices = S.indptr.astype(np.int32), S.indices.astype(np.int32)
    if np.all(np.isfinite(M.data)):
        N = sk.normalize(S, axis=1, norm="l2", copy=True)
        assert ler.same(ler.triple(ler.normalize(M)), (N.indptr, N.indices, N.data)), name
    fast.inplace_csr_row_normalize_l2(S)
    assert ler.same(ler.triple(ler.normalize(M)), (S.indptr, S.indices, S.data)), name


@pytest.mark.parametrize("name", sorted(TRANSPOSE_CASES))
def test_transpose_statement_equals_scipy(name):
    M = TRANSPOSE_CASES[name]()
    T = ler.to_scipy(M).T.tocsr()
    got = ler.transpose(M)
    assert got.shape == T.shape and ler.same(ler.triple(got), (T.indptr, T.indices, T.data)), name
    back = ler.transpose(got)                                            # transposing twice: the canonical order, duplicates kept
    C = ler.to_scipy(M).T.tocsr().T.tocsr()
    assert ler.same(ler.triple(back), (C.indptr, C.indices, C.data))


def test_hstack_statement_equals_scipy():
    Y, X, Z = ler.sparse_edges()
    E = ler.embedding(Y, X)
    H = ler.hstack([E, Z])
    S = smat.hstack([ler.to_scipy(E), ler.to_scipy(Z)], format="csr")
    assert H.shape == S.shape == (4, 7) and np.array_equal(ler.to_scipy(H).toarray().view(np.uint32), S.toarray().view(np.uint32))
    b, e = int(H.indptr[2]), int(H.indptr[3])
    assert H.indices[b:e].tolist() == [6, 5] and e - b == 2                 # label 2: no embedding entries, then Z's row as stored, ids shifted by 5


# ------------------------------------------------------------------------------------------------ the statements against the reference
@pytest.mark.parametrize("normalized_Y", [True, False])
@pytest.mark.parametrize("method", ler.METHODS)
def test_statement_equals_the_recorded_reference(method, normalized_Y):
    Y, X, Z = (ler.from_scipy(M) for M in ler.golden_inputs())
    k = ler.golden_key(method, normalized_Y)
    E = ler.embedding(Y, X, Z, method, normalized_Y)
    assert E.shape == tuple(RECORDED[k + "__shape"])
    assert ler.same(ler.triple(E), (RECORDED[k + "__indptr"], RECORDED[k + "__indices"], RECORDED[k + "__data"]))


def test_recorded_fixture_is_small():
    assert os.path.getsize(os.path.join(GOLDEN, "label_embedding_ref.npz")) < 512 * 1024


# ------------------------------------------------------------------------------------------------ the cases discriminate
def test_mandatory_order_rows():
    """sklearn's bits on the rows of the issue, and the value 1 ulp lower when the row is stored in reverse or walked in reverse."""
    fwd, rev = ler.normalize(ler.order_rows()), ler.normalize(ler.order_rows(True))
    walked_back = ler.normalize(ler.order_rows(), "reversed")
    for r, want in enumerate(ler.ORDER_SKLEARN_BITS):
        assert entry_bits(fwd, r, 1) == want
        assert entry_bits(rev, r, 4096) == want - 1 and entry_bits(walked_back, r, 1) == want - 1
    assert entry_bits(fwd, 3, 1) - entry_bits(rev, 3, 4096) == 1 and entry_bits(fwd, 3, 1) - entry_bits(walked_back, 3, 1) == 1


def test_double_square_variant_differs_on_random_rows():
    M = ler.random_rows()
    a, b = ler.bits(ler.normalize(M).data), ler.bits(ler.normalize(M, "double_square").data)
    assert 0 < int((a != b).sum()) < len(a)


def test_row_reversed_transpose_differs_and_reaches_the_product_bits():
    M = ler.counted_columns()
    assert not ler.same(ler.triple(ler.transpose(M)), ler.triple(ler.transpose(M, "row_reversed")))
    Y, X = ler.transpose_order_case()
    good, bad = ler.embedding(Y, X, normalized_Y=False), ler.embedding(Y, X, normalized_Y=False, variant="row_reversed")
    assert np.array_equal(good.indptr, bad.indptr) and np.array_equal(good.indices, bad.indices)
    assert not np.array_equal(ler.bits(good.data), ler.bits(bad.data))


def test_order_case_is_what_it_claims():
    """feature 0 of label 0: (1e8 + 1) - 1e8 = 0 in fp32, (1e8 - 1e8) + 1 = 1 -- an explicit +0 or a positive entry."""
    for flip, zero in ((False, True), (True, False)):
        Y, X = ler.order_case(flip)
        P = ler.product(ler.transpose(Y), X)
        assert int(P.indices[0]) == 0 and (ler.bits(P.data)[0] == 0) == zero


def test_special_rows_are_what_they_claim():
    N, M = ler.normalize(ler.special_rows()), ler.special_rows()
    row = lambda A, r: ler.bits(A.data)[int(A.indptr[r]):int(A.indptr[r + 1])]  # noqa: E731
    assert np.array_equal(row(N, 0), row(M, 0)) and np.array_equal(row(N, 4), row(M, 4))       # untouched
    assert row(N, 1).tolist() == [0x80000000] + ler.bits(np.float32([0.6, 0.0, -0.8])).tolist()
    assert row(N, 2).tolist() == [0xFFC00000, 0, 0xFFC00000, 0x80000000]
    assert row(N, 3).tolist() == [0x7FC12345, 0x7FC12345, 0x7FC12345, 0xFFC00001]
    assert np.all(row(N, 5) == 0)


# ------------------------------------------------------------------------------------------------ refusals before a GPU is required
@pytest.fixture(scope="module")
def lib():
    from pecos_amd import clib
    return clib


def wrapped(lib, rows, cols, nnz, device=0):
    """a handle around device addresses: no GPU call is made for it"""
    return lib.smat_from_device_csr(device, rows, cols, 256, 256, 256, nnz)


def refused(call, start, needle):
    with pytest.raises(RuntimeError) as e:
        call()
    assert str(e.value).startswith(start + ": ") and needle in str(e.value), str(e.value)


def test_refusals_need_no_gpu(lib):
    hs = [wrapped(lib, 10, 4, 12), wrapped(lib, 10, 6, 5), wrapped(lib, 9, 6, 5), wrapped(lib, 4, 3, 2), wrapped(lib, 5, 3, 2), wrapped(lib, 10, 4, 12, device=1),
          wrapped(lib, 10, 2 ** 32 - 3, 1), wrapped(lib, 4, 2 ** 32 - 6, 1), wrapped(lib, 3, 3, 2 ** 32 - 1)]
    y, x, x9, z, z5, y1, wide, zwide, huge = hs
    try:
        refused(lambda: lib.smat_transpose_device(0), "xrl_smat_transpose_device", "null matrix handle")
        refused(lambda: lib.smat_transpose_device(huge), "xrl_smat_transpose_device", "2^32 - 1")
        refused(lambda: lib.smat_normalize_rows_device(0), "xrl_smat_normalize_rows_device", "null matrix handle")
        fn = lib.clib_float32.xrl_smat_normalize_rows_device
        assert fn(ctypes.c_void_p(y), 0, None, None) == -1
        refused(lib._check, "xrl_smat_normalize_rows_device", "null argument")
        refused(lambda: lib.smat_hstack_device([]), "xrl_smat_hstack_device", "no matrices")
        refused(lambda: lib.smat_hstack_device([y, 0]), "xrl_smat_hstack_device", "null matrix handle")
        refused(lambda: lib.smat_hstack_device([y, x9]), "xrl_smat_hstack_device", "rows")
        refused(lambda: lib.smat_hstack_device([y, y1]), "xrl_smat_hstack_device", "devices 0 and 1")
        refused(lambda: lib.smat_hstack_device([y, wide]), "xrl_smat_hstack_device", "2^32")
        name = "xrl_label_embedding_device"
        refused(lambda: lib.label_embedding_device(0, x), name, "null matrix handle (Y)")
        refused(lambda: lib.label_embedding_device(y, 0), name, "null matrix handle (X)")
        refused(lambda: lib.label_embedding_device(y, x, None, "pifa_lf_concat"), name, "null matrix handle (Z)")
        refused(lambda: lib.label_embedding_device(y, x, method=3), name, "unknown method")
        refused(lambda: lib.label_embedding_device(y, x, method=-1), name, "unknown method")
        refused(lambda: lib.label_embedding_device(y, x9), name, "Y.rows != X.rows")
        refused(lambda: lib.label_embedding_device(y, x, z5, "pifa_lf_concat"), name, "Z.rows != Y.cols")
        refused(lambda: lib.label_embedding_device(y1, x), name, "devices")
        refused(lambda: lib.label_embedding_device(y, x, zwide, "pifa_lf_concat"), name, "2^32")
        refused(lambda: lib.label_embedding_device(huge, None, None, "pii"), name, "2^32 - 1")
        with pytest.raises(NotImplementedError):
            lib.label_embedding_device(y, x, method="pifa_lf_convex_combine")
        assert z and lib.debug_embed_forms()["cap"] == ler.CAP
    finally:
        for h in hs:
            lib.smat_free(h)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_exports_and_signatures():
    import inspect
    import pecos_amd
    from pecos_amd import DeviceMatrix, LabelEmbeddingFactory, label_embedding_device
    assert {"LabelEmbeddingFactory", "label_embedding_device"} <= set(pecos_amd.__all__)
    assert list(inspect.signature(label_embedding_device).parameters) == ["Y", "X", "method", "Z", "normalized_Y", "stream"]
    assert list(inspect.signature(LabelEmbeddingFactory.pifa).parameters) == ["Y", "X", "threads", "normalized_Y"]
    assert list(inspect.signature(LabelEmbeddingFactory.pifa_lf_concat).parameters) == ["Y", "X", "Z", "threads", "normalized_Y"]
    assert list(inspect.signature(LabelEmbeddingFactory.pii).parameters) == ["Y"]
    assert all(hasattr(DeviceMatrix, n) for n in ("transpose", "normalize_rows", "hstack"))


def test_wrappers_refuse_what_is_not_served():
    from pecos_amd import LabelEmbeddingFactory, label_embedding_device
    Y, X, Z = ler.golden_inputs()
    dense = np.ascontiguousarray(X.toarray())
    with pytest.raises(NotImplementedError, match="dense X"):
        LabelEmbeddingFactory.create(Y, dense, method="pifa")
    with pytest.raises(NotImplementedError, match="dense Z"):
        LabelEmbeddingFactory.pifa_lf_concat(Y, X, np.ascontiguousarray(Z.toarray()))
    with pytest.raises(NotImplementedError, match="pifa_lf_convex_combine"):
        LabelEmbeddingFactory.create(Y, X, method="pifa_lf_convex_combine", Z=X, alpha=0.5)
    with pytest.raises(NotImplementedError, match="not implemented"):
        LabelEmbeddingFactory.create(Y, X, method="nope")
    with pytest.raises(NotImplementedError, match="spmatrix"):
        LabelEmbeddingFactory.pifa(dense, X)
    with pytest.raises(NotImplementedError, match="row-major"):
        LabelEmbeddingFactory.pifa(Y, X.tocsc())
    with pytest.raises(ValueError, match="Y must be float32"):
        LabelEmbeddingFactory.pifa(Y.astype(np.float64), X)
    with pytest.raises(ValueError, match="X must be float32"):
        LabelEmbeddingFactory.create(Y, X.astype(np.float64), method="PIFA", threads=4)
    with pytest.raises(ValueError, match="needs Y and X"):
        label_embedding_device(Y)
    with pytest.raises(ValueError, match="needs Y, X and Z"):
        label_embedding_device(Y, X, method="pifa_lf_concat")
    with pytest.raises(NotImplementedError, match="pifa_lf_convex_combine"):
        label_embedding_device(Y, X, method="pifa_lf_convex_combine", Z=Z)
