"""K12D without a GPU: the statement of R3D against scipy and sklearn live, bit for bit; the fused chain differs; refusals before a GPU."""
import numpy as np
import pytest
import scipy.sparse as smat

import dense_embedding_rule as der
import label_embedding_rule as ler

@pytest.fixture(scope="module")
def case():
    YT = ler.transpose(ler.normalize(der.case_Y()))
    X = der.case_X(67)
    return YT, X, der.product(YT, X)


def test_product_statement_equals_scipy(case):
    YT, X, P = case
    S = ler.to_scipy(YT)
    wide = np.full((X.shape[0], X.shape[1] + 3), np.nan, dtype=np.float32)
    wide[:, :X.shape[1]] = X
    for live in (S.dot(X), S.dot(wide[:, :X.shape[1]])):                    # a strided X gives the same bits
        assert live.dtype == np.float32 and np.array_equal(live.view(np.uint32), P.view(np.uint32))


def test_normalize_statement_equals_sklearn_on_the_csr(case):
    sk = pytest.importorskip("sklearn.preprocessing")
    P = case[2]
    N = sk.normalize(smat.csr_matrix(P), axis=1, norm="l2").toarray()
    assert np.array_equal(der.normalize(P).view(np.uint32), N.view(np.uint32))


def test_fused_chain_differs(case):
    YT, X, P = case
    F = der.product(YT, X, fused=True)
    assert 0 < int((F.view(np.uint32) != P.view(np.uint32)).sum())
    swapped = ler.from_rows([[(0, np.float32(1.0)), (2, np.float32(1.0)), (1, np.float32(1.0))]], der.SAMPLES)
    assert P[der.ORDER_LABEL, 0] == 0.0 and der.product(swapped, X)[0, 0] == 1.0           # (1e8 + 1) - 1e8 against (1e8 - 1e8) + 1: the order reaches the bits


def refused(call, start, needle):
    with pytest.raises(RuntimeError) as e:
        call()
    assert str(e.value).startswith(start + ": ") and needle in str(e.value), str(e.value)


M, E, FAKE, BIG = "xrl_smat_matmul_dense_device", "xrl_label_embedding_dense_device", 4096, 1 << 20
# the arguments after the handle (A: 4 x 10; Y: 10 samples x 4 labels), and what the message holds
REFUSALS = {
    "m_null_out": (M, (FAKE, 10, 8, 8, None, 8, 0), "null argument (out)"),
    "m_out_stride": (M, (FAKE, 10, 8, 8, BIG, 9, 2), "row stride of out"),
    "m_inner": (M, (FAKE, 9, 8, 8, BIG, 8, 0), "A.cols != X.rows"),
    "m_overlap": (M, (FAKE, 10, 8, 8, FAKE + 4 * 79, 8, 0), "out overlaps X"),
    "e_method_pii": (E, (FAKE, 8, 8, None, 0, 0, 2, True, BIG, 8), "unknown method"),
    "e_null_Z": (E, (FAKE, 8, 8, None, 3, 3, 1, True, BIG, 11), "null argument (Z)"),
    "e_out_stride": (E, (FAKE, 8, 8, 1 << 16, 3, 3, 1, True, BIG, 10), "row stride of out"),
    "e_overlap_X": (E, (FAKE, 8, 8, None, 0, 0, 0, True, FAKE + 4 * 79, 8), "out overlaps X"),
    "e_overlap_Z": (E, (FAKE, 8, 8, BIG, 3, 3, 1, True, BIG + 4, 11), "out overlaps Z"),
    "e_wide": (E, (FAKE, 2 ** 32 - 2, 2 ** 32 - 2, 1 << 16, 3, 3, 1, True, BIG, 2 ** 32 + 1), "2^32 or more"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_entry_points_refuse_before_a_gpu(name):
    from pecos_amd import clib as lib
    fn, args, needle = REFUSALS[name]
    call = lib.smat_matmul_dense_device if fn == M else lib.label_embedding_dense_device
    h, huge = lib.smat_from_device_csr(0, *((4, 10) if fn == M else (10, 4)), 256, 256, 256, 5), lib.smat_from_device_csr(0, 3, 3, 256, 256, 256, 2 ** 32 - 1)
    try:
        refused(lambda: call(h, *args), fn, needle)
        good = REFUSALS["m_inner" if fn == M else "e_overlap_X"][1]
        refused(lambda: call(0, *good), fn, "null matrix handle")
        if fn == E:
            refused(lambda: call(huge, *good), fn, "2^32 - 1")
    finally:
        lib.smat_free(h)
        lib.smat_free(huge)


def test_python_names_and_their_refusals():
    import pecos_amd
    from pecos_amd.embedding import LabelEmbeddingFactory, label_embedding_dense_device
    assert {"embedding", "label_embedding_dense_device", "sparse_dense_matmul_device"} <= set(pecos_amd.__all__)
    assert issubclass(LabelEmbeddingFactory, pecos_amd.LabelEmbeddingFactory) and pecos_amd.embedding.LabelEmbeddingFactory is LabelEmbeddingFactory
    Y, X, Z = ler.golden_inputs()
    dense = np.ascontiguousarray(X.toarray())
    with pytest.raises(NotImplementedError, match="mix"):
        LabelEmbeddingFactory.pifa_lf_concat(Y, dense, Z)
    with pytest.raises(ValueError, match="2-D float32 CUDA tensor"):
        label_embedding_dense_device(Y, dense)
    with pytest.raises(NotImplementedError, match="dense X"):                # the old names keep their refusals
        pecos_amd.LabelEmbeddingFactory.create(Y, dense, method="pifa")
