"""K12D on the device against the numpy statement of R3D (tests/dense_embedding_rule.py), bits equal; windows; the chain into K11D; sklearn's dense path."""
import functools
import os
import sys

import numpy as np
import pytest

import clustering_rule as cr
import dense_embedding_rule as der
import label_embedding_rule as ler
from conftest import REPO

pytestmark = pytest.mark.gpu

LENGTHS = [len(r) for r in der.label_rows()]
Y_CSR = der.case_Y()
Y_SCIPY = ler.to_scipy(Y_CSR)


@functools.lru_cache(maxsize=None)
def statement(cols, normalized_Y=True):
    return der.embedding(Y_CSR, der.case_X(cols), normalized_Y=normalized_Y)


def same_bits(got, want):
    return np.array_equal(got.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def forms_of(call):
    """(the call's result, rows it served by the narrow, slab and long form)"""
    from pecos_amd import clib
    f0, out, f1 = clib.debug_embed_dense_forms(), call(), clib.debug_embed_dense_forms()
    return out, tuple(f1[k] - f0[k] for k in ("narrow", "slab", "long")) + (f1["long_min"] - der.LONG,)


def expected_forms(cols):
    n_long = sum(n >= der.LONG for n in LENGTHS)
    return (len(LENGTHS) - n_long, 0, n_long, 0) if cols <= 128 else (0, len(LENGTHS) - n_long, n_long, 0)


@pytest.mark.parametrize("cols", der.COLS)
def test_product_against_the_statement(cols):                  # rows stored last sample first: the chain follows the stored order
    import pecos_amd
    import torch
    A = ler.from_rows([r[::-1] for r in der.label_rows()], der.SAMPLES)
    X = der.case_X(cols)
    got, forms = forms_of(lambda: pecos_amd.sparse_dense_matmul_device(ler.to_scipy(A), torch.from_numpy(X).cuda()))
    assert same_bits(got, der.product(A, X))
    assert forms == expected_forms(cols)


@pytest.mark.parametrize("normalized_Y", [True, False])
@pytest.mark.parametrize("cols", der.COLS)
def test_embedding_against_the_statement(cols, normalized_Y):
    import pecos_amd
    import torch
    want = statement(cols, normalized_Y)
    got, forms = forms_of(lambda: pecos_amd.label_embedding_dense_device(Y_SCIPY, torch.from_numpy(der.case_X(cols)).cuda(), normalized_Y=normalized_Y))
    assert same_bits(got, want)
    assert forms == expected_forms(cols)
    assert want[der.ORDER_LABEL, 0] == 0.0 and not want[der.EMPTY_LABEL].any()                      # the order case's element; the label without positives
    if cols == 5:                                                                                   # all-zero features: zero rows stay zero
        got = pecos_amd.label_embedding_dense_device(Y_SCIPY, torch.zeros((der.SAMPLES, cols), device="cuda"), normalized_Y=normalized_Y)
        assert same_bits(got, der.embedding(Y_CSR, der.case_X(cols, zero=True))) and not got.any()


@pytest.mark.parametrize("z_cols", [1, 65])
def test_concat_with_a_dense_Z(z_cols):
    import pecos_amd
    import torch
    cols = 65
    Z = np.random.default_rng(z_cols).standard_normal((len(LENGTHS), z_cols)).astype(np.float32)
    got = pecos_amd.label_embedding_dense_device(Y_SCIPY, torch.from_numpy(der.case_X(cols)).cuda(), "pifa_lf_concat", torch.from_numpy(Z).cuda())
    assert got.shape == (len(LENGTHS), cols + z_cols) and same_bits(got, np.hstack([statement(cols), Z]))


def test_windows_of_wider_tensors_on_a_side_stream():
    """X and out at odd element offsets, row strides of width + 3, NaN all around: the packed answer, operands and padding untouched"""
    import pecos_amd
    import torch
    cols, labels = 257, len(LENGTHS)

    def window(rows, width):
        flat = torch.full((1 + (rows + 2) * (width + 3),), float("nan"), dtype=torch.float32, device="cuda")
        return flat, flat[1:].view(rows + 2, width + 3)[1:rows + 1, :width]

    x_flat, x = window(der.SAMPLES, cols)
    o_flat, out = window(labels, cols)
    x.copy_(torch.from_numpy(der.case_X(cols)))
    x_before, o_before = x_flat.view(torch.int32).clone(), o_flat.view(torch.int32).clone()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = pecos_amd.label_embedding_dense_device(Y_SCIPY, x, out=out, stream=side.cuda_stream)
    torch.cuda.synchronize()
    assert got is out and same_bits(out, statement(cols))
    assert torch.equal(x_flat.view(torch.int32), x_before)
    inside = torch.zeros_like(o_flat, dtype=torch.bool)
    inside[1:].view(labels + 2, cols + 3)[1:labels + 1, :cols] = True
    assert torch.equal(o_flat.view(torch.int32)[~inside], o_before[~inside])


def test_chain_into_the_dense_clustering():
    import pecos_amd
    import torch
    Y, X = ler.golden_inputs()[0], np.ascontiguousarray(ler.golden_inputs()[1].toarray())
    depth, kw = 4, dict(algo=cr.SKMEANS, seed=0, max_iter=20)
    want = der.embedding(ler.from_scipy(Y), X)
    E = pecos_amd.label_embedding_dense_device(Y, torch.from_numpy(X).cuda())
    assert same_bits(E, want)
    host, err = cr.run_library(cr.OURS, want, depth, **kw)
    assert err is None, err
    codes = pecos_amd.run_clustering_device(E, depth, partition_algo=kw["algo"], seed=kw["seed"], kmeans_max_iter=kw["max_iter"])
    assert np.array_equal(codes.cpu().numpy().view(np.uint32), host)


def test_distance_to_sklearns_dense_path():
    """Both paths divide v by a norm of the same `cols` non-negative squares: any fp32 summation order errs by at most (cols - 1) * 2^-24
    relative, halved by the root; sklearn rounds its root and its divide and may not round the squares (2^-24, 2^-24, 2^-25), the device
    rounds once; relative 2^-24 is at most one ulp, one more for the two last places.  Measured: 2 ulp (profiles/label_embedding_dense.md)."""
    pytest.importorskip("sklearn.preprocessing")
    refpy = os.path.join(REPO, "oracle", "_ref", "refpy")
    if not os.path.isdir(os.path.join(refpy, "pecos")):
        pytest.skip("oracle/_ref/refpy (the reference's python package) is not built")
    if refpy not in sys.path:
        sys.path.insert(0, refpy)
    import pecos.xmc.base as xb
    from pecos_amd.embedding import LabelEmbeddingFactory
    Y, X = ler.golden_inputs()[0], np.ascontiguousarray(ler.golden_inputs()[1].toarray())
    ref = xb.LabelEmbeddingFactory.pifa(Y, X.copy())
    got = LabelEmbeddingFactory.create(Y, X, method="pifa")
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == ref.shape
    bound = (X.shape[1] - 1) / 2 + 1 + 1 + 0.5 + 1 + 1
    worst = int(der.ulps(got, ref).max())
    print(f"max ulp distance to sklearn's dense path: {worst} (bound {bound:g}, cols {X.shape[1]})")
    assert worst <= bound
