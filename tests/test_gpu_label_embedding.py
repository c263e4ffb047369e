"""Label embeddings on the device (K12): the transpose, the row normalisation, the hstack and xrl_label_embedding_device against the numpy
statements of the rules (tests/label_embedding_rule.py) and the recorded reference (tests/golden/label_embedding_ref.npz), bit for bit --
row pointer, indices, value bits -- and which kernel form served which row, from the form counters."""
import os

import numpy as np
import pytest

import clustering_rule as cr
import device_views as dv
import label_embedding_rule as ler
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RECORDED = np.load(os.path.join(GOLDEN, "label_embedding_ref.npz"))
_memo = {}


def memo(key, make):
    """a case or a statement's answer, computed once and shared"""
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def to_dev(M, device="cuda:0"):
    """Csr -> (crow int64, col int32, val float32, shape) CUDA tensors holding the same bits"""
    import torch
    return (torch.from_numpy(M.indptr.view(np.int64).copy()).to(device), torch.from_numpy(M.indices.view(np.int32).copy()).to(device),
            torch.from_numpy(M.data.copy()).to(device), M.shape)


def dm(M):
    from pecos_amd import DeviceMatrix
    return DeviceMatrix.from_torch(*to_dev(M))


def host(D, stream=None):
    crow, col, val, shape = D.to_torch(stream=stream)
    return ler.csr(crow.cpu().numpy().view(np.uint64), col.cpu().numpy().view(np.uint32), val.cpu().numpy(), shape)


def assert_same(got, want, what=""):
    assert got.shape == want.shape, f"{what}: shape {got.shape}, want {want.shape}"
    assert np.array_equal(got.indptr, want.indptr), f"{what}: row pointer"
    assert np.array_equal(got.indices, want.indices), f"{what}: indices"
    assert np.array_equal(ler.bits(got.data), ler.bits(want.data)), f"{what}: value bits"


def forms_of(run):
    from pecos_amd import clib
    a = clib.debug_embed_forms()
    out = run()
    b = clib.debug_embed_forms()
    assert a["cap"] == b["cap"] == ler.CAP
    return out, {k: b[k] - a[k] for k in ("t_lds", "t_big", "n_lane", "n_wave")}


# ---------------------------------------------------------------------------------------------------------------- transpose
@pytest.mark.parametrize("unsorted", [True, False])
def test_transpose_by_column_count_and_form(unsorted):
    """columns of 0, 1, 63, 64, 65, CAP - 1, CAP, CAP + 1 and 20 000 entries (two of them one or two more: a duplicate id in a source row);
    empty source rows; unsorted source rows"""
    M = memo(("counted", unsorted), lambda: ler.counted_columns(unsorted=unsorted))
    counts = np.bincount(M.indices, minlength=M.shape[1])
    assert {0, 1, 63, 64, 65, ler.CAP - 1, ler.CAP, ler.CAP + 1} <= set(counts.tolist()) and counts.max() > 20000
    T, forms = forms_of(lambda: host(dm(M).transpose()))
    assert_same(T, memo(("counted_T", unsorted), lambda: ler.transpose(M)))
    assert forms["t_lds"] == int(((counts > 0) & (counts <= ler.CAP)).sum()) and forms["t_big"] == int((counts > ler.CAP).sum()) == 2


@pytest.mark.parametrize("name", ["no_rows", "one_row", "no_entries", "no_columns", "golden_Y"])
def test_transpose_small_shapes(name):
    M = {"no_rows": lambda: ler.from_rows([], 5), "one_row": lambda: ler.from_rows([[(4, 1.0), (0, 2.0), (4, 3.0)]], 5),
         "no_entries": lambda: ler.from_rows([[], [], []], 4), "no_columns": lambda: ler.from_rows([[], []], 0),
         "golden_Y": lambda: ler.from_scipy(ler.golden_inputs()[0])}[name]()
    D = dm(M)
    T = D.transpose()
    assert T.shape == (M.shape[1], M.shape[0]) and T.info["nnz"] == len(M.data)
    assert_same(host(T), ler.transpose(M), name)
    assert_same(host(T.transpose()), ler.transpose(ler.transpose(M)), name + " twice")


def test_transposing_twice_gives_the_canonical_stable_order():
    M = memo(("counted", True), lambda: ler.counted_columns())
    back = host(dm(M).transpose().transpose())
    order = np.concatenate([int(M.indptr[r]) + np.argsort(M.indices[int(M.indptr[r]):int(M.indptr[r + 1])], kind="stable") for r in range(M.shape[0])])
    assert_same(back, ler.csr(M.indptr, M.indices[order], M.data[order], M.shape))
    b, s = int(back.indptr[7]), slice(int(M.indptr[7]), int(M.indptr[7]) + 3)
    assert back.indices[b:b + 3].tolist() == [8, 8, 10]                   # the duplicate id is kept, its two entries in stored order
    assert np.array_equal(ler.bits(back.data[b:b + 2]), ler.bits(M.data[s][M.indices[s] == 8]))


def test_transpose_with_the_largest_column_id():
    """cols = 2^32 - 1 and an entry in column cols - 1: the output has 2^32 - 1 rows, read back through a second transpose and through
    the product that selects some of its rows"""
    cols = 2 ** 32 - 1
    f = np.float32
    M = ler.from_rows([[(cols - 1, f(1.5)), (5, f(2.0))], [], [(cols - 1, f(-3.0)), (0, f(4.0)), (cols - 1, f(0.5))]], cols)
    T = dm(M).transpose()
    assert T.shape == (cols, 3) and T.info["nnz"] == 5
    assert_same(host(T.transpose()), ler.from_rows([[(5, f(2.0)), (cols - 1, f(1.5))], [], [(0, f(4.0)), (cols - 1, f(-3.0)), (cols - 1, f(0.5))]], cols))
    sel = ler.from_rows([[(cols - 1, f(1.0))], [(0, f(1.0))], [(5, f(1.0))], [(7, f(1.0))]], cols)
    P = host(dm(sel).multiply(T, False, False))
    assert_same(P, ler.from_rows([[(0, f(1.5)), (2, f(-2.5))], [(2, f(4.0))], [(0, f(2.0))], []], 3))      # (a product sums the duplicate: -3 + 0.5)
    for j, r in zip((cols - 1, 0, 5), range(3)):
        src, val = ler.transpose_column(M, j)
        assert len(src) > 0 and set(src.tolist()) == set(P.indices[int(P.indptr[r]):int(P.indptr[r + 1])].tolist())
    # ... and normalised (PII of a label matrix this wide): 2^32 - 1 rows in more than one launch
    small = ler.from_rows([[(0, f(1.5)), (2, f(-3.0)), (2, f(0.5))], [(2, f(4.0))], [(0, f(2.0))], []], 3)
    eye = ler.from_rows([[(i, f(1.0))] for i in range(4)], 4)
    assert_same(host(dm(sel).multiply(T.normalize_rows(), False, False)), ler.product(eye, ler.normalize(small)), "normalised")


def wrap_banded(M, offs, val_fill=np.float32(np.nan)):
    from pecos_amd import DeviceMatrix
    fills = (np.int64(0), np.int32(0), val_fill)
    bands = [dv.banded(M.indptr.view(np.int64), offs[0], dv.BAND, fills[0], "cuda"), dv.banded(M.indices.view(np.int32), offs[1], dv.BAND, fills[1], "cuda"),
             dv.banded(M.data, offs[2], dv.BAND, fills[2], "cuda")]
    return bands, fills, DeviceMatrix.from_torch(bands[0][1], bands[1][1], bands[2][1], M.shape)


def test_transpose_of_caller_buffers_at_odd_offsets_on_a_side_stream():
    import torch
    M = memo(("counted", True), lambda: ler.counted_columns())
    bands, fills, D = wrap_banded(M, (1, 3, 1))
    assert bands[0][1].data_ptr() % 16 == 8 and bands[1][1].data_ptr() % 16 == 12 and bands[2][1].data_ptr() % 16 == 4
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        T = host(D.transpose(stream=side.cuda_stream), stream=side.cuda_stream)
    assert_same(T, memo(("counted_T", True), lambda: ler.transpose(M)))
    for (whole, payload), fill in zip(bands, fills):
        dv.assert_bands_intact(whole, payload, fill, "source")
    assert_same(host(D), M, "the source")


# ---------------------------------------------------------------------------------------------------------------- normalise
def test_normalize_by_row_length_and_form():
    """rows of 0, 1, 2, 63, 64, 65, 127, 128, 129, 1025 and 4098 entries, into a new handle and in place"""
    M = memo("rows_1", lambda: ler.random_rows())
    lens = np.diff(M.indptr.astype(np.int64))
    assert set(ler.NORMALIZE_LENGTHS) == set(lens.tolist())
    want = memo("rows_1_N", lambda: ler.normalize(M))
    D = dm(M)
    N, forms = forms_of(lambda: D.normalize_rows())
    assert forms["n_lane"] == int(((lens > 0) & (lens < 64)).sum()) == 4 and forms["n_wave"] == int((lens >= 64).sum()) == 7
    assert_same(host(N), want, "new handle")
    assert_same(host(D), M, "the operand of a new handle")
    assert N.info["val"] != D.info["val"] and N.info["row_ptr"] != D.info["row_ptr"]
    assert D.normalize_rows(in_place=True) is D
    assert_same(host(D), want, "in place")


def test_normalize_the_mandatory_order_rows():
    for rev in (False, True):
        M = memo(("order", rev), lambda: ler.order_rows(rev))
        N = host(dm(M).normalize_rows())
        assert_same(N, memo(("order_N", rev), lambda: ler.normalize(M)), f"reverse={rev}")
        k = 4096 if rev else 1
        got = [int(ler.bits(N.data)[int(N.indptr[r]) + k]) for r in range(3)]
        assert got == [b - 1 if rev else b for b in ler.ORDER_SKLEARN_BITS]
    assert not np.array_equal(ler.bits(ler.normalize(ler.order_rows(), "reversed").data), ler.bits(memo(("order_N", False), lambda: None).data))


@pytest.mark.parametrize("scale", [1e-3, 1e10, 1e-21, 1e-25, 1e25])
def test_normalize_random_rows_at_scale(scale):
    """1e-21: subnormal squares; 1e-25: squares that round to zero (rows left as they are); 1e25: squares overflow (rows of zeros)"""
    M = ler.random_rows(scale=scale)
    want = ler.normalize(M)
    if scale == 1e25:
        assert np.all(want.data == 0)
    if scale == 1e-25:
        assert np.array_equal(ler.bits(want.data), ler.bits(M.data))
    if scale == 1e-21:
        sq = (M.data * M.data)
        assert np.any((sq > 0) & (sq < np.float32(1.17549435e-38)))
    assert_same(host(dm(M).normalize_rows()), want, f"scale {scale}")


def test_normalize_zero_rows_inf_nan_and_signed_zeros():
    M = ler.special_rows()
    want = ler.normalize(M)
    assert np.array_equal(ler.bits(want.data[:3]), ler.bits(M.data[:3]))      # the all-zero row with explicit zeros stays
    assert_same(host(dm(M).normalize_rows()), want)
    D = dm(M)
    D.normalize_rows(in_place=True)
    assert_same(host(D), want, "in place")


def test_normalize_caller_buffers_in_place_on_a_side_stream():
    import torch
    M = memo("rows_1", lambda: ler.random_rows())
    bands, fills, D = wrap_banded(M, (1, 1, 3), val_fill=np.float32(7.0))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        D.normalize_rows(in_place=True, stream=side.cuda_stream)
    side.synchronize()
    want = memo("rows_1_N", lambda: ler.normalize(M))
    assert np.array_equal(ler.bits(bands[2][1].cpu().numpy()), ler.bits(want.data))           # the caller's array was rewritten
    assert np.array_equal(bands[1][1].cpu().numpy().view(np.uint32), M.indices) and np.array_equal(bands[0][1].cpu().numpy().view(np.uint64), M.indptr)
    for (whole, payload), fill in zip(bands, fills):
        dv.assert_bands_intact(whole, payload, fill, "operand")


# ---------------------------------------------------------------------------------------------------------------- embeddings end to end
def recorded(method, normalized_Y):
    k = ler.golden_key(method, normalized_Y)
    return ler.csr(RECORDED[k + "__indptr"], RECORDED[k + "__indices"], RECORDED[k + "__data"], tuple(RECORDED[k + "__shape"]))


@pytest.mark.parametrize("normalized_Y", [True, False])
@pytest.mark.parametrize("method", ler.METHODS)
def test_recorded_reference_embeddings(method, normalized_Y):
    import pecos_amd
    Y, X, Z = memo("golden", ler.golden_inputs)
    want = recorded(method, normalized_Y)
    before = [(M.indptr.copy(), M.indices.copy(), M.data.copy()) for M in (Y, X, Z)]
    ops = [pecos_amd.DeviceMatrix.upload(M) for M in (Y, X, Z)]
    E = pecos_amd.label_embedding_device(ops[0], ops[1], method=method, Z=ops[2], normalized_Y=normalized_Y)
    assert_same(host(E), want, "resident operands")
    for D, M in zip(ops, (Y, X, Z)):
        assert_same(host(D), ler.from_scipy(M), "an operand after the call")
    kw = {} if method == "pii" else dict(normalized_Y=normalized_Y, threads=3)
    if method == "pifa_lf_concat":
        kw["Z"] = Z
    F = pecos_amd.LabelEmbeddingFactory.create(Y, X, method=method, **kw)
    assert F.dtype == np.float32 and F.shape == want.shape
    assert ler.same((F.indptr, F.indices, F.data), ler.triple(want))
    assert all(np.array_equal(a, b) for M, old in zip((Y, X, Z), before) for a, b in zip((M.indptr, M.indices, M.data), old))


@pytest.mark.parametrize("case", ["fwd", "flip", "transpose_order"])
def test_order_of_the_samples_is_the_order_of_the_additions(case):
    import pecos_amd
    Y, X = {"fwd": ler.order_case, "flip": lambda: ler.order_case(True), "transpose_order": ler.transpose_order_case}[case]()
    for normalized_Y in (False, True):
        want = ler.embedding(Y, X, normalized_Y=normalized_Y)
        assert_same(host(pecos_amd.label_embedding_device(to_dev(Y), to_dev(X), normalized_Y=normalized_Y)), want, case)
    raw = ler.product(ler.transpose(Y), X)
    assert int(raw.indices[0]) == 0 and (ler.bits(raw.data)[0] == 0) == (case != "flip")


@pytest.mark.parametrize("method", ler.METHODS)
def test_empty_label_empty_sample_and_duplicate_entries(method):
    import pecos_amd
    Y, X, Z = ler.sparse_edges()
    want = ler.embedding(Y, X, Z, method)
    assert want.indptr[3] - want.indptr[2] == (2 if method == "pifa_lf_concat" else 0)         # label 2 has no sample
    E = pecos_amd.label_embedding_device(to_dev(Y), to_dev(X), method=method, Z=to_dev(Z))
    assert_same(host(E), want, method)


def test_empty_inputs_give_empty_handles():
    import pecos_amd
    Y, X = ler.from_rows([[], [], []], 4), ler.from_rows([[], [], []], 6)
    E = pecos_amd.label_embedding_device(to_dev(Y), to_dev(X))
    assert E.shape == (4, 6) and E.info["nnz"] == 0 and np.array_equal(host(E).indptr, np.zeros(5, np.uint64))
    E = pecos_amd.label_embedding_device(to_dev(ler.from_rows([], 4)), to_dev(ler.from_rows([], 6)), method="pii")
    assert E.shape == (4, 0) and E.info["nnz"] == 0
    N = dm(ler.from_rows([], 3)).normalize_rows()
    assert N.shape == (0, 3) and N.info["nnz"] == 0


# ---------------------------------------------------------------------------------------------------------------- the chain
def recorded_chain():
    return [(tuple(RECORDED[f"chain__{i}__shape"]), RECORDED[f"chain__{i}__indptr"], RECORDED[f"chain__{i}__indices"], RECORDED[f"chain__{i}__data"])
            for i in range(int(RECORDED["chain__levels"][0]))]


def test_embedding_feeds_the_clustering_in_hbm():
    import pecos_amd
    import scipy.sparse as smat
    Y, X, _ = memo("golden", ler.golden_inputs)
    E = pecos_amd.label_embedding_device(Y, X)
    depth = pecos_amd.HierarchicalKMeans.TrainParams(**ler.GOLDEN_CHAIN).infer_binary_tree_depth(E.shape[0])
    codes = pecos_amd.run_clustering_device(E, depth, seed=ler.GOLDEN_CHAIN["seed"]).cpu().numpy().view(np.uint32)
    Eh = E.download()
    assert ler.same((Eh.indptr, Eh.indices, Eh.data), ler.triple(recorded("pifa", True)))
    assert np.array_equal(codes, cr.statement(Eh, depth, seed=ler.GOLDEN_CHAIN["seed"])["codes"])
    shape, indptr, indices, data = recorded_chain()[-1]
    leaf = smat.csc_matrix((data, indices, indptr), shape=shape).tocsr()
    assert shape == (E.shape[0], 1 << depth) and np.array_equal(codes, leaf.indices.astype(np.uint32))


def test_factory_feeds_hierarchical_kmeans_gen():
    from pecos_amd import HierarchicalKMeans, LabelEmbeddingFactory
    Y, X, _ = memo("golden", ler.golden_inputs)
    chain = HierarchicalKMeans.gen(LabelEmbeddingFactory.create(Y, X, method="pifa"), train_params=HierarchicalKMeans.TrainParams(**ler.GOLDEN_CHAIN))
    want = recorded_chain()
    assert len(chain) == len(want)
    for C, (shape, indptr, indices, data) in zip(chain, want):
        C = C.tocsc()
        C.sort_indices()
        assert C.shape == shape and np.array_equal(C.indptr, indptr) and np.array_equal(C.indices, indices) and np.array_equal(C.data, data)


# ---------------------------------------------------------------------------------------------------------------- hstack
def test_hstack_of_one_two_and_three_matrices():
    from pecos_amd import DeviceMatrix
    f = np.float32
    A = ler.from_rows([[], [(2, f(1.0)), (0, f(-0.0))], [(1, f(2.0))], [], [(0, f(3.0)), (0, f(4.0))]], 3)
    B = ler.from_rows([[(0, f(5.0))], [], [(1, f(6.0)), (0, f(7.0))], [], []], 2)
    C = ler.random_rows(lengths=(70, 0, 1, 130, 0), seed=4, cols=900)
    mats = [A, B, C]
    devs = [dm(M) for M in mats]
    for n in (1, 2, 3):
        assert_same(host(DeviceMatrix.hstack(devs[:n])), ler.hstack(mats[:n]), f"{n} matrices")
    assert_same(host(DeviceMatrix.hstack([devs[2], devs[0], devs[2]])), ler.hstack([C, A, C]))


def test_hstack_ids_at_the_width_boundary():
    from pecos_amd import DeviceMatrix
    f = np.float32
    wide = 2 ** 32 - 4
    A = ler.from_rows([[(wide - 1, f(1.0)), (0, f(2.0))], [(7, f(3.0))]], wide)
    B = ler.from_rows([[(2, f(4.0))], [(0, f(5.0)), (2, f(6.0))]], 3)
    H = host(DeviceMatrix.hstack([dm(A), dm(B)]))
    assert H.shape == (2, 2 ** 32 - 1)
    assert_same(H, ler.hstack([A, B]))
    assert H.indices.tolist() == [wide - 1, 0, 2 ** 32 - 2, 7, wide, 2 ** 32 - 2]


def test_refusals_on_the_device(tmp_path):
    import xrl_synth
    from pecos_amd import DeviceMatrix, XLinearModel, clib
    A, B = dm(ler.from_rows([[(0, 1.0)], []], 3)), dm(ler.from_rows([[(0, 1.0)]], 3))
    for call, needle in ((lambda: DeviceMatrix.hstack([A, B]), "rows"), (lambda: DeviceMatrix.hstack([]), "no matrices"),
                         (lambda: DeviceMatrix.hstack([A, dm(ler.from_rows([[], []], 2 ** 32 - 3))]), "2^32")):
        with pytest.raises(RuntimeError, match="xrl_smat_hstack_device: ") as e:
            call()
        assert needle in str(e.value)
    bad = dm(ler.from_rows([[(0, 1.0), (3, 2.0)]], 3))                                           # a column id the matrix does not have
    with pytest.raises(RuntimeError, match="xrl_smat_transpose_device: an entry names a column"):
        bad.transpose()
    xrl_synth.make_model(str(tmp_path), 500, 800, [150, 90, 25], seed=21, shape=[4, 28, 800])
    m = XLinearModel.load(str(tmp_path))
    q = clib.queries_upload(m.model.model_chain, np.ones((2, 500), dtype=np.float32))
    try:
        for call, name in ((lambda: clib.smat_transpose_device(q), "xrl_smat_transpose_device"), (lambda: clib.smat_normalize_rows_device(q), "xrl_smat_normalize_rows_device"),
                           (lambda: clib.smat_hstack_device([A.handle, q]), "xrl_smat_hstack_device"),
                           (lambda: clib.label_embedding_device(A.handle, q), "xrl_label_embedding_device")):
            with pytest.raises(RuntimeError, match=name + ": .*must be a CSR handle"):
                call()
    finally:
        clib.queries_free(q)
