"""Matcher-aware negatives on the device: K14 (xrl_smat_pattern_union_device) against the numpy statement of the union rule; the bound
kernel against the host loop's number; xrl_single_layer_predict_device against this library's host entry point and, where oracle/_ref is
built, the live reference -- labels, order and score bits; train_chain_device / train_device against the reference as recorded in
tests/golden/man_training_ref.npz, both and HierarchicalMLModel.train against the scipy loop over the host entry points, and end to end;
dense X, a relevance chain and a misshapen matching matrix through train and train_device."""
import os

import numpy as np
import pytest
import scipy.sparse as smat

import matching_rule as mr
import ranker_training_rule as rr
from conftest import GOLDEN
from device_views import SENT_IDX, SENT_VAL, assert_bands_intact, sentinel_out

pytestmark = pytest.mark.gpu

RECORDED = np.load(os.path.join(GOLDEN, "man_training_ref.npz"))
CASES = mr.union_cases()
ONE = np.float32(1).view(np.uint32)
F32 = np.float32


def forms():
    from pecos_amd import clib
    return clib.debug_match_forms()


def delta(after, before):
    return {k: after[k] - before[k] for k in ("lds_rows", "big_rows", "read", "written")}


def device_union(mats, stream=None):
    from pecos_amd import DeviceMatrix
    return DeviceMatrix.pattern_union([DeviceMatrix.upload(A) for A in mats], stream=stream).download()


def assert_is_union(got, mats):
    want = mr.union(mats)
    assert mr.same_pattern(got, want)
    assert got.data.dtype == F32 and np.all(got.data.view(np.uint32) == ONE)


# ------------------------------------------------------------------------------------------------ K14
@pytest.mark.parametrize("name", sorted(CASES))
def test_union_against_the_statement(name):
    mats = CASES[name]
    before = forms()
    got = device_union(mats)
    assert_is_union(got, mats)
    d = delta(forms(), before)
    stored = sum(A.nnz for A in mats)
    if stored and mats[0].shape[0]:
        totals = np.sum([np.diff(A.indptr) for A in mats], axis=0)
        assert d == dict(lds_rows=int((totals <= mr.CAP).sum()), big_rows=int((totals > mr.CAP).sum()), read=stored, written=got.nnz), name


def test_which_form_serves_which_row():
    """One row per call: totals up to CAP in LDS, above through the sort in HBM; then the mixed batch of all of them."""
    for total in mr.TOTALS:
        mats = mr.totals_case(2, totals=(total,), seed=total)
        before = forms()
        got = device_union(mats)
        assert_is_union(got, mats)
        d = delta(forms(), before)
        if total:
            assert (d["lds_rows"], d["big_rows"], d["read"]) == ((1, 0, total) if total <= mr.CAP else (0, 1, total)), total
    mats = mr.totals_case(3)
    before = forms()
    assert_is_union(device_union(mats), mats)
    d = delta(forms(), before)
    assert (d["lds_rows"], d["big_rows"], d["read"]) == (len(mr.TOTALS) - 2, 2, sum(mr.TOTALS))


def test_big_rows_in_batches_under_a_small_budget(monkeypatch):
    monkeypatch.setenv("XRL_MATCH_SCRATCH_ENTRIES", "6000")            # 5000 + 1025 entries do not share a batch
    mats = mr.totals_case(2, totals=(5000, 3, mr.CAP + 1, 5000), cols=3000)
    assert_is_union(device_union(mats), mats)


def test_ids_at_the_ends_of_a_2_32_column_matrix():
    cols = (1 << 32) - 1
    A = mr.raw_csr((2, cols), [([cols - 1, 0], [1.0, np.nan]), ([5], [0.0])])
    B = mr.raw_csr((2, cols), [([0, cols - 1, 7], [0.0, -1.0, 2.0]), ([], [])])
    got = device_union([A, B])
    assert np.array_equal(got.indptr, [0, 3, 4]) and np.array_equal(got.indices, [0, 7, cols - 1, 5]) and np.all(got.data.view(np.uint32) == ONE)


def test_result_operands_count_above_stride_and_counts_none():
    import torch
    from pecos_amd import DeviceMatrix
    rs = np.random.RandomState(3)
    rows, k, cols = 70, 6, 40
    idx = np.stack([rs.choice(cols, k, replace=False) for _ in range(rows)]).astype(np.int32)        # best first = not ascending
    val = rs.standard_normal((rows, k)).astype(F32)
    cnt = rs.randint(0, k + 4, rows).astype(np.int32)                                                 # some counts above the stride
    assert (cnt > k).any() and (cnt == 0).any()
    t = [torch.from_numpy(a).cuda() for a in (idx, val, cnt)]
    other = mr.totals_case(1, totals=tuple(rs.randint(0, 9, rows)), cols=cols, seed=9)[0]
    for counts, lens in ((t[2], np.minimum(cnt, k)), (None, np.full(rows, k))):
        as_csr = mr.raw_csr((rows, cols), [(idx[r, :lens[r]], val[r, :lens[r]]) for r in range(rows)])
        got = DeviceMatrix.pattern_union([DeviceMatrix.from_result((t[0], t[1], counts), cols), DeviceMatrix.upload(other)]).download()
        assert_is_union(got, [as_csr, other])


def test_caller_buffers_at_odd_offsets_on_a_side_stream():
    import torch
    from pecos_amd import DeviceMatrix
    mats = mr.totals_case(3, totals=(0, 5, 64, 65, 200, mr.CAP + 1), cols=5000, seed=4)
    poison = 0x5EADBEEF
    held = []

    def embed(arr, dtype, off):
        whole = torch.full((len(arr) + 2 * off + 5,), float("nan"), dtype=torch.float32, device="cuda") if dtype == torch.float32 else \
            torch.full((len(arr) + 2 * off + 5,), poison, dtype=torch.int64, device="cuda").to(dtype)
        whole[off:off + len(arr)] = torch.from_numpy(np.ascontiguousarray(arr)).to(dtype).cuda()
        held.append((whole, whole.clone()))
        return whole[off:off + len(arr)]

    ops = [DeviceMatrix.from_torch(embed(A.indptr, torch.int64, off), embed(A.indices, torch.int32, off + 1), embed(A.data, torch.float32, off + 2), A.shape)
           for A, off in zip(mats, (1, 3, 5))]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = DeviceMatrix.pattern_union(ops, stream=side.cuda_stream).download()
    assert_is_union(got, mats)
    for whole, before in held:
        assert torch.equal(whole.view(torch.int32), before.view(torch.int32)), "an operand or the poison around it changed"


def test_an_id_out_of_range_is_refused_by_the_check_kernel():
    """A refusal returned as an error: the id is a sort key, never an address."""
    from pecos_amd import DeviceMatrix
    cols = 50
    good = mr.raw_csr((3, cols), [([1, 2], [1, 1]), ([], []), ([49], [1])])
    bad = mr.raw_csr((3, cols + 1), [([4], [1]), ([cols, 3], [1, 1]), ([], [])])
    bad._shape = (3, cols)                                                 # the id 50 under 50 columns
    with pytest.raises(RuntimeError, match="xrl_smat_pattern_union_device: an operand stores a column id that is not below 50"):
        DeviceMatrix.pattern_union([DeviceMatrix.upload(good), DeviceMatrix.upload(bad)])
    assert_is_union(device_union([good]), [good])                          # and the next call is served


# ------------------------------------------------------------------------------------------------ the resident single-layer predict
def host_predict(X, codes, W, C, pp, k, bias=1.0):
    return mr.ours_host_backend()[0](X, codes, W, C, pp, k, bias)


def device_predict(X, codes, W, C, pp, k, bias=1.0, wt=None, stride=None, stream=None, out_stride=None):
    """codes: a scipy CSR (made fixed-stride here) or a ready triple of tensors"""
    import torch
    import pecos_amd
    from pecos_amd import DeviceMatrix
    wt = DeviceMatrix.upload(rr.as_stored_transpose(W)) if wt is None else wt
    if codes is not None and smat.issparse(codes):
        codes = tuple(torch.from_numpy(a).cuda() for a in mr.csr_to_codes(codes, stride))
    got = pecos_amd.single_layer_predict_device(X, wt, None if C is None else smat.csr_matrix(C), codes, post_processor=pp, only_topk=k, bias=bias, stream=stream,
                                                out_stride=out_stride)
    return got, mr.result_to_csr(got, W.shape[1])


def check_predict(X, codes, W, C, pp, k, **kw):
    want = host_predict(X, codes, W, C, pp, k)
    triple, got = device_predict(X, codes, W, C, pp, k, **kw)
    assert mr.same_bits(got, want), "differs from the host entry point"
    if mr.refpy_available():
        assert mr.same_bits(got, smat.csr_matrix(mr.reference_backend()[0](X, codes, W, C, pp, k, 1.0))), "differs from the live reference"
    return triple, got


def golden_layers():
    rec = mr.recorded_config(RECORDED, "tfn+man", "l3-hinge")
    return rr.e2e_problem()[0], rec["W"], mr.recorded_chain(RECORDED), rec["M_pred"]


@pytest.mark.parametrize("pp", ["noop", "l3-hinge", "log-l3-hinge"])
def test_predict_the_recorded_layers_feeding_the_output_back(pp):
    from pecos_amd import clib
    X, W, chain, _ = golden_layers()
    t0, p0 = check_predict(X, None, W[0], chain[0], pp, 4)                 # no codes, one cluster
    assert p0.nnz == 500 * 2, "rows shorter than only_topk stay short"
    t1, p1 = check_predict(X, p0, W[1], chain[1], pp, 4)
    check_predict(X, p1, W[2], chain[2], pp, 5)
    # the function's own output, in place, as the next layer's codes
    _, q1 = device_predict(X, t0, W[1], chain[1], pp, 4)
    assert mr.same_bits(q1, p1)
    _, q2 = device_predict(X, t1, W[2], chain[2], pp, 5)
    assert mr.same_bits(q2, host_predict(X, p1, W[2], chain[2], pp, 5))
    Cm = chain[2].tocsc()
    sizes = np.diff(Cm.indptr)
    assert clib.debug_match_forms()["last_bound"] == max(int(sizes[p1.indices[p1.indptr[r]:p1.indptr[r + 1]]].sum()) for r in range(500))


def test_predict_without_codes_under_several_clusters_is_fill_ones():
    X, W, chain, _ = golden_layers()
    check_predict(X, None, W[1], chain[1], "l3-hinge", 4)
    check_predict(X[:65], None, W[2], chain[2], "noop", 5)
    check_predict(X[:3], None, W[2], None, "l3-hinge", 7)                  # C = None: one cluster that holds every label


@pytest.mark.parametrize("k", [1, 8, 64, 70])
def test_predict_only_topk_at_and_above_the_candidates(k):
    X, W, chain, P = golden_layers()
    codes = mr.raw_csr((6, 8), [([3], [0.5]), ([], []), ([1, 6], [0.25, 0.75]), (np.arange(8), np.linspace(0.1, 0.9, 8)), ([2], [1.0]), ([7, 0], [0.5, 0.5])])
    _, got = check_predict(X[:6], codes, W[2], chain[2], "l3-hinge", k)
    assert list(np.diff(got.indptr)) == [min(k, n) for n in (8, 0, 16, 64, 8, 16)]


def wide_layer(seed=11, N=8, d=60, L=300, K=70):
    """A layer with more than 64 parents, for codes of 64 and 65 entries in a row."""
    rs = np.random.RandomState(seed)
    X = rr.rows_csr(d, rs.randint(1, 20, N), seed)
    W = smat.random(d + 1, L, density=0.3, format="csc", dtype=F32, random_state=rs)
    W.sort_indices()
    code = np.concatenate([np.arange(K), rs.randint(0, K, L - K)])
    C = rr.raw_csc((L, K), [(np.flatnonzero(code == k), np.ones(int((code == k).sum()))) for k in range(K)])
    return X, W, C


def test_bound_kernel_against_the_host_loops_number():
    """Rows of 0, 1, 64 and 65 codes, a parent listed twice, a count above the stride; every occurrence of a repeated parent counts."""
    import torch
    from pecos_amd import clib
    X, W, C = wide_layer()
    sizes = np.diff(C.indptr)
    rs = np.random.RandomState(2)
    rows = [[], [5], list(rs.permutation(70)[:64]), list(rs.permutation(70)[:65]), [9, 9], [69, 0, 69], [1], [2, 3]]
    codes = mr.raw_csr((8, 70), [(r, rs.uniform(0.1, 1.0, len(r))) for r in rows])
    check_predict(X, codes, W, C, "l3-hinge", 10)
    assert clib.debug_match_forms()["last_bound"] == max(int(sizes[r].sum()) for r in rows if r)
    for only in ([4], [5]):                                                # one row at a time: the kernel's number is that row's
        sub = mr.raw_csr((1, 70), [(rows[only[0]], np.ones(len(rows[only[0]])))])
        check_predict(X[only], sub, W, C, "noop", 3)
        assert clib.debug_match_forms()["last_bound"] == int(sizes[rows[only[0]]].sum())
    # a count above the stride reads as the stride: the cells beyond do not exist
    idx, val, cnt = mr.csr_to_codes(codes, stride=65)
    cnt = cnt.copy()
    cnt[[1, 3, 6]] += 7
    cnt[3] = 200
    t = tuple(torch.from_numpy(a).cuda() for a in (idx, val, cnt))
    clipped = mr.raw_csr((8, 70), [(idx[r, :min(cnt[r], 65)], val[r, :min(cnt[r], 65)]) for r in range(8)])
    _, got = device_predict(X, t, W, C, "l3-hinge", 10)
    assert mr.same_bits(got, host_predict(X, clipped, W, C, "l3-hinge", 10))
    assert clib.debug_match_forms()["last_bound"] == max(int(sizes[clipped.indices[clipped.indptr[r]:clipped.indptr[r + 1]]].sum()) for r in range(8))


def test_predict_into_a_wider_stride_between_sentinels_on_a_side_stream():
    import torch
    from pecos_amd import DeviceMatrix, clib
    X, W, chain, P = golden_layers()
    rows, k, stride = 65, 5, 9
    Xq = X[:rows]
    codes = smat.csr_matrix(P[2][:rows])
    want = host_predict(Xq, codes, W[2], chain[2], "l3-hinge", k)
    x, wt, ct = DeviceMatrix.upload(Xq), DeviceMatrix.upload(rr.as_stored_transpose(W[2])), DeviceMatrix.upload(rr.as_stored_transpose(chain[2]))
    ci, cv, cc = (torch.from_numpy(a).cuda() for a in mr.csr_to_codes(codes))
    before = [t.clone() for t in (ci, cv, cc)]
    (wi, oi), (wv, ov), (wc, oc) = sentinel_out(rows, stride, (1, 3, 2))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    clib.single_layer_predict_device(x.handle, wt.handle, ct.handle, ci.data_ptr(), cv.data_ptr(), cc.data_ptr(), ci.shape[1], "l3-hinge", k, 1.0, oi.data_ptr(),
                                     ov.data_ptr(), oc.data_ptr(), stride, stream=side.cuda_stream)
    got = mr.result_to_csr((oi, ov, oc), 64)
    assert mr.same_bits(got, want)
    i, v, c = oi.cpu().numpy(), ov.cpu().numpy(), oc.cpu().numpy()
    for r in range(rows):
        assert np.all(i[r, c[r]:] == np.int32(SENT_IDX)) and np.all(v[r, c[r]:] == SENT_VAL), "entries beyond a row's count were touched"
    for whole, view, fill in ((wi, oi, np.int32(SENT_IDX)), (wv, ov, np.float32(SENT_VAL)), (wc, oc, np.int32(SENT_IDX))):
        assert_bands_intact(whole, view, fill)
    for a, b in zip((ci, cv, cc), before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the codes changed"


@pytest.mark.parametrize("rows", [1, 63, 65, 500])
def test_predict_row_counts(rows):
    X, W, chain, P = golden_layers()
    check_predict(X[:rows], smat.csr_matrix(P[2][:rows]), W[2], chain[2], "l3-hinge", 5)


def test_predict_500_rows_in_three_batches(monkeypatch):
    monkeypatch.setenv("XRL_SINGLE_LAYER_MAX_BATCH_ROWS", "200")
    X, W, chain, P = golden_layers()
    check_predict(X, P[2], W[2], chain[2], "l3-hinge", 5)
    check_predict(X, None, W[1], chain[1], "noop", 4)


def test_predict_with_wt_straight_from_training():
    import pecos_amd
    X, Y, C, M = rr.problem(120, 60, 10, 3, 6, 8, 5)
    wt = pecos_amd.train_layer_device(X, Y.tocsr(), C.tocsr(), threshold=0.05, max_iter=30)
    W = mr.wt_to_w(wt.download())
    assert W.nnz > 0
    codes = mr.raw_csr((120, 3), [([r % 3, (r + 1) % 3][: 1 + r % 2], [0.5, 0.25][: 1 + r % 2]) for r in range(120)])
    check_predict(X, codes, W, C, "l3-hinge", 4, wt=wt)
    check_predict(X, None, W, C, "log-l3-hinge", 10, wt=wt)


def test_predict_refusals_on_the_device():
    import torch
    import pecos_amd
    X, W, C = wide_layer()
    codes = mr.raw_csr((8, 71), [([70], [1.0])] + [([1], [1.0])] * 7)
    with pytest.raises(RuntimeError, match=r"xrl_single_layer_predict_device: csr_codes: parent id 70 out of range \(C has 70 columns\)"):
        device_predict(X, codes, W, C, "l3-hinge", 5)
    t = tuple(torch.from_numpy(a).cuda() for a in mr.csr_to_codes(mr.raw_csr((7, 70), [([1], [1.0])] * 7)))
    with pytest.raises(ValueError, match="Instance dimension of query and prev_layer_pred matrix do not match"):
        pecos_amd.single_layer_predict_device(X, rr.as_stored_transpose(W), smat.csr_matrix(C), t)
    t = tuple(torch.from_numpy(a).cuda() for a in mr.csr_to_codes(mr.raw_csr((8, 70), [([1], [1.0])] * 8)))
    with pytest.raises(ValueError, match="Label dimension of prev_layer_pred and C matrix do not match"):
        pecos_amd.single_layer_predict_device(X, rr.as_stored_transpose(W), smat.csr_matrix(C), t + (71,))
    with pytest.raises(RuntimeError, match="only_topk must be positive"):
        pecos_amd.single_layer_predict_device(X, rr.as_stored_transpose(W), smat.csr_matrix(C), t, only_topk=0)
    with pytest.raises(RuntimeError, match="Feature dimension of query and W do not match"):
        pecos_amd.single_layer_predict_device(X, rr.as_stored_transpose(W), smat.csr_matrix(C), t, bias=0.0)


# ------------------------------------------------------------------------------------------------ the chain
def schemes_of(name):
    names = mr.SCHEMES[name]
    return names if isinstance(names, list) else [names] * 3


def pred_params(post):
    from pecos_amd import MLModel
    return [MLModel.PredParams(only_topk=k, post_processor=p) for p, k in mr.layer_pred_params(post)]


@pytest.mark.parametrize("post", mr.POST)
@pytest.mark.parametrize("scheme", sorted(mr.SCHEMES))
def test_chain_against_the_recorded_reference(scheme, post):
    import pecos_amd
    X, Y, _ = rr.e2e_problem()
    chain = mr.recorded_chain(RECORDED)
    weights, matchings, preds = pecos_amd.train_chain_device(X, smat.csr_matrix(Y), chain, schemes_of(scheme), matching_chain=mr.usn_chain() if "usn" in scheme else None,
                                                             train_params=mr.TRAIN_KW, pred_params=pred_params(post), return_matching=True)
    want = mr.recorded_config(RECORDED, scheme, post)
    for t in range(3):
        assert (matchings[t] is None) == (want["M"][t] is None), f"layer {t}: M"
        if want["M"][t] is not None:
            M = smat.csc_matrix(matchings[t].download())
            M.sort_indices()
            assert mr.same_pattern(M, want["M"][t]), f"layer {t}: M's pattern"
        assert (preds[t] is None) == (want["M_pred"][t] is None), f"layer {t}: M_pred"
        if want["M_pred"][t] is not None:
            assert mr.same_bits(mr.result_to_csr(preds[t], chain[t].shape[1]), want["M_pred"][t]), f"layer {t}: M_pred"
        assert mr.same_bits(mr.wt_to_w(weights[t].download()), want["W"][t]), f"layer {t}: W"


def sorted_csc(W):
    W = smat.csc_matrix(W, dtype=F32, copy=True)
    W.sort_indices()
    return W


@pytest.mark.parametrize("scheme", ["tfn", "usn", "tfn+usn"])
def test_chain_equals_train_on_the_schemes_it_serves(scheme):
    """HierarchicalMLModel.train and train_chain_device are one loop; the independent statement is the scipy loop over the per-layer host entry points."""
    import pecos_amd
    from pecos_amd import HierarchicalMLModel
    from pecos_amd.xlinear import MLProblem
    X, Y, _ = rr.e2e_problem()
    chain, usn = mr.recorded_chain(RECORDED), mr.usn_chain()
    want = mr.chain_loop(X, Y, chain, [scheme] * 3, *mr.ours_host_backend(), mr.layer_pred_params("l3-hinge"), matching_chain=usn)["W"]
    model = HierarchicalMLModel.train(MLProblem(X, Y), clustering=chain, matching_chain=usn, negative_sampling_scheme=scheme, **mr.TRAIN_KW)
    weights, matchings, preds = pecos_amd.train_chain_device(X, smat.csr_matrix(Y), chain, scheme, matching_chain=usn, train_params=mr.TRAIN_KW, return_matching=True)
    assert preds == [None, None, None], "no scheme names man: nothing is predicted"
    for t, layer in enumerate(model.layers):
        W = sorted_csc(layer.W)
        assert W.nnz > 0 and mr.same_bits(W, want[t]), f"layer {t}: train"
        assert mr.same_bits(mr.wt_to_w(weights[t].download()), want[t]), f"layer {t}: train_chain_device"


def test_an_empty_scheme_gives_an_empty_m():
    import pecos_amd
    X, Y, _ = rr.e2e_problem()
    chain = mr.recorded_chain(RECORDED)
    weights, matchings, _ = pecos_amd.train_chain_device(X, smat.csr_matrix(Y), chain, "usn", train_params=mr.TRAIN_KW, return_matching=True)
    assert matchings[0] is None and matchings[1].info["nnz"] == 0 and matchings[2].info["nnz"] == 0
    got = mr.chain_loop(X, Y, chain, ["usn"] * 3, *mr.ours_host_backend(), mr.layer_pred_params("l3-hinge"))
    for t in range(3):
        assert mr.same_bits(mr.wt_to_w(weights[t].download()), got["W"][t])


def test_train_device_save_load_predict(tmp_path):
    """XLinearModel.train_device(tfn+man) -> save -> load -> predict equals the predictions of the recorded weights written as a folder."""
    from pecos_amd import HierarchicalMLModel, MLModel, XLinearModel
    X, Y, C = rr.e2e_problem()
    model = XLinearModel.train_device(X, Y, C=C, negative_sampling_scheme="tfn+man", **rr.E2E_KW)
    want = mr.recorded_config(RECORDED, "tfn+man", "l3-hinge")
    chain = mr.recorded_chain(RECORDED)
    assert model.depth == 3
    for t, layer in enumerate(model.model.layers):
        got = smat.csc_matrix(layer.W)
        got.sort_indices()
        assert mr.same_bits(got, want["W"][t]), f"layer {t}: the weights differ from the reference's"
        assert (smat.csc_matrix(layer.C) != chain[t]).nnz == 0
    model.save(str(tmp_path / "ours"))
    loaded = XLinearModel.load(str(tmp_path / "ours"))
    assert (loaded.depth, loaded.nr_features, loaded.nr_labels) == (3, 200, 64)
    pp = MLModel.PredParams(only_topk=rr.E2E_KW["beam_size"], post_processor=rr.E2E_KW["post_processor"])
    last = MLModel.PredParams(only_topk=rr.E2E_KW["only_topk"], post_processor=rr.E2E_KW["post_processor"])
    ref_layers = [MLModel(W=want["W"][t], C=chain[t], bias=1.0, pred_params=last if t == 2 else pp) for t in range(3)]
    XLinearModel(HierarchicalMLModel._from_layers(ref_layers, HierarchicalMLModel.PredParams(model_chain=[pp, pp, last]))).save(str(tmp_path / "ref"))
    recorded_model = XLinearModel.load(str(tmp_path / "ref"))
    Xq = X[:100]
    a, b, c = loaded.predict(Xq), recorded_model.predict(Xq), model.predict(Xq)
    assert a.nnz == 100 * rr.E2E_KW["only_topk"]
    for other in (b, c):
        assert mr.same_bits(a, other)
    # a trained layer on the host predicts through MLModel.predict as the resident form does
    p0 = model.model.layers[0].predict(Xq)
    p1 = model.model.layers[1].predict(Xq, csr_codes=p0)
    assert mr.same_bits(p0, smat.csr_matrix(want["M_pred"][1][:100])) and mr.same_bits(p1, smat.csr_matrix(want["M_pred"][2][:100]))


def test_one_versus_all_goes_through_the_same_function():
    from pecos_amd import XLinearModel, clib
    from pecos_amd.core import ScipyCscF32, ScipyCsrF32
    X, Y, C, M = rr.problem(120, 60, 10, 3, 6, 8, 5)
    want = sorted_csc(clib.xlinear_single_layer_train(ScipyCsrF32(X), ScipyCscF32(Y), None, None, None, threshold=0.05, max_iter=30))
    a = XLinearModel.train(X, Y, threshold=0.05, max_iter=30)
    b = XLinearModel.train_device(X, Y, threshold=0.05, max_iter=30, negative_sampling_scheme="tfn+man")
    Wa, Wb = sorted_csc(a.model.layers[0].W), sorted_csc(b.model.layers[0].W)
    assert Wa.nnz > 0 and mr.same_bits(Wa, want) and mr.same_bits(Wb, want)
    assert mr.same_bits(a.predict(X[:20]), b.predict(X[:20]))


@pytest.mark.parametrize("own", ["C", "C and M", "C, M and R"])
def test_one_layer_from_a_problem_with_its_own_clusters(own):
    """Without a clustering, train returns MLModel.train(prob)'s layer: the problem's own C and M (given, or filled in as Y * C) and R."""
    from pecos_amd import clib
    from pecos_amd.xlinear import MLProblem
    X, Y, C, M = rr.problem(120, 60, 10, 3, 6, 8, 5)
    R = sorted_csc(Y)
    R.data = np.random.RandomState(44).choice(np.array([0, 0.5, 1, 3], F32), R.nnz).astype(F32)
    prob = MLProblem(X, Y, C=C, M=None if own == "C" else M, R=R if own == "C, M and R" else None)
    want = sorted_csc(clib.xlinear_single_layer_train(prob.pX, prob.pY, prob.pC, prob.pM, prob.pR, **SMALL_KW))
    pure = sorted_csc(clib.xlinear_single_layer_train(prob.pX, prob.pY, None, None, prob.pR, **SMALL_KW))
    assert want.nnz > 0 and not mr.same_bits(want, pure), "C and M do not matter on this problem"
    for name, train in trainers():
        model = train(prob, **SMALL_KW)
        assert len(model.layers) == 1 and model.layers[0].nr_codes == 3 and (smat.csc_matrix(model.layers[0].C) != smat.csc_matrix(C)).nnz == 0, name
        assert mr.same_bits(sorted_csc(model.layers[0].W), want), name


# ------------------------------------------------------------------------------------------------ what train took before it became this loop
SMALL_KW = dict(threshold=0.05, max_iter=30)


def small_chain():
    """120 instances x 60 features x 10 labels under the two-layer chain 1 <- 3 <- 10."""
    X, Y, C, _ = rr.problem(120, 60, 10, 3, 6, 8, 5)
    return X, Y, [smat.csc_matrix(np.ones((3, 1), F32)), C]


def trainers():
    from pecos_amd import HierarchicalMLModel
    return (("train", HierarchicalMLModel.train), ("train_device", HierarchicalMLModel.train_device))


def test_dense_x_through_train_and_train_device():
    """Dense X trains as the CSR that stores every entry, zeros included: a row and a column of zeros among them, and then an inf."""
    from pecos_amd import clib
    from pecos_amd.core import ScipyCscF32, ScipyDrmF32
    from pecos_amd.xlinear import MLProblem
    X, Y, chain = small_chain()
    D = np.ascontiguousarray(X.toarray(), dtype=F32)
    D[7, :] = 0
    D[:, 11] = 0
    every = mr.raw_csr(D.shape, [(np.arange(D.shape[1]), D[r]) for r in range(D.shape[0])])
    assert every.nnz == D.size
    pps = [("l3-hinge", 20)] * 2
    want = mr.chain_loop(every, Y, chain, ["tfn"] * 2, *mr.ours_host_backend(SMALL_KW), pps)["W"]
    flat = sorted_csc(clib.xlinear_single_layer_train(ScipyDrmF32(D), ScipyCscF32(Y), None, None, None, **SMALL_KW))
    assert flat.nnz > 0
    for name, train in trainers():
        layers = train(MLProblem(D, Y), clustering=chain, **SMALL_KW).layers
        assert len(layers) == 2
        for t in range(2):
            assert want[t].nnz > 0 and mr.same_bits(sorted_csc(layers[t].W), want[t]), f"{name}: layer {t}"
        assert mr.same_bits(sorted_csc(train(MLProblem(D, Y), **SMALL_KW).layers[0].W), flat), f"{name}: one-versus-all"
    # With finite X a stored zero adds +0 and changes no bit.  One inf in place of a zero makes them count: its w turns inf or NaN, and
    # every other row's stored zero in that column then brings 0 * w = NaN into its sum, which a CSR without the zeros never sees.
    r0, c0 = next((r, c) for r, c in np.argwhere(D == 0) if r != 7 and c != 11)
    D[r0, c0] = np.inf
    every = mr.raw_csr(D.shape, [(np.arange(D.shape[1]), D[r]) for r in range(D.shape[0])])
    want = mr.chain_loop(every, Y, chain, ["tfn"] * 2, *mr.ours_host_backend(SMALL_KW), pps)["W"]
    without_zeros = mr.chain_loop(smat.csr_matrix(D), Y, chain, ["tfn"] * 2, *mr.ours_host_backend(SMALL_KW), pps)["W"]
    assert not all(mr.same_bits(want[t], without_zeros[t]) for t in range(2)), "the stored zeros do not matter on this problem"
    for name, train in trainers():
        layers = train(MLProblem(D, Y), clustering=chain, **SMALL_KW).layers
        for t in range(2):
            assert mr.same_bits(sorted_csc(layers[t].W), want[t]), f"{name}: layer {t} with an inf among the zeros"


def small_relevance():
    """(Y_0, R_0), (Y_1, R_1) of small_chain(): costs on each layer's own labels, a zero and values above 1 among them."""
    X, Y, chain = small_chain()
    out = []
    for t, Yt in enumerate((sorted_csc(Y.tocsr() * chain[1].tocsr()), sorted_csc(Y))):
        R = Yt.copy()
        R.data = np.random.RandomState(40 + t).choice(np.array([0, 0.5, 1, 3], F32), R.nnz).astype(F32)
        R.data[:2] = (0, 3)
        out.append((Yt, R))
    return out


def test_relevance_chain_through_train():
    from pecos_amd import HierarchicalMLModel, clib
    from pecos_amd.core import ScipyCscF32, ScipyCsrF32
    from pecos_amd.xlinear import MLProblem, _ones_column
    X, Y, chain = small_chain()
    (Y0, R0), (Y1, R1) = small_relevance()
    layers = HierarchicalMLModel.train(MLProblem(X, Y), clustering=chain, relevance_chain=[R0, R1], **SMALL_KW).layers
    M1 = mr.binarized(Y0)
    M1.sort_indices()
    for t, (Yt, M, R) in enumerate(((Y0, _ones_column(120), R0), (Y1, M1, R1))):
        want = sorted_csc(clib.xlinear_single_layer_train(ScipyCsrF32(X), ScipyCscF32(Yt), ScipyCscF32(chain[t]), ScipyCscF32(M), ScipyCscF32(R), **SMALL_KW))
        assert want.nnz > 0 and mr.same_bits(sorted_csc(layers[t].W), want), f"layer {t}"
        unweighted = sorted_csc(clib.xlinear_single_layer_train(ScipyCsrF32(X), ScipyCscF32(Yt), ScipyCscF32(chain[t]), ScipyCscF32(M), None, **SMALL_KW))
        assert not mr.same_bits(want, unweighted), f"layer {t}: the costs do not matter on this problem"


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("fault", ["moved", "negative"])
def test_a_bad_relevance_matrix_is_refused_before_any_training(monkeypatch, layer, fault):
    from pecos_amd import HierarchicalMLModel, clib
    from pecos_amd.xlinear import MLProblem
    X, Y, chain = small_chain()
    rel = [R for _, R in small_relevance()]
    bad = rel[layer].copy()
    if fault == "negative":
        bad.data[5] = -0.5
    else:                                                                  # the first entry of column 0 goes to a row that the column does not store
        col = bad.indices[bad.indptr[0]:bad.indptr[1]]
        bad.indices[0] = np.setdiff1d(np.arange(120), col)[0]
    rel[layer] = bad
    launched = []
    monkeypatch.setattr(type(clib), "train_layer_device", lambda self, *a, **kw: launched.append(a) or pytest.fail("a training was launched"))
    with pytest.raises(ValueError, match="Invalid relevance matrix: " + ("got value < 0" if fault == "negative" else r"Y\.indices != R\.indices")):
        HierarchicalMLModel.train(MLProblem(X, Y), clustering=chain, relevance_chain=rel, **SMALL_KW)
    assert not launched


def test_a_matching_chain_entry_of_the_wrong_shape_is_refused():
    from pecos_amd.xlinear import MLProblem
    X, Y, chain = small_chain()
    for name, train in trainers():
        with pytest.raises(ValueError, match=r"a matching matrix has shape \(120, 4\), the layer needs \(120, 3\)"):
            train(MLProblem(X, Y), clustering=chain, matching_chain=[None, smat.csr_matrix((120, 4), dtype=F32)], negative_sampling_scheme="tfn+usn", **SMALL_KW)


def test_against_the_live_reference_train():
    if not mr.refpy_available():
        pytest.skip("oracle/_ref (the compiled reference and its python package) is not built")
    from pecos_amd import XLinearModel
    mr.import_refpy()
    from pecos.xmc.xlinear.model import XLinearModel as RefModel
    X, Y, C = rr.e2e_problem()
    ref = RefModel.train(X, Y, C=C, negative_sampling_scheme="tfn+man", threads=1, **rr.E2E_KW).model.model_chain
    got = XLinearModel.train_device(X, Y, C=C, negative_sampling_scheme="tfn+man", **rr.E2E_KW).model.layers
    assert len(ref) == len(got) == 3
    for t in range(3):
        a, b = smat.csc_matrix(got[t].W), ref[t].W.tocsc()
        a.sort_indices(); b.sort_indices()
        assert mr.same_bits(a, b), f"layer {t}"


def test_embedding_clustering_chain_resident_against_the_host_steps():
    """label_embedding_device -> run_clustering_device -> a chain built from the codes -> train_chain_device(tfn+man), against the same
    steps through the host entry points and the scipy loop of matching_rule."""
    import torch
    import pecos_amd
    from pecos_amd import DeviceMatrix
    X, Y, _, _ = rr.problem(400, 150, 48, 4, 8, 10, 17)
    Ycsr = smat.csr_matrix(Y)
    depth, L = 3, Y.shape[1]
    x, y = DeviceMatrix.upload(X), DeviceMatrix.upload(Ycsr)
    codes = pecos_amd.run_clustering_device(pecos_amd.label_embedding_device(y, x), depth, seed=2)
    dev = codes.device
    ones = lambda n: torch.ones(n, dtype=torch.float32, device=dev)      # noqa: E731
    leaf = DeviceMatrix.from_torch(torch.arange(L + 1, dtype=torch.int64, device=dev), codes.contiguous(), ones(L), (L, 8))
    mid = DeviceMatrix.from_torch(torch.arange(9, dtype=torch.int64, device=dev), (torch.arange(8, dtype=torch.int32, device=dev) // 4).contiguous(), ones(8), (8, 2))
    root = DeviceMatrix.from_torch(torch.arange(3, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev), ones(2), (2, 1))
    pp = pred_params("l3-hinge")
    weights = pecos_amd.train_chain_device(x, y, [root, mid, leaf], "tfn+man", train_params=mr.TRAIN_KW, pred_params=pp)
    # the host steps
    Eh = pecos_amd.LabelEmbeddingFactory.create(Ycsr, X, method="pifa")
    ch, err = __import__("clustering_rule").run_library(rr.OURS, Eh, depth, seed=2)
    assert err is None and np.array_equal(ch, codes.cpu().numpy().view(np.uint32))
    chain = [smat.csc_matrix(np.ones((2, 1), F32)), smat.csc_matrix((np.ones(8, F32), (np.arange(8), np.arange(8) // 4)), shape=(8, 2)),
             smat.csc_matrix((np.ones(L, F32), (np.arange(L), ch.astype(np.int64))), shape=(L, 8))]
    want = mr.chain_loop(X, Y, chain, ["tfn+man"] * 3, *mr.ours_host_backend(), mr.layer_pred_params("l3-hinge"))
    for t in range(3):
        assert want["W"][t].nnz > 0 and mr.same_bits(mr.wt_to_w(weights[t].download()), want["W"][t]), f"layer {t}"
