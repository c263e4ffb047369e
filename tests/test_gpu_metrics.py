"""The device metrics (K8, xrl_metrics_device) on the GPU: d_matched and d_recall_sum equal the numpy restatement of tests/metrics_cases.py
BIT FOR BIT -- the integers and, since the summation order is a function of the inputs only, the fp64 sums -- on every case: rows on both
sides of the 64-row blocks (and one call past 262144 rows, where blocks become 128 rows), strides and topk on both sides of the 64-entry
slots with topk below, at and above the stride, empty rows, counts above the stride, true rows of every length, the order cases, and
caller-owned buffers: odd offsets between poison bands, outputs between sentinels, a row window by pointer offset, a side stream, no rows.
End to end: a golden model's predict_from_torch and an ensemble_device result fed to metrics_device."""
import os

import numpy as np
import pytest

import metrics_cases as mc
from conftest import GOLDEN, load_X
from device_views import BAND, assert_bands_intact, banded

pytestmark = pytest.mark.gpu

SENT_M = 0x5A5A5A5A5A5A5A5A      # the outputs' sentinels
SENT_R = -7.0
OFFSETS = dict(idx=1, val=3, cnt=2, tptr=1, tidx=3, matched=1, recall=1)         # odd ELEMENT offsets from a 16-byte boundary


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def upload(c):
    """Every array of a case inside a larger tensor of the test's, between poison bands: labels / true labels = valid ids that would match,
    scores = +inf (the best), counts = a full row, row pointers = the valid offset 0."""
    poison = dict(idx=np.int32(7), val=np.float32(np.inf), cnt=np.int32(1 << 20), tptr=np.int64(0), tidx=np.int32(7))
    arrays = dict(idx=c["idx"].view(np.int32), val=c["val"], cnt=c["cnt"].view(np.int32), tptr=c["tptr"].view(np.int64),
                  tidx=(c["tidx"] if len(c["tidx"]) else np.zeros(1, np.uint32)).view(np.int32))
    return {k: banded(np.array(a), OFFSETS[k], BAND, poison[k], "cuda") + (poison[k],) for k, a in arrays.items()}


def outputs(topk):
    m = banded(np.full(topk, SENT_M, np.int64), OFFSETS["matched"], BAND, np.int64(SENT_M), "cuda")
    r = banded(np.full(topk, SENT_R, np.float64).view(np.int64), OFFSETS["recall"], BAND, np.float64(SENT_R).view(np.int64), "cuda")
    return m, r


def run(d, rows, stride, topk, row0=0, stream=None, sync=True, out_topk=None):
    """xrl_metrics_device on rows [row0, row0 + rows) of the uploaded case, by pointer offset; returns (matched u64, recall_sum f64)."""
    import torch
    from pecos_amd import clib
    m, r = outputs(out_topk or topk)
    torch.cuda.synchronize()
    a = {k: v[1].data_ptr() for k, v in d.items()}
    clib.metrics_device(0, rows, a["idx"] + 4 * row0 * stride, a["val"] + 4 * row0 * stride, a["cnt"] + 4 * row0, stride, a["tptr"] + 8 * row0, a["tidx"],
                        topk, m[1].data_ptr(), r[1].data_ptr(), stream=stream, sync=sync)
    if stream is not None:
        torch.cuda.synchronize()
    for k, (whole, view, fill) in d.items():
        assert_bands_intact(whole, view, fill, k)
    assert_bands_intact(m[0], m[1], np.int64(SENT_M), "matched")
    assert_bands_intact(r[0], r[1], np.float64(SENT_R).view(np.int64), "recall_sum")
    return m[1].cpu().numpy().view(np.uint64), r[1].cpu().numpy().view(np.float64)


def check(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: matched differs: {got[0][:8]} vs {want[0][:8]}"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{what}: recall_sum differs: {got[1][:8]} vs {want[1][:8]}"


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_sums_equal_the_restatement(name):
    c = mc.case(name)
    rows, stride = c["idx"].shape
    d = upload(c)
    check(run(d, rows, stride, c["topk"]), mc.expected(name), name)
    if name in mc.GOLDEN:                                                # and through them the reference's recorded metrics
        _, prec, recall = mc.golden(name)
        m, s = run(d, rows, stride, c["topk"])
        p, r = mc.from_sums(m, s, rows)
        assert np.array_equal(bits(p), bits(prec))
        assert np.array_equal(bits(r), bits(recall)) if rows <= 64 else float(np.max(np.abs(r - recall))) <= mc.recall_bound(rows)


def test_other_topk_on_the_same_rows():
    # topk below / at / above the stride and above every row's count on one case; an order case needs the ranking at every topk
    c = mc.case("r129_s64_k65")
    d = upload(c)
    for topk in (1, 10, 63, 64, 65, 1024):
        check(run(d, 129, 64, topk), mc.metric_sums(c, topk=topk), f"topk {topk}")
    o = mc.case("order")
    d = upload(o)
    for topk in (1, 2, 4, 65):
        check(run(d, o["idx"].shape[0], 4, topk), mc.metric_sums(o, topk=topk), f"order, topk {topk}")


def test_past_262144_rows_blocks_of_128():
    c = mc.big_case()
    rows = c["idx"].shape[0]
    assert rows == 262145 and mc.rows_per_block(rows) == 128
    want = mc.metric_sums(c)
    assert want[0][0] > 1000 and not np.array_equal(bits(want[1]), bits(mc.metric_sums(c, block=64)[1]))      # the block size shows in the bits
    check(run(upload(c), rows, 2, c["topk"]), want, "262145 rows")


def test_row_window_by_pointer_offset():
    c = mc.case("r129_s10_k10")
    d = upload(c)
    for lo, hi in ((0, 64), (1, 66), (37, 129), (64, 65), (128, 129)):
        w = dict(c)
        w["idx"], w["val"], w["cnt"], w["tptr"] = c["idx"][lo:hi], c["val"][lo:hi], c["cnt"][lo:hi], c["tptr"][lo:hi + 1]
        check(run(d, hi - lo, 10, 10, row0=lo), mc.metric_sums(w), f"rows [{lo}, {hi})")


def test_on_a_side_stream_without_sync():
    import torch
    c = mc.case("r65_s63_k64")
    s = torch.cuda.Stream()
    check(run(upload(c), 65, 63, 64, stream=s.cuda_stream, sync=False), mc.expected("r65_s63_k64"), "side stream")


def test_no_rows_zero_fills():
    c = mc.case("r63_s10_k10")
    m, r = run(upload(c), 0, 10, 10)
    assert not m.any() and np.array_equal(bits(r), np.zeros(10, np.uint64))
    import torch
    from pecos_amd.features import metrics_sums_device
    e = (torch.zeros((0, 5), dtype=torch.int32, device="cuda"), torch.zeros((0, 5), dtype=torch.float32, device="cuda"),
         torch.zeros((0,), dtype=torch.int32, device="cuda"))
    m, r = metrics_sums_device(e, (torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")), topk=4)
    assert m.shape == (4,) and m.dtype == torch.int64 and r.dtype == torch.float64 and not m.any() and not r.any()


# ------------------------------------------------------------------------------------------------------------------ the python surface
def _triple(c):
    import torch
    return tuple(torch.from_numpy(np.array(a)).cuda() for a in (c["idx"].view(np.int32), c["val"], c["cnt"].view(np.int32)))


def test_python_surface_csr_and_device_truth():
    import torch
    from pecos_amd import Metrics, metrics_device, metrics_sums_device
    name = "r129_s10_k10"
    c, (_, prec, recall) = mc.case(name), mc.golden(name)
    res = _triple(c)
    Y = mc.true_csr(c)
    shuffled = Y.copy()                                                  # unsorted indices: sorted into a copy, the caller's matrix stays
    for r in range(Y.shape[0]):
        a, b = Y.indptr[r], Y.indptr[r + 1]
        shuffled.indices[a:b] = Y.indices[a:b][::-1]
    shuffled.has_sorted_indices = False
    before = shuffled.indices.copy()
    pair = (torch.from_numpy(c["tptr"].astype(np.int64)).cuda(), torch.from_numpy(np.array(c["tidx"].view(np.int32))).cuda())
    for truth in (Y, shuffled, pair):
        m, s = metrics_sums_device(res, truth, topk=10, n_cols=None if truth is pair else c["n_cols"])
        assert m.is_cuda and m.dtype == torch.int64 and s.dtype == torch.float64
        check((m.cpu().numpy().view(np.uint64), s.cpu().numpy()), mc.expected(name), "metrics_sums_device")
    assert np.array_equal(shuffled.indices, before)
    got = metrics_device(res, Y, topk=10)
    assert isinstance(got, Metrics) and np.array_equal(bits(got.prec), bits(prec))
    assert float(np.max(np.abs(got.recall - recall))) <= mc.recall_bound(129)
    with pytest.raises(ValueError, match="rows"):
        metrics_sums_device(res, Y[:100], topk=10)
    with pytest.raises(ValueError, match="columns"):
        metrics_sums_device(res, Y, topk=10, n_cols=c["n_cols"] + 1)
    with pytest.raises(ValueError, match=r"xrl_metrics_device: topk must be 1\.\.1024, got 1025"):
        metrics_sums_device(res, Y, topk=1025)
    wide = (torch.zeros((2, 1025), dtype=torch.int32, device="cuda"), torch.zeros((2, 1025), dtype=torch.float32, device="cuda"),
            torch.zeros((2,), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match=r"xrl_metrics_device: stride must be 1\.\.1024, got 1025"):
        metrics_sums_device(wide, Y[:2], topk=10)


def test_golden_model_end_to_end():
    # predict_from_torch equals the reference's predict on this golden (test_gpu_device_inputs), so its metrics are the recorded
    # Metrics.generate of the reference's own predict: 64 rows = one block, prec AND recall bit for bit
    import scipy.sparse as smat
    import torch
    from pecos_amd import XLinearModel, metrics_device
    from pecos_amd.features import predict_from_torch
    z = np.load(os.path.join(mc.GOLDEN_DIR, "e2e_s_eurlex.npz"))
    m = XLinearModel.load(os.path.join(GOLDEN, "synth", "s_eurlex"))
    X = load_X(os.path.join(GOLDEN, "synth", "s_eurlex__X.npz"))
    Y = smat.csr_matrix((np.ones(len(z["tindices"]), np.float32), z["tindices"].astype(np.int64), z["tindptr"]), shape=(X.shape[0], m.nr_pred_cols))
    dev = torch.device("cuda", 0)
    res = predict_from_torch(m, torch.from_numpy(X.indptr.astype(np.int64)).to(dev), torch.from_numpy(X.indices.astype(np.int32)).to(dev),
                             torch.from_numpy(X.data.astype(np.float32)).to(dev), X.shape[1], beam_size=10, only_topk=10)
    for k in (10, 15):
        got = metrics_device(res, Y, topk=k, n_cols=m.nr_pred_cols)
        assert np.array_equal(bits(got.prec), bits(z[f"prec{k}"])) and np.array_equal(bits(got.recall), bits(z[f"recall{k}"])), (k, got)


def test_ensemble_output_feeds_the_metrics():
    import torch
    from ensemble_cases import Case
    from pecos_amd import metrics_sums_device
    from pecos_amd.features import ensemble_device
    e = Case("a")
    t = [(torch.from_numpy(i.view(np.int32)).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(n.view(np.int32)).cuda())
         for i, v, n in zip(e.idx, e.val, e.cnt)]
    out = ensemble_device(t, mode="average")
    rng = np.random.default_rng(8)
    true = [np.unique(rng.integers(0, e.n_cols, size=int(rng.integers(0, 6)))) for _ in range(e.rows)]
    tptr = np.concatenate([[0], np.cumsum([len(x) for x in true])]).astype(np.uint64)
    c = dict(idx=out[0].cpu().numpy().view(np.uint32), val=out[1].cpu().numpy(), cnt=out[2].cpu().numpy().view(np.uint32), tptr=tptr,
             tidx=np.concatenate(true).astype(np.uint32), topk=10, n_cols=e.n_cols)
    pair = (torch.from_numpy(tptr.astype(np.int64)).cuda(), torch.from_numpy(c["tidx"].view(np.int32)).cuda())
    m, s = metrics_sums_device(out, pair, topk=10)
    want = mc.metric_sums(c)
    assert want[0][-1] > 0
    check((m.cpu().numpy().view(np.uint64), s.cpu().numpy()), want, "ensemble_device -> metrics_sums_device")
