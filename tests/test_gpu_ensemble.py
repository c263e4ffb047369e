"""The device ensemble (K6, xrl_ensemble_device) on the GPU: every fixture case (tests/golden/ensemble, the reference's recorded outputs) in
all three modes and every `finish` setting, bit for bit; output / input layouts; a caller's stream; and predict_text / Text2Text.predict end to
end against the host path."""
import numpy as np
import pytest

from ensemble_cases import CASES, FINISH, Case, same_rows

pytestmark = pytest.mark.gpu

SETTINGS = [("average", None, None, "average"), ("rank_average", None, None, "rank_average")] + \
           [("finish", thr, topk, f"finish{i}") for i, (thr, topk) in enumerate(FINISH)]


@pytest.fixture(scope="module", params=CASES)
def dev_case(request):
    import torch
    c = Case(request.param)
    t = [(torch.from_numpy(i.view(np.int32)).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(n.view(np.int32)).cuda())
         for i, v, n in zip(c.idx, c.val, c.cnt)]
    return c, t


def _rows(o_idx, o_sc, o_cnt):
    """(indptr, labels, values) of a fixed-stride device result; entries beyond a row's count are not looked at."""
    idx, sc, cnt = o_idx.cpu().numpy().view(np.uint32), o_sc.cpu().numpy(), o_cnt.cpu().numpy().astype(np.int64)
    assert (cnt <= idx.shape[1]).all()
    mask = np.arange(idx.shape[1])[None, :] < cnt[:, None]
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), idx[mask], sc[mask]


@pytest.mark.parametrize("mode, thr, topk, name", SETTINGS, ids=[s[3] for s in SETTINGS])
def test_modes_equal_the_reference(dev_case, mode, thr, topk, name):
    from pecos_amd.features import ensemble_device
    c, t = dev_case
    out = ensemble_device(t, mode=mode, threshold=thr, only_topk=topk)
    total = sum(i.shape[1] for i in c.idx)
    assert out[0].shape == (c.rows, min(total, topk) if topk else total)
    same_rows(_rows(*out), c.expected(name), f"case {c.name} {name}")


def _raw(c, t, mode, thr, topk, out_stride, stream=None, sync=True, sentinel=0x5A5A5A5A):
    import torch
    from pecos_amd import clib
    o_idx = torch.full((c.rows, out_stride), sentinel, dtype=torch.int32, device="cuda")
    o_sc = torch.full((c.rows, out_stride), -7.0, dtype=torch.float32, device="cuda")
    o_cnt = torch.full((c.rows,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    clib.ensemble_device(0, c.rows, [x[0].data_ptr() for x in t], [x[1].data_ptr() for x in t], [x[2].data_ptr() for x in t],
                         [x[0].shape[1] for x in t], mode, thr, topk, o_idx.data_ptr(), o_sc.data_ptr(), o_cnt.data_ptr(), out_stride,
                         stream=stream, sync=sync)
    return o_idx, o_sc, o_cnt


def test_wider_output_and_input_strides(dev_case):
    import torch
    c, t = dev_case
    total = sum(i.shape[1] for i in c.idx)
    # out_stride larger than needed: same rows, and nothing is written beyond a row's count
    for mode, thr, topk, name in (SETTINGS[0], SETTINGS[3], SETTINGS[1]):
        o = _raw(c, t, mode, thr, topk, total + 5)
        same_rows(_rows(*o), c.expected(name), f"case {c.name} {name}, out_stride + 5")
        cnt = o[2].cpu().numpy()
        tail = np.arange(total + 5)[None, :] >= cnt[:, None]
        assert (o[0].cpu().numpy()[tail] == 0x5A5A5A5A).all() and (o[1].cpu().numpy()[tail] == -7.0).all()
    # input strides larger than the rows (filler behind every row), and counts above the stride where a row is full (read as the stride)
    over = [(i, v, torch.where(n == i.shape[1], n + 4000, n)) for i, v, n in t]
    for pad in (7, 60):                                                  # (+ 60: cases a-c move to 4, 4 and 8 entries per lane)
        if total + pad * c.n_models > 1024:
            continue
        wide = []
        for i, v, n in t:
            wi = torch.full((c.rows, i.shape[1] + pad), 424242, dtype=torch.int32, device="cuda"); wi[:, : i.shape[1]] = i
            wv = torch.full((c.rows, i.shape[1] + pad), 3.5, dtype=torch.float32, device="cuda"); wv[:, : i.shape[1]] = v
            wide.append((wi, wv, n))
        for mode, thr, topk, name in (SETTINGS[0], SETTINGS[1], SETTINGS[3]):
            o = _raw(c, wide, mode, thr, topk, total + pad * c.n_models)
            same_rows(_rows(*o), c.expected(name), f"case {c.name} {name}, input stride + {pad}")
    for mode, thr, topk, name in (SETTINGS[0], SETTINGS[1]):            # (rank_average: mm is the largest CLAMPED length)
        o = _raw(c, over, mode, thr, topk, total)
        same_rows(_rows(*o), c.expected(name), f"case {c.name} {name}, counts above the stride")


def test_on_a_side_stream_without_sync(dev_case):
    import torch
    c, t = dev_case
    total = sum(i.shape[1] for i in c.idx)
    s = torch.cuda.Stream()
    for mode, thr, topk, name in (SETTINGS[0], SETTINGS[1], SETTINGS[3]):
        o = _raw(c, t, mode, thr, topk, min(total, topk) if topk else total, stream=s.cuda_stream, sync=False)
        s.synchronize()
        same_rows(_rows(*o), c.expected(name), f"case {c.name} {name}, side stream")


def test_no_rows():
    import torch
    from pecos_amd.features import ensemble_device
    e = [(torch.zeros((0, 5), dtype=torch.int32, device="cuda"), torch.zeros((0, 5), dtype=torch.float32, device="cuda"),
          torch.zeros((0,), dtype=torch.int32, device="cuda")) for _ in range(2)]
    o = ensemble_device(e, mode="finish", threshold=0.1, only_topk=3)
    assert o[0].shape == (0, 3) and o[2].shape == (0,)


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def text_models(tmp_path_factory):
    import xrl_synth
    from pecos_amd import XLinearModel as XLM
    from pecos_amd.features import Tfidf
    from test_tfidf import _case
    folder, corpus, X = _case("word_bigram_trunc")
    D, H = X.shape[1], 16
    root = tmp_path_factory.mktemp("ens")
    plain, concat = [], []
    for i, seed in enumerate((81, 82, 83)):
        xrl_synth.make_model(str(root / f"p{i}"), D, 600, [120, 60, 20], seed=seed, shape=[6, 48, 600])
        xrl_synth.make_model(str(root / f"c{i}"), D + H, 600, [120, 60, 20], seed=seed + 10, shape=[6, 48, 600])
        plain.append(XLM.load(str(root / f"p{i}"))); concat.append(XLM.load(str(root / f"c{i}")))
    return Tfidf.load(folder), corpus, plain, concat, H


def _same_csr(a, b, what):
    assert a.shape == b.shape, what
    same_rows((a.indptr, a.indices, a.data), (b.indptr, b.indices, b.data), what)


def test_predict_text_device_equals_host(text_models):
    import torch
    from pecos_amd.features import predict_text
    vec, corpus, plain, concat, H = text_models
    for kw in (dict(beam_size=5, only_topk=7), dict(beam_size=10, only_topk=3, post_processor="log-l2-hinge")):
        dev = predict_text(vec, plain, corpus, ensemble="device", **kw)
        _same_csr(dev, predict_text(vec, plain, corpus, ensemble="host", **kw), f"device vs host {kw}")
        _same_csr(predict_text(vec, plain, corpus, **kw), dev, f"auto {kw}")
        assert dev.nnz > len(corpus)
    emb = torch.from_numpy(np.random.default_rng(5).standard_normal((len(corpus), H)).astype(np.float32)).cuda()
    for norm in (True, False):
        kw = dict(X_emb=emb, normalize_emb=norm, beam_size=6, only_topk=6)
        _same_csr(predict_text(vec, concat, corpus, ensemble="device", **kw), predict_text(vec, concat, corpus, ensemble="host", **kw),
                  f"X_emb, normalize_emb={norm}")
    _same_csr(predict_text(vec, plain[:2], corpus, ensemble="device", finish=(0.2, 4), beam_size=5, only_topk=7),
              predict_text(vec, plain[:2], corpus, ensemble="host", finish=(0.2, 4), beam_size=5, only_topk=7), "finish through predict_text")


def test_text2text_predict_equals_finish_of_the_single_predictions(text_models):
    from pecos_amd.features import Text2Text, predict_text
    vec, corpus, plain, _, _ = text_models
    t2t = Text2Text(vec, [(m, {}) for m in plain], [f"item {i}" for i in range(600)])
    for thr, k in ((None, 6), (0.2, 4), (0.0, 1), (-1.0, 3), (0.05, None)):
        kw = dict(beam_size=8) if k is None else dict(beam_size=8, only_topk=k)
        got = t2t.predict(corpus, threshold=thr, **kw)
        singles = [predict_text(vec, m, corpus, **kw) for m in plain]
        _same_csr(got, Text2Text.finish(singles, threshold=thr, only_topk=k), f"threshold {thr}, only_topk {k}")


def test_beyond_capacity_device_raises_and_auto_takes_the_host_path(text_models):
    from pecos_amd.features import predict_text
    vec, corpus, plain, _, _ = text_models
    kw = dict(beam_size=20, only_topk=400)                               # 3 x 400 entries per row > 1024
    with pytest.raises(ValueError, match="more than 1024"):
        predict_text(vec, plain, corpus[:8], ensemble="device", **kw)
    _same_csr(predict_text(vec, plain, corpus[:8], ensemble="auto", **kw), predict_text(vec, plain, corpus[:8], ensemble="host", **kw), "auto beyond capacity")


def test_one_tokenisation_for_three_models(text_models, monkeypatch):
    from pecos_amd.features import Tfidf, predict_text
    vec, corpus, plain, _, _ = text_models
    calls = []
    real = Tfidf.predict_device
    monkeypatch.setattr(Tfidf, "predict_device", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    predict_text(vec, plain, corpus, beam_size=5, only_topk=7)
    assert len(calls) == 1
    predict_text(vec, plain, corpus, ensemble="host", beam_size=5, only_topk=7)
    assert len(calls) == 1 + 3
