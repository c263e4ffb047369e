"""The device ensemble (K6, xrl_ensemble_device) on the GPU: every fixture case (tests/golden/ensemble, the reference's recorded outputs) in
all three modes and every `finish` setting, bit for bit; output / input layouts; a caller's stream; and predict_text / Text2Text.predict end to
end against the host path."""
import numpy as np
import pytest

from ensemble_cases import CASES, FINISH, Case, over_counts, padded, raw_call, rows_of as _rows, same_rows, text_models, untouched_tail, upload  # noqa: F401

pytestmark = pytest.mark.gpu

SETTINGS = [("average", None, None, "average"), ("rank_average", None, None, "rank_average")] + \
           [("finish", thr, topk, f"finish{i}") for i, (thr, topk) in enumerate(FINISH)]


@pytest.fixture(scope="module", params=CASES)
def dev_case(request):
    c = Case(request.param)
    return c, upload(c)


@pytest.mark.parametrize("mode, thr, topk, name", SETTINGS, ids=[s[3] for s in SETTINGS])
def test_modes_equal_the_reference(dev_case, mode, thr, topk, name):
    from pecos_amd.features import ensemble_device
    c, t = dev_case
    out = ensemble_device(t, mode=mode, threshold=thr, only_topk=topk)
    total = sum(i.shape[1] for i in c.idx)
    assert out[0].shape == (c.rows, min(total, topk) if topk else total)
    same_rows(_rows(*out), c.expected(name), f"case {c.name} {name}")


def _raw(c, t, mode, thr, topk, out_stride, stream=None, sync=True):
    return raw_call("ensemble_device", c, t, (mode, thr, topk), out_stride, stream, sync)


def test_wider_output_and_input_strides(dev_case):
    c, t = dev_case
    total = sum(i.shape[1] for i in c.idx)
    # out_stride larger than needed: same rows, and nothing is written beyond a row's count
    for mode, thr, topk, name in (SETTINGS[0], SETTINGS[3], SETTINGS[1]):
        o = _raw(c, t, mode, thr, topk, total + 5)
        same_rows(_rows(*o), c.expected(name), f"case {c.name} {name}, out_stride + 5")
        assert untouched_tail(o)
    # input strides larger than the rows (filler behind every row), and counts above the stride where a row is full (read as the stride)
    for pad in (7, 60):                                                  # (+ 60: cases a-c move to 4, 4 and 8 entries per lane)
        if total + pad * c.n_models > 1024:
            continue
        wide = padded(c, t, pad)
        for mode, thr, topk, name in (SETTINGS[0], SETTINGS[1], SETTINGS[3]):
            o = _raw(c, wide, mode, thr, topk, total + pad * c.n_models)
            same_rows(_rows(*o), c.expected(name), f"case {c.name} {name}, input stride + {pad}")
    over = over_counts(t)
    for mode, thr, topk, name in (SETTINGS[0], SETTINGS[1]):            # (rank_average: mm is the largest CLAMPED length)
        o = _raw(c, over, mode, thr, topk, total)
        same_rows(_rows(*o), c.expected(name), f"case {c.name} {name}, counts above the stride")


def test_the_methods_entry_equals_the_recorded_modes(dev_case):
    # one kernel behind both entry points: xrl_ensemble_methods_device's average / rank_average, uncut and cut, are xrl_ensemble_device's
    # average / rank_average / finish without a threshold, on every entries-per-lane count (1, 4, 16 as recorded; 2 and 8 padded)
    c, t = dev_case
    total = sum(i.shape[1] for i in c.idx)
    runs = [(t, total, "")] + [(padded(c, t, pad), total + pad * c.n_models, f", input stride + {pad}")
                               for name, pad in (("b", 7), ("c", 60)) if c.name == name]
    for tt, stride, what in runs:
        for method, k, name in (("average", 0, "average"), ("rank_average", 0, "rank_average"), ("average", 100, "finish3"),
                                ("average", total, "finish0")):
            o = raw_call("ensemble_methods_device", c, tt, (method, k), stride)
            same_rows(_rows(*o), c.expected(name), f"case {c.name} methods entry {method} only_topk={k} vs {name}{what}")


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
