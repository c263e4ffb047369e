"""The ensemble methods (xrl_ensemble_methods_device) on the GPU: round_robin and the cuts of average / rank_average / round_robin
against the reference's recorded outputs (tests/golden/ensemble_methods) bit for bit; sigmoid_average and softmax_average against the
restatement of the rules (ensemble_methods_rule.py) within the bound derived there for exponentials one fp32 ulp apart; output / input
layouts; a caller's stream; ensemble_prediction_device; predict_text and metrics_device on a round_robin result."""
import numpy as np
import pytest

from ensemble_cases import over_counts, padded, raw_call, rows_of as _rows, same_rows, text_models, untouched_tail, upload as _upload  # noqa: F401
from ensemble_methods_rule import CASES, CUT_METHODS, TOPKS, MCase, close_rows, restate, value_bound

pytestmark = pytest.mark.gpu

DEVICE_EXP_ULP = 1       # the device's fp64 exp and libm's differ by at most one fp32 ulp after rounding (ensemble_methods_rule.py)


@pytest.fixture(scope="module", params=CASES)
def dev_case(request):
    c, full = MCase(request.param), MCase(request.param + "_full")
    return c, _upload(c), full, _upload(full)


_restated = {}


def _restate(c, method, k=0):
    """The restatement of a case, computed once for all the tests that need it."""
    key = (c.name, method, k)
    if key not in _restated:
        _restated[key] = restate(c.idx, c.val, c.cnt, method, k)
    return _restated[key]


def test_round_robin_and_the_cuts_equal_the_reference(dev_case):
    from pecos_amd.features import ensemble_device
    c, t, _, _ = dev_case
    total = sum(i.shape[1] for i in c.idx)
    out = ensemble_device(t, mode="round_robin")
    assert out[0].shape == (c.rows, total)
    same_rows(_rows(*out), c.expected("round_robin"), f"case {c.name} round_robin")
    for method in CUT_METHODS:
        for k in TOPKS:
            out = ensemble_device(t, mode=method, only_topk=k)
            assert out[0].shape == (c.rows, min(total, k))
            same_rows(_rows(*out), c.expected(f"{method}_top{k}"), f"case {c.name} {method} only_topk={k}")


def test_sigmoid_and_softmax_are_within_the_bound_of_the_restatement(dev_case):
    from pecos_amd.features import ensemble_device
    c, t, full, tf = dev_case
    before = [x[1].clone() for x in t]
    for what, case, dev, method in (("sigmoid", c, t, "sigmoid_average"), ("softmax", full, tf, "softmax_average"),
                                    ("softmax with empty segments", c, t, "softmax_average")):
        got = _rows(*ensemble_device(dev, mode=method))
        close_rows(got, _restate(case, method), value_bound(method, case.n_models, DEVICE_EXP_ULP), f"case {case.name} {what}")
    for x, b in zip(t, before):                                          # the device reads its inputs only
        assert np.array_equal(x[1].cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    # the cut of a transformed merge: the restatement's order and length, values within the same bound
    got = _rows(*ensemble_device(t, mode="sigmoid_average", only_topk=3))
    close_rows(got, _restate(c, "sigmoid_average", 3), value_bound("sigmoid_average", c.n_models, DEVICE_EXP_ULP), f"case {c.name} sigmoid top 3")


def _raw(c, t, method, topk, out_stride, stream=None, sync=True):
    return raw_call("ensemble_methods_device", c, t, (method, topk), out_stride, stream, sync)


def _check(c, o, method, topk, what):
    if method in ("sigmoid_average", "softmax_average"):
        close_rows(_rows(*o), _restate(c, method, topk), value_bound(method, c.n_models, DEVICE_EXP_ULP), what)
    else:
        same_rows(_rows(*o), c.expected(f"{method}_top{topk}" if topk else method), what)


SETTINGS = (("round_robin", 0), ("round_robin", 3), ("rank_average", 3), ("average", 100), ("sigmoid_average", 0), ("softmax_average", 0))


def test_wider_output_and_input_strides(dev_case):
    c, t, _, _ = dev_case
    total = sum(i.shape[1] for i in c.idx)
    # out_stride larger than needed: same rows, and nothing is written beyond a row's count
    for method, topk in SETTINGS:
        o = _raw(c, t, method, topk, total + 5)
        _check(c, o, method, topk, f"case {c.name} {method} top {topk}, out_stride + 5")
        assert untouched_tail(o)
    # input strides larger than the rows (filler behind every row), and counts above the stride where a row is full (read as the stride)
    for pad in (7, 60):                                                  # (+ 60: cases a-c move to 4, 4 and 8 entries per lane)
        if total + pad * c.n_models > 1024:
            continue
        wide = padded(c, t, pad)
        for method, topk in SETTINGS:
            o = _raw(c, wide, method, topk, total + pad * c.n_models)
            _check(c, o, method, topk, f"case {c.name} {method} top {topk}, input stride + {pad}")
    over = over_counts(t)
    for method, topk in SETTINGS[:3]:                                    # (mm is the largest CLAMPED length)
        o = _raw(c, over, method, topk, total)
        _check(c, o, method, topk, f"case {c.name} {method} top {topk}, counts above the stride")


def test_on_a_side_stream_without_sync(dev_case):
    import torch
    c, t, _, _ = dev_case
    total = sum(i.shape[1] for i in c.idx)
    s = torch.cuda.Stream()
    for method, topk in SETTINGS:
        o = _raw(c, t, method, topk, min(total, topk) if topk else total, stream=s.cuda_stream, sync=False)
        s.synchronize()
        _check(c, o, method, topk, f"case {c.name} {method} top {topk}, side stream")


def test_no_rows():
    import torch
    from pecos_amd.features import ensemble_device
    e = [(torch.zeros((0, 5), dtype=torch.int32, device="cuda"), torch.zeros((0, 5), dtype=torch.float32, device="cuda"),
          torch.zeros((0,), dtype=torch.int32, device="cuda")) for _ in range(2)]
    for mode, k, width in (("round_robin", 3, 3), ("softmax_average", None, 10), ("rank_average", 4, 4)):
        o = ensemble_device(e, mode=mode, only_topk=k)
        assert o[0].shape == (0, width) and o[2].shape == (0,)


def test_ensemble_prediction_device():
    from pecos_amd.features import ensemble_prediction_device
    c = MCase("a")                                                       # two models: model 0 plays the transformer, model 1 the concat model
    t = _upload(c)
    for k in TOPKS:
        for method in CUT_METHODS:
            same_rows(_rows(*ensemble_prediction_device(t[0], t[1], k, method)), c.expected(f"{method}_top{k}"), f"{method} only_topk={k}")
        for method, m in (("transformer-only", 0), ("concat-only", 1)):
            want = restate(c.idx[m:m + 1], c.val[m:m + 1], c.cnt[m:m + 1], "average", k)
            same_rows(_rows(*ensemble_prediction_device(t[0], t[1], k, method)), want, f"{method} only_topk={k}")
    with pytest.raises(ValueError, match="Unknown ensemble method sigmoid_average"):
        ensemble_prediction_device(t[0], t[1], 3, "sigmoid_average")


def test_metrics_of_a_round_robin_result():
    # the whole print_ens comparison in HBM: metrics_device on the device's round_robin equals the host sums of the reference's recorded rows
    import metrics_cases as mc
    from pecos_amd import metrics_sums_device
    from pecos_amd.features import ensemble_device
    import torch
    c = MCase("a")
    out = ensemble_device(_upload(c), mode="round_robin")
    ip, ix, dv = c.expected("round_robin")
    n = np.diff(ip)
    stride = out[0].shape[1]
    idx = np.zeros((c.rows, stride), np.uint32); val = np.zeros((c.rows, stride), np.float32)
    mask = np.arange(stride)[None, :] < n[:, None]
    idx[mask], val[mask] = ix, dv
    rng = np.random.default_rng(8)
    true = [np.unique(rng.integers(0, c.n_cols, size=int(rng.integers(0, 6)))) for _ in range(c.rows)]
    tptr = np.concatenate([[0], np.cumsum([len(x) for x in true])]).astype(np.uint64)
    ref = dict(idx=idx, val=val, cnt=n.astype(np.uint32), tptr=tptr, tidx=np.concatenate(true).astype(np.uint32), topk=10, n_cols=c.n_cols)
    pair = (torch.from_numpy(tptr.astype(np.int64)).cuda(), torch.from_numpy(ref["tidx"].view(np.int32)).cuda())
    m, s = metrics_sums_device(out, pair, topk=10)
    want = mc.metric_sums(ref)
    assert want[0][-1] > 0
    assert np.array_equal(m.cpu().numpy().view(np.uint64), want[0])
    assert np.array_equal(s.cpu().numpy().view(np.uint64), want[1].view(np.uint64))


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_predict_text_round_robin_device_equals_host(text_models):
    from pecos_amd.features import predict_text
    vec, corpus, plain, _, _ = text_models
    kw = dict(beam_size=5, only_topk=7, ensemble_method="round_robin")
    dev = predict_text(vec, plain, corpus, ensemble="device", **kw)
    host = predict_text(vec, plain, corpus, ensemble="host", **kw)
    assert dev.shape == host.shape and dev.nnz > len(corpus) and dev.dtype == np.float32 and host.dtype == np.float32
    same_rows((dev.indptr, dev.indices, dev.data), (host.indptr, host.indices, host.data), "round_robin, device vs host")
    avg = predict_text(vec, plain, corpus, ensemble="device", beam_size=5, only_topk=7)
    assert not np.array_equal(avg.data, dev.data)                       # (the default is still the average)
