"""The ensemble methods (xrl_ensemble_methods_device) without a GPU: the restatement of its rules (ensemble_methods_rule.py) against
the reference's recorded outputs, the host implementation behind predict_text's fallback against the restatement, the entry point's
export, binding and argument checks (all made before a GPU is required).  The kernel's resources: test_ensemble_cpu.py."""
import ctypes

import numpy as np
import pytest

from ensemble_cases import compact_labels, fixed_to_csr, same_rows
from ensemble_methods_rule import (CASES, CUT_METHODS, METHODS, TOPKS, MCase, close_rows, longest_segment_per_entry, restate, value_bound)


@pytest.fixture(scope="module", params=CASES)
def case(request):
    return MCase(request.param), MCase(request.param + "_full")


def test_restatement_equals_the_reference_bit_for_bit(case):
    c, _ = case
    same_rows(restate(c.idx, c.val, c.cnt, "round_robin"), c.expected("round_robin"), f"{c.name} round_robin")
    for method in CUT_METHODS:
        for k in TOPKS:
            same_rows(restate(c.idx, c.val, c.cnt, method, k), c.expected(f"{method}_top{k}"), f"{c.name} {method} only_topk={k}")


def test_restatement_is_within_the_bound_of_the_reference(case):
    c, full = case
    want = c.expected("sigmoid_average")
    close_rows(restate(c.idx, c.val, c.cnt, "sigmoid_average"), want, value_bound("sigmoid_average", c.n_models, c.exp_ulp),
               f"{c.name} sigmoid_average")
    want = full.expected("softmax_average")
    n = longest_segment_per_entry(want[0], full.idx, full.cnt)           # numpy adds the n terms of a denominator in fp32, in its own order
    close_rows(restate(full.idx, full.val, full.cnt, "softmax_average"), want, value_bound("softmax_average", full.n_models, full.exp_ulp, n),
               f"{full.name} softmax_average")


def test_fixtures_hold_what_the_tests_rely_on():
    tot = lambda k: set(sum(np.minimum(n, i.shape[1]).astype(np.int64) for n, i in zip(k.cnt, k.idx)).tolist())      # noqa: E731
    b, c, d = MCase("b"), MCase("c"), MCase("d")
    assert {62, 63, 64} <= tot(b) and {127, 128, 129, 130} <= tot(c) and 1024 in tot(d) and 0 in tot(d)
    assert (d.expected("round_robin")[1] == 0xFFFFFFFE).any() and (d.expected("round_robin")[1] == 0).any()
    for name in CASES:
        full = MCase(name + "_full")
        assert all((n > 0).all() for n in full.cnt), "an empty segment in a softmax fixture"
        assert np.isnan(full.expected("softmax_average")[2]).any()       # a segment with +inf, or all -inf
        plain = MCase(name)
        assert any((n == 0).any() for n in plain.cnt) and 0 <= plain.exp_ulp <= 4
    # equal quotients of different sums: average's own order (by sum) and its cut (by value, then label) differ somewhere in case b
    ip, ix, _ = restate(b.idx, b.val, b.cnt, "average")
    jp, jx, _ = b.expected("average_top100")
    assert np.array_equal(ip, jp) and not np.array_equal(ix, jx)


def test_host_implementation_equals_the_restatement(case):
    # features.ensemble_host serves predict_text where the device merge does not; the plain fixtures have empty segments (softmax too)
    from pecos_amd.features import ensemble_host
    c, _ = case
    idx, table, n_cols = c.idx, None, c.n_cols
    if n_cols > 1 << 31:
        idx, table = compact_labels(c.idx, c.cnt)
        n_cols = len(table)
    csrs = [fixed_to_csr(i, v, n, n_cols) for i, v, n in zip(idx, c.val, c.cnt)]
    before = [(m.indices.copy(), m.data.copy()) for m in csrs]
    back = (lambda ix: ix.astype(np.uint32)) if table is None else (lambda ix: table[ix].astype(np.uint32))
    for method, k in [(m, None) for m in METHODS] + [(m, 3) for m in METHODS]:
        Y = ensemble_host(csrs, method, only_topk=k)
        same_rows((Y.indptr.astype(np.int64), back(Y.indices), Y.data.astype(np.float32)), restate(c.idx, c.val, c.cnt, method, k or 0),
                  f"{c.name} {method} only_topk={k}")
    for m, (ix, dv) in zip(csrs, before):                                # the inputs are only read
        assert np.array_equal(m.indices, ix) and np.array_equal(m.data.view(np.uint32), dv.view(np.uint32))
    with pytest.raises(ValueError, match="expected one of"):
        ensemble_host(csrs, "median")


def test_entry_point_is_exported_and_bound():
    from pecos_amd import clib, features
    fn = clib.clib_float32.xrl_ensemble_methods_device
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    assert callable(clib.ensemble_methods_device)
    assert clib.ENSEMBLE_METHODS == {"average": 0, "finish": 1, "rank_average": 2, "sigmoid_average": 3, "softmax_average": 4, "round_robin": 5}
    assert clib.ENSEMBLE_MODES == {"average": 0, "finish": 1, "rank_average": 2}
    assert callable(features.ensemble_prediction_device) and set(features.ENSEMBLE_METHOD_NAMES) == set(METHODS)


def _call(n_models=2, rows=1, idx=True, val=True, cnt=True, strides=(10, 10), method=5, only_topk=0, out=(True, True, True), out_stride=20,
          null_entry=None):
    """xrl_ensemble_methods_device on made-up, never dereferenced addresses: every check under test comes before the first use of the GPU."""
    from pecos_amd import clib
    lib = clib.clib_float32
    n = len(strides) if strides is not None else 2

    def tab(given, which):
        if not given:
            return None
        return (ctypes.c_void_p * n)(*[None if null_entry == (which, m) else 0x1000 * (m + 1) for m in range(n)])
    st = (ctypes.c_uint32 * n)(*strides) if strides is not None else None
    o = [ctypes.c_void_p(0x9000 if g else 0) for g in out]
    rc = lib.xrl_ensemble_methods_device(0, n_models, rows, tab(idx, 0), tab(val, 1), tab(cnt, 2), st, method, only_topk, o[0], o[1], o[2],
                                         out_stride, None, 1)
    err = lib.xrl_last_error()
    lib.xrl_clear_error()
    return rc, (err or b"").decode()


@pytest.mark.parametrize("kw, message", [
    (dict(idx=False), "null argument"), (dict(val=False), "null argument"), (dict(cnt=False), "null argument"), (dict(strides=None), "null argument"),
    (dict(out=(False, True, True)), "null argument"), (dict(out=(True, False, True)), "null argument"), (dict(out=(True, True, False)), "null argument"),
    (dict(null_entry=(0, 1)), "null device pointer for model 1"), (dict(null_entry=(2, 0)), "null device pointer for model 0"),
    (dict(n_models=0), "n_models must be 1..8, got 0"), (dict(n_models=9, strides=(1,) * 9), "n_models must be 1..8, got 9"),
    (dict(strides=(512, 513), out_stride=2000), "sum to 1025, more than 1024"),
    (dict(n_models=3, strides=(0xFFFFFFFF, 0xFFFFFFFF, 3), out_stride=0xFFFFFFFF), "more than 1024"),      # (no 32-bit wrap-around of the sum)
    (dict(out_stride=19), "out_stride 19 smaller than the longest possible row, 20"),
    (dict(method=3, out_stride=19), "out_stride 19 smaller than the longest possible row, 20"),
    (dict(method=0, only_topk=5, out_stride=4), "out_stride 4 smaller than the longest possible row, 5"),
    (dict(method=4, only_topk=50, out_stride=19), "out_stride 19 smaller than the longest possible row, 20"),
    (dict(method=1), "method 1 (finish) is served by xrl_ensemble_device"),
    (dict(method=-1), "unknown method -1"), (dict(method=6), "unknown method 6"),
])
def test_argument_errors_come_before_the_gpu(kw, message):
    rc, err = _call(**kw)
    assert rc == -1 and err.startswith("xrl_ensemble_methods_device: ") and message in err, (rc, err)


def test_valid_arguments_without_rows_or_without_a_gpu():
    from pecos_amd import clib
    for method in (0, 2, 3, 4, 5):
        assert _call(rows=0, method=method) == (0, "")                   # a successful no-op, GPU or not
    assert _call(rows=0, method=5, only_topk=3, out_stride=3) == (0, "")
    if clib.device_count() == 0:                                         # the checks passed: what is missing is the device
        rc, err = _call()
        assert rc == -1 and "no HIP device visible" in err, err


def test_python_argument_errors():
    from pecos_amd.features import ensemble_device, ensemble_prediction_device, predict_text
    with pytest.raises(ValueError, match="expected one of"):
        ensemble_device([], mode="median")
    with pytest.raises(ValueError, match="expected one of"):
        predict_text(None, [object(), object()], ["x"], ensemble_method="median")
    with pytest.raises(ValueError, match="goes with 'average' only"):
        predict_text(None, [object(), object()], ["x"], ensemble_method="round_robin", finish=(0.1, 3))
    t = (np.zeros((2, 3), np.int32), np.zeros((2, 3), np.float32), np.zeros(2, np.int32))
    with pytest.raises(ValueError, match="Unknown ensemble method softmax_average"):
        ensemble_prediction_device(t, t, 3, "softmax_average")
    with pytest.raises(ValueError, match="Transformer/concat prediction mismatch"):
        ensemble_prediction_device(t, (t[0][:1], t[1][:1], t[2][:1]), 3, "average")
