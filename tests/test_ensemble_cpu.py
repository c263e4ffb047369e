"""The device ensemble (K6, xrl_ensemble_device) without a GPU: the fixtures pinned on today's host code, the entry point's export and
binding, its argument checks (all made before a GPU is required), and the compiled kernels' resources."""
import ctypes
import re

import numpy as np
import pytest

from ensemble_cases import CASES, FINISH, Case, same_rows


@pytest.fixture(scope="module", params=CASES)
def case(request):
    return Case(request.param)


def test_fixtures_equal_the_host_path(case):
    # the recorded outputs are the reference's; the host mirrors (features.ensemble_average / Text2Text.finish) must give the same bits
    from pecos_amd.features import Text2Text, ensemble_average
    csrs, table = case.host_inputs()
    back = (lambda ix: ix.astype(np.uint32)) if table is None else (lambda ix: table[ix].astype(np.uint32))
    avg = ensemble_average(csrs) if len(csrs) > 1 else Text2Text.finish(csrs)          # (one model: 0 + A, sorted, / 1)
    same_rows((avg.indptr, back(avg.indices), avg.data), case.expected("average"), f"{case.name} average")
    for i, (thr, topk) in enumerate(FINISH):
        Y = Text2Text.finish(csrs, threshold=thr, only_topk=topk)
        same_rows((Y.indptr, back(Y.indices), Y.data), case.expected(f"finish{i}"), f"{case.name} finish{FINISH[i]}")


def test_fixtures_hold_what_the_gpu_tests_rely_on():
    b, c, d = Case("b"), Case("c"), Case("d")
    tot = lambda k: set(sum(np.minimum(n, i.shape[1]).astype(np.int64) for n, i in zip(k.cnt, k.idx)).tolist())      # noqa: E731
    assert {62, 63, 64} <= tot(b) and {127, 128, 129, 130} <= tot(c) and 1024 in tot(d) and 0 in tot(d)
    assert (d.expected("average")[1] == 0xFFFFFFFE).any() and (d.expected("average")[1] == 0).any()
    assert np.isnan(Case("a").expected("average")[2]).any()
    e = Case("e").expected("average")[2]
    assert (e.view(np.uint32) == 0x80000000).any()                   # one model: -0.0 survives


def test_entry_point_is_exported_and_bound():
    from pecos_amd import clib
    fn = clib.clib_float32.xrl_ensemble_device
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 16
    assert callable(clib.ensemble_device) and clib.ENSEMBLE_MODES == {"average": 0, "finish": 1, "rank_average": 2}
    from pecos_amd import features
    assert callable(features.ensemble_device)


def _call(n_models=2, rows=1, idx=True, val=True, cnt=True, strides=(10, 10), mode=0, threshold=None, only_topk=0, out=(True, True, True),
          out_stride=20, null_entry=None):
    """xrl_ensemble_device on made-up, never dereferenced addresses: every check under test comes before the first use of the GPU."""
    from pecos_amd import clib
    lib = clib.clib_float32
    n = len(strides) if strides is not None else 2

    def tab(given, which):
        if not given:
            return None
        return (ctypes.c_void_p * n)(*[None if null_entry == (which, m) else 0x1000 * (m + 1) for m in range(n)])
    st = (ctypes.c_uint32 * n)(*strides) if strides is not None else None
    thr = None if threshold is None else ctypes.byref(ctypes.c_float(threshold))
    o = [ctypes.c_void_p(0x9000 if g else 0) for g in out]
    rc = lib.xrl_ensemble_device(0, n_models, rows, tab(idx, 0), tab(val, 1), tab(cnt, 2), st, mode, thr, only_topk, o[0], o[1], o[2], out_stride, None, 1)
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
    (dict(mode=2, out_stride=19), "out_stride 19 smaller than the longest possible row, 20"),
    (dict(mode=1, only_topk=5, out_stride=4), "out_stride 4 smaller than the longest possible row, 5"),
    (dict(mode=1, only_topk=50, out_stride=19), "out_stride 19 smaller than the longest possible row, 20"),
    (dict(mode=3), "unknown mode 3"), (dict(mode=-1), "unknown mode -1"),
    (dict(mode=0, threshold=0.5), "belong to mode finish"), (dict(mode=2, only_topk=3), "belong to mode finish"),
])
def test_argument_errors_come_before_the_gpu(kw, message):
    rc, err = _call(**kw)
    assert rc == -1 and err.startswith("xrl_ensemble_device: ") and message in err, (rc, err)


def test_valid_arguments_without_rows_or_without_a_gpu():
    from pecos_amd import clib
    assert _call(rows=0) == (0, "")                                     # a successful no-op, GPU or not
    assert _call(rows=0, mode=1, threshold=0.1, only_topk=3, out_stride=3) == (0, "")
    if clib.device_count() == 0:                                         # the checks passed: what is missing is the device
        rc, err = _call()
        assert rc == -1 and "no HIP device visible" in err, err


def test_predict_text_rejects_an_unknown_ensemble_value():
    # (the routing itself needs model handles, i.e. a GPU: tests/test_gpu_ensemble.py)
    from pecos_amd.features import predict_text
    with pytest.raises(ValueError, match="expected 'auto', 'device' or 'host'"):
        predict_text(None, [object(), object()], ["x"], ensemble="gpu")


def test_k6_resources(tmp_path):
    # every instantiation of the one kernel: no scratch, no spills to memory, wavefront-private LDS of at most 8 KB per wavefront (4 wavefronts per workgroup)
    from test_kernel_resources import demangle, kernel_notes
    notes = kernel_notes(tmp_path)
    nice = demangle(sorted(notes))
    seen = set()
    for k, d in notes.items():
        got = re.search(r"ensemble_kernel<(\d+), (\d+)>", nice[k])
        if not got:
            continue
        ns, method = int(got.group(1)), int(got.group(2))
        seen.add((ns, method))
        assert d["scratch"] == 0 and d["vgpr_spill"] == 0, (nice[k], d)      # (the 16-entry instantiations park some SGPRs in VGPR lanes: no memory)
        assert d["lds"] == ns * 64 * 8 * 4 and d["lds"] <= 8192 * 4, (nice[k], d)
    assert seen == {(ns, m) for ns in (1, 2, 4, 8, 16) for m in (0, 2, 3, 4, 5)}, sorted(seen)    # (finish, 1, runs in average's)
    assert not [k for k in notes if "ensemble_methods_kernel" in nice[k]]
    mm = [v for k, v in notes.items() if "ensemble_max_len_kernel" in nice[k]]
    assert len(mm) == 1 and mm[0]["scratch"] == 0
