"""xrl_run_clustering_dense_device refuses what it can before a GPU is required: the device pointers are fake and never dereferenced."""
import ctypes

import pytest

import clustering_rule as cr

FAKE = 4096
#           d_val, d_codes, cols, row_stride, depth, param
CASES = {
    "null_d_val": (None, FAKE, 8, 8, 2, {}),
    "null_d_codes": (FAKE, None, 8, 8, 2, {}),
    "row_stride_below_cols": (FAKE, FAKE, 8, 7, 2, {}),
    "depth_above_rows": (FAKE, FAKE, 8, 8, 7, {}),
    "depth_31": (FAKE, FAKE, 8, 8, 31, {}),
    "invalid_rate": (FAKE, FAKE, 8, 8, 2, dict(min_rate=0.0)),
    "partition_algo_3": (FAKE, FAKE, 8, 8, 2, dict(algo=3)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_resident_form_refuses_before_a_gpu(name):
    d_val, d_codes, cols, stride, depth, kw = CASES[name]
    lib = cr.load(cr.OURS)
    fn = lib.xrl_run_clustering_dense_device
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p]
    param = cr.make_param(**kw)
    assert fn(0, 100, cols, d_val, stride, depth, ctypes.byref(param), d_codes, None, None) == -1
    assert cr.last_error(lib).startswith("xrl_run_clustering_dense_device: "), cr.last_error(lib)
