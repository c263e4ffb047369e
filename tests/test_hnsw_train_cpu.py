"""HNSW graph construction (K19) without a GPU: the host's level plan against the recordings under tests/golden/hnsw/, every refusal that
is made before a GPU is required, and the Python surface (pecos_amd.hnsw.HNSW beside the unchanged refusals of pecos_amd.ann.HNSW)."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as smat

import hnsw_rule as hr
from clustering_rule import last_error

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hnsw")
X_CSR, X_DRM = hr.sparse_items(6, 10, 3, 1), hr.dense_items(6, 10, 2)


@pytest.mark.parametrize("name", ["csr_ip", "csr_l2", "drm_ip", "drm_l2"])
def test_level_plan_of_the_goldens(name):
    from pecos_amd import clib
    ix = hr.read_folder(os.path.join(GOLDEN, name))
    level = clib.debug_hnsw_levels(ix.num_node, 8, -1)
    assert int(level.max()) == ix.max_level == ix.l1_levels
    assert int(np.argmax(level)) == ix.init_node                   # (the first node that reaches the maximum)
    capped = clib.debug_hnsw_levels(ix.num_node, 8, 1)
    assert np.array_equal(capped, np.minimum(level, 1))


def train_error(X, M=8, efC=100, metric=b"ip", handle=True, null_x=False):
    lib = hr.ours()
    view, keep, kind = hr._view(X)
    fn = getattr(lib, "xrl_hnsw_train_%s_f32" % kind)
    fn.restype = ctypes.c_int
    h = ctypes.c_void_p()
    rc = fn(None if null_x else ctypes.byref(view), ctypes.c_uint32(M), ctypes.c_uint32(efC), ctypes.c_int32(1), ctypes.c_int32(-1), metric, 0, ctypes.byref(h) if handle else None)
    assert rc == -1 and not h.value
    return last_error(lib)


@pytest.mark.parametrize("X", [X_CSR, X_DRM], ids=["csr", "drm"])
@pytest.mark.parametrize("kw, text", [(dict(M=1), "M = 1 is below 2"), (dict(M=0), "M = 0 is below 2"), (dict(M=129), "M = 129 is above 128"), (dict(efC=0), "efC == 0"),
                                      (dict(efC=1025), "efC = 1025 is above CAP = 1024"), (dict(metric=b"cos"), "metric = cos is not implemented"),
                                      (dict(metric=None), "null argument (metric)"), (dict(handle=False), "null argument (handle)"), (dict(null_x=True), "null X")])
def test_refusals_before_a_gpu(X, kw, text):
    err = train_error(X, **kw)
    assert err.startswith("xrl_hnsw_train_") and text in err, err


def test_no_rows_and_the_other_entry_points():
    assert "X has no rows" in train_error(X_CSR[:0]) and "X has no rows" in train_error(X_DRM[:0])
    lib = hr.ours()
    h = ctypes.c_void_p()
    dev = lib.xrl_hnsw_train_device
    dev.restype = ctypes.c_int
    args = lambda rows, cols, stride, M: (0, ctypes.c_uint32(rows), ctypes.c_uint32(cols), None, ctypes.c_uint64(stride), None, None, ctypes.c_uint64(0), None, ctypes.c_uint32(M),
                                          ctypes.c_uint32(100), ctypes.c_int32(1), ctypes.c_int32(-1), b"ip", None, ctypes.byref(h))
    for a, text in ((args(4, 8, 7, 8), "row_stride = 7 is below feat_dim = 8"), (args(4, 8, 8, 1), "M = 1 is below 2"), (args(0, 8, 8, 8), "X has no rows"),
                    (args(4, 8, 8, 8), "null argument (the items)")):
        assert dev(*a) == -1 and text in last_error(lib)
    lib.xrl_hnsw_save.restype = ctypes.c_int
    assert lib.xrl_hnsw_save(None, b"/nowhere") == -1 and "null index handle" in last_error(lib)
    assert lib.xrl_debug_hnsw_levels(ctypes.c_uint32(4), ctypes.c_uint32(1), ctypes.c_int32(-1), None) == -1 and "null argument" in last_error(lib)
    out = np.zeros(4, dtype=np.uint32)
    assert lib.xrl_debug_hnsw_levels(ctypes.c_uint32(4), ctypes.c_uint32(1), ctypes.c_int32(-1), ctypes.c_void_p(out.ctypes.data)) == -1 and "is below 2" in last_error(lib)


def test_python_surface():
    import pecos_amd
    served, pinned = pecos_amd.hnsw.HNSW, pecos_amd.ann.HNSW
    assert pecos_amd.HNSW is pinned and issubclass(served, pinned) and served is not pinned
    tp = served.TrainParams()
    assert (tp.M, tp.efC, tp.threads, tp.max_level_upper_bound, tp.metric_type) == (32, 100, -1, -1, "ip")
    assert served.TrainParams.from_dict(dict(M=8, metric_type="l2", unknown=1)).metric_type == "l2"
    with pytest.raises(NotImplementedError, match="building the graph is not served"):
        pinned.train(X_DRM)
    with pytest.raises(NotImplementedError, match="is not written back"):
        pinned.save(object.__new__(pinned), "/nowhere")
    with pytest.raises(ValueError, match="is NOT supported"):
        served.train([[1.0, 2.0]])
    with pytest.raises(RuntimeError, match="M = 1 is below 2"):
        served.train(X_DRM, dict(M=1))
    with pytest.raises(RuntimeError, match="metric = cos is not implemented"):
        served.train(smat.csr_matrix(X_CSR), dict(M=8, metric_type="cos"))
