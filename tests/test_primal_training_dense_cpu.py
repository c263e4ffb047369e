"""xrl_train_layer_newton_dense_device refuses what it can before a GPU is required, in xrl_train_layer_dense_device's words under its own
name (the device pointers and the handles' arrays are fake and never read); the forms call's limits; and the Python dispatch of a tensor X
under the primal solver."""
import ctypes

import pytest

import ranker_training_rule as rr
from test_ranker_training_cpu import _fake_handle

FAKE = 4096
N, D, L, K = 30, 12, 6, 2
START = "xrl_train_layer_newton_dense_device: "
YT = (0, L, N, 3)
#        d_X, rows, cols, row_stride, solver, (Yt, Ct, Mt, Rt) as (device, rows, cols, nnz) or None, message
CASES = {
    "l2_dual": (FAKE, N, D, D, 1, (YT, None, None, None), "solver L2R_L2LOSS_SVC_DUAL is served by the entry point without `newton` in its name (xrl_train_layer_dense_device)"),
    "l1_dual": (FAKE, N, D, D, 3, (YT, None, None, None), "solver L2R_L1LOSS_SVC_DUAL is served by the entry point without `newton` in its name (xrl_train_layer_dense_device)"),
    "lr_dual": (FAKE, N, D, D, 7, (YT, None, None, None), "solver L2R_LR_DUAL is not served on the device"),
    "unknown_solver": (FAKE, N, D, D, 4, (YT, None, None, None), "unknown solver_type 4 (2 = L2R_L2LOSS_SVC_PRIMAL)"),
    "null_x": (None, N, D, D, 2, (YT, None, None, None), "null X"),
    "stride_below_cols": (FAKE, N, D, D - 1, 2, (YT, None, None, None), "row_stride 11 is below cols 12"),
    "too_wide": (FAKE, N, 16385, 16385, 2, (YT, None, None, None), "16385 columns: a dense X is served up to 16384"),
    "too_many_rows": (FAKE, 1 << 31, D, D, 2, (YT, None, None, None), "2^31 rows or more"),
    "null_yt": (FAKE, N, D, D, 2, (None, None, None, None), "null matrix handle (Yt)"),
    "ct_without_mt": (FAKE, N, D, D, 2, (YT, (0, K, L, 3), None, None), "Ct comes without Mt"),
    "yt_cols": (FAKE, N, D, D, 2, ((0, L, N + 1, 3), None, None, None), "Yt.cols != X.rows (31 != 30)"),
    "ct_cols": (FAKE, N, D, D, 2, (YT, (0, K, L + 1, 3), (0, K, N, 3), None), "Ct.cols != Yt.rows (7 != 6)"),
    "mt_cols": (FAKE, N, D, D, 2, (YT, (0, K, L, 3), (0, K, N + 1, 3), None), "Mt.cols != X.rows (31 != 30)"),
    "mt_rows": (FAKE, N, D, D, 2, (YT, (0, K, L, 3), (0, K + 1, N, 3), None), "Mt.rows != Ct.rows (3 != 2)"),
    "rt_pattern": (FAKE, N, D, D, 2, (YT, None, None, (0, L, N, 4)), "Rt does not share Yt's pattern (shape or stored entries)"),
    "two_devices": (FAKE, N, D, D, 2, ((1, L, N, 3), None, None, None), "the operands are on devices 0 and 1; training needs all on one"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusals_before_a_gpu_through_the_binding(name):
    from pecos_amd import clib
    d_X, rows, cols, stride, solver, handles, message = CASES[name]
    lib = rr.load(rr.OURS)
    lib.xrl_smat_free.argtypes = [ctypes.c_void_p]
    hs = [None if h is None else _fake_handle(lib, h[0], h[1], h[2], nnz=h[3]) for h in handles]
    try:
        with pytest.raises(RuntimeError) as e:
            clib.train_layer_newton_dense_device(0, d_X, rows, cols, stride, *hs, solver_type=solver)
        assert str(e.value).startswith(START + message), str(e.value)
    finally:
        for h in hs:
            if h:
                lib.xrl_smat_free(h)


def test_forms_export_and_limits():
    """The vectors' eight arrays of `lds_cols` floats and the row tile fill the 64 KB a workgroup gets, twice inside a CU's 160 KB."""
    from pecos_amd import clib
    f = clib.debug_newton_dense_forms()
    assert (f["lds_cols"], f["max_cols"]) == (1780, 16384) and f["lds_jobs"] >= 0 and f["scratch_jobs"] >= 0
    assert 8 * 4 * f["lds_cols"] + 4 * (64 * 33 + 32) <= 64 << 10 < 8 * 4 * (f["lds_cols"] + 1) + 4 * (64 * 33 + 32)


def test_python_dispatch_of_a_tensor():
    torch = pytest.importorskip("torch")
    import scipy.sparse as smat
    import pecos_amd
    Y = smat.csr_matrix([[1, 0], [0, 1], [1, 0], [0, 1]], dtype="float32")
    with pytest.raises(ValueError, match="train_layer_device: a tensor X must be a 2-D float32 CUDA tensor"):
        pecos_amd.train_layer_device(torch.zeros((4, 3)), Y, solver_type="L2R_L2LOSS_SVC_PRIMAL")
