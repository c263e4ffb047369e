"""Sparse matrix products (K10), the half that needs no GPU: the numpy restatement of the rule against the compiled reference, the
precondition of the order test, the python wrapper's dispatch and errors, every refusal that comes before a GPU is needed, and the
reference's own binding resolving all six sparse-operation symbols to this library."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as smat

import sparse_matmul_rule as R
from conftest import REPO
from oracle import xrl_oracle

OURS = os.environ.get("PECOS_XRL_AMD_SO") or os.path.join(REPO, "pecos_amd", "lib", "libxrl_amd.so")
CASES = R.cpu_cases()


@pytest.fixture(scope="module")
def ref():
    if not xrl_oracle.ref_available():
        pytest.skip("oracle/_ref (the compiled reference) is not built")
    return R.ref_lib()


@pytest.fixture(scope="module")
def ours():
    lib = C.CDLL(OURS)
    lib.xrl_last_error.restype = C.c_char_p
    for name in ("xrl_smat_upload_csr", "xrl_smat_from_device_csr", "xrl_smat_from_device_result", "xrl_sparse_matmul_device"):
        getattr(lib, name).restype = C.c_void_p
    lib.xrl_smat_from_device_csr.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    lib.xrl_smat_from_device_result.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.xrl_sparse_matmul_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.xrl_smat_upload_csr.argtypes = [C.c_int, C.c_void_p]
    lib.xrl_smat_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]
    lib.xrl_smat_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.xrl_smat_copy_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.xrl_smat_free.argtypes = [C.c_void_p]
    lib.xrl_debug_spgemm_forms.argtypes = [C.POINTER(C.c_uint64), C.c_uint32]
    return lib


def _err(lib):
    e = lib.xrl_last_error()
    return e.decode() if e else None


# ------------------------------------------------------------------------------------------------------- the rule is the reference's
# (every case but the one of 2^32 - 1 columns: the reference's dense accumulator of that length does not fit a test machine, and the GPU
# half compares that case with the restatement alone)
@pytest.mark.parametrize("name", sorted(n for n in CASES if R.reference_can_run(*CASES[n])))
def test_restatement_equals_the_compiled_reference(ref, name):
    A, B = CASES[name]
    for ez, si in R.SETTINGS:
        want = R.rule(A, B, ez, si)
        one, calls = R.native_matmul(ref, A, B, "csr", ez, si, threads=1)
        assert R.same(one, want), (name, ez, si)                                   # the whole allocator buffer, the stale tail included
        assert calls == [(False, A.shape[0], B.shape[1], len(want[1]))]            # one call, the count BEFORE elimination
        eight, _ = R.native_matmul(ref, A, B, "csr", ez, si, threads=8)
        assert R.same(eight, one), (name, ez, si, "threads")
        # the CSC entry point on the transposes' arrays returns the same arrays
        csc, calls = R.native_matmul(ref, R.transpose_view(B), R.transpose_view(A), "csc", ez, si, threads=1)
        assert R.same(csc, want) and calls == [(True, B.shape[1], A.shape[0], len(want[1]))], (name, ez, si, "csc")


def test_eliminate_zeros_leaves_a_stale_tail_in_the_cases():
    # what makes the whole-buffer comparison more than the logical one
    A, B = CASES["numeric_edges"]
    full, cut = R.rule(A, B, False, True), R.rule(A, B, True, True)
    n = int(cut[0][-1])
    assert 0 < n < len(cut[1]) == len(full[1])
    assert np.array_equal(cut[1][n:], full[1][n:]) and np.array_equal(R.bits(cut[2][n:]), R.bits(full[2][n:]))
    assert np.isnan(cut[2][:n]).any() and not (cut[2][:n] == 0).any()


def test_left_row_order_changes_the_reference_s_own_answer(ref):
    # the precondition of the GPU half's order test: a kernel that reorders the left rows is caught by values, not only by layout
    A, B = R.shuffled_pair()
    a, _ = R.native_matmul(ref, A, B)
    b, _ = R.native_matmul(ref, R.sort_left_rows(A), B)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert int((R.bits(a[2]) != R.bits(b[2])).sum()) >= 1


def test_first_touch_order_differs_from_sorted_order_in_the_cases():
    A, B = R.shuffled_pair()
    assert not np.array_equal(R.rule(A, B, False, False)[1], R.rule(A, B, False, True)[1])


# --------------------------------------------------------------------------------------------------------------- the python wrapper
class _Recording:
    """Stands in for the loaded library: the two entry points are the compiled reference's, and every call is noted."""

    def __init__(self, ref):
        self.ref, self.calls = ref, []

    def xrl_last_error(self):
        return None

    def __getattr__(self, name):
        assert name.startswith("c_sparse_matmul_"), name
        fn = getattr(self.ref, name)
        fn.restype, fn.argtypes = None, None

        def call(pX, pY, alloc, ez, si, threads):
            self.calls.append((name, type(pX).__name__, type(pY).__name__))
            fn(C.byref(pX), C.byref(pY), alloc, C.c_bool(ez), C.c_bool(si), C.c_int(threads))
        return call


def test_wrapper_dispatch_table(ref):
    from pecos_amd.core import corelib
    z = np.load(os.path.join(R.GOLDEN_DIR, "wrapper.npz"))
    lib = corelib()
    lib._lib = rec = _Recording(ref)
    for tag, want_fmt in (("left_larger", {("csc", "csr"): "csc", ("csr", "csc"): "csr"}), ("right_larger", {("csc", "csr"): "csr", ("csr", "csc"): "csc"})):
        X, Y = (smat.csr_matrix((z[f"{tag}__{n}_data"], z[f"{tag}__{n}_indices"], z[f"{tag}__{n}_indptr"]), shape=tuple(z[f"{tag}__{n}_shape"])) for n in "XY")
        for fx, fy in R.WRAPPER_COMBOS:
            fmt = fx if fx == fy else want_fmt[(fx, fy)]            # the operand with FEWER entries is the one converted (base.py:1499-1528)
            for ez, si in R.SETTINGS:
                rec.calls.clear()
                Z = lib.sparse_matmul(X.asformat(fx), Y.asformat(fy), eliminate_zeros=ez, sorted_indices=si)
                view = {"csr": "ScipyCsrF32", "csc": "ScipyCscF32"}[fmt]
                assert rec.calls == [(f"c_sparse_matmul_{fmt}_f32", view, view)], (tag, fx, fy, rec.calls)
                key = f"{tag}__{fx}_{fy}__{int(ez)}{int(si)}"
                assert Z.format == str(z[key + "__format"]) == fmt and Z.shape == (X.shape[0], Y.shape[1])
                # (the reference's matrix class keeps the allocator's arrays whole, stale tail included; scipy's own prunes them to
                # indptr[-1].  The stored entries are compared here, the whole buffers at the C entry points.)
                n = int(z[key + "__indptr"][-1])
                assert np.array_equal(Z.indptr, z[key + "__indptr"]) and np.array_equal(Z.indices[:n], z[key + "__indices"][:n]), key
                assert Z.nnz == n and np.array_equal(R.bits(Z.data[:n]), R.bits(z[key + "__data"][:n])), key


def test_wrapper_errors():
    from pecos_amd import clib
    X = smat.csr_matrix(np.ones((3, 4), dtype=np.float32))
    with pytest.raises(ValueError, match=r"X\.shape\[1\]=4 != Y\.shape\[0\]=3"):
        clib.sparse_matmul(X, X)
    with pytest.raises(ValueError, match="should be either csr_matrix/csc_matrix"):
        clib.sparse_matmul(X, np.ones((4, 2), dtype=np.float32))
    with pytest.raises(ValueError, match="should be either csr_matrix/csc_matrix"):
        clib.sparse_matmul(X.tocoo(), X.T.tocsr())


# ------------------------------------------------------------------------------------------ refusals that need no GPU (and touch none)
def _mat(M):
    return R._view(M, "csr")


def test_host_entry_points_refuse_before_a_gpu_is_needed(ours):
    A, B = CASES["shape_one_row"]
    alloc = R.Allocator()
    cb = R._ALLOC(alloc)
    for fmt in ("csr", "csc"):
        name = f"c_sparse_matmul_{fmt}_f32"
        fn = getattr(ours, name)
        fn.restype, fn.argtypes = None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_bool, C.c_bool, C.c_int]
        # (the CSC entry point takes the transposes' arrays: X = B^T, Y = A^T)
        L, Rt = (A, B) if fmt == "csr" else (R.transpose_view(B), R.transpose_view(A))
        a, b = _mat(L), _mat(Rt)
        fn(None, C.byref(b), cb, False, True, 1)
        assert _err(ours) == f"{name}: X: null matrix"
        fn(C.byref(a), None, cb, False, True, 1)
        assert _err(ours) == f"{name}: Y: null matrix"
        fn(C.byref(a), C.byref(b), None, False, True, 1)
        assert _err(ours) == f"{name}: null allocator"
        nul = _mat(L); nul.ptr = None
        fn(C.byref(nul), C.byref(b), cb, False, True, 1)
        assert _err(ours) == f"{name}: X: null row pointer"
        nul = _mat(Rt); nul.val = None
        fn(C.byref(a), C.byref(nul), cb, False, True, 1)
        assert _err(ours) == f"{name}: Y: null indices or values"
        fn(C.byref(a), C.byref(a), cb, False, True, 1)                   # 1 x 2 by 1 x 2; 6 x 2 by 6 x 2
        assert _err(ours) == f"{name}: X.cols != W.rows"
    assert alloc.calls == []                                            # a refused call never reaches the allocator


def test_device_handles_refuse_before_a_gpu_is_needed(ours):
    fake = 0x1000                                                       # wrapped, never read: no call below reaches a kernel
    a0 = ours.xrl_smat_from_device_csr(0, 3, 4, fake, fake, fake, 5)
    b0 = ours.xrl_smat_from_device_csr(0, 5, 2, fake, fake, fake, 5)
    b1 = ours.xrl_smat_from_device_csr(1, 4, 2, fake, fake, fake, 5)
    assert a0 and b0 and b1 and _err(ours) is None
    try:
        out = (C.c_uint64 * 7)()
        assert ours.xrl_smat_info(a0, out, 7) == 0 and list(out) == [3, 4, 5, 0, fake, fake, fake]
        assert ours.xrl_sparse_matmul_device(a0, b1, 0, 1, None) is None
        assert _err(ours) == "xrl_sparse_matmul_device: the operands are on devices 0 and 1; a product needs both on one"
        assert ours.xrl_sparse_matmul_device(a0, b0, 0, 1, None) is None
        assert _err(ours) == "xrl_sparse_matmul_device: X.cols != W.rows (4 != 5)"
        assert ours.xrl_sparse_matmul_device(None, b0, 0, 1, None) is None and _err(ours) == "xrl_sparse_matmul_device: null matrix handle"
        assert ours.xrl_sparse_matmul_device(a0, None, 0, 1, None) is None and _err(ours) == "xrl_sparse_matmul_device: null matrix handle"
    finally:
        for h in (a0, b0, b1):
            ours.xrl_smat_free(h)
    ours.xrl_smat_free(None)
    assert ours.xrl_smat_from_device_csr(0, 3, 4, None, fake, fake, 5) is None and _err(ours) == "xrl_smat_from_device_csr: null device pointer"
    assert ours.xrl_smat_from_device_csr(0, 3, 4, fake, None, fake, 5) is None and _err(ours) == "xrl_smat_from_device_csr: null device pointer"
    assert ours.xrl_smat_from_device_csr(-1, 3, 4, fake, fake, fake, 5) is None and _err(ours) == "xrl_smat_from_device_csr: negative device"
    assert ours.xrl_smat_from_device_result(0, 3, 4, None, fake, None, 10, None) is None and _err(ours) == "xrl_smat_from_device_result: null device pointer"
    assert ours.xrl_smat_upload_csr(0, None) is None and _err(ours) == "xrl_smat_upload_csr: null matrix"
    assert ours.xrl_smat_info(None, (C.c_uint64 * 7)(), 7) == -1 and _err(ours) == "xrl_smat_info: null matrix handle"
    assert ours.xrl_smat_download(None, None, None, None) == -1 and _err(ours) == "xrl_smat_download: null matrix handle"
    assert ours.xrl_smat_copy_device(None, None, None, None, None) == -1 and _err(ours) == "xrl_smat_copy_device: null matrix handle"
    assert ours.xrl_debug_spgemm_forms(None, 5) == -1 and _err(ours) == "xrl_debug_spgemm_forms: null argument"
    out = (C.c_uint64 * 5)()
    assert ours.xrl_debug_spgemm_forms(out, 5) == 0 and out[0] == 1024   # CAP, as xrl_abi.h states it


def test_the_python_device_wrapper_names_the_missing_column_count():
    from pecos_amd.features import DeviceMatrix, _as_device_matrix
    with pytest.raises(ValueError, match="needs its column count"):
        _as_device_matrix((None, None, None), 0, None, None)
    with pytest.raises(TypeError, match="operand of type"):
        _as_device_matrix(np.ones((2, 2)), 0, None, None)
    assert DeviceMatrix(None).handle is None                            # (nothing to free)


# ------------------------------------------------------------------------------------------------- the reference's own binding layer
def test_reference_link_sparse_operations_binds_all_six_to_this_library():
    from test_reference_binding import _bind
    pcb, lib, Mixed, ours_lib = _bind()
    six = {"c_sparse_matmul_csr_f32", "c_sparse_matmul_csc_f32", "c_sparse_inner_products_csr2csc_f32", "c_sparse_inner_products_drm2csc_f32",
           "c_sparse_inner_products_csr2dcm_f32", "c_sparse_inner_products_drm2dcm_f32"}
    assert six <= Mixed.taken, sorted(six - Mixed.taken)
    for name in six:
        assert getattr(ours_lib, name)                                  # exported by this library itself, not only found through the loader
    fn = lib.clib_float32.c_sparse_matmul_csr_f32
    assert fn.restype is None and len(fn.argtypes) == 6
