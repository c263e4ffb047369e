// Sparse matrix products (K10, xrl_spgemm.hip): c_sparse_matmul_csr_f32 / c_sparse_matmul_csc_f32 with the reference's signatures
// (libpecos.cpp:320-334 -> smat_x_smat, matrix.hpp:1075-1292), and the device matrix handles of xrl_smat_* / xrl_sparse_matmul_device, whose
// operands and product stay in HBM.  Every argument is checked before a GPU is required.
#include <atomic>
#include <memory>

#include "xrl_abi_common.h"
#include "xrl_spgemm.h"

using namespace xrl;

namespace {

// a matrix handle: a Queries (xrl_predict.h) whose view is a CSR
Queries* as_smat(const char* what, void* p) {
    if (!p) fail(std::string(what) + ": null matrix handle");
    return static_cast<Queries*>(p);
}

std::atomic<uint64_t> g_forms[4];                          // rows served by the LDS form, by the big form; batches; products computed (calls)

void count_forms(const SpgemmOut& Z) { g_forms[0] += Z.lds_rows; g_forms[1] += Z.big_rows; g_forms[2] += Z.batches; g_forms[3] += 1; }

void check_host_csr(const std::string& what, const void* p, uint32_t rows, const uint64_t* row_ptr, const uint32_t* col_idx, const float* val) {
    if (!p) fail(what + "null matrix");
    if (!row_ptr) fail(what + "null row pointer");
    if (rows && row_ptr[rows] && (!col_idx || !val)) fail(what + "null indices or values");
}

// Z = A * B of two host CSRs through the allocator.  is_col_major: the arrays are the CSC arrays of the transposes, and the allocator is told
// so; z_rows x z_cols is the shape it is given (matrix.hpp:1209-1213).
void matmul_to_host(const char* what, const ScipyCsrF32& a, const ScipyCsrF32& b, bool is_col_major, uint64_t z_rows, uint64_t z_cols,
                    py_sparse_allocator_t alloc, bool eliminate_zeros, bool sorted_indices) {
    require_gpu();
    use_device(g_device);
    DevCsr A, B;
    QueriesDev Av, Bv;
    upload_x(HostX(&a), A.ptr, A.idx, A.val, Av);
    upload_x(HostX(&b), B.ptr, B.idx, B.val, Bv);
    SpgemmOut Z;
    spgemm_device(Av, Bv, eliminate_zeros, sorted_indices, nullptr, Z);
    count_forms(Z);
    const uint64_t nnz = Z.z.nnz;
    uint32_t* indices = nullptr; uint64_t* indptr = nullptr; float* data = nullptr;
    alloc(is_col_major, z_rows, z_cols, nnz, &indices, &indptr, &data);
    if (!indptr || (nnz && (!indices || !data))) fail(std::string(what) + ": allocator returned null");
    // the reference compacts in place inside arrays sized for the count before elimination: past the compacted entries the arrays keep
    // what the un-compacted product held there
    if (nnz) {
        XRL_HIP(hipMemcpy(indices, Z.z.idx.p, (size_t)nnz * 4, hipMemcpyDeviceToHost));
        XRL_HIP(hipMemcpy(data, Z.z.val.p, (size_t)nnz * 4, hipMemcpyDeviceToHost));
    }
    if (eliminate_zeros && Z.e.nnz) {
        XRL_HIP(hipMemcpy(indices, Z.e.idx.p, (size_t)Z.e.nnz * 4, hipMemcpyDeviceToHost));
        XRL_HIP(hipMemcpy(data, Z.e.val.p, (size_t)Z.e.nnz * 4, hipMemcpyDeviceToHost));
    }
    XRL_HIP(hipMemcpy(indptr, eliminate_zeros ? Z.e.ptr.p : Z.z.ptr.p, ((size_t)a.rows + 1) * 8, hipMemcpyDeviceToHost));
}

}  // namespace

extern "C" {

void c_sparse_matmul_csr_f32(const ScipyCsrF32* pX, const ScipyCsrF32* pY, py_sparse_allocator_t pred_alloc, const bool eliminate_zeros,
                             const bool sorted_indices, int threads) {
    (void)threads;
    guarded([&] {
        const std::string what = "c_sparse_matmul_csr_f32: ";
        if (!pred_alloc) fail(what + "null allocator");
        check_host_csr(what + "X: ", pX, pX ? pX->rows : 0, pX ? pX->row_ptr : nullptr, pX ? pX->col_idx : nullptr, pX ? pX->val : nullptr);
        check_host_csr(what + "Y: ", pY, pY ? pY->rows : 0, pY ? pY->row_ptr : nullptr, pY ? pY->col_idx : nullptr, pY ? pY->val : nullptr);
        if (pX->cols != pY->rows) fail(what + "X.cols != W.rows");
        matmul_to_host("c_sparse_matmul_csr_f32", *pX, *pY, false, pX->rows, pY->cols, pred_alloc, eliminate_zeros, sorted_indices);
    });
}

// X * Y in CSC = the CSR of (X * Y)^T = Y^T * X^T, and the CSC arrays of a matrix are the CSR arrays of its transpose
void c_sparse_matmul_csc_f32(const ScipyCscF32* pX, const ScipyCscF32* pY, py_sparse_allocator_t pred_alloc, const bool eliminate_zeros,
                             const bool sorted_indices, int threads) {
    (void)threads;
    guarded([&] {
        const std::string what = "c_sparse_matmul_csc_f32: ";
        if (!pred_alloc) fail(what + "null allocator");
        check_host_csr(what + "X: ", pX, pX ? pX->cols : 0, pX ? pX->col_ptr : nullptr, pX ? pX->row_idx : nullptr, pX ? pX->val : nullptr);
        check_host_csr(what + "Y: ", pY, pY ? pY->cols : 0, pY ? pY->col_ptr : nullptr, pY ? pY->row_idx : nullptr, pY ? pY->val : nullptr);
        if (pX->cols != pY->rows) fail(what + "X.cols != W.rows");
        const ScipyCsrF32 yt{pY->cols, pY->rows, pY->col_ptr, pY->row_idx, pY->val}, xt{pX->cols, pX->rows, pX->col_ptr, pX->row_idx, pX->val};
        matmul_to_host("c_sparse_matmul_csc_f32", yt, xt, true, pX->rows, pY->cols, pred_alloc, eliminate_zeros, sorted_indices);
    });
}

void* xrl_smat_upload_csr(int device, const ScipyCsrF32* X) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const std::string what = "xrl_smat_upload_csr: ";
        if (device < 0) fail(what + "negative device");
        check_host_csr(what, X, X ? X->rows : 0, X ? X->row_ptr : nullptr, X ? X->col_idx : nullptr, X ? X->val : nullptr);
        require_gpu();
        return upload_handle(HostX(X), device);
    });
}

void* xrl_smat_from_device_csr(int device, uint32_t rows, uint32_t cols, const uint64_t* d_row_ptr, const uint32_t* d_col_idx, const float* d_val, uint64_t nnz) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const std::string what = "xrl_smat_from_device_csr: ";
        if (device < 0) fail(what + "negative device");
        if (!d_row_ptr || (nnz && (!d_col_idx || !d_val))) fail(what + "null device pointer");
        auto m = std::make_unique<Queries>();
        set_view(*m, device, csr_view(rows, cols, d_row_ptr, d_col_idx, d_val, nnz));
        return m.release();
    });
}

void* xrl_smat_from_device_result(int device, uint32_t rows, uint32_t cols, const uint32_t* d_idx, const float* d_val, const uint32_t* d_cnt, uint32_t stride,
                                  void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const std::string what = "xrl_smat_from_device_result: ";
        if (device < 0) fail(what + "negative device");
        if (rows && stride && (!d_idx || !d_val)) fail(what + "null device pointer");
        require_gpu();
        use_device(device);
        auto m = std::make_unique<Queries>();
        topk_to_csr_device(rows, d_idx, d_val, d_cnt, stride, static_cast<hipStream_t>(hip_stream), m->own);
        set_own_csr(*m, device, rows, cols);
        return m.release();
    });
}

int xrl_smat_info(void* h, uint64_t* out, uint32_t cap) {
    return guarded_value(-1, [&] {
        const Queries& m = *as_smat("xrl_smat_info", h);
        if (!out) fail("xrl_smat_info: null argument");
        const uint64_t v[7] = {m.dev.rows, m.dev.cols, m.dev.nnz, (uint64_t)m.device, (uint64_t)(uintptr_t)m.dev.row_ptr, (uint64_t)(uintptr_t)m.dev.col_idx,
                               (uint64_t)(uintptr_t)m.dev.val};
        for (uint32_t i = 0; i < cap && i < 7; ++i) out[i] = v[i];
        return 0;
    });
}

int xrl_smat_download(void* h, uint64_t* row_ptr, uint32_t* col_idx, float* val) {
    return guarded_value(-1, [&] {
        const Queries& m = *as_smat("xrl_smat_download", h);
        if (!row_ptr || (m.dev.nnz && (!col_idx || !val))) fail("xrl_smat_download: null argument");
        require_gpu();
        use_device(m.device);
        XRL_HIP(hipDeviceSynchronize());
        download_csr(m.dev, row_ptr, col_idx, val);
        return 0;
    });
}

int xrl_smat_copy_device(void* h, uint64_t* d_row_ptr, uint32_t* d_col_idx, float* d_val, void* hip_stream) {
    return guarded_value(-1, [&] {
        const Queries& m = *as_smat("xrl_smat_copy_device", h);
        const QueriesDev& v = m.dev;
        if (!d_row_ptr || (v.nnz && (!d_col_idx || !d_val))) fail("xrl_smat_copy_device: null device pointer");
        require_gpu();
        use_device(m.device);
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        XRL_HIP(hipMemcpyAsync(d_row_ptr, v.row_ptr, ((size_t)v.rows + 1) * 8, hipMemcpyDeviceToDevice, s));
        if (v.nnz) {
            XRL_HIP(hipMemcpyAsync(d_col_idx, v.col_idx, (size_t)v.nnz * 4, hipMemcpyDeviceToDevice, s));
            XRL_HIP(hipMemcpyAsync(d_val, v.val, (size_t)v.nnz * 4, hipMemcpyDeviceToDevice, s));
        }
        XRL_HIP(hipStreamSynchronize(s));
        return 0;
    });
}

void xrl_smat_free(void* h) { guarded([&] { free_handle(h); }); }

void* xrl_sparse_matmul_device(void* A, void* B, int eliminate_zeros, int sorted_indices, void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const Queries& a = *as_smat("xrl_sparse_matmul_device", A);
        const Queries& b = *as_smat("xrl_sparse_matmul_device", B);
        if (a.device != b.device)
            fail("xrl_sparse_matmul_device: the operands are on devices " + std::to_string(a.device) + " and " + std::to_string(b.device) + "; a product needs both on one");
        if (a.dev.cols != b.dev.rows) fail("xrl_sparse_matmul_device: X.cols != W.rows (" + std::to_string(a.dev.cols) + " != " + std::to_string(b.dev.rows) + ")");
        require_gpu();
        use_device(a.device);
        SpgemmOut Z;
        spgemm_device(a.dev, b.dev, eliminate_zeros != 0, sorted_indices != 0, static_cast<hipStream_t>(hip_stream), Z);
        count_forms(Z);
        auto m = std::make_unique<Queries>();
        m->own = std::move(eliminate_zeros ? Z.e : Z.z);
        set_own_csr(*m, a.device, a.dev.rows, b.dev.cols);
        return m.release();
    });
}

int xrl_debug_spgemm_forms(uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&] {
        if (!out) fail("xrl_debug_spgemm_forms: null argument");
        const uint64_t v[5] = {kSpgemmCap, g_forms[0].load(), g_forms[1].load(), g_forms[2].load(), g_forms[3].load()};
        for (uint32_t i = 0; i < n && i < 5; ++i) out[i] = v[i];
        return 0;
    });
}

}  // extern "C"
