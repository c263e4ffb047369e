// Sparse matrix products (K10, xrl_spgemm.hip): c_sparse_matmul_csr_f32 / c_sparse_matmul_csc_f32 with the reference's signatures
// (libpecos.cpp:320-334 -> smat_x_smat, matrix.hpp:1075-1292), and the device matrix handles of xrl_smat_* / xrl_sparse_matmul_device, whose
// operands and product stay in HBM.  Every argument is checked before a GPU is required.
#include <atomic>
#include <memory>

#include "xrl_abi_common.h"
#include "xrl_spgemm.h"

using namespace xrl;

namespace {

// A CSR on one device: a view of arrays the handle owns (ptr / idx / val) or of the caller's.
struct Smat {
    int device = 0;
    CsrDev v;
    DevBuf ptr, idx, val;
    void own(int dev, uint32_t rows, uint32_t cols, uint64_t nnz) {
        device = dev;
        v.rows = rows; v.cols = cols; v.nnz = nnz;
        v.row_ptr = ptr.as<uint64_t>(); v.col_idx = idx.as<uint32_t>(); v.val = val.as<float>();
    }
};

Smat* as_smat(const char* what, void* p) {
    if (!p) fail(std::string(what) + ": null matrix handle");
    return static_cast<Smat*>(p);
}

std::atomic<uint64_t> g_forms[4];                          // rows served by the LDS form, by the big form; batches; products computed (calls)

void count_forms(const SpgemmOut& Z) { g_forms[0] += Z.lds_rows; g_forms[1] += Z.big_rows; g_forms[2] += Z.batches; g_forms[3] += 1; }

// a host CSR (checked by check_host_csr) copied to the current device
void upload_csr(uint32_t rows, uint32_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const float* val, Smat& m, int device) {
    const uint64_t nnz = rows ? row_ptr[rows] : 0;
    if (rows) m.ptr.upload_raw(row_ptr, ((size_t)rows + 1) * 8);
    else { m.ptr.reserve(8); XRL_HIP(hipMemset(m.ptr.p, 0, 8)); }
    m.idx.upload_raw(col_idx, nnz * 4);
    m.val.upload_raw(val, nnz * 4);
    m.own(device, rows, cols, nnz);
}

void check_host_csr(const std::string& what, const void* p, uint32_t rows, const uint64_t* row_ptr, const uint32_t* col_idx, const float* val) {
    if (!p) fail(what + "null matrix");
    if (!row_ptr) fail(what + "null row pointer");
    if (rows && row_ptr[rows] && (!col_idx || !val)) fail(what + "null indices or values");
}

// Z = A * B of two host CSRs through the allocator.  is_col_major: the arrays are the CSC arrays of the transposes, and the allocator is told
// so; z_rows x z_cols is the shape it is given (matrix.hpp:1209-1213).
void matmul_to_host(const char* what, uint32_t a_rows, uint32_t a_cols, const uint64_t* a_ptr, const uint32_t* a_idx, const float* a_val,
                    uint32_t b_rows, uint32_t b_cols, const uint64_t* b_ptr, const uint32_t* b_idx, const float* b_val,
                    bool is_col_major, uint64_t z_rows, uint64_t z_cols, py_sparse_allocator_t alloc, bool eliminate_zeros, bool sorted_indices) {
    require_gpu();
    use_device(g_device);
    Smat A, B;
    upload_csr(a_rows, a_cols, a_ptr, a_idx, a_val, A, g_device);
    upload_csr(b_rows, b_cols, b_ptr, b_idx, b_val, B, g_device);
    SpgemmOut Z;
    spgemm_device(A.v, B.v, eliminate_zeros, sorted_indices, nullptr, Z);
    count_forms(Z);
    uint32_t* indices = nullptr; uint64_t* indptr = nullptr; float* data = nullptr;
    alloc(is_col_major, z_rows, z_cols, Z.nnz, &indices, &indptr, &data);
    if (!indptr || (Z.nnz && (!indices || !data))) fail(std::string(what) + ": allocator returned null");
    // the reference compacts in place inside arrays sized for the count before elimination: past the compacted entries the arrays keep
    // what the un-compacted product held there
    if (Z.nnz) {
        XRL_HIP(hipMemcpy(indices, Z.idx.p, (size_t)Z.nnz * 4, hipMemcpyDeviceToHost));
        XRL_HIP(hipMemcpy(data, Z.val.p, (size_t)Z.nnz * 4, hipMemcpyDeviceToHost));
    }
    if (eliminate_zeros && Z.e_nnz) {
        XRL_HIP(hipMemcpy(indices, Z.e_idx.p, (size_t)Z.e_nnz * 4, hipMemcpyDeviceToHost));
        XRL_HIP(hipMemcpy(data, Z.e_val.p, (size_t)Z.e_nnz * 4, hipMemcpyDeviceToHost));
    }
    XRL_HIP(hipMemcpy(indptr, eliminate_zeros ? Z.e_ptr.p : Z.ptr.p, ((size_t)a_rows + 1) * 8, hipMemcpyDeviceToHost));
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
        matmul_to_host("c_sparse_matmul_csr_f32", pX->rows, pX->cols, pX->row_ptr, pX->col_idx, pX->val, pY->rows, pY->cols, pY->row_ptr, pY->col_idx, pY->val,
                       false, pX->rows, pY->cols, pred_alloc, eliminate_zeros, sorted_indices);
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
        matmul_to_host("c_sparse_matmul_csc_f32", pY->cols, pY->rows, pY->col_ptr, pY->row_idx, pY->val, pX->cols, pX->rows, pX->col_ptr, pX->row_idx, pX->val,
                       true, pX->rows, pY->cols, pred_alloc, eliminate_zeros, sorted_indices);
    });
}

void* xrl_smat_upload_csr(int device, const ScipyCsrF32* X) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const std::string what = "xrl_smat_upload_csr: ";
        if (device < 0) fail(what + "negative device");
        check_host_csr(what, X, X ? X->rows : 0, X ? X->row_ptr : nullptr, X ? X->col_idx : nullptr, X ? X->val : nullptr);
        require_gpu();
        use_device(device);
        auto m = std::make_unique<Smat>();
        upload_csr(X->rows, X->cols, X->row_ptr, X->col_idx, X->val, *m, device);
        return m.release();
    });
}

void* xrl_smat_from_device_csr(int device, uint32_t rows, uint32_t cols, const uint64_t* d_row_ptr, const uint32_t* d_col_idx, const float* d_val, uint64_t nnz) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const std::string what = "xrl_smat_from_device_csr: ";
        if (device < 0) fail(what + "negative device");
        if (!d_row_ptr || (nnz && (!d_col_idx || !d_val))) fail(what + "null device pointer");
        auto m = std::make_unique<Smat>();
        m->device = device;
        m->v.rows = rows; m->v.cols = cols; m->v.nnz = nnz;
        m->v.row_ptr = d_row_ptr; m->v.col_idx = d_col_idx; m->v.val = d_val;
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
        auto m = std::make_unique<Smat>();
        const uint64_t nnz = topk_to_csr_device(rows, d_idx, d_val, d_cnt, stride, static_cast<hipStream_t>(hip_stream), m->ptr, m->idx, m->val);
        m->own(device, rows, cols, nnz);
        return m.release();
    });
}

int xrl_smat_info(void* h, uint64_t* out, uint32_t cap) {
    return guarded_value(-1, [&] {
        const Smat& m = *as_smat("xrl_smat_info", h);
        if (!out) fail("xrl_smat_info: null argument");
        const uint64_t v[7] = {m.v.rows, m.v.cols, m.v.nnz, (uint64_t)m.device, (uint64_t)(uintptr_t)m.v.row_ptr, (uint64_t)(uintptr_t)m.v.col_idx,
                               (uint64_t)(uintptr_t)m.v.val};
        for (uint32_t i = 0; i < cap && i < 7; ++i) out[i] = v[i];
        return 0;
    });
}

int xrl_smat_download(void* h, uint64_t* row_ptr, uint32_t* col_idx, float* val) {
    return guarded_value(-1, [&] {
        const Smat& m = *as_smat("xrl_smat_download", h);
        if (!row_ptr || (m.v.nnz && (!col_idx || !val))) fail("xrl_smat_download: null argument");
        require_gpu();
        use_device(m.device);
        XRL_HIP(hipDeviceSynchronize());
        XRL_HIP(hipMemcpy(row_ptr, m.v.row_ptr, ((size_t)m.v.rows + 1) * 8, hipMemcpyDeviceToHost));
        if (m.v.nnz) {
            XRL_HIP(hipMemcpy(col_idx, m.v.col_idx, (size_t)m.v.nnz * 4, hipMemcpyDeviceToHost));
            XRL_HIP(hipMemcpy(val, m.v.val, (size_t)m.v.nnz * 4, hipMemcpyDeviceToHost));
        }
        return 0;
    });
}

int xrl_smat_copy_device(void* h, uint64_t* d_row_ptr, uint32_t* d_col_idx, float* d_val, void* hip_stream) {
    return guarded_value(-1, [&] {
        const Smat& m = *as_smat("xrl_smat_copy_device", h);
        if (!d_row_ptr || (m.v.nnz && (!d_col_idx || !d_val))) fail("xrl_smat_copy_device: null device pointer");
        require_gpu();
        use_device(m.device);
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        XRL_HIP(hipMemcpyAsync(d_row_ptr, m.v.row_ptr, ((size_t)m.v.rows + 1) * 8, hipMemcpyDeviceToDevice, s));
        if (m.v.nnz) {
            XRL_HIP(hipMemcpyAsync(d_col_idx, m.v.col_idx, (size_t)m.v.nnz * 4, hipMemcpyDeviceToDevice, s));
            XRL_HIP(hipMemcpyAsync(d_val, m.v.val, (size_t)m.v.nnz * 4, hipMemcpyDeviceToDevice, s));
        }
        XRL_HIP(hipStreamSynchronize(s));
        return 0;
    });
}

void xrl_smat_free(void* h) {
    guarded([&] {
        Smat* m = static_cast<Smat*>(h);
        if (!m) return;
        if (m->ptr.p || m->idx.p || m->val.p) (void)hipSetDevice(m->device);    // (its buffers are freed with their device set)
        delete m;
    });
}

void* xrl_sparse_matmul_device(void* A, void* B, int eliminate_zeros, int sorted_indices, void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const Smat& a = *as_smat("xrl_sparse_matmul_device", A);
        const Smat& b = *as_smat("xrl_sparse_matmul_device", B);
        if (a.device != b.device)
            fail("xrl_sparse_matmul_device: the operands are on devices " + std::to_string(a.device) + " and " + std::to_string(b.device) + "; a product needs both on one");
        if (a.v.cols != b.v.rows) fail("xrl_sparse_matmul_device: X.cols != W.rows (" + std::to_string(a.v.cols) + " != " + std::to_string(b.v.rows) + ")");
        require_gpu();
        use_device(a.device);
        SpgemmOut Z;
        spgemm_device(a.v, b.v, eliminate_zeros != 0, sorted_indices != 0, static_cast<hipStream_t>(hip_stream), Z);
        count_forms(Z);
        auto m = std::make_unique<Smat>();
        if (eliminate_zeros) { m->ptr = std::move(Z.e_ptr); m->idx = std::move(Z.e_idx); m->val = std::move(Z.e_val); m->own(a.device, a.v.rows, b.v.cols, Z.e_nnz); }
        else { m->ptr = std::move(Z.ptr); m->idx = std::move(Z.idx); m->val = std::move(Z.val); m->own(a.device, a.v.rows, b.v.cols, Z.nnz); }
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
