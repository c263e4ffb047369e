// What the units behind the extern "C" surface share (xrl_abi.cpp, xrl_host_pipeline.cpp, xrl_single_layer.cpp, xrl_tfidf_abi.cpp, xrl_smat_abi.cpp, xrl_embed_abi.cpp):
// the per-thread error and device state, the exception barrier of every entry point, the makers of X's device view, the upload of a caller's host X,
// and the bodies the query and matrix handles share.
#pragma once
#include "../../include/xrl_abi.h"

#include <string>

#include "xrl_predict.h"

namespace xrl {

// per calling thread: what xrl_last_error() reports, and the device xrl_set_device() chose (defined in xrl_abi.cpp)
extern thread_local std::string g_err;
extern thread_local bool g_has_err;
extern thread_local int g_device;

void set_err(const std::string& s);

// Every entry point catches all C++ exceptions and records them for xrl_last_error(); nothing is ever thrown across the C boundary.
template <class F> void guarded(F&& fn) {
    g_has_err = false;
    try { fn(); }
    catch (const std::exception& e) { set_err(e.what()); }
    catch (...) { set_err("unknown error"); }
}

// ... for the entry points that return a value: fn()'s, or `on_error` after an exception
template <class T, class F> T guarded_value(T on_error, F&& fn) {
    guarded([&] { on_error = fn(); });
    return on_error;
}

Model* as_model(void* p);
void use_device(int dev);
void require_gpu();

// The caller's host X, CSR or dense row-major, as one view: built once at the entry point from ScipyCsrF32 / ScipyDrmF32.
struct HostX {
    bool given = false;                  // false: the caller passed a null X (reported where the arrays are first needed, as "null X")
    bool csr = false;
    uint32_t rows = 0, cols = 0;
    const uint64_t* row_ptr = nullptr;   // CSR only
    const uint32_t* col_idx = nullptr;   // CSR only
    const float* val = nullptr;
    HostX() = default;
    explicit HostX(const ScipyCsrF32* X) { if (X) { given = true; csr = true; rows = X->rows; cols = X->cols; row_ptr = X->row_ptr; col_idx = X->col_idx; val = X->val; } }
    explicit HostX(const ScipyDrmF32* X) { if (X) { given = true; rows = X->rows; cols = X->cols; val = X->val; } }
    // elements (CSR: (column id, value) pairs; dense: values) before row r, in all rows, and the bytes one of them takes on its way to the device
    uint64_t elem_at(uint32_t r) const { return csr ? row_ptr[r] : (uint64_t)r * cols; }
    uint64_t elems() const { return csr ? (rows ? row_ptr[rows] : 0) : (uint64_t)rows * cols; }
    uint32_t elem_bytes() const { return csr ? 8u : 4u; }
};

// The two forms of X on the device.  Every QueriesDev is made by one of them, so `dense`, `nnz` and the null CSR arrays of a dense X
// cannot disagree (k1q_row clamps with X.nnz).
inline QueriesDev csr_view(uint32_t rows, uint32_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const float* val, uint64_t nnz) {
    QueriesDev d{};
    d.row_ptr = row_ptr; d.col_idx = col_idx; d.val = val;
    d.rows = rows; d.cols = cols; d.dense = 0; d.nnz = nnz;
    return d;
}
inline QueriesDev dense_view(uint32_t rows, uint32_t cols, const float* val) {
    QueriesDev d{};
    d.val = val;
    d.rows = rows; d.cols = cols; d.dense = 1; d.nnz = 0;
    return d;
}
// ... of a host X whose device copy lives (or will live) in these buffers
inline QueriesDev device_view(const HostX& x, const DevBuf& ptr, const DevBuf& idx, const DevBuf& val) {
    return x.csr ? csr_view(x.rows, x.cols, ptr.as<uint64_t>(), idx.as<uint32_t>(), val.as<float>(), x.elems()) : dense_view(x.rows, x.cols, val.as<float>());
}

// The only writer of a handle's device and view: from a view of arrays it may or may not own ...
inline void set_view(Queries& q, int device, const QueriesDev& v) { q.device = device; q.dev = v; }
// ... or as a CSR of the q.own.nnz entries in its own buffers
inline void set_own_csr(Queries& q, int device, uint32_t rows, uint32_t cols) {
    set_view(q, device, csr_view(rows, cols, q.own.ptr.as<uint64_t>(), q.own.idx.as<uint32_t>(), q.own.val.as<float>(), q.own.nnz));
}

// A CSR matrix handle, named `name` in the refusals; `what` is the whole prefix of the message, its separator included.
inline const Queries& csr_handle(const std::string& what, const void* p, const std::string& name) {
    if (!p) fail(what + "null matrix handle (" + name + ")");
    const Queries& m = *static_cast<const Queries*>(p);
    if (m.dev.dense) fail(what + name + " must be a CSR handle");
    return m;
}

// synchronous upload of the whole X into the given buffers (dense X: `val` only; a CSR without rows: a zero ptr[0]); `d` describes the device copy
void upload_x(const HostX& x, DevBuf& ptr, DevBuf& idx, DevBuf& val, QueriesDev& d);

// What the xrl_queries_* and xrl_smat_* entry points share (xrl_abi.cpp), after their own argument checks: a host X as a handle on
// `device` that owns its copy; a CSR view into the caller's host arrays (synchronous); a handle's end, its buffers freed with their device set.
Queries* upload_handle(const HostX& x, int device);
void download_csr(const QueriesDev& v, uint64_t* row_ptr, uint32_t* col_idx, float* val);
void free_handle(void* h);

}  // namespace xrl
