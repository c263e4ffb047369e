// The building blocks the producers of a CSR in HBM share (K9 xrl_tokenize.hip, K10 xrl_spgemm.hip, the output constraint, the big K2):
// grid sizes, rocPRIM's two-call form, the exclusive scan with or without its total on the host, and the copy of rows of (u32, f32)
// pairs (xrl_devprim.hip, which also holds the single-block scan of the counting sorts, declared in xrl_kernels.h).  The device-side
// pieces -- lanes_below, lower_bound, segment_of -- are in xrl_device.h.
#pragma once
#include <rocprim/device/device_scan.hpp>

#include "xrl_common.h"

namespace xrl {

// workgroups of `per` elements that cover n; `what` names the family in the message
inline uint32_t blocks_of(uint64_t n, uint32_t per, const char* what) {
    const uint64_t b = (n + per - 1) / per;
    if (b > 0x7FFFFFFFull) fail(std::string(what) + ": grid too large");
    return (uint32_t)b;
}

// rocPRIM's two calls: call(nullptr, bytes) sizes the temporary storage, call(tmp.p, bytes) runs with it
template <class F> void with_rocprim_tmp(DevBuf& tmp, F&& call) {
    size_t bytes = 0;
    XRL_HIP(call(nullptr, bytes));
    tmp.reserve(bytes);
    XRL_HIP(call(tmp.p, bytes));
}

template <class T> void exclusive_scan(DevBuf& tmp, const T* in, T* out, size_t n, hipStream_t s) {
    with_rocprim_tmp(tmp, [&](void* t, size_t& bytes) { return rocprim::exclusive_scan(t, bytes, in, out, T(0), n, rocprim::plus<T>(), s); });
}

// counts in[0, n) (in[n] may hold anything) -> offsets out[0, n], and the total out[n] on the host: one copy, one synchronise of s
template <class T> T scan_total(DevBuf& tmp, const T* in, T* out, size_t n, hipStream_t s) {
    T total = 0;
    exclusive_scan(tmp, in, out, n + 1, s);
    XRL_HIP(hipMemcpyAsync(&total, out + n, sizeof(T), hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    return total;
}

// One wavefront per row r copies the row's ptr[r + 1] - ptr[r] pairs to ptr[r], from src_off[r] or, with src_off null, from r * stride
// (then a row holds at most stride).  Checks the launch.
void launch_copy_rows(const uint64_t* ptr, uint64_t rows, const uint64_t* src_off, uint32_t stride, const uint32_t* s_idx, const float* s_val,
                      uint32_t* idx, float* val, const char* what, hipStream_t s);
// The same copy loop for hstack (K12): row r of the CSR (s_ptr, s_idx, s_val) of s_nnz entries, its span clamped to them, goes to dst[r]
// with col_add added to every column id.
void launch_copy_csr_rows(const uint64_t* dst, uint64_t rows, const uint64_t* s_ptr, const uint32_t* s_idx, const float* s_val, uint64_t s_nnz, uint32_t col_add,
                          uint32_t* idx, float* val, const char* what, hipStream_t s);

}  // namespace xrl
