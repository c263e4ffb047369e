// The kernels more than one family uses (xrl_devprim.h): the single-block scan of the counting sorts and of K1G's block starts, and the
// row copy that ends K9's batches, K10's fixed-stride result -> CSR and K12's hstack.
#include "xrl_devprim.h"
#include "xrl_kernels.h"

namespace xrl {

namespace {

// single block: exclusive scan of v[0..n) in place; v[n] = grand total
__global__ void __launch_bounds__(1024) block_scan_kernel(uint32_t* __restrict__ v, uint32_t n) {
    __shared__ uint32_t part[1024];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t x = i < n ? v[i] : 0u;
        part[threadIdx.x] = x;
        __syncthreads();
        for (uint32_t off = 1; off < 1024; off <<= 1) {
            const uint32_t t = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
            __syncthreads();
            part[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < n) v[i] = carry + part[threadIdx.x] - x;
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) v[n] = carry;
}

// dst = ptr[r].  The row's length and source: ptr[r + 1] - ptr[r] pairs from src_off[r] or r * stride; with len_ptr (hstack) row r of the
// CSR (len_ptr, s_idx, s_val) of len_nnz entries, clamped to them.  col_add is added to every id.
__global__ void __launch_bounds__(256)
copy_rows_kernel(const uint64_t* __restrict__ ptr, uint64_t rows, const uint64_t* __restrict__ src_off, uint32_t stride, const uint32_t* __restrict__ s_idx,
                 const float* __restrict__ s_val, uint32_t* __restrict__ idx, float* __restrict__ val, const uint64_t* __restrict__ len_ptr, uint64_t len_nnz,
                 uint32_t col_add) {
    const uint64_t r = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= rows) return;
    const uint64_t dst = ptr[r];
    uint64_t src, n;
    if (len_ptr) {
        const uint64_t e0 = len_ptr[r + 1], b0 = len_ptr[r], e = e0 < len_nnz ? e0 : len_nnz;
        src = b0 < e ? b0 : e; n = e - src;
    } else {
        const uint64_t len = ptr[r + 1] - dst;
        src = src_off ? src_off[r] : r * stride; n = src_off ? len : min(len, (uint64_t)stride);
    }
    for (uint64_t x = threadIdx.x & 63u; x < n; x += 64u) { idx[dst + x] = s_idx[src + x] + col_add; val[dst + x] = s_val[src + x]; }
}

}  // namespace

void launch_block_scan(uint32_t* v, uint32_t n, hipStream_t s) { hipLaunchKernelGGL(block_scan_kernel, dim3(1), dim3(1024), 0, s, v, n); }

void launch_copy_rows(const uint64_t* ptr, uint64_t rows, const uint64_t* src_off, uint32_t stride, const uint32_t* s_idx, const float* s_val,
                      uint32_t* idx, float* val, const char* what, hipStream_t s) {
    hipLaunchKernelGGL(copy_rows_kernel, dim3(blocks_of(rows, 4, what)), dim3(256), 0, s, ptr, rows, src_off, stride, s_idx, s_val, idx, val,
                       (const uint64_t*)nullptr, (uint64_t)0, 0u);
    XRL_LAUNCH_CHECK();
}

void launch_copy_csr_rows(const uint64_t* dst, uint64_t rows, const uint64_t* s_ptr, const uint32_t* s_idx, const float* s_val, uint64_t s_nnz, uint32_t col_add,
                          uint32_t* idx, float* val, const char* what, hipStream_t s) {
    hipLaunchKernelGGL(copy_rows_kernel, dim3(blocks_of(rows, 4, what)), dim3(256), 0, s, dst, rows, (const uint64_t*)nullptr, 0u, s_idx, s_val, idx, val, s_ptr,
                       s_nnz, col_add);
    XRL_LAUNCH_CHECK();
}

}  // namespace xrl
