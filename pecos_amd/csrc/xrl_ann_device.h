// Device code the ANN kernels share (K17 xrl_hnsw.hip, K18 xrl_pairwise.hip): libstdc++'s heaps restated over a pair of arrays, the two
// distance rules of the reference's FeatVec{Dense,Sparse}{IP,L2}Simd, and the checks of a query matrix.  Item rows are a
// dense base or a CSR, the query is a row; nothing here knows an index type.
#pragma once
#include "xrl_device.h"

namespace xrl {

enum : uint32_t { kBadOrder = 1u, kBadRange = 2u, kBadValue = 4u, kBadPtr = 8u };

__device__ __forceinline__ void wave_sync_mem() {          // LDS and HBM written by one lane, read by another of the same wavefront
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ uint32_t lane0(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ float lane0(float v) { return __uint_as_float(lane0(__float_as_uint(v))); }

// ---- libstdc++'s heaps (bits/stl_heap.h), over a pair of arrays; MAX: std::less (a max-heap), else std::greater.  The comparator reads the
// distance only, so __push_heap / __adjust_heap decide which of two equal distances leaves first.
template <bool MAX> __device__ __forceinline__ bool heap_comp(float a, float b) { return MAX ? a < b : a > b; }

template <bool MAX> __device__ __forceinline__ void heap_push_at(float* d, uint32_t* id, int hole, int top, float vd, uint32_t vi) {   // __push_heap
    int parent = (hole - 1) / 2;
    while (hole > top && heap_comp<MAX>(d[parent], vd)) {              // hole halves: at most the heap's depth
        d[hole] = d[parent]; id[hole] = id[parent];
        hole = parent; parent = (hole - 1) / 2;
    }
    d[hole] = vd; id[hole] = vi;
}
template <bool MAX> __device__ __forceinline__ void heap_adjust(float* d, uint32_t* id, int hole, int len, float vd, uint32_t vi) {    // __adjust_heap
    const int top = hole;
    int child = hole;
    while (child < (len - 1) / 2) {                                    // child doubles: at most the heap's depth
        child = 2 * (child + 1);
        if (heap_comp<MAX>(d[child], d[child - 1])) --child;
        d[hole] = d[child]; id[hole] = id[child];
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        d[hole] = d[child - 1]; id[hole] = id[child - 1];
        hole = child - 1;
    }
    heap_push_at<MAX>(d, id, hole, top, vd, vi);
}
// std::pop_heap over [0, n): the top goes to position n - 1
template <bool MAX> __device__ __forceinline__ void heap_pop(float* d, uint32_t* id, int n) {
    if (n > 1) {
        const float vd = d[n - 1]; const uint32_t vi = id[n - 1];
        d[n - 1] = d[0]; id[n - 1] = id[0];
        heap_adjust<MAX>(d, id, 0, n - 1, vd, vi);
    }
}

// ---- distances
// A NaN distance carries the host's default NaN.  The loaders and the check kernels admit finite values only, so no operand of either rule is
// ever a NaN of the caller's: every NaN is born of an invalid operation on finite or infinite values (inf + -inf), which an x86 host answers
// with 0xFFC00000 -- sign bit set -- and then carries unchanged through the later additions and the final (float)(1.0 - (double)s) or
// -2 * dot.  The device's default NaN is 0x7FC00000, and a negated operand flips a NaN's sign, so the bits are set once, at the end.  (K10's
// host_nan in xrl_spgemm.hip also hands on a caller's NaN payload; there is none to hand on here.)  The comparisons stay the reference's.
__device__ __forceinline__ float host_default_nan(float d) { return d == d ? d : __uint_as_float(0xFFC00000u); }

// Dense, the avx512f clone: called by all 64 lanes, the 16 lanes of a group share `node`; every lane of the group returns the distance.
// feat: the items' base, rows of feat_dim floats; q: the query's feat_dim floats (LDS or HBM).
__device__ __forceinline__ float dense_dist(const float* __restrict__ feat, uint32_t feat_dim, int l2, const float* __restrict__ q, uint32_t node, uint32_t lane) {
    const float* __restrict__ v = feat + (uint64_t)node * feat_dim;
    const uint32_t len = feat_dim, n16 = len / 16u, l = lane & 15u, jj = lane & 3u;
    const int base = (int)(lane & ~15u);
    float acc = 0.0f;
    for (uint32_t i = 0; i < n16; ++i) {                               // fused, lane l owns acc[l]
        const float x = q[16u * i + l], y = v[16u * i + l];
        if (l2) { const float df = __fsub_rn(x, y); acc = __fmaf_rn(df, df, acc); }
        else acc = __fmaf_rn(x, y, acc);
    }
    const float a0 = __shfl(acc, base + (int)jj), a1 = __shfl(acc, base + 4 + (int)jj), a2 = __shfl(acc, base + 8 + (int)jj), a3 = __shfl(acc, base + 12 + (int)jj);
    float qj = __fadd_rn(__fadd_rn(a0, a1), __fadd_rn(a2, a3));
    uint32_t k = n16 * 16u;
    for (; k + 4u <= len; k += 4u) {                                   // every further whole group of 4: NOT fused
        const float x = q[k + jj], y = v[k + jj];
        float p;
        if (l2) { const float df = __fsub_rn(x, y); p = __fmul_rn(df, df); }
        else p = __fmul_rn(x, y);
        qj = __fadd_rn(qj, p);
    }
    const float q0 = __shfl(qj, base), q1 = __shfl(qj, base + 1), q2 = __shfl(qj, base + 2), q3 = __shfl(qj, base + 3);
    float s = __fadd_rn(__fadd_rn(__fadd_rn(q0, q1), q2), q3);
    for (; k < len; ++k) {                                             // the last len % 4 elements: fused
        const float x = q[k], y = v[k];
        if (l2) { const float df = __fsub_rn(x, y); s = __fmaf_rn(df, df, s); }
        else s = __fmaf_rn(x, y, s);
    }
    return host_default_nan(l2 ? s : (float)(1.0 - (double)s));
}

// Sparse: one lane merges the query's entries [qb, qe) of (q_idx, q_val) with row `node` of the items' CSR; the products of the matching ids are
// added one by one in ascending id order.  l2 is the reference's x_sq + y_sq - 2 * dot with both squares 0 (it measures each vector against
// itself): -2 * dot.
__device__ __forceinline__ float sparse_dist(const uint64_t* __restrict__ row_ptr, const uint32_t* __restrict__ idx, const float* __restrict__ val, int l2,
                                             const uint32_t* q_idx, const float* q_val, uint64_t qb, uint64_t qe, uint32_t node) {
    uint64_t ib = row_ptr[node];
    const uint64_t ie = row_ptr[node + 1];
    float dot = 0.0f;
    while (qb < qe && ib < ie) {                                       // at most the two rows' lengths
        const uint32_t x = q_idx[qb], y = idx[ib];
        if (x == y) { dot = __fadd_rn(dot, __fmul_rn(q_val[qb], val[ib])); ++qb; ++ib; }
        else if (x < y) ++qb;
        else ++ib;
    }
    return host_default_nan(l2 ? (float)((double)__fadd_rn(0.0f, 0.0f) - 2.0 * (double)dot) : (float)(1.0 - (double)dot));
}

// ---- checks of a matrix, by a grid of 256-thread blocks; the flags of what the calling thread met
// CSR rows: ids strictly ascending and below cols, values finite, row pointers ascending and within nnz
__device__ __forceinline__ uint32_t check_csr_rows(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const float* __restrict__ val, uint32_t rows,
                                                   uint32_t cols, uint64_t nnz) {
    uint32_t f = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * 256u) {
        const uint64_t b = ptr[r], e = ptr[r + 1];
        if (b > e || e > nnz) { f |= kBadPtr; continue; }
        for (uint64_t p = b; p < e; ++p) {
            if (idx[p] >= cols) f |= kBadRange;
            if (p > b && idx[p] <= idx[p - 1]) f |= kBadOrder;
            if ((__float_as_uint(val[p]) & 0x7F800000u) == 0x7F800000u) f |= kBadValue;
        }
    }
    return f;
}
__device__ __forceinline__ uint32_t check_drm_rows(const float* __restrict__ val, uint32_t rows, uint32_t cols, uint64_t stride) {
    const uint64_t n = (uint64_t)rows * cols;
    uint32_t f = 0;
    for (uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x; x < n; x += (uint64_t)gridDim.x * 256u) {
        const uint64_t r = x / cols, c = x % cols;
        if ((__float_as_uint(val[r * stride + c]) & 0x7F800000u) == 0x7F800000u) f |= kBadValue;
    }
    return f;
}

}  // namespace xrl
