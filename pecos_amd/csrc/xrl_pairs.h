// Device half of the CSC route that the pair kernels share (xrl_pairs.hip: K3, K4, K1C; xrl_select_plan.hip: K4 on the planned slots of K7):
// one (query row, weight column) inner product per group of PG = 16 lanes, against W in CSC form.
//
// Arithmetic contract of the CSC route (vector_ops::inner_product, inference.hpp:1018-1078), bit for bit:
//   sparse X:  res = 0;  res += fl32(bias * w_bias) if the column's last entry is the bias row;  res += dot
//              where dot = 0, then dot = fl32(dot + fl32(x_f * w_f)) over the matching indices in ASCENDING order
//              (do_dot_product, matrix.hpp:836-859: summed separately, then added -- unlike the chunked route)
//   dense X:   bias > 0:  res = fl32(bias * w_bias) first, then res = fl32(res + fl32(x[idx] * w)) over the non-bias
//              entries in order;  bias <= 0: the same chain over all entries
//
// The 16 lanes of a group read 16 consecutive entries of the SHORTER index list per step (coalesced 64-byte segments), each lane binary-
// searches its index in the longer list, and the matches' products -- computed in parallel -- are folded into the running
// sum in lane order, which is ascending index order: the same chain of fp32 additions the reference performs.
#pragma once
#include <hip/hip_runtime.h>

#include "xrl_device.h"
#include "xrl_kernels.h"

namespace xrl {

constexpr int PG = 16;            // lanes per pair
constexpr int PAIRS_PER_BLOCK = 256 / PG;

// acc = fl32(acc + p_b) for the lanes b of this group whose bit is set in gm, in lane order
__device__ __forceinline__ float fold_in_lane_order(float acc, float prod, uint32_t gm, int gbase) {
    float p[PG];
#pragma unroll
    for (int b = 0; b < PG; ++b) p[b] = __shfl(prod, gbase + b, 64);   // independent of the chain: all in flight together
#pragma unroll
    for (int b = 0; b < PG; ++b) { const float s = __fadd_rn(acc, p[b]); acc = ((gm >> b) & 1u) ? s : acc; }
    return acc;
}

// do_dot_product(sparse, sparse), matrix.hpp:836-859: matches in ascending index order, ret starts at 0
__device__ __forceinline__ float dot_sparse_sparse(const uint32_t* __restrict__ xi, const float* __restrict__ xv, uint32_t xn,
                                                   const uint32_t* __restrict__ wi, const float* __restrict__ wv, uint32_t wn,
                                                   int lig, int gbase) {
    // stream the shorter list, search the longer one (the set of matches and their order do not depend on the choice)
    const bool sx = xn <= wn;
    const uint32_t* __restrict__ ai = sx ? xi : wi; const float* __restrict__ av = sx ? xv : wv; const uint32_t an = sx ? xn : wn;
    const uint32_t* __restrict__ bi = sx ? wi : xi; const float* __restrict__ bv = sx ? wv : xv; const uint32_t bn = sx ? wn : xn;
    float dot = 0.0f;
    for (uint32_t c0 = 0; c0 < an; c0 += PG) {
        const uint32_t t = c0 + (uint32_t)lig;
        const bool ok = t < an;
        const uint32_t key = ai[ok ? t : 0u];
        const float a = av[ok ? t : 0u];
        const uint32_t pos = ok && bn ? lower_bound(bi, bn, key) : bn;
        const bool hit = pos < bn && bi[pos] == key;
        const float prod = hit ? __fmul_rn(a, bv[pos]) : 0.0f;
        const uint32_t gm = (uint32_t)(__ballot(hit) >> gbase) & 0xFFFFu;
        if (gm) dot = fold_in_lane_order(dot, prod, gm, gbase);
    }
    return dot;
}

// The same walk CONTINUING a running value: acc = fl32(acc + fl32(x_f * w_f)) over the matching indices in ascending order -- the chunked
// route's single chain (chunk_ops<csr, *>, inference.hpp:705-735, 769-813), where the products join the sum the bias may already be part of
__device__ __forceinline__ float chain_sparse_sparse(float acc, const uint32_t* __restrict__ xi, const float* __restrict__ xv, uint32_t xn,
                                                     const uint32_t* __restrict__ wi, const float* __restrict__ wv, uint32_t wn,
                                                     int lig, int gbase) {
    const bool sx = xn <= wn;
    const uint32_t* __restrict__ ai = sx ? xi : wi; const float* __restrict__ av = sx ? xv : wv; const uint32_t an = sx ? xn : wn;
    const uint32_t* __restrict__ bi = sx ? wi : xi; const float* __restrict__ bv = sx ? wv : xv; const uint32_t bn = sx ? wn : xn;
    for (uint32_t c0 = 0; c0 < an; c0 += PG) {
        const uint32_t t = c0 + (uint32_t)lig;
        const bool ok = t < an;
        const uint32_t key = ai[ok ? t : 0u];
        const float a = av[ok ? t : 0u];
        const uint32_t pos = ok && bn ? lower_bound(bi, bn, key) : bn;
        const bool hit = pos < bn && bi[pos] == key;
        const float prod = hit ? __fmul_rn(a, bv[pos]) : 0.0f;
        const uint32_t gm = (uint32_t)(__ballot(hit) >> gbase) & 0xFFFFu;
        if (gm) acc = fold_in_lane_order(acc, prod, gm, gbase);
    }
    return acc;
}

// res = fl32(res + fl32(x[idx_s] * w_s)) over s in [0, n) in order: do_dot_product(dense, sparse) / the dense-X bias-first loop
__device__ __forceinline__ float chain_dense_x(float res, const float* __restrict__ x, uint32_t x_cols, const uint32_t* __restrict__ wi,
                                               const float* __restrict__ wv, uint32_t n, int lig, int gbase) {
    for (uint32_t c0 = 0; c0 < n; c0 += PG) {
        const uint32_t t = c0 + (uint32_t)lig;
        const bool ok = t < n;
        const uint32_t f = wi[ok ? t : 0u];
        const float prod = ok ? __fmul_rn(f < x_cols ? x[f] : 0.0f, wv[t]) : 0.0f;
        const uint32_t cnt = min((uint32_t)PG, n - c0);
        res = fold_in_lane_order(res, prod, cnt >= 16 ? 0xFFFFu : ((1u << cnt) - 1u), gbase);
    }
    return res;
}

struct CscDev { const uint64_t* col_ptr; const uint32_t* row_idx; const float* val; uint32_t w_rows; float bias; };

// vector_ops::inner_product for column j (original column id) against query row q
__device__ __forceinline__ float csc_route_product(const CscDev& W, const QueriesDev& X, uint64_t q, uint32_t j, int lig, int gbase) {
    const uint64_t cb = W.col_ptr[j], ce = W.col_ptr[j + 1];
    const uint32_t wn = (uint32_t)(ce - cb);
    const uint32_t* __restrict__ wi = W.row_idx + cb; const float* __restrict__ wv = W.val + cb;
    const bool use_bias = W.bias > 0.0f;
    const bool has_b = use_bias && wn > 0 && wi[wn - 1] == W.w_rows - 1;
    float res = 0.0f;
    if (has_b) res = __fadd_rn(res, __fmul_rn(W.bias, wv[wn - 1]));
    if (X.dense) {
        const float* __restrict__ x = X.val + q * X.cols;
        return chain_dense_x(res, x, X.cols, wi, wv, (use_bias && has_b) ? wn - 1 : wn, lig, gbase);
    }
    const uint64_t xb = X.row_ptr[q];
    const uint32_t xn = (uint32_t)(X.row_ptr[q + 1] - xb);
    return __fadd_rn(res, dot_sparse_sparse(X.col_idx + xb, X.val + xb, xn, wi, wv, wn, lig, gbase));
}

// The CHUNKED routes' arithmetic for column j against query row q, from the CSC copy of W (oracle/xrl_oracle.c
// orc_layer_predict).  Sparse X: one chain from +0.0 over the matching features in ascending order, the bias product -- only for a column
// that holds a bias entry -- LAST (BINARY_SEARCH_CHUNKED) or FIRST (HASH_CHUNKED, bias_first).  Dense X is bias first, then every entry of
// the column in order, in every layout: csc_route_product's dense branch.
__device__ __forceinline__ float chunked_route_product(const CscDev& W, const QueriesDev& X, uint64_t q, uint32_t j, int bias_first, int lig, int gbase) {
    if (X.dense) return csc_route_product(W, X, q, j, lig, gbase);
    const uint64_t cb = W.col_ptr[j], ce = W.col_ptr[j + 1];
    const uint32_t wn = (uint32_t)(ce - cb);
    const uint32_t* __restrict__ wi = W.row_idx + cb; const float* __restrict__ wv = W.val + cb;
    const bool has_b = W.bias > 0.0f && wn > 0 && wi[wn - 1] == W.w_rows - 1;
    const float bprod = has_b ? __fmul_rn(W.bias, wv[wn - 1]) : 0.0f;
    float acc = 0.0f;
    if (has_b && bias_first) acc = __fadd_rn(acc, bprod);
    const uint64_t xb = X.row_ptr[q];
    acc = chain_sparse_sparse(acc, X.col_idx + xb, X.val + xb, (uint32_t)(X.row_ptr[q + 1] - xb), wi, wv, has_b ? wn - 1 : wn, lig, gbase);
    if (has_b && !bias_first) acc = __fadd_rn(acc, bprod);
    return acc;
}

}  // namespace xrl
