// K10: Z = A * B, both CSR, with the reference's smat_x_smat arithmetic (matrix.hpp:1075-1292): per output row the products a * b in the
// order of the (s, t) walk -- s over the stored entries of A's row, t over the stored entries of the B row entry s names -- added to their
// column's accumulator one after the other (__fmul_rn, then __fadd_rn from +0; a NaN result takes the bits the reference's host gives
// it), no FMA, no float atomics.
//
//   k10_flops        F_i = the products of row i (thread per row); counts the rows above CAP; flags an entry of A outside B's rows
//   k10_lds<FILL>    one wavefront per row with F_i <= CAP (xrl_spgemm.h).  64 entries of A a step: their B row lengths are prefix-summed
//                    over the lanes, then the lanes take the step's products 64 at a time (a product finds its entry by bisection of the 64
//                    offsets) and write (column << 32 | q) and a * b to LDS, q = the product's sequence number.  A bitonic sort of the
//                    keys; a lane whose key starts a column's run walks the run -- ascending q, the reference's order of additions -- and
//                    owns the sum.  Output slot: the run's rank by column (sorted_indices) or by first q (first touch; a bitmap of the
//                    first q's, ranked by popcount).  FILL = false only counts the runs.
//   big form         rows above CAP, in batches under the scratch budget: k10_big_expand writes the keys and products to HBM, one rocPRIM
//                    segmented radix sort of the 64-bit keys (no reliance on stability), k10_big_flags marks the run heads at their
//                    output rank's position, an exclusive scan ranks them, k10_big_cnt / k10_big_fill count / sum and write.
//   counts -> exclusive scan (u64) -> fill; eliminate_zeros is one more counted, scanned and copied pass (k10_nz<FILL>).
//   k10_topk_cnt, then the shared row copy (xrl_devprim.h): a fixed-stride result as a CSR.
//
// Bounds: every row span is clamped to the operand's nnz; an LDS index is below CAP and a scratch index below its row's share before the
// write; an output index is below the row's end in the scanned row pointer.
#include "xrl_spgemm.h"
#include "xrl_device.h"
#include "xrl_devprim.h"
#include "xrl_predict.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace xrl {

namespace {

constexpr const char* kWhat = "sparse_matmul";         // the family in a "grid too large" message

struct K10Args {
    const uint64_t* a_ptr; const uint32_t* a_col; const float* a_val; uint64_t a_nnz;
    const uint64_t* b_ptr; const uint32_t* b_col; const float* b_val; uint64_t b_nnz;
    uint32_t rows, inner, row0;
    int sorted;
    const uint64_t* flops;                                 // [rows]
    uint64_t* cnt;                                         // [rows + 1] the count passes' output
    const uint64_t* out_ptr; uint32_t* out_col; float* out_val;   // the fill passes' output
};

// The NaN the reference's host (x86 SSE) leaves: a NaN operand comes back quieted, the first operand's first; an invalid operation
// (0 * inf, inf - inf) gives the default NaN, whose sign bit is set.  r = x op y as the device computed it.
__device__ __forceinline__ float host_nan(float r, float x, float y) {
    if (r == r) return r;
    if (x != x) return __uint_as_float(__float_as_uint(x) | 0x00400000u);
    if (y != y) return __uint_as_float(__float_as_uint(y) | 0x00400000u);
    return __uint_as_float(0xFFC00000u);
}
__device__ __forceinline__ float ref_mul(float a, float b) { return host_nan(__fmul_rn(a, b), a, b); }
__device__ __forceinline__ float ref_add(float acc, float p) { return host_nan(__fadd_rn(acc, p), acc, p); }

__global__ void __launch_bounds__(256) k10_flops(K10Args a, uint64_t* __restrict__ flops, unsigned long long* __restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.rows) return;
    uint64_t ab, ae, f = 0;
    row_span(a.a_ptr, i, a.a_nnz, ab, ae);
    bool bad = false;
    for (uint64_t s = ab; s < ae; ++s) {
        const uint32_t k = a.a_col[s];
        if (k >= a.inner) { bad = true; continue; }
        uint64_t kb, ke;
        row_span(a.b_ptr, k, a.b_nnz, kb, ke);
        f += ke - kb;
    }
    flops[i] = f;
    if (f > kSpgemmCap) atomicAdd(&words[0], 1ull);
    if (f >= (1ull << 31)) atomicMax(&words[2], 1ull);
    if (bad) atomicMax(&words[1], 1ull);
}

template <bool FILL>
__global__ void __launch_bounds__(64) k10_lds(K10Args a) {
    __shared__ uint64_t s_key[kSpgemmCap];
    __shared__ float s_val[FILL ? kSpgemmCap : 1];
    __shared__ uint64_t s_kb[64];
    __shared__ uint32_t s_off[64];
    __shared__ float s_a[64];
    __shared__ uint32_t s_bm[kSpgemmCap / 32];
    const uint32_t lane = threadIdx.x;
    const uint64_t i = (uint64_t)a.row0 + blockIdx.x;
    const uint64_t F = a.flops[i];
    if (F == 0 || F > kSpgemmCap) return;                  // (the counts start at zero; the big form serves the rows above CAP)

    // ---- products, in the order of the (s, t) walk
    uint64_t ab, ae;
    row_span(a.a_ptr, i, a.a_nnz, ab, ae);
    uint32_t q = 0;
    for (uint64_t s0 = ab; s0 < ae; s0 += 64u) {
        const uint64_t s = s0 + lane;
        uint64_t kb = 0;
        uint32_t len = 0;
        float av = 0.0f;
        if (s < ae) {
            const uint32_t k = a.a_col[s];
            av = a.a_val[s];
            if (k < a.inner) {
                uint64_t ke;
                row_span(a.b_ptr, k, a.b_nnz, kb, ke);
                len = (uint32_t)min(ke - kb, (uint64_t)kSpgemmCap + 1u);   // (F <= CAP: every length is; the clamp keeps the sums small whatever the arrays hold)
            }
        }
        uint32_t incl = len;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += t;
        }
        const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
        if (total == 0) continue;                          // (uniform)
        s_off[lane] = incl - len; s_kb[lane] = kb; s_a[lane] = av;
        __syncthreads();                                   // one wavefront per workgroup
        for (uint32_t p0 = 0; p0 < total; p0 += 64u) {
            const uint32_t p = p0 + lane, qq = q + p;
            if (p < total && qq < kSpgemmCap) {
                const uint32_t lo = segment_of(s_off, 64u, p);             // the last entry whose products start at or before p
                const uint64_t at = s_kb[lo] + (p - s_off[lo]);
                s_key[qq] = ((uint64_t)a.b_col[at] << 32) | qq;
                if (FILL) s_val[qq] = ref_mul(s_a[lo], a.b_val[at]);
            }
        }
        q += total;
        __syncthreads();
    }
    const uint32_t nf = min(q, kSpgemmCap);
    if (nf == 0) return;

    // ---- order by (column, q)
    uint32_t P = 64;
    while (P < nf) P <<= 1;
    for (uint32_t x = nf + lane; x < P; x += 64u) s_key[x] = ~0ull;             // (q < CAP: no key is all ones)
    if (lane < kSpgemmCap / 32) s_bm[lane] = 0u;
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < P / 2; t += 64u) {
                const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
                const uint64_t x = s_key[lo], y = s_key[hi];
                if ((x > y) == ((lo & k) == 0)) { s_key[lo] = y; s_key[hi] = x; }
            }
            __syncthreads();
        }

    // ---- runs: their number, and (first touch order) the bitmap of their first q
    if (!FILL || !a.sorted) {
        uint32_t nr = 0;
        for (uint32_t x0 = 0; x0 < nf; x0 += 64u) {
            const uint32_t x = x0 + lane;
            const bool head = x < nf && (x == 0 || (uint32_t)(s_key[x] >> 32) != (uint32_t)(s_key[x - 1] >> 32));
            if (FILL && head) { const uint32_t q0 = (uint32_t)s_key[x]; atomicOr(&s_bm[q0 >> 5], 1u << (q0 & 31u)); }
            nr += (uint32_t)__popcll(__ballot(head));
        }
        if (!FILL) { if (lane == 0) a.cnt[i] = nr; return; }
        __syncthreads();
    }

    // ---- every run summed by the lane that holds its head, in ascending q
    const uint64_t base = a.out_ptr[i], end = a.out_ptr[i + 1];
    uint32_t r0 = 0;
    for (uint32_t x0 = 0; x0 < nf; x0 += 64u) {
        const uint32_t x = x0 + lane;
        const bool head = x < nf && (x == 0 || (uint32_t)(s_key[x] >> 32) != (uint32_t)(s_key[x - 1] >> 32));
        const unsigned long long m = __ballot(head);
        if (head) {
            const uint64_t k0 = s_key[x];
            const uint32_t col = (uint32_t)(k0 >> 32), q0 = (uint32_t)k0;
            float acc = 0.0f;
            uint32_t j = x;
            do { acc = ref_add(acc, s_val[(uint32_t)s_key[j] & (kSpgemmCap - 1u)]); ++j; } while (j < nf && (uint32_t)(s_key[j] >> 32) == col);
            uint32_t slot;
            if (a.sorted) slot = r0 + lanes_below(m);
            else {
                const uint32_t w = q0 >> 5;
                slot = (uint32_t)__popc(s_bm[w] & ((1u << (q0 & 31u)) - 1u));
                for (uint32_t y = 0; y < w; ++y) slot += (uint32_t)__popc(s_bm[y]);
            }
            if (base + slot < end) { a.out_col[base + slot] = col; a.out_val[base + slot] = acc; }
        }
        r0 += (uint32_t)__popcll(m);
    }
}

// ---- big form
// one workgroup per row of the batch: key (column << 32 | q) and, for the fill, the product of every (s, t), at the row's offset
__global__ void __launch_bounds__(256)
k10_big_expand(K10Args a, const uint32_t* __restrict__ big_row, const uint32_t* __restrict__ off, uint64_t* __restrict__ keys, float* __restrict__ prod) {
    const uint32_t sg = blockIdx.x;
    const uint64_t i = big_row[sg];
    const uint32_t base = off[sg], lim = off[sg + 1] - base;
    uint64_t ab, ae, q = 0;
    row_span(a.a_ptr, i, a.a_nnz, ab, ae);
    for (uint64_t s = ab; s < ae; ++s) {
        const uint32_t k = a.a_col[s];
        if (k >= a.inner) continue;
        const float av = a.a_val[s];
        uint64_t kb, ke;
        row_span(a.b_ptr, k, a.b_nnz, kb, ke);
        const uint64_t len = ke - kb;
        for (uint64_t t = threadIdx.x; t < len; t += 256u) {
            const uint64_t qq = q + t;
            if (qq < lim) {
                keys[base + qq] = ((uint64_t)a.b_col[kb + t] << 32) | qq;
                if (prod) prod[base + qq] = ref_mul(av, a.b_val[kb + t]);
            }
        }
        q += len;
    }
}

// flag <- 1 at the position whose exclusive scan is the run's output rank: the head's own (by column) or its row's offset + first q
__global__ void __launch_bounds__(256)
k10_big_flags(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ off, uint32_t n_seg, uint32_t total, int sorted, uint32_t* __restrict__ flag) {
    const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (x >= total) return;
    const uint32_t sg = segment_of(off, n_seg, (uint32_t)x), b = off[sg];
    if (x != b && (uint32_t)(keys[x] >> 32) == (uint32_t)(keys[x - 1] >> 32)) return;
    const uint32_t pos = sorted ? (uint32_t)x : b + (uint32_t)keys[x];
    if (pos < off[sg + 1]) flag[pos] = 1u;
}

__global__ void __launch_bounds__(256)
k10_big_cnt(const uint32_t* __restrict__ slot, const uint32_t* __restrict__ big_row, const uint32_t* __restrict__ off, uint32_t n_seg, uint64_t* __restrict__ cnt) {
    const uint32_t sg = blockIdx.x * 256u + threadIdx.x;
    if (sg < n_seg) cnt[big_row[sg]] = slot[off[sg + 1]] - slot[off[sg]];
}

// the thread at a run's head walks the run (ascending q) and writes the sum at the run's rank
__global__ void __launch_bounds__(256)
k10_big_fill(K10Args a, const uint64_t* __restrict__ keys, const float* __restrict__ prod, const uint32_t* __restrict__ slot, const uint32_t* __restrict__ big_row,
             const uint32_t* __restrict__ off, uint32_t n_seg, uint32_t total) {
    const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (x >= total) return;
    const uint32_t sg = segment_of(off, n_seg, (uint32_t)x), b = off[sg], e = off[sg + 1];
    const uint32_t col = (uint32_t)(keys[x] >> 32);
    if (x != b && col == (uint32_t)(keys[x - 1] >> 32)) return;
    float acc = 0.0f;
    uint64_t j = x;
    do {
        const uint32_t qj = (uint32_t)keys[j];
        if (b + qj < e) acc = ref_add(acc, prod[b + qj]);
        ++j;
    } while (j < e && (uint32_t)(keys[j] >> 32) == col);
    const uint32_t pos = a.sorted ? (uint32_t)x : b + (uint32_t)keys[x];
    if (pos >= e) return;
    const uint64_t i = big_row[sg];
    const uint64_t at = a.out_ptr[i] + (slot[pos] - slot[b]);
    if (at < a.out_ptr[i + 1]) { a.out_col[at] = col; a.out_val[at] = acc; }
}

// ---- eliminate_zeros: one wavefront per row keeps the entries with val != 0 (NaN stays) in their order
template <bool FILL>
__global__ void __launch_bounds__(256)
k10_nz(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ col, const float* __restrict__ val, uint64_t rows, uint64_t* __restrict__ cnt,
       const uint64_t* __restrict__ e_ptr, uint32_t* __restrict__ e_col, float* __restrict__ e_val) {
    const uint64_t r = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= rows) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t b = ptr[r], e = ptr[r + 1];
    uint64_t n = 0;
    const uint64_t dst = FILL ? e_ptr[r] : 0, dst_end = FILL ? e_ptr[r + 1] : 0;
    for (uint64_t x0 = b; x0 < e; x0 += 64u) {
        const uint64_t x = x0 + lane;
        const float v = x < e ? val[x] : 0.0f;
        const bool keep = x < e && v != 0.0f;
        const unsigned long long m = __ballot(keep);
        if (FILL && keep) {
            const uint64_t at = dst + n + lanes_below(m);
            if (at < dst_end) { e_col[at] = col[x]; e_val[at] = v; }
        }
        n += (uint64_t)__popcll(m);
    }
    if (!FILL && lane == 0) cnt[r] = n;
}

// ---- fixed-stride result -> CSR
__global__ void __launch_bounds__(256) k10_topk_cnt(const uint32_t* __restrict__ d_cnt, uint32_t stride, uint64_t rows, uint64_t* __restrict__ cnt) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r < rows) cnt[r] = d_cnt ? min(d_cnt[r], stride) : stride;
}

constexpr uint32_t kLdsGridRows = 1u << 30;                // rows of one launch of the LDS form

template <bool FILL> void launch_lds(K10Args a, hipStream_t s) {
    for (uint64_t r0 = 0; r0 < a.rows; r0 += kLdsGridRows) {
        a.row0 = (uint32_t)r0;
        const uint32_t n = (uint32_t)std::min<uint64_t>(kLdsGridRows, a.rows - r0);
        hipLaunchKernelGGL(k10_lds<FILL>, dim3(n), dim3(64), 0, s, a);
        XRL_LAUNCH_CHECK();
    }
}

// The big form over all its rows, batch by batch: fill = false writes a.cnt of every big row, fill = true their entries.
struct BigScratch { DevBuf row, off, keys, keys2, prod, flag, slot, tmp; };

uint64_t run_big(K10Args a, const std::vector<uint32_t>& big, const std::vector<uint64_t>& F, bool fill, hipStream_t s, BigScratch& B) {
    uint64_t budget = 0;
    if (const char* e = std::getenv("XRL_SPGEMM_SCRATCH_PRODUCTS")) budget = std::strtoull(e, nullptr, 10);   // (tests: a small budget cuts few rows into batches)
    if (!budget) budget = kCandBudgetBytes / kSpgemmBigBytesPerProduct;
    uint64_t batches = 0;
    std::vector<uint32_t> row, off;
    for (size_t g0 = 0; g0 < big.size();) {
        row.clear(); off.assign(1, 0u);
        size_t g1 = g0;
        while (g1 < big.size()) {
            const uint64_t f = F[big[g1]];
            if (g1 > g0 && (uint64_t)off.back() + f > budget) break;       // (a single row above the budget is a batch of its own; f < 2^31)
            if ((uint64_t)off.back() + f > 0xFFFFFFF0ull) break;
            row.push_back(big[g1]); off.push_back(off.back() + (uint32_t)f);
            ++g1;
        }
        const uint32_t n_seg = (uint32_t)row.size(), total = off.back();
        if (batches) XRL_HIP(hipStreamSynchronize(s));     // the uploads reuse the buffers the last batch's kernels read
        B.row.upload(row); B.off.upload(off);
        B.keys.reserve((size_t)total * 8); B.keys2.reserve((size_t)total * 8);
        if (fill) B.prod.reserve((size_t)total * 4);
        B.flag.reserve(((size_t)total + 1) * 4); B.slot.reserve(((size_t)total + 1) * 4);
        const uint32_t* d_row = B.row.as<uint32_t>(); const uint32_t* d_off = B.off.as<uint32_t>();
        hipLaunchKernelGGL(k10_big_expand, dim3(n_seg), dim3(256), 0, s, a, d_row, d_off, B.keys.as<uint64_t>(), fill ? B.prod.as<float>() : nullptr);
        XRL_LAUNCH_CHECK();
        with_rocprim_tmp(B.tmp, [&](void* t, size_t& bytes) {
            return rocprim::segmented_radix_sort_keys(t, bytes, B.keys.as<uint64_t>(), B.keys2.as<uint64_t>(), total, n_seg, d_off, d_off + 1, 0u, 64u, s);
        });
        XRL_HIP(hipMemsetAsync(B.flag.p, 0, ((size_t)total + 1) * 4, s));
        hipLaunchKernelGGL(k10_big_flags, dim3(blocks_of(total, 256, kWhat)), dim3(256), 0, s, B.keys2.as<uint64_t>(), d_off, n_seg, total, a.sorted, B.flag.as<uint32_t>());
        XRL_LAUNCH_CHECK();
        exclusive_scan(B.tmp, B.flag.as<uint32_t>(), B.slot.as<uint32_t>(), (size_t)total + 1, s);
        if (!fill) hipLaunchKernelGGL(k10_big_cnt, dim3(blocks_of(n_seg, 256, kWhat)), dim3(256), 0, s, B.slot.as<uint32_t>(), d_row, d_off, n_seg, a.cnt);
        else hipLaunchKernelGGL(k10_big_fill, dim3(blocks_of(total, 256, kWhat)), dim3(256), 0, s, a, B.keys2.as<uint64_t>(), B.prod.as<float>(), B.slot.as<uint32_t>(), d_row, d_off, n_seg, total);
        XRL_LAUNCH_CHECK();
        ++batches;
        g0 = g1;
    }
    return batches;
}

}  // namespace

void spgemm_device(const QueriesDev& A, const QueriesDev& Bm, bool eliminate_zeros, bool sorted_indices, hipStream_t s, SpgemmOut& out) {
    const uint64_t rows = A.rows;
    DevCsr& Z = out.z;
    DevCsr& E = out.e;
    Z.ptr.reserve((rows + 1) * 8);
    XRL_HIP(hipMemsetAsync(Z.ptr.p, 0, (rows + 1) * 8, s));
    Z.nnz = E.nnz = 0;
    if (eliminate_zeros) { E.ptr.reserve((rows + 1) * 8); XRL_HIP(hipMemsetAsync(E.ptr.p, 0, (rows + 1) * 8, s)); }
    if (rows == 0 || A.nnz == 0 || Bm.nnz == 0 || Bm.rows == 0) { XRL_HIP(hipStreamSynchronize(s)); return; }

    K10Args a{};
    a.a_ptr = A.row_ptr; a.a_col = A.col_idx; a.a_val = A.val; a.a_nnz = A.nnz;
    a.b_ptr = Bm.row_ptr; a.b_col = Bm.col_idx; a.b_val = Bm.val; a.b_nnz = Bm.nnz;
    a.rows = A.rows; a.inner = Bm.rows; a.sorted = sorted_indices ? 1 : 0;
    DevBuf d_flops, d_cnt, d_words, d_tmp;
    d_flops.reserve(rows * 8); d_cnt.reserve((rows + 1) * 8); d_words.reserve(24);
    XRL_HIP(hipMemsetAsync(d_cnt.p, 0, (rows + 1) * 8, s));
    XRL_HIP(hipMemsetAsync(d_words.p, 0, 24, s));
    a.flops = d_flops.as<uint64_t>(); a.cnt = d_cnt.as<uint64_t>();
    hipLaunchKernelGGL(k10_flops, dim3(blocks_of(rows, 256, kWhat)), dim3(256), 0, s, a, d_flops.as<uint64_t>(), d_words.as<unsigned long long>());
    XRL_LAUNCH_CHECK();
    // the LDS form's counts go ahead of the answer to "does any row need the big form": the common case synchronises once, so this
    // scan reads its total back next to the words instead of through scan_total
    launch_lds<false>(a, s);
    exclusive_scan(d_tmp, d_cnt.as<uint64_t>(), Z.ptr.as<uint64_t>(), (size_t)rows + 1, s);
    uint64_t words[3] = {0, 0, 0};
    XRL_HIP(hipMemcpyAsync(words, d_words.p, 24, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipMemcpyAsync(&Z.nnz, Z.ptr.as<uint64_t>() + rows, 8, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    if (words[1]) fail("sparse_matmul: an entry of the left operand names a row the right operand does not have");
    if (words[2]) fail("sparse_matmul: a row of the product takes 2^31 multiplications or more; split the left operand's row");
    std::vector<uint32_t> big;
    std::vector<uint64_t> F;
    BigScratch scratch;
    if (words[0]) {
        F.resize(rows);
        XRL_HIP(hipMemcpyAsync(F.data(), d_flops.p, rows * 8, hipMemcpyDeviceToHost, s));
        XRL_HIP(hipStreamSynchronize(s));
        for (uint64_t i = 0; i < rows; ++i) if (F[i] > kSpgemmCap) big.push_back((uint32_t)i);
        out.batches = run_big(a, big, F, false, s, scratch);
        Z.nnz = scan_total(d_tmp, d_cnt.as<uint64_t>(), Z.ptr.as<uint64_t>(), rows, s);
    }
    out.big_rows = big.size();
    out.lds_rows = rows - big.size();

    Z.idx.reserve(Z.nnz * 4); Z.val.reserve(Z.nnz * 4);
    if (Z.nnz) {
        a.out_ptr = Z.ptr.as<uint64_t>(); a.out_col = Z.idx.as<uint32_t>(); a.out_val = Z.val.as<float>();
        if (big.size() < rows) launch_lds<true>(a, s);
        if (!big.empty()) run_big(a, big, F, true, s, scratch);
    }
    if (eliminate_zeros && Z.nnz) {
        hipLaunchKernelGGL(k10_nz<false>, dim3(blocks_of(rows, 4, kWhat)), dim3(256), 0, s, Z.ptr.as<uint64_t>(), Z.idx.as<uint32_t>(), Z.val.as<float>(), rows,
                           d_cnt.as<uint64_t>(), (const uint64_t*)nullptr, (uint32_t*)nullptr, (float*)nullptr);
        XRL_LAUNCH_CHECK();
        E.nnz = scan_total(d_tmp, d_cnt.as<uint64_t>(), E.ptr.as<uint64_t>(), rows, s);
        E.idx.reserve(E.nnz * 4); E.val.reserve(E.nnz * 4);
        if (E.nnz) {
            hipLaunchKernelGGL(k10_nz<true>, dim3(blocks_of(rows, 4, kWhat)), dim3(256), 0, s, Z.ptr.as<uint64_t>(), Z.idx.as<uint32_t>(), Z.val.as<float>(), rows,
                               (uint64_t*)nullptr, E.ptr.as<uint64_t>(), E.idx.as<uint32_t>(), E.val.as<float>());
            XRL_LAUNCH_CHECK();
        }
    }
    XRL_HIP(hipStreamSynchronize(s));                      // the scratch goes with this scope
}

void topk_to_csr_device(uint32_t rows, const uint32_t* d_idx, const float* d_val, const uint32_t* d_cnt, uint32_t stride, hipStream_t s, DevCsr& out) {
    out.ptr.reserve(((size_t)rows + 1) * 8);
    XRL_HIP(hipMemsetAsync(out.ptr.p, 0, ((size_t)rows + 1) * 8, s));
    out.nnz = 0;
    if (rows == 0 || stride == 0) { XRL_HIP(hipStreamSynchronize(s)); return; }
    DevBuf d_n, d_tmp;
    d_n.reserve(((size_t)rows + 1) * 8);
    XRL_HIP(hipMemsetAsync(d_n.p, 0, ((size_t)rows + 1) * 8, s));
    hipLaunchKernelGGL(k10_topk_cnt, dim3(blocks_of(rows, 256, kWhat)), dim3(256), 0, s, d_cnt, stride, (uint64_t)rows, d_n.as<uint64_t>());
    XRL_LAUNCH_CHECK();
    out.nnz = scan_total(d_tmp, d_n.as<uint64_t>(), out.ptr.as<uint64_t>(), rows, s);
    out.idx.reserve(out.nnz * 4); out.val.reserve(out.nnz * 4);
    if (out.nnz) {
        launch_copy_rows(out.ptr.as<uint64_t>(), rows, nullptr, stride, d_idx, d_val, out.idx.as<uint32_t>(), out.val.as<float>(), kWhat, s);
        XRL_HIP(hipStreamSynchronize(s));
    }
}

}  // namespace xrl
