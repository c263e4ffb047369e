// K14: the union of the patterns of n CSR operands of one shape, as a CSR of ones with strictly ascending rows -- the matching matrix of
// a layer's training (pecos/xmc/base.py:1544-1565: M += binarized(A) per source, then sort_indices(); the trainer reads only M's pattern).
// No floating-point arithmetic: column ids are gathered, ordered and compared.
//
//   k14_totals       T_i = the stored entries of row i over all operands (one wavefront per row); counts the rows above CAP; flags a
//                    column id that is not below cols (the check kernel: such an id is a key here, never an address)
//   k14_lds<FILL>    one wavefront per row with T_i <= CAP (xrl_match.h).  The operands' column ids go to LDS 64 a step, in operand order;
//                    a bitonic sort; a lane whose key differs from its predecessor's is a head (one ballot per 64 keys, no atomics); the
//                    head's rank is its output slot.  FILL = false only counts the heads.
//   big form         rows above CAP, in batches under the scratch budget: k14_big_expand copies the ids to HBM, one rocPRIM segmented
//                    radix sort of the 32-bit keys, k14_big_heads<FILL> walks a row's sorted ids 64 a step with the same ballot.
//   counts -> exclusive scan (u64, xrl_devprim.h) -> fill.
//   k14_beam_bound   a beam in HBM against a layer's child ranges: per row the sum over listed parents of their child counts, the
//                    maximum in one u64 (what the host form of the single-layer predict computes in a loop over csr_codes)
//   k14_fill_ones    the beam of fill_ones
//   k14_check_relevance  does R store exactly Y's entries and no value below 0 (MLProblem's check of a relevance matrix; rule C in
//                    include/xrl_abi.h): one wavefront per row compares the row's ends, then -- where the spans agree -- the column ids
//                    position by position and R's values against 0; the least (code << 40 | row) over the offending rows lands in one
//                    u64 by atomicMin: one pass, one 8-byte readback
//
// Bounds: every row span is clamped to the operand's nnz; an LDS index is below CAP and a scratch index below its row's share before the
// write; an output index is below the row's end in the scanned row pointer; a parent id is below n_parents before chunk_col is read; the
// check reads entries only inside a span that both matrices' clamped row pointers agree on.
#include "xrl_match.h"
#include "xrl_device.h"
#include "xrl_devprim.h"
#include "xrl_predict.h"

#include <algorithm>
#include <cstdlib>

#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace xrl {

namespace {

constexpr const char* kWhat = "pattern_union";           // the family in a "grid too large" message
constexpr uint32_t kPad = 0xFFFFFFFFu;                    // above every id below cols <= 2^32 - 1

struct K14Op { const uint64_t* ptr; const uint32_t* idx; uint64_t nnz; };

struct K14Args {
    const K14Op* ops; uint32_t n_ops;
    uint32_t rows, cols, row0;
    const uint64_t* total;                                 // [rows]
    uint64_t* cnt;                                         // [rows + 1] the count passes' output
    const uint64_t* out_ptr; uint32_t* out_col; float* out_val;   // the fill passes' output
};

// words: [0] rows above CAP, [1] an id not below cols, [2] a row of 2^31 entries or more, [3] entries read
__global__ void __launch_bounds__(256) k14_totals(K14Args a, uint64_t* __restrict__ total, unsigned long long* __restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= a.rows) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t T = 0;
    bool bad = false;
    for (uint32_t o = 0; o < a.n_ops; ++o) {
        const K14Op op = a.ops[o];
        uint64_t b, e;
        row_span(op.ptr, i, op.nnz, b, e);
        T += e - b;
        for (uint64_t x = b + lane; x < e; x += 64u) bad = bad || op.idx[x] >= a.cols;
    }
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane != 0) return;
    total[i] = T;
    if (T) atomicAdd(&words[3], (unsigned long long)T);
    if (T > kMatchCap) atomicAdd(&words[0], 1ull);
    if (T >= (1ull << 31)) atomicMax(&words[2], 1ull);
    if (any_bad) atomicMax(&words[1], 1ull);
}

template <bool FILL>
__global__ void __launch_bounds__(64) k14_lds(K14Args a) {
    __shared__ uint32_t s_key[kMatchCap];
    const uint32_t lane = threadIdx.x;
    const uint64_t i = (uint64_t)a.row0 + blockIdx.x;
    const uint64_t T = a.total[i];
    if (T == 0 || T > kMatchCap) return;                   // (the counts start at zero; the big form serves the rows above CAP)

    // ---- the operands' ids, in operand order
    uint32_t q = 0;
    for (uint32_t o = 0; o < a.n_ops; ++o) {
        const K14Op op = a.ops[o];
        uint64_t b, e;
        row_span(op.ptr, i, op.nnz, b, e);
        const uint64_t len = min(e - b, (uint64_t)kMatchCap + 1u);   // (T <= CAP: every length is; the clamp keeps q small whatever the arrays hold)
        for (uint64_t t0 = 0; t0 < len; t0 += 64u) {
            const uint64_t t = t0 + lane;
            if (t < len && q + t < kMatchCap) s_key[q + (uint32_t)t] = op.idx[b + t];
        }
        q = (uint32_t)min((uint64_t)q + len, (uint64_t)kMatchCap);
    }
    const uint32_t nf = q;
    if (nf == 0) return;

    // ---- ascending
    uint32_t P = 64;
    while (P < nf) P <<= 1;                                // (<= CAP, a power of two)
    for (uint32_t x = nf + lane; x < P; x += 64u) s_key[x] = kPad;
    __syncthreads();                                       // one wavefront per workgroup
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < P / 2; t += 64u) {
                const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
                const uint32_t x = s_key[lo], y = s_key[hi];
                if ((x > y) == ((lo & k) == 0)) { s_key[lo] = y; s_key[hi] = x; }
            }
            __syncthreads();
        }

    // ---- equal neighbours collapse: a key that differs from its predecessor is a head, its rank the output slot
    const uint64_t base = FILL ? a.out_ptr[i] : 0, end = FILL ? a.out_ptr[i + 1] : 0;
    uint32_t r0 = 0;
    for (uint32_t x0 = 0; x0 < nf; x0 += 64u) {
        const uint32_t x = x0 + lane;
        const bool head = x < nf && (x == 0 || s_key[x] != s_key[x - 1]);
        const unsigned long long m = __ballot(head);
        if (FILL && head) {
            const uint64_t at = base + r0 + lanes_below(m);
            if (at < end) { a.out_col[at] = s_key[x]; a.out_val[at] = 1.0f; }
        }
        r0 += (uint32_t)__popcll(m);
    }
    if (!FILL && lane == 0) a.cnt[i] = r0;
}

// ---- big form
// one workgroup per row of the batch: the ids of every operand's row, at the row's offset
__global__ void __launch_bounds__(256) k14_big_expand(K14Args a, const uint32_t* __restrict__ big_row, const uint32_t* __restrict__ off, uint32_t* __restrict__ keys) {
    const uint32_t sg = blockIdx.x;
    const uint64_t i = big_row[sg];
    const uint32_t base = off[sg], lim = off[sg + 1] - base;
    uint64_t q = 0;
    for (uint32_t o = 0; o < a.n_ops; ++o) {
        const K14Op op = a.ops[o];
        uint64_t b, e;
        row_span(op.ptr, i, op.nnz, b, e);
        const uint64_t len = e - b;
        for (uint64_t t = threadIdx.x; t < len; t += 256u)
            if (q + t < lim) keys[base + (uint32_t)(q + t)] = op.idx[b + t];
        q += len;
    }
}

// one wavefront per row of the batch walks its sorted ids 64 a step
template <bool FILL>
__global__ void __launch_bounds__(64) k14_big_heads(K14Args a, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ big_row, const uint32_t* __restrict__ off) {
    const uint32_t sg = blockIdx.x, lane = threadIdx.x;
    const uint64_t i = big_row[sg];
    const uint32_t b = off[sg], e = off[sg + 1];
    const uint64_t base = FILL ? a.out_ptr[i] : 0, end = FILL ? a.out_ptr[i + 1] : 0;
    uint64_t r0 = 0;
    for (uint64_t x0 = b; x0 < e; x0 += 64u) {
        const uint64_t x = x0 + lane;
        const bool head = x < e && (x == b || keys[x] != keys[x - 1]);
        const unsigned long long m = __ballot(head);
        if (FILL && head) {
            const uint64_t at = base + r0 + lanes_below(m);
            if (at < end) { a.out_col[at] = keys[x]; a.out_val[at] = 1.0f; }
        }
        r0 += (uint64_t)__popcll(m);
    }
    if (!FILL && lane == 0) a.cnt[i] = r0;
}

constexpr uint32_t kLdsGridRows = 1u << 30;                // rows of one launch of the LDS form

template <bool FILL> void launch_lds(K14Args a, hipStream_t s) {
    for (uint64_t r0 = 0; r0 < a.rows; r0 += kLdsGridRows) {
        a.row0 = (uint32_t)r0;
        const uint32_t n = (uint32_t)std::min<uint64_t>(kLdsGridRows, a.rows - r0);
        hipLaunchKernelGGL(k14_lds<FILL>, dim3(n), dim3(64), 0, s, a);
        XRL_LAUNCH_CHECK();
    }
}

// The big form over all its rows, batch by batch: fill = false writes a.cnt of every big row, fill = true their entries.
struct BigScratch { DevBuf row, off, keys, keys2, tmp; };

void run_big(K14Args a, const std::vector<uint32_t>& big, const std::vector<uint64_t>& T, bool fill, hipStream_t s, BigScratch& B) {
    uint64_t budget = 0;
    if (const char* e = std::getenv("XRL_MATCH_SCRATCH_ENTRIES")) budget = std::strtoull(e, nullptr, 10);   // (tests: a small budget cuts few rows into batches)
    if (!budget) budget = kCandBudgetBytes / kMatchBigBytesPerEntry;
    bool first = true;
    std::vector<uint32_t> row, off;
    for (size_t g0 = 0; g0 < big.size();) {
        row.clear(); off.assign(1, 0u);
        size_t g1 = g0;
        while (g1 < big.size()) {
            const uint64_t t = T[big[g1]];
            if (g1 > g0 && (uint64_t)off.back() + t > budget) break;       // (a single row above the budget is a batch of its own; t < 2^31)
            if ((uint64_t)off.back() + t > 0xFFFFFFF0ull) break;
            row.push_back(big[g1]); off.push_back(off.back() + (uint32_t)t);
            ++g1;
        }
        const uint32_t n_seg = (uint32_t)row.size(), total = off.back();
        if (!first) XRL_HIP(hipStreamSynchronize(s));      // the uploads reuse the buffers the last batch's kernels read
        first = false;
        B.row.upload(row); B.off.upload(off);
        B.keys.reserve((size_t)total * 4); B.keys2.reserve((size_t)total * 4);
        const uint32_t* d_row = B.row.as<uint32_t>(); const uint32_t* d_off = B.off.as<uint32_t>();
        hipLaunchKernelGGL(k14_big_expand, dim3(n_seg), dim3(256), 0, s, a, d_row, d_off, B.keys.as<uint32_t>());
        XRL_LAUNCH_CHECK();
        with_rocprim_tmp(B.tmp, [&](void* t, size_t& bytes) {
            return rocprim::segmented_radix_sort_keys(t, bytes, B.keys.as<uint32_t>(), B.keys2.as<uint32_t>(), total, n_seg, d_off, d_off + 1, 0u, 32u, s);
        });
        if (fill) hipLaunchKernelGGL(k14_big_heads<true>, dim3(n_seg), dim3(64), 0, s, a, B.keys2.as<uint32_t>(), d_row, d_off);
        else hipLaunchKernelGGL(k14_big_heads<false>, dim3(n_seg), dim3(64), 0, s, a, B.keys2.as<uint32_t>(), d_row, d_off);
        XRL_LAUNCH_CHECK();
        g0 = g1;
    }
}

// word <- max over the rows of (the row's candidate count), or of (1 << 63 | id) for a row that lists a parent the layer does not have
__global__ void __launch_bounds__(256) k14_beam_bound(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ cnt, uint32_t stride, uint32_t rows,
                                                      const uint32_t* __restrict__ chunk_col, uint32_t n_parents, unsigned long long* __restrict__ word) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    unsigned long long v = 0;
    if (r < rows) {
        const uint32_t n = min(cnt[r], stride);
        unsigned long long sum = 0;
        uint32_t bad_id = 0;
        bool bad = false;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t p = idx[r * stride + j];
            if (p >= n_parents) { bad = true; bad_id = max(bad_id, p); }
            else sum += chunk_col[p + 1] - chunk_col[p];
        }
        v = bad ? ((1ull << 63) | bad_id) : sum;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w > v ? w : v;
    }
    if ((threadIdx.x & 63u) == 0 && v) atomicMax(word, v);
}

__global__ void __launch_bounds__(256) k14_fill_ones(uint32_t* __restrict__ idx, float* __restrict__ val, uint32_t* __restrict__ cnt, uint64_t rows, uint32_t n_parents) {
    const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (x >= rows * n_parents) return;
    const uint32_t p = (uint32_t)(x % n_parents);
    idx[x] = p; val[x] = 1.0f;
    if (p == 0) cnt[x / n_parents] = n_parents;
}

// ---- the relevance check: does R store exactly Y's entries, and no value below 0?
// One wavefront per row.  word <- the least (code << 40 | row) over the rows that offend: code 1 = the row's end (row 0: also its start)
// differs between the row pointers, 2 = a column id differs at some position of a row whose span is the same in both, 3 = a value of R in
// such a row is below 0 (-0.0 and NaN are not).  The least key is the first check that fails in check_relevance's order, at its first row.
__global__ void __launch_bounds__(256)
k14_check_relevance(const uint64_t* __restrict__ y_ptr, const uint32_t* __restrict__ y_idx, uint64_t y_nnz, const uint64_t* __restrict__ r_ptr,
                    const uint32_t* __restrict__ r_idx, const float* __restrict__ r_val, uint64_t r_nnz, uint32_t rows, unsigned long long* __restrict__ word) {
    const uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= rows) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t code = 0;
    if (y_ptr[i + 1] != r_ptr[i + 1] || (i == 0 && y_ptr[0] != r_ptr[0])) code = 1;
    else if (y_ptr[i] == r_ptr[i]) {                       // (a start that differs is the row above's end: reported there)
        uint64_t b, e, rb, re;
        row_span(y_ptr, i, y_nnz, b, e);
        row_span(r_ptr, i, r_nnz, rb, re);
        if (rb != b || re != e) code = 1;                  // (the clamps differ: a pointer past one matrix's entries)
        else {
            bool ids = false, neg = false;
            for (uint64_t x = b + lane; x < e; x += 64u) {
                ids = ids || y_idx[x] != r_idx[x];
                neg = neg || r_val[x] < 0.0f;
            }
            if (__ballot(ids)) code = 2;
            else if (__ballot(neg)) code = 3;
        }
    }
    if (lane == 0 && code) atomicMin(word, ((unsigned long long)code << 40) | i);
}

}  // namespace

void check_relevance_device(const QueriesDev& Y, const QueriesDev& R, hipStream_t s, uint64_t status[2]) {
    status[0] = 0; status[1] = 0;
    if (Y.rows == 0) { XRL_HIP(hipStreamSynchronize(s)); return; }
    DevBuf d_word;
    d_word.reserve(8);
    XRL_HIP(hipMemsetAsync(d_word.p, 0xFF, 8, s));
    hipLaunchKernelGGL(k14_check_relevance, dim3(blocks_of(Y.rows, 4, "check_relevance")), dim3(256), 0, s, Y.row_ptr, Y.col_idx, Y.nnz, R.row_ptr, R.col_idx, R.val, R.nnz,
                       Y.rows, d_word.as<unsigned long long>());
    XRL_LAUNCH_CHECK();
    uint64_t key = 0;
    XRL_HIP(hipMemcpyAsync(&key, d_word.p, 8, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    if (key != ~0ull) { status[0] = key >> 40; status[1] = key & ((1ull << 40) - 1); }
}

void pattern_union_device(const char* what_c, const std::vector<QueriesDev>& ops, uint32_t rows_u, uint32_t cols, hipStream_t s, DevCsr& Z, MatchCounters& c) {
    const std::string what = std::string(what_c) + ": ";
    const uint64_t rows = rows_u;
    Z.ptr.reserve((rows + 1) * 8);
    XRL_HIP(hipMemsetAsync(Z.ptr.p, 0, (rows + 1) * 8, s));
    Z.nnz = 0;
    uint64_t stored = 0;
    for (const QueriesDev& o : ops) stored += o.nnz;
    if (rows == 0 || stored == 0) { XRL_HIP(hipStreamSynchronize(s)); return; }

    std::vector<K14Op> table;
    for (const QueriesDev& o : ops) table.push_back(K14Op{o.row_ptr, o.col_idx, o.nnz});
    DevBuf d_ops, d_total, d_cnt, d_words, d_tmp;
    d_ops.upload(table);
    K14Args a{};
    a.ops = d_ops.as<K14Op>(); a.n_ops = (uint32_t)table.size(); a.rows = rows_u; a.cols = cols;
    d_total.reserve(rows * 8); d_cnt.reserve((rows + 1) * 8); d_words.reserve(32);
    XRL_HIP(hipMemsetAsync(d_cnt.p, 0, (rows + 1) * 8, s));
    XRL_HIP(hipMemsetAsync(d_words.p, 0, 32, s));
    a.total = d_total.as<uint64_t>(); a.cnt = d_cnt.as<uint64_t>();
    hipLaunchKernelGGL(k14_totals, dim3(blocks_of(rows, 4, kWhat)), dim3(256), 0, s, a, d_total.as<uint64_t>(), d_words.as<unsigned long long>());
    XRL_LAUNCH_CHECK();
    // the LDS form's counts go ahead of the answer to "does any row need the big form": the common case synchronises once
    launch_lds<false>(a, s);
    exclusive_scan(d_tmp, d_cnt.as<uint64_t>(), Z.ptr.as<uint64_t>(), (size_t)rows + 1, s);
    uint64_t words[4] = {0, 0, 0, 0};
    XRL_HIP(hipMemcpyAsync(words, d_words.p, 32, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipMemcpyAsync(&Z.nnz, Z.ptr.as<uint64_t>() + rows, 8, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    if (words[1]) { Z.nnz = 0; fail(what + "an operand stores a column id that is not below " + std::to_string(cols)); }
    if (words[2]) { Z.nnz = 0; fail(what + "a row stores 2^31 entries or more over the operands"); }
    std::vector<uint32_t> big;
    std::vector<uint64_t> T;
    BigScratch scratch;
    if (words[0]) {
        T.resize(rows);
        XRL_HIP(hipMemcpyAsync(T.data(), d_total.p, rows * 8, hipMemcpyDeviceToHost, s));
        XRL_HIP(hipStreamSynchronize(s));
        for (uint64_t i = 0; i < rows; ++i) if (T[i] > kMatchCap) big.push_back((uint32_t)i);
        run_big(a, big, T, false, s, scratch);
        Z.nnz = scan_total(d_tmp, d_cnt.as<uint64_t>(), Z.ptr.as<uint64_t>(), rows, s);
    }
    c.big_rows += big.size();
    c.lds_rows += rows - big.size();
    c.read += words[3];
    c.written += Z.nnz;

    Z.idx.reserve(Z.nnz * 4); Z.val.reserve(Z.nnz * 4);
    if (Z.nnz) {
        a.out_ptr = Z.ptr.as<uint64_t>(); a.out_col = Z.idx.as<uint32_t>(); a.out_val = Z.val.as<float>();
        if (big.size() < rows) launch_lds<true>(a, s);
        if (!big.empty()) run_big(a, big, T, true, s, scratch);
    }
    XRL_HIP(hipStreamSynchronize(s));                      // the scratch goes with this scope
}

uint64_t beam_cand_bound_device(const uint32_t* idx, const uint32_t* cnt, uint32_t stride, uint32_t rows, const uint32_t* chunk_col, uint32_t n_parents,
                                hipStream_t s, bool& bad_parent) {
    bad_parent = false;
    if (rows == 0 || stride == 0) return 0;
    DevBuf d_word;
    d_word.reserve(8);
    XRL_HIP(hipMemsetAsync(d_word.p, 0, 8, s));
    hipLaunchKernelGGL(k14_beam_bound, dim3(blocks_of(rows, 256, "beam_bound")), dim3(256), 0, s, idx, cnt, stride, rows, chunk_col, n_parents,
                       d_word.as<unsigned long long>());
    XRL_LAUNCH_CHECK();
    uint64_t v = 0;
    XRL_HIP(hipMemcpyAsync(&v, d_word.p, 8, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    if (v >> 63) { bad_parent = true; return v & 0xFFFFFFFFull; }
    return v;
}

void fill_ones_beam_device(uint32_t* idx, float* val, uint32_t* cnt, uint32_t rows, uint32_t n_parents, hipStream_t s) {
    const uint64_t n = (uint64_t)rows * n_parents;
    if (n == 0) return;
    hipLaunchKernelGGL(k14_fill_ones, dim3(blocks_of(n, 256, "fill_ones")), dim3(256), 0, s, idx, val, cnt, (uint64_t)rows, n_parents);
    XRL_LAUNCH_CHECK();
}

}  // namespace xrl
