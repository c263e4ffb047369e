// K12: the primitives of the label embeddings (xrl_embed.h; the rules R1 / R2 are stated in include/xrl_abi.h at xrl_label_embedding_device).
//
//   transpose        k12_t_count     histogram of the column ids (integer atomics; flags an id >= cols)
//                    exclusive scan  -> the output row pointer
//                    k12_t_classify  lists the output rows above CAP, counts the forms
//                    k12_t_scatter   every entry's SOURCE POSITION into its column's segment, slots claimed by integer atomics: any order
//                    k12_t_rows      one wavefront per 64 output rows, a row at a time: the segment's positions are ordered ascending -- by
//                                    counting when they fit the lanes, by a bitonic sort in LDS up to CAP -- which is the stable order
//                                    (source row ascending, stored order inside it); then (source row of the position, val[position]) is
//                                    gathered, the source row by bisection of the source's row pointer
//                    big form        rows above CAP: one rocPRIM segmented radix sort of the positions in HBM, k12_t_big_gather
//   normalise        k12_normalize<NORM>  one wavefront per 64 rows (fewer when the rows are long on average).  NORM = 2 (R1): the sum of a row is ONE fp64 chain in
//                                    stored order of the rounded fp32 squares: rows below 64 entries one per lane, longer ones by the wavefront (64 squares a
//                                    step, the adds serial on every lane).  NORM = 1 (R1a): the same chain over |v| widened to double, no square root.
//                                    NORM = 3 (R1b): the fp32 maximum of |v| -- order-free, so the wavefront form keeps a maximum per lane and the lanes
//                                    meet in a butterfly; a NaN entry is found by ballot, never by the maximum.  The divide pass walks the 64 rows' entries
//                                    64 at a time, an entry finding its row by bisection of the 64 row starts in LDS.  NaN results take the bits the
//                                    reference's host gives them (R1b: a NaN).
//                    k12_check_ascending  R1b only, before anything is written: a row whose ids are not strictly ascending is refused
//   hstack           k12_add_lens (counts, then the write cursors) around the shared row copy of xrl_devprim.h
//
// Bounds: every row span is clamped to the arrays' nnz; a claimed slot and a sorted position are below nnz before they index; an LDS index
// is below CAP (the padded size of a sort is at most CAP).
#include "xrl_embed.h"
#include "xrl_device.h"
#include "xrl_devprim.h"

#include <algorithm>

#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace xrl {

namespace {

constexpr uint32_t kNoPos = 0xFFFFFFFFu;                   // above every position (nnz < 2^32 - 1): the padding of a sort
constexpr uint32_t kQuiet = 0x00400000u;
constexpr uint64_t kGridRows = 1ull << 30;                 // output rows of one launch of the per-row kernels (a grid holds fewer than 2^32 threads)

struct K12T {
    const uint64_t* a_ptr; const uint32_t* a_col; const float* a_val;
    uint64_t nnz;
    uint32_t rows, cols;                                   // of the source: the output has `cols` rows
    const uint64_t* out_ptr; uint32_t* out_col; float* out_val;
    const uint32_t* pos;                                   // [nnz] source positions, by output row, unordered inside a row
};

__global__ void __launch_bounds__(256)
k12_t_count(const uint32_t* __restrict__ col, uint64_t nnz, uint32_t cols, unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ words) {
    const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (x >= nnz) return;
    const uint32_t c = col[x];
    if (c >= cols) { atomicMax(&words[0], 1ull); return; }
    atomicAdd(&cnt[c], 1ull);
}

// words[1] <- output rows above CAP (listed in big_row, any order), words[2] <- output rows of 1 .. CAP entries
__global__ void __launch_bounds__(256)
k12_t_classify(const uint64_t* __restrict__ out_ptr, uint64_t row0, uint32_t orows, uint32_t big_cap, uint32_t* __restrict__ big_row,
               unsigned long long* __restrict__ words) {
    const uint64_t r = row0 + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint64_t len = 0;
    if (r < orows) len = out_ptr[r + 1] - out_ptr[r];
    const bool big = len > kEmbedCap;
    if (big) {
        const unsigned long long i = atomicAdd(&words[1], 1ull);
        if (i < big_cap) big_row[i] = (uint32_t)r;
    }
    const unsigned long long ml = __ballot(len > 0 && !big);
    if ((threadIdx.x & 63u) == 0 && ml) atomicAdd(&words[2], (unsigned long long)__popcll(ml));
}

__global__ void __launch_bounds__(256)
k12_t_scatter(const uint32_t* __restrict__ col, uint64_t nnz, uint32_t cols, unsigned long long* __restrict__ cursor, uint32_t* __restrict__ pos) {
    const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (x >= nnz) return;
    const uint32_t c = col[x];
    if (c >= cols) return;
    const unsigned long long slot = atomicAdd(&cursor[c], 1ull);
    if (slot < nnz) pos[slot] = (uint32_t)x;
}

// entry `at` of the output <- the source entry at position p
__device__ __forceinline__ void gather_entry(const K12T& a, uint64_t at, uint32_t p) {
    if (p >= a.nnz) return;
    a.out_col[at] = segment_of(a.a_ptr, a.rows, (uint64_t)p);
    a.out_val[at] = a.a_val[p];
}

__global__ void __launch_bounds__(64) k12_t_rows(K12T a, uint64_t row0) {
    __shared__ uint32_t s_pos[kEmbedCap];
    const uint32_t lane = threadIdx.x;
    const uint64_t r = row0 + (uint64_t)blockIdx.x * 64u + lane;
    uint64_t b = 0, e = 0;
    if (r < a.cols) row_span(a.out_ptr, r, a.nnz, b, e);
    const uint64_t len = e - b;
    unsigned long long todo = __ballot(len > 0 && len <= kEmbedCap);
    while (todo) {                                         // (uniform)
        const int i = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint64_t wb = __shfl(b, i);
        const uint32_t n = (uint32_t)__shfl(len, i);
        if (n <= 64u) {                                    // rank by counting: the positions are distinct
            const uint32_t p = lane < n ? a.pos[wb + lane] : kNoPos;
            uint32_t rank = 0;
            for (uint32_t j = 0; j < n; ++j) rank += (uint32_t)__shfl((int)p, (int)j) < p ? 1u : 0u;
            if (lane < n && rank < n) gather_entry(a, wb + rank, p);
            continue;
        }
        uint32_t P = 128;
        while (P < n) P <<= 1;                             // n <= CAP, a power of two: P <= CAP
        for (uint32_t x = lane; x < P; x += 64u) s_pos[x] = x < n ? a.pos[wb + x] : kNoPos;
        __syncthreads();                                   // one wavefront per workgroup
        for (uint32_t k = 2; k <= P; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t t = lane; t < P / 2; t += 64u) {
                    const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
                    const uint32_t x = s_pos[lo], y = s_pos[hi];
                    if ((x > y) == ((lo & k) == 0)) { s_pos[lo] = y; s_pos[hi] = x; }
                }
                __syncthreads();
            }
        for (uint32_t x = lane; x < n; x += 64u) gather_entry(a, wb + x, s_pos[x]);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
k12_t_big_segs(const uint32_t* __restrict__ big_row, uint32_t n_big, const uint64_t* __restrict__ out_ptr, uint64_t nnz, uint32_t* __restrict__ seg_b,
               uint32_t* __restrict__ seg_e) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_big) return;
    uint64_t b, e;
    row_span(out_ptr, big_row[g], nnz, b, e);
    seg_b[g] = (uint32_t)b; seg_e[g] = (uint32_t)e;
}

// one workgroup per row of the big form, over its sorted positions
__global__ void __launch_bounds__(256) k12_t_big_gather(K12T a, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ big_row) {
    uint64_t b, e;
    row_span(a.out_ptr, big_row[blockIdx.x], a.nnz, b, e);
    for (uint64_t x = b + threadIdx.x; x < e; x += 256u) gather_entry(a, x, sorted[x]);
}

// ---- normalise
// NORM = 2: rule R1 (the sum of the rounded fp32 squares, n = sqrt); 1: R1a (the sum of |v| widened to double, n = s); 3: R1b (the fp32
// maximum of |v|, order-free).  One row's term of the chain, and what a NaN entry leaves as the NaN of the row.
template <int NORM> __device__ __forceinline__ double k12_term(float v) {
    if (NORM == 2) return (double)__fmul_rn(v, v);
    return fabs((double)v);                                // (NORM == 3: |v| widened exactly; the maximum of widened floats is a float)
}
template <int NORM> __device__ __forceinline__ uint32_t k12_row_nan(float v) {
    if (NORM == 2) return __float_as_uint(v) | kQuiet;
    if (NORM == 1) return (__float_as_uint(v) & 0x7FFFFFFFu) | kQuiet;     // fabs clears the sign before the chain sees the NaN
    return 0x7FC00000u;                                    // R1b: "a NaN" (numpy's reduction order picks the payload on the host)
}

// words[0] <- rows (with entries) summed one per lane, words[1] <- by the wavefront
template <int NORM>
__global__ void __launch_bounds__(256)
k12_normalize(const uint64_t* __restrict__ ptr, const float* val, float* out, uint64_t row0, uint64_t rows, uint64_t nnz, uint32_t per_wave,
              unsigned long long* __restrict__ words) {
    __shared__ uint64_t s_b[4][64];
    __shared__ double s_n[4][64];
    __shared__ uint32_t s_nan[4][64];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t r0 = row0 + ((uint64_t)blockIdx.x * 4u + w) * per_wave;                                // per_wave <= 64 rows to a wavefront
    if (r0 >= rows) return;                                // (per wavefront: no workgroup barrier below)
    const uint32_t n_valid = (uint32_t)min((uint64_t)per_wave, rows - r0);
    const bool valid = lane < n_valid;
    uint64_t b = 0, e = 0;
    if (valid) row_span(ptr, r0 + lane, nnz, b, e);
    const bool wave = valid && e - b >= kEmbedWaveRow;
    // s: the fp64 chain from +0 of the row's terms, in stored order (NORM = 3: their maximum).  nanb: the first NaN entry, quieted -- what
    // the host's chain, square root and division hand on as the NaN of the row
    double s = 0.0;
    uint32_t nanb = 0;
    if (valid && !wave)
        for (uint64_t x = b; x < e; ++x) {
            const float v = val[x];
            if (v != v && !nanb) nanb = k12_row_nan<NORM>(v);
            if (NORM == 3) { if (v == v) s = fmax(s, k12_term<NORM>(v)); }
            else s = __dadd_rn(s, k12_term<NORM>(v));
        }
    unsigned long long todo = __ballot(wave);
    const unsigned long long m_lane = __ballot(valid && !wave && e > b);
    if (lane == 0) {
        if (m_lane) atomicAdd(&words[0], (unsigned long long)__popcll(m_lane));
        if (todo) atomicAdd(&words[1], (unsigned long long)__popcll(todo));
    }
    while (todo) {                                         // (uniform)
        const int i = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint64_t wb = __shfl(b, i), we = __shfl(e, i);
        double t = 0.0;
        uint32_t tn = 0;
        for (uint64_t x0 = wb; x0 < we; x0 += 64u) {
            const uint64_t x = x0 + lane;
            const float v = x < we ? val[x] : 0.0f;
            const double p = k12_term<NORM>(v);
            const unsigned long long mn = __ballot(v != v);
            if (!tn && mn) tn = k12_row_nan<NORM>(__uint_as_float((uint32_t)__shfl((int)__float_as_uint(v), __ffsll((long long)mn) - 1)));
            if (NORM == 3) { if (v == v) t = fmax(t, p); }         // (per lane; the lanes meet below.  Which lane saw a NaN does not matter: the ballot)
            else {
                const uint32_t n = (uint32_t)min((uint64_t)64u, we - x0);
                t = wave_chain(t, p, n);
            }
        }
        if (NORM == 3) {
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) t = fmax(t, __shfl_xor(t, d, 64));
        }
        if ((int)lane == i) { s = t; nanb = tn; }
    }
    const uint64_t lo = __shfl(b, 0), hi = __shfl(e, (int)n_valid - 1);
    s_b[w][lane] = valid ? b : hi;
    s_n[w][lane] = (nanb == 0 && s == 0.0) ? 0.0 : (NORM == 2 ? sqrt(s) : s);      // 0: the row stays as it is
    s_nan[w][lane] = nanb;
    wave_sync_lds();
    for (uint64_t x0 = lo; x0 < hi; x0 += 64u) {
        const uint64_t x = x0 + lane;
        if (x >= hi) continue;
        const uint32_t i = segment_of(s_b[w], 64u, x);
        const float v = val[x];
        const double nn = s_n[w][i];
        const uint32_t nb = s_nan[w][i];
        float o = v;
        if (nb) o = __uint_as_float(v != v ? (__float_as_uint(v) | kQuiet) : nb);
        else if (nn != 0.0) {
            o = NORM == 3 ? __fdiv_rn(v, (float)nn) : (float)((double)v / nn);
            if (o != o) o = __uint_as_float(0xFFC00000u);  // inf / inf: the host's default NaN
        }
        out[x] = o;
    }
}

// R1b refuses a row that is not strictly ascending (sklearn sums duplicate ids before its maximum): word <- max of (rows - r) over such rows r
__global__ void __launch_bounds__(256)
k12_check_ascending(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ col, uint64_t nnz, uint32_t rows, unsigned long long* __restrict__ word) {
    const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (x == 0 || x >= nnz || col[x] > col[x - 1]) return;
    const uint32_t r = segment_of(ptr, rows, x);
    uint64_t b, e;
    row_span(ptr, r, nnz, b, e);
    if (x > b && x < e) atomicMax(word, (unsigned long long)(rows - r));
}

// ---- hstack
__global__ void __launch_bounds__(256) k12_add_lens(uint64_t* __restrict__ acc, const uint64_t* __restrict__ ptr, uint64_t nnz, uint64_t rows) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= rows) return;
    uint64_t b, e;
    row_span(ptr, r, nnz, b, e);
    acc[r] += e - b;
}

}  // namespace

void transpose_device(const char* what, const QueriesDev& A, hipStream_t s, DevCsr& out, EmbedForms& forms) {
    const uint64_t orows = A.cols, nnz = A.nnz;
    if (nnz >= kNoPos) fail(std::string(what) + ": a transpose serves fewer than 2^32 - 1 stored entries");
    out.ptr.reserve((orows + 1) * 8);
    XRL_HIP(hipMemsetAsync(out.ptr.p, 0, (orows + 1) * 8, s));
    out.nnz = 0;
    if (nnz == 0 || A.rows == 0) { XRL_HIP(hipStreamSynchronize(s)); return; }

    DevBuf cnt, words, tmp, pos, pos2, big, segs;
    cnt.reserve((orows + 1) * 8); words.reserve(24);
    XRL_HIP(hipMemsetAsync(cnt.p, 0, (orows + 1) * 8, s));
    XRL_HIP(hipMemsetAsync(words.p, 0, 24, s));
    const uint32_t big_cap = (uint32_t)(nnz / (kEmbedCap + 1u)) + 1u;
    big.reserve((size_t)big_cap * 4);
    const uint32_t entry_blocks = blocks_of(nnz, 256, what);
    hipLaunchKernelGGL(k12_t_count, dim3(entry_blocks), dim3(256), 0, s, A.col_idx, nnz, A.cols, cnt.as<unsigned long long>(), words.as<unsigned long long>());
    XRL_LAUNCH_CHECK();
    exclusive_scan(tmp, cnt.as<uint64_t>(), out.ptr.as<uint64_t>(), (size_t)orows + 1, s);
    for (uint64_t r0 = 0; r0 < orows; r0 += kGridRows) {
        hipLaunchKernelGGL(k12_t_classify, dim3(blocks_of(std::min<uint64_t>(kGridRows, orows - r0), 256, what)), dim3(256), 0, s, out.ptr.as<uint64_t>(), r0, A.cols,
                           big_cap, big.as<uint32_t>(), words.as<unsigned long long>());
        XRL_LAUNCH_CHECK();
    }
    uint64_t h[3] = {0, 0, 0};
    XRL_HIP(hipMemcpyAsync(h, words.p, 24, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    if (h[0]) fail(std::string(what) + ": an entry names a column the matrix does not have");
    const uint32_t n_big = (uint32_t)std::min<uint64_t>(h[1], big_cap);
    forms.t_big += n_big; forms.t_lds += h[2];

    out.nnz = nnz;
    out.idx.reserve(nnz * 4); out.val.reserve(nnz * 4); pos.reserve(nnz * 4);
    XRL_HIP(hipMemcpyAsync(cnt.p, out.ptr.p, orows * 8, hipMemcpyDeviceToDevice, s));                  // the write cursors
    hipLaunchKernelGGL(k12_t_scatter, dim3(entry_blocks), dim3(256), 0, s, A.col_idx, nnz, A.cols, cnt.as<unsigned long long>(), pos.as<uint32_t>());
    XRL_LAUNCH_CHECK();
    K12T a{A.row_ptr, A.col_idx, A.val, nnz, A.rows, A.cols, out.ptr.as<uint64_t>(), out.idx.as<uint32_t>(), out.val.as<float>(), pos.as<uint32_t>()};
    for (uint64_t r0 = 0; r0 < orows; r0 += kGridRows) {
        hipLaunchKernelGGL(k12_t_rows, dim3(blocks_of(std::min<uint64_t>(kGridRows, orows - r0), 64, what)), dim3(64), 0, s, a, r0);
        XRL_LAUNCH_CHECK();
    }
    if (n_big) {
        pos2.reserve(nnz * 4); segs.reserve((size_t)n_big * 8);
        uint32_t* seg_b = segs.as<uint32_t>();
        uint32_t* seg_e = seg_b + n_big;
        hipLaunchKernelGGL(k12_t_big_segs, dim3(blocks_of(n_big, 256, what)), dim3(256), 0, s, big.as<uint32_t>(), n_big, out.ptr.as<uint64_t>(), nnz, seg_b, seg_e);
        XRL_LAUNCH_CHECK();
        with_rocprim_tmp(tmp, [&](void* t, size_t& bytes) {
            return rocprim::segmented_radix_sort_keys(t, bytes, pos.as<uint32_t>(), pos2.as<uint32_t>(), (unsigned int)nnz, n_big, seg_b, seg_e, 0u, 32u, s);
        });
        hipLaunchKernelGGL(k12_t_big_gather, dim3(n_big), dim3(256), 0, s, a, pos2.as<uint32_t>(), big.as<uint32_t>());
        XRL_LAUNCH_CHECK();
    }
    XRL_HIP(hipStreamSynchronize(s));                      // the scratch goes with this scope
}

void normalize_rows_device(const char* what, const QueriesDev& A, float* out_val, hipStream_t s, EmbedForms& forms, int norm) {
    if (A.rows == 0 || A.nnz == 0) { XRL_HIP(hipStreamSynchronize(s)); return; }
    DevBuf words;
    words.reserve(24);
    XRL_HIP(hipMemsetAsync(words.p, 0, 24, s));
    if (norm == 3) {                                       // before a value is written: an in-place call leaves a refused matrix as it was
        hipLaunchKernelGGL(k12_check_ascending, dim3(blocks_of(A.nnz, 256, what)), dim3(256), 0, s, A.row_ptr, A.col_idx, A.nnz, A.rows, words.as<unsigned long long>() + 2);
        XRL_LAUNCH_CHECK();
        uint64_t bad = 0;
        XRL_HIP(hipMemcpyAsync(&bad, words.as<uint64_t>() + 2, 8, hipMemcpyDeviceToHost, s));
        XRL_HIP(hipStreamSynchronize(s));
        if (bad) fail(std::string(what) + ": norm = max: row " + std::to_string(A.rows - bad) + " does not store its column ids strictly ascending (a repeated id is summed by the reference before its maximum; not served)");
    }
    // a wavefront sums its long rows one after the other: it gets fewer rows the longer they are on average (about 4096 entries' worth)
    uint32_t per_wave = 64;
    while (per_wave > 1 && A.nnz / A.rows * per_wave > 4096) per_wave >>= 1;
    const uint64_t per_launch = (1ull << 25) * per_wave;   // rows of one launch: 2^23 workgroups
    auto* kernel = norm == 1 ? k12_normalize<1> : norm == 3 ? k12_normalize<3> : k12_normalize<2>;
    for (uint64_t r0 = 0; r0 < A.rows; r0 += per_launch) {
        hipLaunchKernelGGL(kernel, dim3(blocks_of(std::min<uint64_t>(per_launch, A.rows - r0), 4 * per_wave, what)), dim3(256), 0, s, A.row_ptr, A.val, out_val, r0,
                           (uint64_t)A.rows, A.nnz, per_wave, words.as<unsigned long long>());
        XRL_LAUNCH_CHECK();
    }
    uint64_t h[2] = {0, 0};
    XRL_HIP(hipMemcpyAsync(h, words.p, 16, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    forms.n_lane += h[0]; forms.n_wave += h[1];
}

void hstack_device(const char* what, const std::vector<QueriesDev>& mats, hipStream_t s, DevCsr& out) {
    const uint64_t rows = mats.empty() ? 0 : mats[0].rows;
    out.ptr.reserve((rows + 1) * 8);
    XRL_HIP(hipMemsetAsync(out.ptr.p, 0, (rows + 1) * 8, s));
    out.nnz = 0;
    if (rows == 0) { XRL_HIP(hipStreamSynchronize(s)); return; }
    DevBuf acc, tmp;
    acc.reserve((rows + 1) * 8);
    XRL_HIP(hipMemsetAsync(acc.p, 0, (rows + 1) * 8, s));
    const uint32_t row_blocks = blocks_of(rows, 256, what);
    auto add_lens = [&](const QueriesDev& m) {
        hipLaunchKernelGGL(k12_add_lens, dim3(row_blocks), dim3(256), 0, s, acc.as<uint64_t>(), m.row_ptr, m.nnz, rows);
        XRL_LAUNCH_CHECK();
    };
    for (const QueriesDev& m : mats) add_lens(m);
    out.nnz = scan_total(tmp, acc.as<uint64_t>(), out.ptr.as<uint64_t>(), rows, s);
    out.idx.reserve(out.nnz * 4); out.val.reserve(out.nnz * 4);
    if (out.nnz) {
        XRL_HIP(hipMemcpyAsync(acc.p, out.ptr.p, rows * 8, hipMemcpyDeviceToDevice, s));               // where the next matrix's entries of a row go
        uint64_t col0 = 0;
        for (const QueriesDev& m : mats) {
            if (m.nnz) launch_copy_csr_rows(acc.as<uint64_t>(), rows, m.row_ptr, m.col_idx, m.val, m.nnz, (uint32_t)col0, out.idx.as<uint32_t>(), out.val.as<float>(), what, s);
            add_lens(m);
            col0 += m.cols;
        }
    }
    XRL_HIP(hipStreamSynchronize(s));
}

}  // namespace xrl
