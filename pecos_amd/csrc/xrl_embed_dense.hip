// K12D: the label embedding over DENSE features -- out = A * X for a CSR A (u64 row pointer, u32 ids, f32 values) and a dense row-major
// X in HBM, with the row normalisation R1 fused behind it (xrl_embed.h; the rule R3D is stated in include/xrl_abi.h at
// xrl_label_embedding_dense_device; the reference: scipy's csr_matvecs under LabelEmbeddingFactory.pifa, pecos/xmc/base.py:1967-1975).
//
// The rule fixes the order: out[r, k] starts at +0.0 and takes the row's stored entries (i, a) in stored order, y = fl32(y + fl32(a *
// x[i, k])).  One fp32 chain per output element, so the work is split over rows and columns and never over a row's entries; what the
// kernels buy is memory parallelism under the serial adds.
//   k12d_rows<4>   the slab form.  A workgroup owns one row of A; a lane owns 4 consecutive columns (one 16-byte load per gathered row of
//                  X), a wavefront a slab of 256, the workgroup min(16, slabs) wavefronts, which loop when there are more slabs than that.
//                  The row's entries are read 64 a step, one (id, value) per lane, coalesced, and broadcast by lane reads, so the base of
//                  a gathered row is uniform.  kDepth = 8 gathered rows are requested before the first of their mul/adds: the loads do
//                  not depend on the chain, only the adds are serial.  8 x 4 floats are 32 VGPRs of loads in flight per lane, which with
//                  the addresses stays below the 128 VGPRs a 16-wavefront workgroup may use; 16 doubled the registers for loads whose
//                  latency 8 x 16 bytes per lane x the wavefronts of a CU already cover (not measured against each other: the profile
//                  note says so).
//   k12d_rows<1>   the long form.  Rows of kEmbedDenseLong entries and more (listed by k12d_classify) get one column per lane, 64-column
//                  slabs: four times the wavefronts walk the row's entries side by side, each with kDepthLong = 32 loads of 4 bytes in
//                  flight per lane -- the registers of the slab form's 8 x 16 bytes, a quarter of the memory round trips on the
//                  row's serial path.
//   k12d_narrow    cols <= 128: ceil(cols / 4) lanes, rounded up to a power of two, serve a row, and 64 / that rows share a wavefront
//                  (K17's packing of dense neighbours).  Every lane group walks its own row, so the entries are read per lane (one
//                  address per group) in batches of kDepth.
// VEC false: X's base or row stride is not a multiple of 16 bytes, every load is scalar.  VEC true: a lane whose 4 columns are all below
// cols loads 16 bytes, the edge lane of cols % 4 != 0 loads scalars.  Stores are 16 bytes where out's window allows it.
// NORM: the workgroup that holds the row hands its values through LDS to wavefront 0, which rounds the squares to fp32 and adds them in
// fp64 in column order, 64 a step (K12's wavefront form); the norm comes back through LDS, the divide is done in registers and E is
// written once.  More than 4096 columns (1024 in the long form): the passes write the product and the workgroup divides its own
// stores afterwards.  The narrow form's groups chain over their own lanes.
// Bounds: a row span is clamped to nnz; an id that is not below x_rows is flagged and read as row 0 (the host refuses x_rows == 0 with
// entries); a lane reads and writes columns below cols only; LDS indexes are below the pass's width.
// MFMA has no place here: the operand is a gather and the order of the additions is the contract.
#include "xrl_embed.h"
#include "xrl_device.h"
#include "xrl_devprim.h"

#include <algorithm>

namespace xrl {
namespace {

constexpr uint32_t kQuiet = 0x00400000u;
constexpr uint32_t kDepth = 8;               // gathered rows of X in flight ahead of the chain, 16 bytes each per lane
constexpr uint32_t kDepthLong = 32;          // ... in the long form, 4 bytes each per lane: the same registers, a quarter of the round trips
constexpr uint32_t kMaxWaves = 16;           // wavefronts of a workgroup of k12d_rows

struct K12D {
    const uint64_t* a_ptr; const uint32_t* a_col; const float* a_val;
    uint64_t nnz;
    uint32_t rows, x_rows;                   // of A
    const float* x; uint64_t x_stride; uint32_t cols;
    float* out; uint64_t out_stride;         // out: the window's first column (the column offset is added by the host)
    uint32_t long_min;                       // rows of this many entries and more are the long form's
    int out_vec;                             // the window's rows start at multiples of 16 bytes
    unsigned long long* words;               // [0] an id was not below x_rows, [1] long rows listed
};

// the n <= CPL valid columns at p (the rest read as 0)
template <int CPL, bool VEC> __device__ __forceinline__ void k12d_load(const float* __restrict__ p, uint32_t n, float (&v)[CPL]) {
    if (CPL == 4 && VEC && n == 4u) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[CPL > 1 ? 1 : 0] = t.y; v[CPL > 2 ? 2 : 0] = t.z; v[CPL > 3 ? 3 : 0] = t.w;
        return;
    }
#pragma unroll
    for (int k = 0; k < CPL; ++k) v[k] = (uint32_t)k < n ? p[k] : 0.0f;
}

template <int CPL> __device__ __forceinline__ void k12d_store(const K12D& a, uint64_t r, uint32_t c, uint32_t n, const float (&v)[CPL]) {
    float* p = a.out + r * a.out_stride + c;
    if (CPL == 4 && a.out_vec && n == 4u) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[CPL > 1 ? 1 : 0], v[CPL > 2 ? 2 : 0], v[CPL > 3 ? 3 : 0]); return; }
#pragma unroll
    for (int k = 0; k < CPL; ++k) if ((uint32_t)k < n) p[k] = v[k];
}

// R1's last step: v over the norm nn (0: the row stays as it is), nb the first NaN of the row, quieted (0: none)
__device__ __forceinline__ float k12d_divide(float v, double nn, uint32_t nb) {
    if (nb) return __uint_as_float(v != v ? (__float_as_uint(v) | kQuiet) : nb);
    if (nn == 0.0) return v;
    const float o = (float)((double)v / nn);
    return o != o ? __uint_as_float(0xFFC00000u) : o;      // inf / inf: the host's default NaN
}

// acc[k] <- the chain over entries [b, e) of a_col / a_val of a * x[id][c + k], k < n.  Called by whole wavefronts: the entries are read
// 64 a step, one per lane, and broadcast.
template <int CPL, bool VEC, uint32_t DEPTH>
__device__ __forceinline__ void k12d_walk(const K12D& a, uint64_t b, uint64_t e, uint32_t c, uint32_t n, uint32_t lane, float (&acc)[CPL], bool& bad) {
    for (uint64_t p0 = b; p0 < e; p0 += 64u) {
        const uint32_t m = (uint32_t)min((uint64_t)64u, e - p0);
        uint32_t id = 0;
        float av = 0.0f;
        if (lane < m) { id = a.a_col[p0 + lane]; av = a.a_val[p0 + lane]; }
        if (id >= a.x_rows) { bad = true; id = 0; }
        uint32_t j = 0;
        for (; j + DEPTH <= m; j += DEPTH) {
            float v[DEPTH][CPL];
#pragma unroll
            for (uint32_t u = 0; u < DEPTH; ++u) {
                const uint32_t row = (uint32_t)__shfl((int)id, (int)(j + u));
                k12d_load<CPL, VEC>(a.x + (uint64_t)row * a.x_stride + c, n, v[u]);
            }
#pragma unroll
            for (uint32_t u = 0; u < DEPTH; ++u) {
                const float y = __shfl(av, (int)(j + u));
#pragma unroll
                for (int k = 0; k < CPL; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(y, v[u][k]));
            }
        }
        for (; j < m; ++j) {
            float v[CPL];
            const uint32_t row = (uint32_t)__shfl((int)id, (int)j);
            k12d_load<CPL, VEC>(a.x + (uint64_t)row * a.x_stride + c, n, v);
            const float y = __shfl(av, (int)j);
#pragma unroll
            for (int k = 0; k < CPL; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(y, v[k]));
        }
    }
}

// One workgroup of blockDim.x / 64 <= 16 wavefronts per row of A: row row0 + blockIdx.x, or list[blockIdx.x] (the long form).
template <int CPL, bool VEC, bool NORM>
__global__ void __launch_bounds__(64 * kMaxWaves) k12d_rows(K12D a, uint64_t row0, const uint32_t* __restrict__ list) {
    __shared__ float s_v[kMaxWaves * 64 * CPL];
    __shared__ double s_norm;
    __shared__ uint32_t s_nan;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t r = list ? (uint64_t)list[blockIdx.x] : row0 + blockIdx.x;
    if (r >= a.rows) return;                               // (uniform)
    uint64_t b, e;
    row_span(a.a_ptr, r, a.nnz, b, e);
    if (!list && e - b >= a.long_min) return;              // (uniform) the long form's row
    const uint32_t pass_cols = blockDim.x * CPL;
    const uint32_t at = threadIdx.x * CPL;                 // this lane's first column inside a pass
    const uint32_t passes = (a.cols + pass_cols - 1) / pass_cols;
    bool bad = false;
    double s = 0.0;                                        // (wavefront 0) R1's chain from +0.0, and the first NaN of the row
    uint32_t nanb = 0;
    float acc[CPL];
    uint32_t c = 0, n = 0;
    for (uint32_t pass = 0; pass < passes; ++pass) {
        const uint32_t col0 = pass * pass_cols;
        c = col0 + at;
        n = c < a.cols ? min((uint32_t)CPL, a.cols - c) : 0u;
#pragma unroll
        for (int k = 0; k < CPL; ++k) acc[k] = 0.0f;
        if (col0 + w * 64u * CPL < a.cols) k12d_walk<CPL, VEC, (CPL == 1 ? kDepthLong : kDepth)>(a, b, e, c, n, lane, acc, bad);       // (uniform in a wavefront)
        if (NORM) {
#pragma unroll
            for (int k = 0; k < CPL; ++k) s_v[at + k] = (uint32_t)k < n ? acc[k] : 0.0f;
            __syncthreads();
            if (w == 0) {
                const uint32_t width = min(pass_cols, a.cols - col0);
                for (uint32_t f0 = 0; f0 < width; f0 += 64u) {
                    const uint32_t m = min(64u, width - f0);
                    const float v = lane < m ? s_v[f0 + lane] : 0.0f;
                    const unsigned long long mn = __ballot(v != v);
                    if (!nanb && mn) nanb = (uint32_t)__shfl((int)__float_as_uint(v), __ffsll((long long)mn) - 1) | kQuiet;
                    s = wave_chain(s, (double)__fmul_rn(v, v), m);
                }
            }
            __syncthreads();
        }
        if (!NORM || passes > 1) k12d_store<CPL>(a, r, c, n, acc);
    }
    if (bad) atomicMax(&a.words[0], 1ull);
    if (!NORM) return;
    if (threadIdx.x == 0) {
        s_norm = (nanb == 0 && s == 0.0) ? 0.0 : sqrt(s);
        s_nan = nanb;
    }
    __syncthreads();
    const double nn = s_norm;
    const uint32_t nb = s_nan;
    if (nb == 0 && nn == 0.0 && passes > 1) return;        // the row stays as the passes wrote it
    for (uint32_t pass = 0; pass < passes; ++pass) {
        if (passes > 1) {                                  // this lane's own stores of that pass
            c = pass * pass_cols + at;
            n = c < a.cols ? min((uint32_t)CPL, a.cols - c) : 0u;
            const float* p = a.out + r * a.out_stride + c;
#pragma unroll
            for (int k = 0; k < CPL; ++k) acc[k] = (uint32_t)k < n ? p[k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < CPL; ++k) acc[k] = k12d_divide(acc[k], nn, nb);
        k12d_store<CPL>(a, r, c, n, acc);
    }
}

// cols <= 128: lpr = 2^lpr_log2 lanes per row, 64 / lpr rows per wavefront, 4 wavefronts per workgroup
template <bool VEC, bool NORM>
__global__ void __launch_bounds__(256) k12d_narrow(K12D a, uint64_t row0, uint32_t lpr_log2) {
    const uint32_t lane = threadIdx.x & 63u, lpr = 1u << lpr_log2, per_wave = 64u >> lpr_log2;
    const uint64_t r0 = row0 + ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * per_wave;
    if (r0 >= a.rows) return;                              // (per wavefront: no workgroup barrier below)
    const uint64_t r = r0 + (lane >> lpr_log2);
    const uint32_t c = (lane & (lpr - 1u)) * 4u;
    uint64_t b = 0, e = 0;
    bool mine = r < a.rows;
    if (mine) {
        row_span(a.a_ptr, r, a.nnz, b, e);
        if (e - b >= a.long_min) { mine = false; e = b; }  // the long form's row
    }
    const uint32_t n = mine && c < a.cols ? min(4u, a.cols - c) : 0u;
    bool bad = false;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint64_t p0 = b; p0 < e; p0 += kDepth) {          // (per lane group; nothing crosses lanes in here)
        uint32_t id[kDepth];
        float av[kDepth], v[kDepth][4];
#pragma unroll
        for (uint32_t u = 0; u < kDepth; ++u) {
            const bool in = p0 + u < e;
            id[u] = in ? a.a_col[p0 + u] : 0u;
            av[u] = in ? a.a_val[p0 + u] : 0.0f;
            if (id[u] >= a.x_rows) { bad = true; id[u] = 0; }
        }
#pragma unroll
        for (uint32_t u = 0; u < kDepth; ++u) k12d_load<4, VEC>(a.x + (uint64_t)id[u] * a.x_stride + c, p0 + u < e ? n : 0u, v[u]);
#pragma unroll
        for (uint32_t u = 0; u < kDepth; ++u)
            if (p0 + u < e) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(av[u], v[u][k]));
            }
    }
    if (bad) atomicMax(&a.words[0], 1ull);
#pragma unroll
    for (int k = 0; k < 4; ++k) if ((uint32_t)k >= n) acc[k] = 0.0f;
    if (NORM) {                                            // every lane of a group walks the group's columns in order: the same chain
        double s = 0.0;
        uint32_t nanb = 0;
        for (uint32_t i = 0; i < lpr; ++i) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = __shfl(acc[k], (int)i, (int)lpr);
                if (v != v && !nanb) nanb = __float_as_uint(v) | kQuiet;
                s = __dadd_rn(s, (double)__fmul_rn(v, v));
            }
        }
        const double nn = (nanb == 0 && s == 0.0) ? 0.0 : sqrt(s);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = k12d_divide(acc[k], nn, nanb);
    }
    if (mine) k12d_store<4>(a, r, c, n, acc);
}

// words[1] <- rows of long_min entries and more, listed in `list` (any order: a row is a workgroup's own)
__global__ void __launch_bounds__(256)
k12d_classify(const uint64_t* __restrict__ ptr, uint64_t nnz, uint32_t rows, uint32_t long_min, uint32_t cap, uint32_t* __restrict__ list,
              unsigned long long* __restrict__ words) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= rows) return;
    uint64_t b, e;
    row_span(ptr, r, nnz, b, e);
    if (e - b < long_min) return;
    const unsigned long long i = atomicAdd(&words[1], 1ull);
    if (i < cap) list[i] = (uint32_t)r;
}

// dst[r, k] <- src[r, k], k < cols: Z into the right block of [E | Z]
__global__ void __launch_bounds__(256)
k12d_copy_block(const float* __restrict__ src, uint64_t src_stride, float* __restrict__ dst, uint64_t dst_stride, uint64_t rows, uint32_t cols) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= rows * cols) return;
    const uint64_t r = i / cols, k = i - r * cols;
    dst[r * dst_stride + k] = src[r * src_stride + k];
}

template <int CPL, bool NORM> auto rows_kernel(bool vec) { return vec ? k12d_rows<CPL, true, NORM> : k12d_rows<CPL, false, NORM>; }
template <bool NORM> auto narrow_kernel(bool vec) { return vec ? k12d_narrow<true, NORM> : k12d_narrow<false, NORM>; }

}  // namespace

void spmm_dense_device(const char* what, const QueriesDev& A, const float* x, uint64_t x_stride, uint32_t cols, float* out, uint64_t out_stride, uint64_t out_col0,
                       bool normalize, uint32_t long_min, hipStream_t s, EmbedDenseForms& forms) {
    if (A.rows == 0 || cols == 0) { XRL_HIP(hipStreamSynchronize(s)); return; }
    if (A.nnz && A.cols == 0) fail(std::string(what) + ": an entry names a column the matrix does not have");
    DevBuf words, list;
    words.reserve(16);
    XRL_HIP(hipMemsetAsync(words.p, 0, 16, s));
    const uint32_t cap = (uint32_t)std::min<uint64_t>(A.rows, A.nnz / long_min + 1);
    list.reserve((size_t)cap * 4);
    K12D a{A.row_ptr, A.col_idx, A.val, A.nnz, A.rows, A.cols, x, x_stride, cols, out + out_col0, out_stride, long_min, 0, words.as<unsigned long long>()};
    a.out_vec = (reinterpret_cast<uintptr_t>(a.out) % 16 == 0 && out_stride % 4 == 0) ? 1 : 0;
    const bool vec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && x_stride % 4 == 0;
    hipLaunchKernelGGL(k12d_classify, dim3(blocks_of(A.rows, 256, what)), dim3(256), 0, s, A.row_ptr, A.nnz, A.rows, long_min, cap, list.as<uint32_t>(),
                       words.as<unsigned long long>());
    XRL_LAUNCH_CHECK();
    const uint32_t quads = (cols + 3) / 4;
    if (quads <= 32) {
        uint32_t lg = 0;
        while ((1u << lg) < quads) ++lg;
        const uint64_t per_block = 4ull * (64u >> lg), per_launch = per_block << 22;
        auto* kernel = normalize ? narrow_kernel<true>(vec) : narrow_kernel<false>(vec);
        for (uint64_t r0 = 0; r0 < A.rows; r0 += per_launch) {
            hipLaunchKernelGGL(kernel, dim3(blocks_of(std::min<uint64_t>(per_launch, A.rows - r0), (uint32_t)per_block, what)), dim3(256), 0, s, a, r0, lg);
            XRL_LAUNCH_CHECK();
        }
    } else {
        const uint32_t waves = std::min<uint32_t>(kMaxWaves, (cols + 255) / 256);
        const uint64_t per_launch = (1ull << 31) / (64 * waves);                                        // a grid holds fewer than 2^32 threads
        auto* kernel = normalize ? rows_kernel<4, true>(vec) : rows_kernel<4, false>(vec);
        for (uint64_t r0 = 0; r0 < A.rows; r0 += per_launch) {
            hipLaunchKernelGGL(kernel, dim3((uint32_t)std::min<uint64_t>(per_launch, A.rows - r0)), dim3(64 * waves), 0, s, a, r0, (const uint32_t*)nullptr);
            XRL_LAUNCH_CHECK();
        }
    }
    uint64_t h[2] = {0, 0};
    XRL_HIP(hipMemcpyAsync(h, words.p, 16, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    const uint32_t n_long = (uint32_t)std::min<uint64_t>(h[1], cap);
    if (n_long) {
        const uint32_t waves = std::min<uint32_t>(kMaxWaves, (cols + 63) / 64);
        const uint32_t per_launch = (uint32_t)((1ull << 31) / (64 * waves));
        auto* kernel = normalize ? rows_kernel<1, true>(false) : rows_kernel<1, false>(false);
        for (uint32_t i0 = 0; i0 < n_long; i0 += per_launch) {
            hipLaunchKernelGGL(kernel, dim3(std::min(per_launch, n_long - i0)), dim3(64 * waves), 0, s, a, (uint64_t)0, list.as<uint32_t>() + i0);
            XRL_LAUNCH_CHECK();
        }
        XRL_HIP(hipMemcpyAsync(h, words.p, 8, hipMemcpyDeviceToHost, s));
    }
    XRL_HIP(hipStreamSynchronize(s));                      // the list goes with this scope
    if (h[0]) fail(std::string(what) + ": an entry names a column the matrix does not have");
    (quads <= 32 ? forms.narrow : forms.slab) += A.rows - n_long;
    forms.lng += n_long;
}

void copy_block_device(const char* what, const float* src, uint64_t src_stride, float* dst, uint64_t dst_stride, uint64_t rows, uint32_t cols, hipStream_t s) {
    if (rows == 0 || cols == 0) return;
    hipLaunchKernelGGL(k12d_copy_block, dim3(blocks_of(rows * cols, 256, what)), dim3(256), 0, s, src, src_stride, dst, dst_stride, rows, cols);
    XRL_LAUNCH_CHECK();
}

}  // namespace xrl
