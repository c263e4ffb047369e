// K11D: K11's "make the centre" and "score" for a dense row-major feature matrix in HBM, x[r * row_stride + f] (the rule: include/xrl_abi.h
// at xrl_run_clustering_device, on rows whose stored entries are all `cols` columns in ascending order; the reference: do_axpy and
// do_dot_product over dense_vec_t, matrix.hpp:862-868, 964-969, under clustering.hpp:224-401 at threads = 1).  The levels, the iterations,
// the split, the flags, the sampled levels' permutation and the codes are cluster_levels (xrl_cluster.hip), called, not copied.
//
// A dense matrix needs no layout: every run (node, feature) is a whole column of the node, and after a split each half of a node is
// sorted by id, so "the half's elements in stored order" are the half's positions of `elements` in order.  No keys, no sort, no scratch
// per entry: the centres are c[node * cols + f] (SKMEANS: the right half's sum, and c2 the left half's, until k11d_combine).
//   k11d_centre<SK>  one wavefront per (node, 64 consecutive features[, side]); lane l owns feature f0 + l, so a row's slice is one
//                    coalesced 256-byte read.  The half's element ids are read 64 a step, one per lane, and broadcast by readlane, so the
//                    row base is uniform.  The loads do not depend on the chain: kCentreBatch rows are requested before the first of
//                    their adds, only the adds are serial.
//   k11d_score       a workgroup of 128 lanes takes 128 consecutive positions of `elements` and walks the features 64 at a time: the
//                    [128 x 64] slice is read coalesced along the rows (wavefront w reads rows w, w + 2, ...; 64 loads in flight per
//                    lane) into registers while the lanes consume the previous slice from a padded LDS tile (row pitch 65 floats: both
//                    the row-wise store and the lane-per-row walk are free of bank conflicts); each lane walks its own row's chain.
//                    One-node form: every position of the tile is in one node, its centre slice is staged in LDS with the tile and
//                    broadcast.  Mixed form: the tile spans nodes, each lane reads its own node's centre from c.
// Offsets are 64-bit: rows * row_stride may exceed 2^32.  Every product and every addition is rounded on its own (__fmul_rn / __fadd_rn;
// the file is built with -ffp-contract=off).  MFMA has no place here: the order of the additions is the contract.
#include "xrl_cluster.h"
#include "xrl_device.h"
#include "xrl_devprim.h"

namespace xrl {
namespace {

constexpr const char* kWhat = "clustering";
constexpr uint32_t kNoElem = 0xFFFFFFFFu;
constexpr uint32_t kCentreBatch = 16;        // rows in flight ahead of a centre chain's adds
constexpr uint32_t kScoreTile = 128;         // positions per workgroup of k11d_score (= its lanes)
constexpr uint32_t kScoreFeat = 64;          // features per slice
constexpr uint32_t kScorePitch = kScoreFeat + 1;

struct K11DLevel : ClusterLevelDev {
    const float* x; uint64_t stride; uint32_t cols;
    float* c; float* c2;                     // [nodes * cols]
    unsigned long long* counts;              // {one-node tiles, mixed tiles, centre chains}
};

// iteration 0: the centre is x_r - x_l per feature (clustering.hpp:306-315, 362-372): (0 + v_r) + (-v_l)
__global__ void __launch_bounds__(256) k11d_first_centre(K11DLevel a, const uint32_t* __restrict__ r_pos, const uint32_t* __restrict__ l_pos) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)a.nodes * a.cols) return;
    const uint32_t nd = (uint32_t)(i / a.cols), f = (uint32_t)(i - (uint64_t)nd * a.cols);
    if (!a.active[nd]) return;
    const uint32_t er = a.elem[r_pos[nd]], el = a.elem[l_pos[nd]];
    if (er >= a.rows || el >= a.rows) return;
    a.c[i] = __fadd_rn(__fadd_rn(0.0f, a.x[(uint64_t)er * a.stride + f]), -a.x[(uint64_t)el * a.stride + f]);
}

// acc = acc + x[elem[p]][f] * alpha over p = b .. e-1 in order (MUL false: the plain sum, v * 1 is v); f is this lane's feature, ok
// whether it is below cols.  64 ids a step by lane, then kCentreBatch row slices requested before their adds.
template <bool MUL>
__device__ __forceinline__ float k11d_walk(const K11DLevel& a, float acc, uint32_t b, uint32_t e, float alpha, uint32_t f, bool ok, uint32_t lane) {
    for (uint32_t p0 = b; p0 < e; p0 += 64u) {
        const uint32_t n = min(64u, e - p0);
        uint32_t id = lane < n ? a.elem[p0 + lane] : 0u;
        if (id >= a.rows) id = 0u;
        uint32_t j = 0;
        for (; j + kCentreBatch <= n; j += kCentreBatch) {
            float v[kCentreBatch];
#pragma unroll
            for (uint32_t u = 0; u < kCentreBatch; ++u) {
                const uint32_t row = (uint32_t)__shfl((int)id, (int)(j + u));
                v[u] = ok ? a.x[(uint64_t)row * a.stride + f] : 0.0f;
            }
#pragma unroll
            for (uint32_t u = 0; u < kCentreBatch; ++u) acc = __fadd_rn(acc, MUL ? __fmul_rn(v[u], alpha) : v[u]);
        }
        for (; j < n; ++j) {
            const uint32_t row = (uint32_t)__shfl((int)id, (int)j);
            const float v = ok ? a.x[(uint64_t)row * a.stride + f] : 0.0f;
            acc = __fadd_rn(acc, MUL ? __fmul_rn(v, alpha) : v);
        }
    }
    return acc;
}

// One wavefront per (node, tile of 64 features) and, SKMEANS, per side.  KMEANS (clustering.hpp:317-324): one accumulator, the right
// half's rows then the left half's, each alpha * v.  SKMEANS (:374-380): one plain sum per side.
template <bool SK> __global__ void __launch_bounds__(256) k11d_centre(K11DLevel a, const float* __restrict__ alpha, uint32_t tiles) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    constexpr uint32_t kSides = SK ? 2u : 1u;
    if (w >= (uint64_t)a.nodes * tiles * kSides) return;
    const uint32_t side = (uint32_t)(w % kSides), tile = (uint32_t)((w / kSides) % tiles), nd = (uint32_t)(w / kSides / tiles);
    if (!a.active[nd]) return;
    const uint32_t f = tile * 64u + lane;
    const bool ok = f < a.cols;
    const uint32_t b = a.beg[nd], wend = a.work_end[nd], mid = (uint32_t)(((uint64_t)b + wend) >> 1);
    float acc = 0.0f;
    if (SK) {
        acc = side ? k11d_walk<false>(a, acc, b, mid, 1.0f, f, ok, lane) : k11d_walk<false>(a, acc, mid, wend, 1.0f, f, ok, lane);
    } else {
        acc = k11d_walk<true>(a, acc, mid, wend, alpha[2 * nd], f, ok, lane);
        acc = k11d_walk<true>(a, acc, b, mid, alpha[2 * nd + 1], f, ok, lane);
    }
    if (ok) (side ? a.c2 : a.c)[(uint64_t)nd * a.cols + f] = acc;
    if (lane == 0) atomicAdd(a.counts + 2, (unsigned long long)min(64u, a.cols - tile * 64u));
}

// One wavefront per (side, node): ||c||^2 as one fp32 chain of c[f] * c[f] in ascending f (matrix.hpp:862-868), then the scale
// 1.0 / sqrt((double)||c||^2) when it is positive (clustering.hpp:375-384); -1 stands for "not scaled", as in k11_norm.
__global__ void __launch_bounds__(256) k11d_norm(K11DLevel a, double* __restrict__ scale) {
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= 2 * a.nodes) return;
    const uint32_t side = w / a.nodes, nd = w - side * a.nodes;      // side 0: right (c), side 1: left (c2)
    if (!a.active[nd]) return;
    const float* c = (side ? a.c2 : a.c) + (uint64_t)nd * a.cols;
    float acc = 0.0f;
    for (uint32_t f0 = 0; f0 < a.cols; f0 += 64u) {
        const uint32_t f = f0 + lane;
        float p = 0.0f;
        if (f < a.cols) { const float v = c[f]; p = __fmul_rn(v, v); }
        acc = wave_chain(acc, p, min(64u, a.cols - f0));
    }
    if (lane == 0) scale[w] = acc > 0.0f ? 1.0 / sqrt((double)acc) : -1.0;
}

// c = c1 * s1 - c2 * s2, each scaled value the double product rounded to float (matrix.hpp:1027-1047), the difference c1 + (-c2)
__global__ void __launch_bounds__(256) k11d_combine(K11DLevel a, const double* __restrict__ scale) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)a.nodes * a.cols) return;
    const uint32_t nd = (uint32_t)(i / a.cols);
    if (!a.active[nd]) return;
    const double s1 = scale[nd], s2 = scale[a.nodes + nd];
    float c1 = a.c[i], c2 = a.c2[i];
    if (s1 >= 0.0) c1 = (float)((double)c1 * s1);
    if (s2 >= 0.0) c2 = (float)((double)c2 * s2);
    a.c[i] = __fadd_rn(c1, -c2);
}

// score[e] = the chain from +0 over f = 0 .. cols-1 of c[node(e)][f] * x[e][f] (matrix.hpp:870-877); `end`: the end of each node's
// scored range.  See the file header for the tile.
__global__ void __launch_bounds__(kScoreTile) k11d_score(K11DLevel a, const uint32_t* __restrict__ end) {
    __shared__ float s_x[kScoreTile * kScorePitch];
    __shared__ float s_c[kScoreFeat];
    __shared__ uint32_t s_row[kScoreTile];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint32_t p0 = blockIdx.x * kScoreTile, p = p0 + t;
    const uint32_t last = min(p0 + kScoreTile, a.rows) - 1u;
    const uint32_t nd0 = segment_of(a.beg, a.nodes, p0);
    const bool one = a.beg[nd0 + 1] > last;                          // uniform: the whole tile lies in node nd0
    if (one && (!a.active[nd0] || p0 >= end[nd0])) return;           // uniform: nothing of the tile is scored
    uint32_t nd = nd0, e = kNoElem;
    if (p <= last) {
        if (!one) nd = segment_of(a.beg, a.nodes, p);
        if (a.active[nd] && p < end[nd]) { e = a.elem[p]; if (e >= a.rows) e = kNoElem; }
    }
    s_row[t] = e;
    if (!__syncthreads_or(e != kNoElem)) return;                     // a tile of converged nodes
    if (t == 0) atomicAdd(a.counts + (one ? 0 : 1), 1ull);
    const float* cn = a.c + (uint64_t)nd * a.cols;

    float pre[kScoreFeat], cpre = 0.0f;
    auto request = [&](uint32_t f0) {
        const uint32_t f = f0 + lane;
        const bool ok = f < a.cols;
#pragma unroll
        for (uint32_t i = 0; i < kScoreFeat; ++i) {
            const uint32_t row = s_row[2u * i + wv];
            pre[i] = ok && row != kNoElem ? a.x[(uint64_t)row * a.stride + f] : 0.0f;
        }
        if (one && wv == 0) cpre = ok ? cn[f] : 0.0f;
    };
    request(0);
    float acc = 0.0f;
    for (uint32_t f0 = 0; f0 < a.cols; f0 += kScoreFeat) {
        __syncthreads();                                              // the previous slice has been consumed
#pragma unroll
        for (uint32_t i = 0; i < kScoreFeat; ++i) s_x[(2u * i + wv) * kScorePitch + lane] = pre[i];
        if (one && wv == 0) s_c[lane] = cpre;
        __syncthreads();
        if (f0 + kScoreFeat < a.cols) request(f0 + kScoreFeat);     // in flight under the walk below
        const uint32_t n = min(kScoreFeat, a.cols - f0);
        if (e != kNoElem) {
            const float* row = s_x + t * kScorePitch;
            if (one) for (uint32_t j = 0; j < n; ++j) acc = __fadd_rn(acc, __fmul_rn(s_c[j], row[j]));
            else for (uint32_t j = 0; j < n; ++j) acc = __fadd_rn(acc, __fmul_rn(cn[f0 + j], row[j]));
        }
    }
    if (e != kNoElem) a.score[e] = acc;
}

uint32_t grid(uint64_t n) { return blocks_of(n ? n : 1, 256, kWhat); }

struct DenseFeatures final : ClusterFeatures {
    const std::string what;
    const bool SK;
    K11DLevel a{};
    uint64_t cells = 0;                     // nodes * cols
    DevBuf c, c2, scale, counts;

    DenseFeatures(const std::string& what_, const float* base, uint64_t cols, uint64_t stride, bool SK_, hipStream_t s) : what(what_), SK(SK_) {
        a.x = base; a.stride = stride; a.cols = (uint32_t)cols;
        counts.reserve(24);
        XRL_HIP(hipMemsetAsync(counts.p, 0, 24, s));
        a.counts = counts.as<unsigned long long>();
    }

    void begin_level(uint32_t d, const ClusterLevel&, const ClusterLevelDev& lvl, hipStream_t s) override {
        static_cast<ClusterLevelDev&>(a) = lvl;
        cells = (uint64_t)lvl.nodes * a.cols;
        // scratch of one level beyond what the split needs per row: the centres, 4 bytes per (node, feature), twice for SKMEANS, and
        // the two scales per node
        const uint64_t need = (SK ? 8ull : 4ull) * cells + 16ull * lvl.nodes + 64;
        size_t free_b = 0, total_b = 0;
        XRL_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b + c.cap + c2.cap + scale.cap)
            fail(what + "the centres of level " + std::to_string(d) + " need " + std::to_string(need) + " bytes of scratch, " + std::to_string(free_b) + " are free");
        c.reserve(((size_t)cells + 1) * 4);
        XRL_HIP(hipMemsetAsync(c.p, 0, ((size_t)cells + 1) * 4, s));       // max_iter = 0: the final assignment scores with a zero centre
        if (SK) { c2.reserve(((size_t)cells + 1) * 4); scale.reserve((size_t)lvl.nodes * 16); }
        a.c = c.as<float>(); a.c2 = c2.as<float>();
    }

    void first_centre(const uint32_t* r_pos, const uint32_t* l_pos, hipStream_t s) override {
        hipLaunchKernelGGL(k11d_first_centre, dim3(grid(cells)), dim3(256), 0, s, a, r_pos, l_pos);
        XRL_LAUNCH_CHECK();
    }

    void centre(const float* alpha, hipStream_t s) override {
        const uint32_t tiles = (a.cols + 63u) / 64u;
        const uint64_t waves = (uint64_t)a.nodes * tiles * (SK ? 2u : 1u);
        if (!waves) return;
        if (!SK) {
            hipLaunchKernelGGL(k11d_centre<false>, dim3(blocks_of(waves, 4, kWhat)), dim3(256), 0, s, a, alpha, tiles);
            XRL_LAUNCH_CHECK();
            return;
        }
        hipLaunchKernelGGL(k11d_centre<true>, dim3(blocks_of(waves, 4, kWhat)), dim3(256), 0, s, a, (const float*)nullptr, tiles);
        XRL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k11d_norm, dim3(blocks_of(2ull * a.nodes, 4, kWhat)), dim3(256), 0, s, a, scale.as<double>());
        XRL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k11d_combine, dim3(grid(cells)), dim3(256), 0, s, a, scale.as<double>());
        XRL_LAUNCH_CHECK();
    }

    void score(const uint32_t* end, hipStream_t s) override {
        hipLaunchKernelGGL(k11d_score, dim3(blocks_of(a.rows, kScoreTile, kWhat)), dim3(kScoreTile), 0, s, a, end);
        XRL_LAUNCH_CHECK();
    }
};

}  // namespace

void cluster_dense_device(const char* what_c, const float* base, uint64_t rows, uint64_t cols, uint64_t row_stride, const ClusterPlan& plan,
                          const ClusteringParam& param, uint32_t* d_codes, float* d_scores, hipStream_t s, ClusterForms& forms) {
    const std::string what = std::string(what_c) + ": ";
    if (rows != plan.rows) fail(what + "the plan is for another row count");
    if (row_stride < cols) fail(what + "row_stride " + std::to_string(row_stride) + " is below cols " + std::to_string(cols));
    if (cols > 0xFFFFFFC0ull) fail(what + "too many columns");
    forms = ClusterForms{};
    DenseFeatures feat(what, base, cols, row_stride, param.partition_algo == 5, s);
    cluster_levels(plan, param, feat, d_codes, d_scores, s, forms);
    unsigned long long h[3] = {0, 0, 0};
    XRL_HIP(hipMemcpyAsync(h, feat.counts.p, 24, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    forms.one_node_tiles = h[0]; forms.mixed_tiles = h[1]; forms.centre_chains = h[2];
}

}  // namespace xrl
