// K11: balanced hierarchical 2-means on the device, all nodes of a level in the same launches (the rule: include/xrl_abi.h at
// xrl_run_clustering_device; the reference: pecos/core/utils/clustering.hpp:189-503 at threads = 1).
//
// Once per level: k11_rowlen + scan + k11_expand write one 64-bit key (feature, element id) per stored entry of X, in the order of
//   `elements`; one segmented radix sort (segments = the nodes' entry ranges) orders them per node by (feature, element id);
//   k11_heads / scan / k11_runs find the runs (node, feature) and store, per entry of X, the run it belongs to.  The layout is fixed
//   for the level: only the side of each element (its position against the node's midpoint) changes between iterations.
// Per iteration: k11_centre walks every run as one ordered chain -- 64 runs per wavefront, a run below 64 entries by its lane, a longer
//   one by the whole wavefront (64 entries loaded per step, added in order through readlane); SKMEANS then takes the two norms
//   (k11_norm, one wavefront per node and side, in run order or, past the switch, in the order of first touch, which one segmented
//   sort per iteration provides) and k11_combine scales and subtracts; k11_score is one chain per element over its entries;
//   the split is a segmented sort of (score key, id), a segmented sort of each half by id, and k11_commit's "changed" flag per node.
//   The host reads the nodes' flags once per iteration; converged nodes are skipped by every kernel.
// Every product and every addition is rounded on its own (__fmul_rn / __fadd_rn; the file is built with -ffp-contract=off).
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "xrl_cluster.h"
#include "xrl_device.h"
#include "xrl_devprim.h"

namespace xrl {
namespace {

constexpr const char* kWhat = "clustering";
constexpr uint32_t kNoElem = 0xFFFFFFFFu;

struct K11Level {
    // X
    const uint64_t* x_ptr; const float* x_val;
    uint32_t rows;
    // elements
    uint32_t* elem; uint32_t* pos_of; float* score;
    // the level's nodes
    uint32_t nodes;
    const uint32_t* beg;        // [nodes + 1]
    const uint32_t* work_end;   // [nodes]  end of the range the iterations work on
    const uint32_t* active;     // [nodes]
    // the level's layout
    const uint64_t* keys;       // [nnz] sorted (feature << 32 | element id), per node
    const uint32_t* xent;       // [nnz] the entry of X behind each key
    const uint32_t* run_start;  // [runs + 1]
    const uint32_t* run_node;   // [runs]
    const uint32_t* run_of;     // [nnz of X] run of each entry of X
    const uint32_t* node_run;   // [nodes + 1]
    uint32_t runs;
    float* c; float* c2;        // [runs] the centre (SKMEANS: the right side's sum until k11_combine); the left side's sum
    uint32_t* first;            // [2 * runs] lowest element id of the right / left side in the run (kNoElem: none)
};

__global__ void __launch_bounds__(256)
k11_check(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ col, uint32_t rows, uint32_t cols, uint64_t nnz, uint32_t* __restrict__ bad) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= rows) return;
    const uint64_t b = ptr[r], e = ptr[r + 1];
    if (b > e || e > nnz || (r == 0 && b != 0) || (r == rows - 1 && e != nnz)) { atomicOr(bad, 2u); return; }
    for (uint64_t j = b; j < e; ++j)
        if (col[j] >= cols || (j > b && col[j] <= col[j - 1])) { atomicOr(bad, 1u); return; }
}

__global__ void __launch_bounds__(256) k11_iota(uint32_t* __restrict__ a, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) a[i] = i;
}

__global__ void __launch_bounds__(256) k11_gather(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) { const uint32_t p = perm[i]; out[i] = p < n ? in[p] : 0u; }
}

// pos_of and the entry count of each position's row
__global__ void __launch_bounds__(256)
k11_rowlen(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ elem, uint32_t n, uint32_t* __restrict__ pos_of, uint32_t* __restrict__ len) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t e = elem[p];
    if (e >= n) { len[p] = 0; return; }
    pos_of[e] = p;
    len[p] = (uint32_t)(ptr[e + 1] - ptr[e]);
}

// one wavefront per position
__global__ void __launch_bounds__(256)
k11_expand(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ col, const uint32_t* __restrict__ elem, const uint32_t* __restrict__ ent_off, uint32_t n,
           uint64_t* __restrict__ keys, uint32_t* __restrict__ xent) {
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (p >= n) return;
    const uint32_t e = elem[p];
    if (e >= n) return;
    const uint64_t b = ptr[e];
    const uint32_t o = ent_off[p], len = ent_off[p + 1] - o;
    for (uint32_t j = lane; j < len; j += 64u) { keys[o + j] = ((uint64_t)col[b + j] << 32) | e; xent[o + j] = (uint32_t)(b + j); }
}

__global__ void __launch_bounds__(256)
k11_node_ent(const uint32_t* __restrict__ beg, const uint32_t* __restrict__ ent_off, uint32_t nodes, uint32_t* __restrict__ node_ent) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i <= nodes) node_ent[i] = ent_off[beg[i]];
}

__global__ void __launch_bounds__(256)
k11_heads(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ node_ent, uint32_t nodes, uint32_t total, uint32_t* __restrict__ flag) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= total) return;
    const uint32_t b = node_ent[segment_of(node_ent, nodes, x)];
    flag[x] = (x == b || (uint32_t)(keys[x] >> 32) != (uint32_t)(keys[x - 1] >> 32)) ? 1u : 0u;
}

__global__ void __launch_bounds__(256)
k11_runs(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ slot, const uint32_t* __restrict__ xent, const uint32_t* __restrict__ node_ent, uint32_t nodes,
         uint32_t total, uint32_t runs, uint32_t* __restrict__ run_of, uint32_t* __restrict__ run_start, uint32_t* __restrict__ run_node) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x == 0) run_start[runs] = total;
    if (x >= total) return;
    const uint32_t f = flag[x], r = slot[x] + f - 1u;
    if (r >= runs) return;
    run_of[xent[x]] = r;
    if (f) { run_start[r] = x; run_node[r] = segment_of(node_ent, nodes, x); }
}

__global__ void __launch_bounds__(256)
k11_node_run(const uint32_t* __restrict__ node_ent, const uint32_t* __restrict__ slot, uint32_t nodes, uint32_t* __restrict__ node_run) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i <= nodes) node_run[i] = slot[node_ent[i]];
}

__global__ void __launch_bounds__(256) k11_count_forms(const uint32_t* __restrict__ run_start, uint32_t runs, unsigned long long* __restrict__ out) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const bool ok = r < runs;
    const bool wave = ok && run_start[r + 1] - run_start[r] >= kClusterWaveRun;
    const unsigned long long mw = __ballot(wave), ml = __ballot(ok && !wave);
    if ((threadIdx.x & 63u) == 0) {
        if (ml) atomicAdd(out, (unsigned long long)__popcll(ml));
        if (mw) atomicAdd(out + 1, (unsigned long long)__popcll(mw));
    }
}

// iteration 0: the centre is x_r - x_l per feature (clustering.hpp:306-315, 362-372): (0 + v_r) + (-v_l)
__global__ void __launch_bounds__(256) k11_first_centre(K11Level a, const uint32_t* __restrict__ r_pos, const uint32_t* __restrict__ l_pos) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.runs) return;
    const uint32_t nd = a.run_node[r];
    if (!a.active[nd]) return;
    const uint32_t b = a.run_start[r], n = a.run_start[r + 1] - b;
    const uint64_t f = a.keys[b] & 0xFFFFFFFF00000000ull;
    const uint32_t er = a.elem[r_pos[nd]], el = a.elem[l_pos[nd]];
    float c = 0.0f;
    uint32_t at = lower_bound(a.keys + b, n, f | er);
    if (at < n && a.keys[b + at] == (f | er)) c = __fadd_rn(c, a.x_val[a.xent[b + at]]);
    at = lower_bound(a.keys + b, n, f | el);
    if (at < n && a.keys[b + at] == (f | el)) c = __fadd_rn(c, -a.x_val[a.xent[b + at]]);
    a.c[r] = c;
}

// which side of its node an element is on: 1 right, 0 left, 2 outside the sampled range
__device__ __forceinline__ uint32_t side_of(const K11Level& a, uint32_t e, uint32_t wend, uint32_t mid) {
    const uint32_t pos = a.pos_of[e];
    return pos >= wend ? 2u : (pos >= mid ? 1u : 0u);
}

// One wavefront per 64 runs.  KMEANS (clustering.hpp:317-324): one accumulator, the right side's entries then the left side's, each
// alpha * v.  SKMEANS (:374-380): one accumulator per side, alpha = 1 (v * 1 is v).
template <bool SK> __global__ void __launch_bounds__(256) k11_centre(K11Level a, const float* __restrict__ alpha) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u + lane;
    bool valid = r < a.runs;
    uint32_t nd = 0, b = 0, e = 0, wend = 0, mid = 0;
    float aR = 1.0f, aL = 1.0f;
    if (valid) {
        nd = a.run_node[r];
        valid = a.active[nd] != 0;
        b = a.run_start[r]; e = a.run_start[r + 1];
        wend = a.work_end[nd]; mid = (uint32_t)(((uint64_t)a.beg[nd] + wend) >> 1);
        if (!SK) { aR = alpha[2 * nd]; aL = alpha[2 * nd + 1]; }
    }
    const bool wave = valid && e - b >= kClusterWaveRun;
    float accR = 0.0f, accL = 0.0f;
    uint32_t firstR = kNoElem, firstL = kNoElem;
    if (valid && !wave) {
        if (SK) {
            for (uint32_t x = b; x < e; ++x) {
                const uint32_t el = (uint32_t)a.keys[x], sd = side_of(a, el, wend, mid);
                if (sd == 2u) continue;
                const float v = a.x_val[a.xent[x]];
                if (sd) { accR = __fadd_rn(accR, v); if (firstR == kNoElem) firstR = el; }
                else { accL = __fadd_rn(accL, v); if (firstL == kNoElem) firstL = el; }
            }
        } else {
            for (uint32_t want = 2; want-- > 0;)
                for (uint32_t x = b; x < e; ++x) {
                    const uint32_t el = (uint32_t)a.keys[x];
                    if (side_of(a, el, wend, mid) != want) continue;
                    accR = __fadd_rn(accR, __fmul_rn(a.x_val[a.xent[x]], want ? aR : aL));
                }
        }
    }
    unsigned long long todo = __ballot(wave);
    while (todo) {
        const int i = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t wb = __shfl(b, i), we = __shfl(e, i), wwend = __shfl(wend, i), wmid = __shfl(mid, i);
        const float waR = __shfl(aR, i), waL = __shfl(aL, i);
        float sR = 0.0f, sL = 0.0f;
        uint32_t fR = kNoElem, fL = kNoElem;
        for (uint32_t pass = 0; pass < (SK ? 1u : 2u); ++pass)
            for (uint32_t x0 = wb; x0 < we; x0 += 64u) {
                const uint32_t x = x0 + lane;
                uint32_t el = 0, sd = 2u;
                float v = 0.0f;
                if (x < we) { el = (uint32_t)a.keys[x]; sd = side_of(a, el, wwend, wmid); v = a.x_val[a.xent[x]]; }
                if (SK) {
                    unsigned long long mR = __ballot(sd == 1u), mL = __ballot(sd == 0u);
                    if (fR == kNoElem && mR) fR = __shfl(el, __ffsll((long long)mR) - 1);
                    if (fL == kNoElem && mL) fL = __shfl(el, __ffsll((long long)mL) - 1);
                    for (; mR; mR &= mR - 1) sR = __fadd_rn(sR, __shfl(v, __ffsll((long long)mR) - 1));
                    for (; mL; mL &= mL - 1) sL = __fadd_rn(sL, __shfl(v, __ffsll((long long)mL) - 1));
                } else {
                    const uint32_t want = 1u - pass;
                    const float p = __fmul_rn(v, want ? waR : waL);
                    for (unsigned long long m = __ballot(sd == want); m; m &= m - 1) sR = __fadd_rn(sR, __shfl(p, __ffsll((long long)m) - 1));
                }
            }
        if ((int)lane == i) { accR = sR; accL = sL; firstR = fR; firstL = fL; }
    }
    if (!valid) return;
    a.c[r] = accR;
    if (SK) { a.c2[r] = accL; a.first[r] = firstR; a.first[a.runs + r] = firstL; }
}

// first-touch order of a node's runs, per side: (lowest element id of the side in the run, feature); runs the side never touched go last
__global__ void __launch_bounds__(256) k11_norm_keys(const uint32_t* __restrict__ first, uint32_t runs2, uint32_t runs, uint64_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < runs2) keys[i] = ((uint64_t)first[i] << 32) | (i < runs ? i : i - runs);
}

__global__ void __launch_bounds__(256) k11_norm_segs(const uint32_t* __restrict__ node_run, uint32_t nodes, uint32_t runs, uint32_t* __restrict__ seg) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < nodes) { seg[i] = node_run[i]; seg[nodes + i] = runs + node_run[i]; }
    if (i == 0) seg[2 * nodes] = 2 * runs;
}

// One wavefront per (side, node): ||c||^2 as one fp32 chain of c[f] * c[f] (matrix.hpp:862-868, or :886-897 past the switch), then the
// scale 1.0 / sqrt((double)||c||^2) when it is positive (clustering.hpp:375-384).  A chain that overflows to +inf is positive: its scale
// is 1.0 / inf = 0.0 and the centre becomes zeros, as the reference's does.  -1 stands for "not scaled": a real scale is never negative.
__global__ void __launch_bounds__(256) k11_norm(K11Level a, const uint64_t* __restrict__ order /* null: run order */, double* __restrict__ scale) {
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= 2 * a.nodes) return;
    const uint32_t side = w / a.nodes, nd = w - side * a.nodes;      // side 0: right (c), side 1: left (c2)
    if (!a.active[nd]) return;
    const float* c = side ? a.c2 : a.c;
    const uint32_t b = a.node_run[nd], e = a.node_run[nd + 1];
    float acc = 0.0f;
    for (uint32_t x0 = b; x0 < e; x0 += 64u) {
        const uint32_t x = x0 + lane;
        float p = 0.0f;
        if (x < e) { const float v = c[order ? (uint32_t)order[(uint64_t)side * a.runs + x] : x]; p = __fmul_rn(v, v); }
        const uint32_t n = min(64u, e - x0);
        acc = wave_chain(acc, p, n);
    }
    if (lane == 0) scale[w] = acc > 0.0f ? 1.0 / sqrt((double)acc) : -1.0;
}

// c = c1 * s1 - c2 * s2, each scaled value the double product rounded to float (matrix.hpp:1027-1047), the difference c1 + (-c2)
__global__ void __launch_bounds__(256) k11_combine(K11Level a, const double* __restrict__ scale) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.runs) return;
    const uint32_t nd = a.run_node[r];
    if (!a.active[nd]) return;
    const double s1 = scale[nd], s2 = scale[a.nodes + nd];
    float c1 = a.c[r], c2 = a.c2[r];
    if (s1 >= 0.0) c1 = (float)((double)c1 * s1);
    if (s2 >= 0.0) c2 = (float)((double)c2 * s2);
    a.c[r] = __fadd_rn(c1, -c2);
}

// score[e] = the chain over row e's stored entries of c[f] * v (matrix.hpp:870-877); `end`: the end of each node's scored range
__global__ void __launch_bounds__(256) k11_score(K11Level a, const uint32_t* __restrict__ end) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.rows) return;
    const uint32_t nd = segment_of(a.beg, a.nodes, p);
    if (!a.active[nd] || p >= end[nd]) return;
    const uint32_t e = a.elem[p];
    float acc = 0.0f;
    for (uint64_t j = a.x_ptr[e], je = a.x_ptr[e + 1]; j < je; ++j) acc = __fadd_rn(acc, __fmul_rn(a.c[a.run_of[j]], a.x_val[j]));
    a.score[e] = acc;
}

// the split's sort keys and segments: the scored range of every active node, and its two halves
__global__ void __launch_bounds__(256)
k11_split_keys(K11Level a, const uint32_t* __restrict__ end, uint64_t* __restrict__ keys, uint32_t* __restrict__ seg_b, uint32_t* __restrict__ seg_e,
               uint32_t* __restrict__ half_b, uint32_t* __restrict__ half_e) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < a.nodes) {
        const uint32_t b = a.beg[p], e = a.active[p] ? end[p] : b, mid = (uint32_t)(((uint64_t)b + e) >> 1);
        seg_b[p] = b; seg_e[p] = e;
        half_b[2 * p] = b; half_e[2 * p] = mid; half_b[2 * p + 1] = mid; half_e[2 * p + 1] = e;
    }
    if (p >= a.rows) return;
    const uint32_t e = a.elem[p];
    keys[p] = ((uint64_t)score_key(a.score[e]) << 32) | e;
}

__global__ void __launch_bounds__(256) k11_split_ids(const uint64_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ ids) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < n) ids[p] = (uint32_t)keys[p];
}

// the new order of every active node's scored range; changed[node] when its first half differs from what it was (clustering.hpp:202-212)
__global__ void __launch_bounds__(256) k11_commit(K11Level a, const uint32_t* __restrict__ end, const uint32_t* __restrict__ ids, uint32_t* __restrict__ changed) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.rows) return;
    const uint32_t nd = segment_of(a.beg, a.nodes, p);
    if (!a.active[nd] || p >= end[nd]) return;
    const uint32_t b = a.beg[nd], mid = (uint32_t)(((uint64_t)b + end[nd]) >> 1), e = ids[p];
    if (e >= a.rows) return;
    if (p < mid && a.elem[p] != e) changed[nd] = 1u;
    a.elem[p] = e;
    a.pos_of[e] = p;
}

__global__ void __launch_bounds__(256) k11_flags(uint32_t* __restrict__ active, uint32_t* __restrict__ changed, uint32_t nodes) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < nodes) { active[i] = active[i] && changed[i] ? 1u : 0u; changed[i] = 0u; }
}

__global__ void __launch_bounds__(256)
k11_codes(const uint32_t* __restrict__ elem, const uint32_t* __restrict__ leaf_beg, uint32_t leaves, uint32_t n, uint32_t* __restrict__ codes) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t e = elem[p];
    if (e < n) codes[e] = segment_of(leaf_beg, leaves, p);
}

uint32_t grid(uint64_t n) { return blocks_of(n ? n : 1, 256, kWhat); }

}  // namespace

void cluster_device(const char* what_c, const QueriesDev& X, const ClusterPlan& plan, const ClusteringParam& param, uint32_t* d_codes, float* d_scores,
                    hipStream_t s, ClusterForms& forms) {
    const std::string what = std::string(what_c) + ": ";
    const uint32_t L = plan.rows, depth = plan.depth;
    const uint64_t nnz = X.nnz;
    const bool SK = param.partition_algo == 5;
    if (X.dense || !X.row_ptr) fail(what + "the feature matrix must be a CSR");
    if (X.rows != L) fail(what + "the plan is for another row count");
    if (nnz > 0xFFFFFFF0ull) fail(what + "more than 2^32 - 16 stored entries");
    forms = ClusterForms{};
    forms.switch_level = SK ? plan.switch_level : kClusterNoSwitch;
    forms.iters.assign(depth, 0u);

    // scratch of one level: per entry two 8-byte keys, two entry ids, the head flag, its scan and the run id (36 bytes), then per run
    // up to 60 bytes; per row 48
    size_t free_b = 0, total_b = 0;
    XRL_HIP(hipMemGetInfo(&free_b, &total_b));
    const uint64_t need_entries = 36ull * nnz + 48ull * L + (64ull << 10) * 2;
    if (need_entries > free_b) fail(what + "the scratch of one level needs " + std::to_string(need_entries) + " bytes, " + std::to_string(free_b) + " are free");

    DevBuf bad, tmp;
    bad.reserve(4);
    XRL_HIP(hipMemsetAsync(bad.p, 0, 4, s));
    hipLaunchKernelGGL(k11_check, dim3(grid(L)), dim3(256), 0, s, X.row_ptr, X.col_idx, L, X.cols, nnz, bad.as<uint32_t>());
    XRL_LAUNCH_CHECK();
    uint32_t h_bad = 0;
    XRL_HIP(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    if (h_bad & 2u) fail(what + "row pointers must ascend from 0 to nnz");
    if (h_bad) fail(what + "a row's column ids must be strictly ascending and below cols");

    DevBuf elem, elem2, ids, pos_of, score, len, ent_off, keys, keys2, xent, xent2, flag, slot, run_of, skeys, skeys2;
    DevBuf beg, work_end, whole_end, active, changed, r_pos, l_pos, alpha, perm, node_ent, node_run, seg, half, counts, leaf_beg;
    DevBuf run_start, run_node, c, c2, first, nkeys, nkeys2, nseg, scale;
    for (DevBuf* b : {&elem, &elem2, &ids, &pos_of, &score, &len, &ent_off}) b->reserve(((size_t)L + 1) * 4);
    skeys.reserve((size_t)L * 8); skeys2.reserve((size_t)L * 8);
    keys.reserve((size_t)nnz * 8); keys2.reserve((size_t)nnz * 8);
    xent.reserve((size_t)nnz * 4); xent2.reserve((size_t)nnz * 4); run_of.reserve((size_t)nnz * 4);
    flag.reserve(((size_t)nnz + 1) * 4); slot.reserve(((size_t)nnz + 1) * 4);
    counts.reserve(16);
    XRL_HIP(hipMemsetAsync(counts.p, 0, 16, s));
    XRL_HIP(hipMemsetAsync(score.p, 0, (size_t)L * 4, s));
    hipLaunchKernelGGL(k11_iota, dim3(grid(L)), dim3(256), 0, s, elem.as<uint32_t>(), L);
    XRL_LAUNCH_CHECK();

    auto seg_sort = [&](auto&& call) { with_rocprim_tmp(tmp, call); ++forms.seg_sorts; };
    // the sorts look only at the key bits that can differ: a feature id is below cols, an element id below L
    auto bits_of = [](uint64_t below) { unsigned b = 1; while (b < 32 && ((below - 1) >> b)) ++b; return b; };
    const unsigned feature_bits = bits_of(std::max<uint64_t>(X.cols, 1)), element_bits = bits_of(L);

    for (uint32_t d = 0; d < depth; ++d) {
        const ClusterLevel& lv = plan.levels[d];
        const uint32_t nodes = 1u << d;
        XRL_HIP(hipStreamSynchronize(s));              // the uploads below reuse what the last level's kernels read
        beg.upload(lv.beg); work_end.upload(lv.work_end);
        whole_end.upload_raw(lv.beg.data() + 1, (size_t)nodes * 4);
        std::vector<uint32_t> h_active(nodes, 1u);
        active.upload(h_active);
        changed.reserve((size_t)nodes * 4);
        XRL_HIP(hipMemsetAsync(changed.p, 0, (size_t)nodes * 4, s));
        if (param.kmeans_max_iter) { r_pos.upload(lv.r_pos); l_pos.upload(lv.l_pos); }
        if (!SK) {
            // alpha_R = float(1.0 / |right|), alpha_L = float(-1.0 / |left|) (clustering.hpp:318-323)
            std::vector<float> h_alpha(2 * (size_t)nodes);
            for (uint32_t i = 0; i < nodes; ++i) {
                const uint32_t mid = (uint32_t)(((uint64_t)lv.beg[i] + lv.work_end[i]) >> 1);
                h_alpha[2 * i] = (float)(+1.0 / (double)(lv.work_end[i] - mid));
                h_alpha[2 * i + 1] = (float)(-1.0 / (double)(mid - lv.beg[i]));
            }
            alpha.upload(h_alpha);
        }
        if (lv.sampled) {
            perm.upload(lv.perm);
            hipLaunchKernelGGL(k11_gather, dim3(grid(L)), dim3(256), 0, s, perm.as<uint32_t>(), elem.as<uint32_t>(), elem2.as<uint32_t>(), L);
            XRL_LAUNCH_CHECK();
            std::swap(elem, elem2);
        }

        // ---- the level's layout
        hipLaunchKernelGGL(k11_rowlen, dim3(grid(L)), dim3(256), 0, s, X.row_ptr, elem.as<uint32_t>(), L, pos_of.as<uint32_t>(), len.as<uint32_t>());
        XRL_LAUNCH_CHECK();
        exclusive_scan(tmp, len.as<uint32_t>(), ent_off.as<uint32_t>(), (size_t)L + 1, s);
        node_ent.reserve(((size_t)nodes + 1) * 4); node_run.reserve(((size_t)nodes + 1) * 4);
        hipLaunchKernelGGL(k11_node_ent, dim3(grid(nodes + 1)), dim3(256), 0, s, beg.as<uint32_t>(), ent_off.as<uint32_t>(), nodes, node_ent.as<uint32_t>());
        XRL_LAUNCH_CHECK();
        uint32_t runs = 0;
        if (nnz) {
            hipLaunchKernelGGL(k11_expand, dim3(blocks_of(L, 4, kWhat)), dim3(256), 0, s, X.row_ptr, X.col_idx, elem.as<uint32_t>(), ent_off.as<uint32_t>(), L,
                               keys.as<uint64_t>(), xent.as<uint32_t>());
            XRL_LAUNCH_CHECK();
            seg_sort([&](void* t, size_t& bytes) {
                return rocprim::segmented_radix_sort_pairs(t, bytes, keys.as<uint64_t>(), keys2.as<uint64_t>(), xent.as<uint32_t>(), xent2.as<uint32_t>(), (unsigned int)nnz,
                                                           nodes, node_ent.as<uint32_t>(), node_ent.as<uint32_t>() + 1, 0u, 32u + feature_bits, s);
            });
            hipLaunchKernelGGL(k11_heads, dim3(grid(nnz)), dim3(256), 0, s, keys2.as<uint64_t>(), node_ent.as<uint32_t>(), nodes, (uint32_t)nnz, flag.as<uint32_t>());
            XRL_LAUNCH_CHECK();
            runs = scan_total(tmp, flag.as<uint32_t>(), slot.as<uint32_t>(), (size_t)nnz, s);
        } else {
            XRL_HIP(hipMemsetAsync(slot.p, 0, 4, s));
        }
        const uint64_t need_runs = 60ull * runs + 64;
        XRL_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need_runs > free_b + run_start.cap + run_node.cap + c.cap + c2.cap + first.cap + nkeys.cap + nkeys2.cap)
            fail(what + "the runs of level " + std::to_string(d) + " need " + std::to_string(need_runs) + " bytes of scratch, " + std::to_string(free_b) + " are free");
        run_start.reserve(((size_t)runs + 1) * 4); run_node.reserve(((size_t)runs + 1) * 4);
        c.reserve(((size_t)runs + 1) * 4);
        XRL_HIP(hipMemsetAsync(c.p, 0, ((size_t)runs + 1) * 4, s));       // max_iter = 0: the final assignment scores with a zero centre
        if (SK) {
            c2.reserve(((size_t)runs + 1) * 4); first.reserve(((size_t)runs + 1) * 8); scale.reserve((size_t)nodes * 16);
            if (lv.first_touch) { nkeys.reserve(((size_t)runs + 1) * 16); nkeys2.reserve(((size_t)runs + 1) * 16); nseg.reserve((2 * (size_t)nodes + 1) * 4); }
        }
        hipLaunchKernelGGL(k11_runs, dim3(grid(nnz)), dim3(256), 0, s, flag.as<uint32_t>(), slot.as<uint32_t>(), xent2.as<uint32_t>(), node_ent.as<uint32_t>(), nodes,
                           (uint32_t)nnz, runs, run_of.as<uint32_t>(), run_start.as<uint32_t>(), run_node.as<uint32_t>());
        XRL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k11_node_run, dim3(grid(nodes + 1)), dim3(256), 0, s, node_ent.as<uint32_t>(), slot.as<uint32_t>(), nodes, node_run.as<uint32_t>());
        XRL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k11_count_forms, dim3(grid(runs)), dim3(256), 0, s, run_start.as<uint32_t>(), runs, counts.as<unsigned long long>());
        XRL_LAUNCH_CHECK();
        if (SK && lv.first_touch) {
            hipLaunchKernelGGL(k11_norm_segs, dim3(grid(nodes)), dim3(256), 0, s, node_run.as<uint32_t>(), nodes, runs, nseg.as<uint32_t>());
            XRL_LAUNCH_CHECK();
        }

        K11Level a{};
        a.x_ptr = X.row_ptr; a.x_val = X.val; a.rows = L;
        a.elem = elem.as<uint32_t>(); a.pos_of = pos_of.as<uint32_t>(); a.score = score.as<float>();
        a.nodes = nodes; a.beg = beg.as<uint32_t>(); a.work_end = work_end.as<uint32_t>(); a.active = active.as<uint32_t>();
        a.keys = keys2.as<uint64_t>(); a.xent = xent2.as<uint32_t>(); a.run_start = run_start.as<uint32_t>(); a.run_node = run_node.as<uint32_t>();
        a.run_of = run_of.as<uint32_t>(); a.node_run = node_run.as<uint32_t>(); a.runs = runs;
        a.c = c.as<float>(); a.c2 = c2.as<float>(); a.first = first.as<uint32_t>();
        seg.reserve((size_t)nodes * 8); half.reserve((size_t)nodes * 16);
        uint32_t* seg_b = seg.as<uint32_t>(); uint32_t* seg_e = seg_b + nodes;
        uint32_t* half_b = half.as<uint32_t>(); uint32_t* half_e = half_b + 2 * (size_t)nodes;

        // score the range [beg, end) of every active node with the current centre and split it
        auto assign = [&](const uint32_t* end) {
            hipLaunchKernelGGL(k11_score, dim3(grid(L)), dim3(256), 0, s, a, end);
            XRL_LAUNCH_CHECK();
            hipLaunchKernelGGL(k11_split_keys, dim3(grid(std::max(L, nodes))), dim3(256), 0, s, a, end, skeys.as<uint64_t>(), seg_b, seg_e, half_b, half_e);
            XRL_LAUNCH_CHECK();
            seg_sort([&](void* t, size_t& bytes) {
                return rocprim::segmented_radix_sort_keys(t, bytes, skeys.as<uint64_t>(), skeys2.as<uint64_t>(), L, nodes, seg_b, seg_e, 0u, 64u, s);
            });
            hipLaunchKernelGGL(k11_split_ids, dim3(grid(L)), dim3(256), 0, s, skeys2.as<uint64_t>(), L, elem2.as<uint32_t>());
            XRL_LAUNCH_CHECK();
            seg_sort([&](void* t, size_t& bytes) {
                return rocprim::segmented_radix_sort_keys(t, bytes, elem2.as<uint32_t>(), ids.as<uint32_t>(), L, 2 * nodes, half_b, half_e, 0u, element_bits, s);
            });
            hipLaunchKernelGGL(k11_commit, dim3(grid(L)), dim3(256), 0, s, a, end, ids.as<uint32_t>(), changed.as<uint32_t>());
            XRL_LAUNCH_CHECK();
        };

        for (uint64_t k = 0; k < param.kmeans_max_iter; ++k) {
            if (k == 0) {
                hipLaunchKernelGGL(k11_first_centre, dim3(grid(runs)), dim3(256), 0, s, a, r_pos.as<uint32_t>(), l_pos.as<uint32_t>());
                XRL_LAUNCH_CHECK();
            } else if (!SK) {
                hipLaunchKernelGGL(k11_centre<false>, dim3(grid(runs)), dim3(256), 0, s, a, alpha.as<float>());
                XRL_LAUNCH_CHECK();
            } else {
                hipLaunchKernelGGL(k11_centre<true>, dim3(grid(runs)), dim3(256), 0, s, a, (const float*)nullptr);
                XRL_LAUNCH_CHECK();
                const uint64_t* order = nullptr;
                if (lv.first_touch && runs) {
                    hipLaunchKernelGGL(k11_norm_keys, dim3(grid(2ull * runs)), dim3(256), 0, s, first.as<uint32_t>(), 2 * runs, runs, nkeys.as<uint64_t>());
                    XRL_LAUNCH_CHECK();
                    seg_sort([&](void* t, size_t& bytes) {
                        return rocprim::segmented_radix_sort_keys(t, bytes, nkeys.as<uint64_t>(), nkeys2.as<uint64_t>(), 2 * runs, 2 * nodes, nseg.as<uint32_t>(),
                                                                  nseg.as<uint32_t>() + 1, 0u, 64u, s);
                    });
                    order = nkeys2.as<uint64_t>();
                }
                hipLaunchKernelGGL(k11_norm, dim3(blocks_of(2ull * nodes, 4, kWhat)), dim3(256), 0, s, a, order, scale.as<double>());
                XRL_LAUNCH_CHECK();
                hipLaunchKernelGGL(k11_combine, dim3(grid(runs)), dim3(256), 0, s, a, scale.as<double>());
                XRL_LAUNCH_CHECK();
            }
            assign(work_end.as<uint32_t>());
            hipLaunchKernelGGL(k11_flags, dim3(grid(nodes)), dim3(256), 0, s, active.as<uint32_t>(), changed.as<uint32_t>(), nodes);
            XRL_LAUNCH_CHECK();
            XRL_HIP(hipMemcpyAsync(h_active.data(), active.p, (size_t)nodes * 4, hipMemcpyDeviceToHost, s));
            XRL_HIP(hipStreamSynchronize(s));
            ++forms.iters[d];
            if (std::find(h_active.begin(), h_active.end(), 1u) == h_active.end()) break;
        }
        if (lv.sampled) {
            // the node's real children are the halves of its whole range: one more assignment with the last centre (clustering.hpp:331-337)
            XRL_HIP(hipStreamSynchronize(s));
            h_active.assign(nodes, 1u);
            active.upload(h_active);
            assign(whole_end.as<uint32_t>());
        }
        if (d_scores) XRL_HIP(hipMemcpyAsync(d_scores + (size_t)d * L, score.p, (size_t)L * 4, hipMemcpyDeviceToDevice, s));
    }
    XRL_HIP(hipStreamSynchronize(s));
    leaf_beg.upload(plan.leaf_beg);
    hipLaunchKernelGGL(k11_codes, dim3(grid(L)), dim3(256), 0, s, elem.as<uint32_t>(), leaf_beg.as<uint32_t>(), 1u << depth, L, d_codes);
    XRL_LAUNCH_CHECK();
    unsigned long long h_counts[2] = {0, 0};
    XRL_HIP(hipMemcpyAsync(h_counts, counts.p, 16, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    forms.lane_runs = h_counts[0]; forms.wave_runs = h_counts[1];
}

}  // namespace xrl
