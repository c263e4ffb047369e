// K7: predict_on_selected_outputs planned and scored on the device (xrl_predict_selected_device).
//
//   k7_select_plan_kernel    the reference's walk of the tree for a given set of labels per row (HierarchicalMLModel::predict_on_selected_outputs,
//                            inference.hpp:2507-2571; prolongate_sparse_predictions, :1302-1358), as index arrays
//   k4_selected_dev_kernel   one layer of the planned slots through the CSC route (K4's arithmetic, xrl_pairs.h)
//
// What the walk computes, in closed form.  In a tree every node has one parent, so with
//   A[T-1] = the row's labels, sorted;   A[l-1] = the sorted, distinct parents of A[l]
// the reference emits the nodes of layer l for a row in ascending order of the key
//   (position of the node's parent in the row's ORDERED list of layer l-1,  position of the node inside its parent's column of C as stored)
// and layer 0 hangs under the implicit root at position 0.  (tests/select_plan.py states this in numpy and checks it against the oracle.)
//
// One wavefront per row; entry j = i * 64 + lane of a list is slot i of its lane (NS slots per lane, NS chosen on the host from sel_stride the
// way K6 chooses, capacity 64 * NS <= 1024).  Wavefront-private LDS holds the 64-bit sort keys, the sorted set of the layer at hand and,
// top-down, the ordered position of every entry of that set.  One launch, per row:
//   load      the labels;  flag the row if one is >= nr_labels
//   bottom-up l = T-1 .. 0: sort, drop repeats (a repeat among the labels flags the row), store the sorted set A[l] and its size in the layer's
//             scratch row, look up the parents (bounds-checked; kSelectNone flags the row: pruned tree)
//   top-down  l = 0 .. T-1: key = (ordered position of the parent -- binary search in A[l-1], then rank -> position -- , crank, index in A[l]);
//             sort;  the sorted position IS the walk's position: write node[l][pos], ppos[l][pos] (the last layer's nodes and count go to
//             the caller's buffers), remember position-by-rank for the next layer
// A flagged row gets count 0 in every layer and the caller's d_out_cnt, and enters the status word by atomicMin -- the only atomic; every
// output slot below a row's count is written once, slots beyond it are left untouched.
//
// The sort is a bitonic network over the 64-bit keys in LDS, not K6's ranking by counting: keys are unique, so both give the permutation, but
// at 1024 entries counting costs 1024 list steps x 16 register slots x (64-bit compare + add) ~ 50 000 instructions per sort, the network
// 55 steps x 8 pairs per lane x ~16 instructions ~ 7 000 -- and 2 x depth sorts run per row.  The network spans the next power of two of
// the row's length, so rows of some tens of labels pay 15-21 steps of one pair per lane.  The key is 64 bits wide because the position of a
// node inside its parent's column can need all 32 bits and positions reach 1023: (10 | 32 | 10 bits of index) = 52.
#include "xrl_pairs.h"

namespace xrl {

template <int NS> constexpr int select_waves() { return NS >= 16 ? 2 : 4; }   // wavefronts (= rows) per workgroup: 16 bytes of LDS per entry, <= 32 KB per workgroup

// ascending bitonic sort of key[0, n); key[n, next power of two) must hold the all-ones pad
__device__ __forceinline__ void select_sort(uint64_t* key, uint32_t n, int lane) {
    wave_sync_lds();
    if (n < 2u) return;
    uint32_t n2 = 2u;
    while (n2 < n) n2 <<= 1;
    for (uint32_t k = 2u; k <= n2; k <<= 1) {
        for (uint32_t js = k >> 1; js > 0u; js >>= 1) {
            for (uint32_t t = (uint32_t)lane; t < (n2 >> 1); t += 64u) {
                const uint32_t i = ((t & ~(js - 1u)) << 1) | (t & (js - 1u)), p = i | js;    // the pair (i, i ^ js), i < p
                const uint64_t a = key[i], b = key[p];
                const bool up = (i & k) == 0u;
                if ((a > b) == up) { key[i] = b; key[p] = a; }
            }
            wave_sync_lds();
        }
    }
}

// the distinct high words of the sorted key[0, n), in order, into set[]; returns their number
template <int NS>
__device__ __forceinline__ uint32_t select_unique(const uint64_t* key, uint32_t n, uint32_t* set, int lane) {
    uint32_t base = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
        uint32_t v = 0; bool lead = false;
        if (j < n) { v = (uint32_t)(key[j] >> 32); lead = j == 0u || (uint32_t)(key[j - 1u] >> 32) != v; }
        const unsigned long long m = __ballot(lead);
        if (lead) set[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = v;
        base += (uint32_t)__popcll(m);
    }
    wave_sync_lds();
    return base;
}

template <int NS>
__global__ void __launch_bounds__(select_waves<NS>() * 64)
k7_select_plan_kernel(SelectPlanArgs A) {
    constexpr int WAVES = select_waves<NS>();
    constexpr uint32_t CAP = (uint32_t)NS * 64u;
    __shared__ uint64_t s_key[WAVES][CAP];
    __shared__ uint32_t s_set[WAVES][CAP];
    __shared__ uint32_t s_pos[WAVES][CAP];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const uint32_t r = blockIdx.x * (uint32_t)WAVES + (uint32_t)wave;
    if (r >= A.nrows) return;                                          // (whole wavefronts; no workgroup barrier below)
    uint64_t* key = s_key[wave];
    uint32_t* set = s_set[wave];
    uint32_t* pos = s_pos[wave];
    const uint64_t grow = (uint64_t)A.row0 + r;                        // the row in the caller's arrays
    const uint32_t T = A.depth, stride = A.sel_stride;                 // stride <= CAP (host check)
    const uint32_t n_in = min(A.sel_cnt ? A.sel_cnt[grow] : stride, stride);
    uint32_t* __restrict__ node_row = A.node + (uint64_t)r * stride;   // + l * layer_elems
    uint32_t* __restrict__ ppos_row = A.ppos + (uint64_t)r * stride;
    uint32_t* __restrict__ cnt_row = A.cnt + r;                        // + l * layer_rows

    // ---- load
    bool oor = false;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
        uint64_t k = ~0ull;
        if (j < n_in) { const uint32_t lab = A.sel_idx[grow * stride + j]; oor |= lab >= A.nr_labels; k = (uint64_t)lab << 32; }
        key[j] = k;
    }
    select_sort(key, n_in, lane);
    uint32_t n = select_unique<NS>(key, n_in, set, lane);
    uint32_t code = n != n_in ? (uint32_t)kSelectTwice : (__any(oor) ? (uint32_t)kSelectOutOfRange : (uint32_t)kSelectOk);

    // ---- bottom-up: set[0, n) is A[l]
    for (uint32_t l = T; l-- > 0u && code == kSelectOk;) {
        const SelectTreeLayer tl = A.tree[l];
        bool orphan = false;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
            uint64_t k = ~0ull;
            if (j < n) {
                const uint32_t v = set[j];
                node_row[l * A.layer_elems + j] = v;
                const uint32_t p = v < tl.c_rows ? tl.parent[v] : kSelectNone;
                orphan |= p == kSelectNone;
                k = (uint64_t)p << 32;
            }
            key[j] = k;
        }
        if (lane == 0) cnt_row[l * A.layer_rows] = n;
        if (__any(orphan)) { code = kSelectNoParent; break; }
        if (l == 0u) break;
        select_sort(key, n, lane);
        n = select_unique<NS>(key, n, set, lane);
    }
    if (code != kSelectOk) {
        if (lane == 0) {
            for (uint32_t l = 0; l < T; ++l) cnt_row[l * A.layer_rows] = 0u;
            A.out_cnt[grow] = 0u;
            atomicMin(A.status, (unsigned long long)((grow << 32) | code));
        }
        return;
    }
    __threadfence_block();                                             // the counts lane 0 stored are read by every lane below

    // ---- top-down: set[0, n_prev) is A[l-1] and pos[] the ordered position of each of its entries
    uint32_t n_prev = 0;
    for (uint32_t l = 0; l < T; ++l) {
        const SelectTreeLayer tl = A.tree[l];
        const uint32_t n_l = min(cnt_row[l * A.layer_rows], stride);
        uint32_t a[NS]; uint64_t kk[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
            a[i] = 0u; kk[i] = ~0ull;
            if (j < n_l) {
                a[i] = node_row[l * A.layer_elems + j];                // < c_rows, and its parent is in A[l-1]: both established bottom-up
                uint32_t pp = 0u;
                if (l > 0u) {
                    const uint32_t p = tl.parent[a[i]];
                    uint32_t lo = 0u, hi = n_prev;
                    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (set[mid] < p) lo = mid + 1u; else hi = mid; }
                    pp = pos[lo < n_prev ? lo : 0u];
                }
                kk[i] = ((uint64_t)pp << 42) | ((uint64_t)tl.crank[a[i]] << 10) | (uint64_t)j;
            }
        }
        wave_sync_lds();                                               // every lane has read A[l-1] and its positions: both are rewritten below
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
            key[j] = kk[i];
            if (j < n_l) set[j] = a[i];
        }
        select_sort(key, n_l, lane);
        const bool last = l + 1u == T;
        uint32_t* __restrict__ on = last ? A.out_idx + grow * A.out_stride : node_row + l * A.layer_elems;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
            if (j < n_l) {
                const uint64_t k = key[j];
                const uint32_t idx = (uint32_t)k & 1023u;
                pos[idx] = j;
                on[j] = set[idx];
                ppos_row[l * A.layer_elems + j] = (uint32_t)(k >> 42);
            }
        }
        if (last && lane == 0) A.out_cnt[grow] = n_l;
        wave_sync_lds();
        n_prev = n_l;
    }
}

template <int NS>
static void launch_select_plan_ns(const SelectPlanArgs& A, hipStream_t s) {
    constexpr uint32_t W = (uint32_t)select_waves<NS>();
    hipLaunchKernelGGL((k7_select_plan_kernel<NS>), dim3((A.nrows + W - 1u) / W), dim3(W * 64u), 0, s, A);
    XRL_LAUNCH_CHECK();
}

void launch_select_plan(const SelectPlanArgs& A, hipStream_t s) {
    if (A.nrows == 0) return;
    if (A.sel_stride == 0 || A.sel_stride > kSelectMaxStride || A.depth == 0) fail("select plan: shape outside the kernel's capacity");
    switch (ensemble_slots(A.sel_stride)) {
    case 1: launch_select_plan_ns<1>(A, s); break;
    case 2: launch_select_plan_ns<2>(A, s); break;
    case 4: launch_select_plan_ns<4>(A, s); break;
    case 8: launch_select_plan_ns<8>(A, s); break;
    default: launch_select_plan_ns<16>(A, s); break;
    }
}

template <int PPC>
__global__ void __launch_bounds__(256) k4_selected_dev_kernel(SelectScoreArgs a, QueriesDev X, int pp_kind, int pp_p) {
    const int lane = threadIdx.x & 63, lig = lane % PG, gbase = lane - lig;
    const uint64_t i = (uint64_t)blockIdx.x * PAIRS_PER_BLOCK + threadIdx.x / PG;
    const uint64_t r = i / a.sel_stride;
    if (r >= a.nrows) return;
    const uint32_t at = (uint32_t)(i - r * a.sel_stride);
    if (at >= a.cnt[r]) return;
    const CscDev W{a.col_ptr, a.row_idx, a.val, a.w_rows, a.bias};
    const float res = csc_route_product(W, X, (uint64_t)a.row0 + r, a.node[r * a.node_stride + at], lig, gbase);
    if (lig == 0) {
        float v = pp_transform<PPC>(pp_kind, pp_p, res);
        if (a.prev_val) v = pp_combine(pp_kind, v, a.prev_val[r * a.sel_stride + a.ppos[r * a.sel_stride + at]]);
        a.out_val[r * a.out_stride + at] = v;
    }
}

void launch_k4_selected_dev(const SelectScoreArgs& A, const QueriesDev& X, const PostProc& pp, hipStream_t s) {
    if (A.nrows == 0) return;
    const uint64_t slots = (uint64_t)A.nrows * A.sel_stride;
    const uint64_t blocks = (slots + PAIRS_PER_BLOCK - 1) / PAIRS_PER_BLOCK;
    if (blocks > 0x7FFFFFFFull) fail("k4: too many (query, label) slots in one launch");
    if (pp_class(pp)) hipLaunchKernelGGL(k4_selected_dev_kernel<1>, dim3((uint32_t)blocks), dim3(256), 0, s, A, X, pp.kind, pp.p);
    else hipLaunchKernelGGL(k4_selected_dev_kernel<0>, dim3((uint32_t)blocks), dim3(256), 0, s, A, X, pp.kind, pp.p);
    XRL_LAUNCH_CHECK();
}

}  // namespace xrl
