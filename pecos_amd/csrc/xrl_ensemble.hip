// K6: ensembles on the device -- the fixed-stride result rows of up to 8 models (the output form of xrl_predict_device) merged into
// one fixed-stride result, with the arithmetic and the orderings of the reference's host code:
//
//   average        CsrEnsembler.average (pecos/utils/smat_util.py:828-842): sum(args), sorted_csr, data /= M
//   finish         Text2Text.predict's tail (pecos/apps/text2text/model.py:418-427): average, threshold, sorted_csr(only_topk)
//   rank_average   CsrEnsembler.rank_average (smat_util.py:845-859 with get_relevance_csr, :638-659)
//
// One wavefront per row.  The row's T = sum_m min(cnt_m, stride_m) entries are numbered j = 0 .. T-1 in MODEL order (model 0's entries
// best first, then model 1's, ...); entry j = i * 64 + lane lives in register slot i of its lane (NS slots per lane, NS chosen on the
// host from sum_m stride_m <= 1024), so every input is read once and coalesced.  The entries also go to wavefront-private LDS
// (8 bytes each, at most 8 KB), and every lane walks that list once per phase with wave-uniform addresses (LDS broadcast reads):
//
//   phase 1  union of the labels: the entry with no EARLIER holder of its label leads the label, and adds the later holders' scores to
//            its own in list order = model order -- ((A0 + A1) + A2 of Python's sum(), each add rounded to fp32
//   phase 2  the leaders that survive the mode's drops publish (ordering key, label) in place of their entry
//   phase 3  a surviving leader's output position is the number of published pairs that order before it; the pairs are distinct
//            (labels are), so the positions are a permutation and every output is written once
//
// No global atomics, no scratch; the work per row is O(T^2 / 64) LDS reads, a few microseconds of one wavefront at T = 1024 and
// nothing at the T of some tens that ensembles of top-10 predictions produce.
#include <hip/hip_runtime.h>

#include <cmath>

#include "xrl_device.h"
#include "xrl_kernels.h"

namespace xrl {

// mm of rank_average: the largest row length over all models and all rows of the call (smat_util.py:855), row lengths clamped to
// the stride.  One workgroup, so that the result is a plain store.
__global__ void __launch_bounds__(1024)
ensemble_max_len_kernel(EnsembleArgs A, uint32_t* __restrict__ mm) {
    __shared__ uint32_t part[16];
    uint32_t best = 0;
#pragma unroll
    for (int m = 0; m < kEnsembleMaxModels; ++m) {
        if ((uint32_t)m < A.n_models) {
            const uint32_t* __restrict__ c = A.cnt[m];
            const uint32_t st = A.stride[m];
            for (uint32_t r = threadIdx.x; r < A.rows; r += 1024u) best = max(best, min(c[r], st));
        }
    }
    best = wave_max_u32(best);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) best = max(best, part[w]);
        *mm = best;
    }
}

// RANK: rank_average (integer relevance sums) instead of the average family (fp32 sums)
template <int NS, bool RANK>
__global__ void __launch_bounds__(kEnsembleWaves * 64)
ensemble_kernel(EnsembleArgs A, const uint32_t* __restrict__ mm_ptr) {
    __shared__ uint2 lds[kEnsembleWaves][NS * 64];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const uint32_t r = blockIdx.x * (uint32_t)kEnsembleWaves + (uint32_t)wave;
    if (r >= A.rows) return;                                           // (whole wavefronts; no workgroup barrier below)
    uint2* sc = lds[wave];
    const uint32_t M = A.n_models;
    const uint32_t mm = RANK ? *mm_ptr : 0u;

    // ---- load: entry j of the row's list sits at element (j - pre_m) of model m's row, pre_m = entries of the models before m
    uint32_t pre[kEnsembleMaxModels + 1];
    pre[0] = 0;
#pragma unroll
    for (int m = 0; m < kEnsembleMaxModels; ++m)
        pre[m + 1] = pre[m] + ((uint32_t)m < M ? min(A.cnt[m][r], A.stride[m]) : 0u);
    const uint32_t T = pre[kEnsembleMaxModels];                        // <= sum of the strides <= NS * 64 (checked on the host)

    uint32_t lab[NS], acc[NS];                                         // label; score bits (RANK: relevance mm - position)
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
        lab[i] = 0; acc[i] = 0;
        if (j < T) {
            const uint32_t* pi = A.idx[0];
            const float* pv = A.val[0];
            uint64_t at = (uint64_t)r * A.stride[0] + j;
            uint32_t pos = j;
#pragma unroll
            for (int m = 1; m < kEnsembleMaxModels; ++m) {
                const bool in = j >= pre[m] && (uint32_t)m < M;        // (the last model that starts at or before j holds it)
                pi = in ? A.idx[m] : pi; pv = in ? A.val[m] : pv;
                at = in ? (uint64_t)r * A.stride[m] + (j - pre[m]) : at;
                pos = in ? j - pre[m] : pos;
            }
            lab[i] = pi[at];
            acc[i] = RANK ? mm - pos : __float_as_uint(pv[at]);
            sc[j] = make_uint2(lab[i], acc[i]);
        }
    }
    wave_sync_lds();

    // ---- phase 1: leaders and their sums in model order
    uint32_t leader = 0;                                               // bit i: slot i leads its label
#pragma unroll
    for (int i = 0; i < NS; ++i) leader |= ((uint32_t)i * 64u + (uint32_t)lane < T ? 1u : 0u) << i;
#pragma unroll 2
    for (uint32_t jj = 0; jj < T; ++jj) {
        const uint2 e = sc[jj];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
            const bool same = e.x == lab[i];
            if (same && jj < j) leader &= ~(1u << i);
            if (same && jj > j)
                acc[i] = RANK ? acc[i] + e.y : __float_as_uint(__fadd_rn(__uint_as_float(acc[i]), __uint_as_float(e.y)));
        }
    }
    wave_sync_lds();                                                   // every lane has read the entries: the list is rewritten below

    // ---- phase 2: value, drops and ordering key per mode; survivors publish (key, label)
    const float fm = (float)M;
    uint32_t key[NS], outv[NS], n_kept = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
        bool keep = (leader >> i) & 1u;
        uint32_t k = 0, v = 0;
        if (RANK) {
            k = acc[i];                                                // >= 1: every relevance is
            v = __float_as_uint((float)((double)acc[i] / (double)M));  // float64 in the reference, returned as fp32
        } else {
            const float s = __uint_as_float(acc[i]);
            const float q = __fdiv_rn(s, fm);
            if (M >= 2u && s == 0.0f) keep = false;                    // scipy's CSR addition stores no exact zero (either sign; NaN stays)
            if (A.mode == kEnsembleFinish) {
                if (A.has_threshold && (q <= A.threshold || q == 0.0f)) keep = false;   // data[data <= t] = 0; eliminate_zeros()
                k = ensemble_key(q);
            } else {
                k = ensemble_key(s);                                   // average sorts the SUM: equal quotients keep the sums' order
            }
            v = __float_as_uint(q);
        }
        key[i] = keep ? k : 0u; outv[i] = v;
        n_kept += (uint32_t)__popcll(__ballot(keep));
        if (j < T) sc[j] = make_uint2(key[i], lab[i]);
    }
    wave_sync_lds();

    // ---- phase 3: position = pairs that order before mine (key descending, label ascending)
    uint32_t rank[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) rank[i] = 0;
#pragma unroll 2
    for (uint32_t jj = 0; jj < T; ++jj) {
        const uint2 e = sc[jj];
#pragma unroll
        for (int i = 0; i < NS; ++i) rank[i] += (e.x > key[i] || (e.x == key[i] && e.y < lab[i])) ? 1u : 0u;
    }
    const uint32_t limit = (A.mode == kEnsembleFinish && A.only_topk) ? min(n_kept, A.only_topk) : n_kept;   // <= out_stride (host check)
    uint32_t* __restrict__ oi = A.out_idx + (uint64_t)r * A.out_stride;
    float* __restrict__ ov = A.out_val + (uint64_t)r * A.out_stride;
#pragma unroll
    for (int i = 0; i < NS; ++i)
        if (key[i] != 0u && rank[i] < limit) { oi[rank[i]] = lab[i]; ov[rank[i]] = __uint_as_float(outv[i]); }
    if (lane == 0) A.out_cnt[r] = limit;
}

template <int NS>
static void launch_ensemble_ns(const EnsembleArgs& A, const uint32_t* mm, hipStream_t s) {
    const dim3 grid((A.rows + (uint32_t)kEnsembleWaves - 1u) / (uint32_t)kEnsembleWaves), block(kEnsembleWaves * 64);
    if (A.mode == kEnsembleRankAverage) hipLaunchKernelGGL((ensemble_kernel<NS, true>), grid, block, 0, s, A, mm);
    else hipLaunchKernelGGL((ensemble_kernel<NS, false>), grid, block, 0, s, A, mm);
    XRL_LAUNCH_CHECK();
}

uint32_t ensemble_slots(uint32_t stride_sum) {
    uint32_t ns = 1;
    while (ns * 64u < stride_sum) ns *= 2u;
    return ns;
}

void launch_ensemble_max_len(const EnsembleArgs& A, uint32_t* mm, hipStream_t s) {
    hipLaunchKernelGGL(ensemble_max_len_kernel, dim3(1), dim3(1024), 0, s, A, mm);
    XRL_LAUNCH_CHECK();
}

void launch_ensemble(const EnsembleArgs& A, uint32_t* mm_scratch, hipStream_t s) {
    if (A.rows == 0) return;
    uint32_t stride_sum = 0;
    for (uint32_t m = 0; m < A.n_models; ++m) stride_sum += A.stride[m];
    if (A.n_models == 0 || A.n_models > (uint32_t)kEnsembleMaxModels || stride_sum > kEnsembleMaxTotal) fail("ensemble: shape outside the kernel's capacity");
    if (A.mode == kEnsembleRankAverage) {
        if (!mm_scratch) fail("ensemble: rank_average needs its device scalar");
        launch_ensemble_max_len(A, mm_scratch, s);
    }
    switch (ensemble_slots(stride_sum)) {
    case 1: launch_ensemble_ns<1>(A, mm_scratch, s); break;
    case 2: launch_ensemble_ns<2>(A, mm_scratch, s); break;
    case 4: launch_ensemble_ns<4>(A, mm_scratch, s); break;
    case 8: launch_ensemble_ns<8>(A, mm_scratch, s); break;
    default: launch_ensemble_ns<16>(A, mm_scratch, s); break;
    }
}

}  // namespace xrl
