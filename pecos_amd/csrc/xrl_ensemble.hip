// K6: ensembles on the device -- the fixed-stride result rows of up to 8 models (the output form of xrl_predict_device) merged into
// one fixed-stride result, with the arithmetic and the orderings of the reference's host code:
//
//   average          CsrEnsembler.average (pecos/utils/smat_util.py:828-842): sum(args), sorted_csr, data /= M
//   finish           Text2Text.predict's tail (pecos/apps/text2text/model.py:418-427): average, threshold, sorted_csr(only_topk)
//   rank_average     CsrEnsembler.rank_average (smat_util.py:845-859 with get_relevance_csr, :638-659)
//   sigmoid_average  CsrEnsembler.sigmoid_average (smat_util.py:862-881): z -> 1 / (1 + exp(-z)) in fp32 steps, then average
//   softmax_average  CsrEnsembler.softmax_average (:884-900, csr_row_softmax :788-811): scipy.special.softmax per model and row, then average
//   round_robin      CsrEnsembler.round_robin (:903-923 with get_relevance_csr, :638-659): fp64 relevance, maximum over the holders
//   only_topk > 0    the cut of TransformerMatcher.ensemble_prediction (pecos/xmc/xtransformer/matcher.py:535-579), for every method:
//                    sorted_csr(pred.astype(float32), only_topk), the merged row ranked again by its fp32 VALUE, cut
//
// One kernel, ensemble_kernel<NS, METHOD>; finish is the average instantiation with A.mode == kEnsembleFinish (a runtime branch: it
// ranks by the value like a cut does, and may drop by a threshold).
//
// One wavefront per row.  The row's T = sum_m min(cnt_m, stride_m) entries are numbered j = 0 .. T-1 in MODEL order (model 0's entries
// best first, then model 1's, ...); entry j = i * 64 + lane lives in register slot i of its lane (NS slots per lane, NS chosen on the
// host from sum_m stride_m <= 1024), so every input is read once and coalesced.  The entries also go to wavefront-private LDS
// (8 bytes each, at most 8 KB), and every lane walks that list once per phase with wave-uniform addresses (LDS broadcast reads):
//
//   transform  sigmoid_average and softmax_average only (below)
//   phase 1  union of the labels: the entry with no EARLIER holder of its label leads the label, and adds the later holders' scores to
//            its own in list order = model order -- ((A0 + A1) + A2 of Python's sum(), each add rounded to fp32
//   phase 2  the leaders that survive the mode's drops publish (ordering key, label) in place of their entry
//   phase 3  a surviving leader's output position is the number of published pairs that order before it; the pairs are distinct
//            (labels are), so the positions are a permutation and every output is written once
//
// No global atomics, no scratch; the work per row is O(T^2 / 64) LDS reads, a few microseconds of one wavefront at T = 1024 and
// nothing at the T of some tens that ensembles of top-10 predictions produce.
//
// The transform of the scores between the load and phase 1, and round_robin's integers:
//
//   sigmoid  e = ref_expf(-z); 1 + e and 1 / (.) each rounded to fp32 (numpy on a float32 array).  The exponentials run in ONE rolled
//            loop over the LDS list (a lane takes entries lane, lane + 64, ...), so the fp64 exp is in the code once, not once per slot.
//   softmax  per segment (one model's entries of the row; <= 8 wave reductions under a membership mask, registers only):
//            x_max = maximum, NaN when the segment holds a NaN; e_j = ref_expf(x_j - x_max) in the rolled loop; the denominator is the
//            fp64 sum of the fp32 e_j rounded once to fp32; value = e_j / denominator in fp32.
//            ORDER OF THE fp64 SUM (a function of the inputs only): every lane adds its entries of the segment in ascending j starting
//            from 0.0, then the 64 lane sums meet in six exchange steps s[l] = s[l] + s[l ^ d], d = 1, 2, 4, 8, 16, 32 (fp64 addition
//            commutes, so every lane ends with the same bits).  tests/ensemble_methods_rule.py restates it.
//            A segment whose maximum is +inf, or that is all -inf, comes out NaN by IEEE arithmetic (inf - inf), as scipy's does.  An
//            EMPTY segment contributes nothing; the reference raises ValueError there (amax of an empty array).
//   round_robin   scores are not read.  The entry at position p of model m has relevance (double)(mm - p) + (double)(M - m) * base,
//            base = 1.0 / (M + 1.0).  0 < (M - m) * base <= 8/9 and distinct m differ by >= 1/9, so the doubles order exactly like the
//            integers (mm - p) * 16 + (M - m): those go through phases 1 (maximum over the holders) and 3, the double is formed once per
//            leader with __dmul_rn / __dadd_rn / __ddiv_rn (no contraction).
#include <hip/hip_runtime.h>

#include <cmath>

#include "xrl_device.h"
#include "xrl_kernels.h"

namespace xrl {

// mm of rank_average and round_robin: the largest row length over all models and all rows of the call (smat_util.py:855), row
// lengths clamped to the stride.  One workgroup, so that the result is a plain store.
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

__device__ __forceinline__ float wave_all_fmaxf(float x) {             // every lane receives the maximum (fmaxf: a NaN operand is ignored)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x = fmaxf(x, __shfl_xor(x, d));
    return x;
}

__device__ __forceinline__ double wave_all_dadd(double s) {            // the six exchange steps of the file header
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s = __dadd_rn(s, __shfl_xor(s, d));
    return s;
}

// METHOD: A.mode, with finish served by the average instantiation
template <int NS, int METHOD>
__global__ void __launch_bounds__(kEnsembleWaves * 64)
ensemble_kernel(EnsembleArgs A, const uint32_t* __restrict__ mm_ptr) {
    constexpr bool RANK = METHOD == kEnsembleRankAverage, RR = METHOD == kEnsembleRoundRobin;
    constexpr bool SIGMOID = METHOD == kEnsembleSigmoidAverage, SOFTMAX = METHOD == kEnsembleSoftmaxAverage;
    constexpr bool INTEGER = RANK || RR;                               // phase 1 merges integers, not fp32 scores
    __shared__ uint2 lds[kEnsembleWaves][NS * 64];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const uint32_t r = blockIdx.x * (uint32_t)kEnsembleWaves + (uint32_t)wave;
    if (r >= A.rows) return;                                           // (whole wavefronts; no workgroup barrier below)
    uint2* sc = lds[wave];
    const uint32_t M = A.n_models;
    const uint32_t mm = INTEGER ? *mm_ptr : 0u;

    // ---- load: entry j of the row's list sits at element (j - pre_m) of model m's row, pre_m = entries of the models before m
    uint32_t pre[kEnsembleMaxModels + 1];
    pre[0] = 0;
#pragma unroll
    for (int m = 0; m < kEnsembleMaxModels; ++m)
        pre[m + 1] = pre[m] + ((uint32_t)m < M ? min(A.cnt[m][r], A.stride[m]) : 0u);
    const uint32_t T = pre[kEnsembleMaxModels];                        // <= sum of the strides <= NS * 64 (checked on the host)

    uint32_t lab[NS], acc[NS];                                         // label; score bits (RANK: mm - p; RR: (mm - p) * 16 + (M - m))
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
        lab[i] = 0; acc[i] = 0;
        if (j < T) {
            const uint32_t* pi = A.idx[0];
            const float* pv = A.val[0];
            uint64_t at = (uint64_t)r * A.stride[0] + j;
            uint32_t pos = j, mi = 0;
#pragma unroll
            for (int m = 1; m < kEnsembleMaxModels; ++m) {
                const bool in = j >= pre[m] && (uint32_t)m < M;        // (the last model that starts at or before j holds it)
                pi = in ? A.idx[m] : pi; pv = in ? A.val[m] : pv;
                at = in ? (uint64_t)r * A.stride[m] + (j - pre[m]) : at;
                pos = in ? j - pre[m] : pos; mi = in ? (uint32_t)m : mi;
            }
            lab[i] = pi[at];
            acc[i] = RANK ? mm - pos : RR ? (mm - pos) * 16u + (M - mi) : __float_as_uint(pv[at]);   // (pos < cnt <= mm: never 0)
            sc[j] = make_uint2(lab[i], acc[i]);
        }
    }

    // ---- transform: the list's scores become sigmoid(z) / softmax of their segment
    if (SIGMOID || SOFTMAX) {
        float xm[kEnsembleMaxModels];                                  // softmax: the segments' maxima (wave-uniform)
        if (SOFTMAX) {
#pragma unroll
            for (int m = 0; m < kEnsembleMaxModels; ++m) {
                xm[m] = 0.0f;
                if ((uint32_t)m < M && pre[m + 1] > pre[m]) {          // (wave-uniform)
                    float mx = -INFINITY;
                    bool nan = false;
#pragma unroll
                    for (int i = 0; i < NS; ++i) {
                        const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
                        const float v = __uint_as_float(acc[i]);
                        if (j >= pre[m] && j < pre[m + 1]) { nan = nan || v != v; mx = fmaxf(mx, v); }
                    }
                    mx = wave_all_fmaxf(mx);
                    xm[m] = __ballot(nan) ? __builtin_nanf("") : mx;   // numpy's amax: a NaN in the segment makes it NaN
                }
            }
        }
        wave_sync_lds();
#pragma unroll 1
        for (uint32_t j = (uint32_t)lane; j < T; j += 64u) {
            uint2 e = sc[j];
            const float z = __uint_as_float(e.y);
            float v;
            if (SOFTMAX) {
                float x_max = xm[0];
#pragma unroll
                for (int m = 1; m < kEnsembleMaxModels; ++m) x_max = (j >= pre[m] && (uint32_t)m < M) ? xm[m] : x_max;
                v = ref_expf(__fsub_rn(z, x_max));
            } else {
                v = __fdiv_rn(1.0f, __fadd_rn(1.0f, ref_expf(-z)));
            }
            e.y = __float_as_uint(v);
            sc[j] = e;                                                 // (the lane's own entries: slot i of this lane is entry i * 64 + lane)
        }
        wave_sync_lds();
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
            if (j < T) acc[i] = sc[j].y;
        }
        if (SOFTMAX) {
#pragma unroll
            for (int m = 0; m < kEnsembleMaxModels; ++m) {
                if ((uint32_t)m < M && pre[m + 1] > pre[m]) {
                    double s = 0.0;
#pragma unroll
                    for (int i = 0; i < NS; ++i) {
                        const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
                        if (j >= pre[m] && j < pre[m + 1]) s = __dadd_rn(s, (double)__uint_as_float(acc[i]));
                    }
                    const float den = (float)wave_all_dadd(s);
#pragma unroll
                    for (int i = 0; i < NS; ++i) {
                        const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
                        if (j >= pre[m] && j < pre[m + 1]) {
                            acc[i] = __float_as_uint(__fdiv_rn(__uint_as_float(acc[i]), den));
                            sc[j].y = acc[i];
                        }
                    }
                }
            }
        }
    }
    wave_sync_lds();

    // ---- phase 1: leaders; sums in model order (round_robin: the maximum over the holders)
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
                acc[i] = RR ? max(acc[i], e.y) : RANK ? acc[i] + e.y : __float_as_uint(__fadd_rn(__uint_as_float(acc[i]), __uint_as_float(e.y)));
        }
    }
    wave_sync_lds();                                                   // every lane has read the entries: the list is rewritten below

    // ---- phase 2: value, drops and ordering key; survivors publish (key, label)
    const float fm = (float)M;
    const double dm = (double)M, base = __ddiv_rn(1.0, __dadd_rn(dm, 1.0));
    const bool cut = A.only_topk != 0u;
    constexpr bool AVERAGE = METHOD == kEnsembleAverage;               // (finish lives here and nowhere else)
    const bool by_value = cut || (AVERAGE && A.mode == kEnsembleFinish);   // rank by the fp32 value, as sorted_csr(pred.astype(float32), only_topk)
    uint32_t key[NS], outv[NS], n_kept = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
        bool keep = (leader >> i) & 1u;
        uint32_t k;
        float v;
        if (RR) {
            const double rel = __dadd_rn((double)(acc[i] >> 4), __dmul_rn((double)(acc[i] & 15u), base));
            v = (float)__ddiv_rn(rel, dm);
            k = acc[i];                                                // >= 16 for an entry
        } else if (RANK) {
            v = (float)__ddiv_rn((double)acc[i], dm);                  // every relevance is float64 in the reference, returned as fp32
            k = acc[i];                                                // >= 1 for an entry
        } else {
            const float s = __uint_as_float(acc[i]);
            v = __fdiv_rn(s, fm);
            if (M >= 2u && s == 0.0f) keep = false;                    // scipy's CSR addition stores no exact zero (either sign; NaN stays)
            if (AVERAGE && A.has_threshold && (v <= A.threshold || v == 0.0f)) keep = false;   // finish: data[data <= t] = 0; eliminate_zeros()
            k = ensemble_key(s);                                       // average sorts the SUM: equal quotients keep the sums' order
        }
        if (by_value) k = ensemble_key(v);
        key[i] = keep ? k : 0u; outv[i] = __float_as_uint(v);
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
    const uint32_t limit = cut ? min(n_kept, A.only_topk) : n_kept;    // <= out_stride (host check)
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
    switch (A.mode) {
    case kEnsembleAverage:
    case kEnsembleFinish: hipLaunchKernelGGL((ensemble_kernel<NS, kEnsembleAverage>), grid, block, 0, s, A, mm); break;
    case kEnsembleRankAverage: hipLaunchKernelGGL((ensemble_kernel<NS, kEnsembleRankAverage>), grid, block, 0, s, A, mm); break;
    case kEnsembleSigmoidAverage: hipLaunchKernelGGL((ensemble_kernel<NS, kEnsembleSigmoidAverage>), grid, block, 0, s, A, mm); break;
    case kEnsembleSoftmaxAverage: hipLaunchKernelGGL((ensemble_kernel<NS, kEnsembleSoftmaxAverage>), grid, block, 0, s, A, mm); break;
    case kEnsembleRoundRobin: hipLaunchKernelGGL((ensemble_kernel<NS, kEnsembleRoundRobin>), grid, block, 0, s, A, mm); break;
    default: fail("ensemble: unknown mode");
    }
    XRL_LAUNCH_CHECK();
}

uint32_t ensemble_slots(uint32_t stride_sum) {
    uint32_t ns = 1;
    while (ns * 64u < stride_sum) ns *= 2u;
    return ns;
}

void launch_ensemble(const EnsembleArgs& A, uint32_t* mm_scratch, hipStream_t s) {
    if (A.rows == 0) return;
    uint32_t stride_sum = 0;
    for (uint32_t m = 0; m < A.n_models; ++m) stride_sum += A.stride[m];
    if (A.n_models == 0 || A.n_models > (uint32_t)kEnsembleMaxModels || stride_sum > kEnsembleMaxTotal) fail("ensemble: shape outside the kernel's capacity");
    if (A.mode == kEnsembleRankAverage || A.mode == kEnsembleRoundRobin) {
        if (!mm_scratch) fail("ensemble: rank_average and round_robin need their device scalar");
        hipLaunchKernelGGL(ensemble_max_len_kernel, dim3(1), dim3(1024), 0, s, A, mm_scratch);
        XRL_LAUNCH_CHECK();
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
