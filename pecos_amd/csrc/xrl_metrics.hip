// K8: metrics on the device -- the sums behind precision and recall at 1 .. topk of one fixed-stride result (the output form of
// xrl_predict_device / xrl_ensemble_device) against the true labels, as the reference's smat_util.Metrics.generate
// (pecos/utils/smat_util.py:968-997) computes them on the host:
//
//   pY = sorted_csr(pY)                           every row ordered by (value descending, -0.0 tied with +0.0, NaN last, label ascending)
//   matched = isin(row[:topk], truth)             explicit zeros stay entries
//   cum = cumsum(matched)                         cum[p] = matched entries of rank <= p; positions past the row carry its last value
//   total_matched += cum;  recall += cum / max(len(truth), 1)        a row without entries adds nothing
//
// One wavefront per row, NS entries per lane (entry j = i * 64 + lane, NS chosen on the host from max(stride, topk) <= 1024), as in K6:
// the row's (key, label) pairs go to wavefront-private LDS (8 bytes each, at most 8 KB) and every entry's rank is the number of pairs
// that order before it (labels are distinct, so the ranks are a permutation).  The stored order of a row is NOT trusted: predict breaks
// ties by candidate position, the reference's metrics by label.  Every lane binary-searches the sorted true row in global memory for its
// labels; the flags are scattered to LDS by rank, and per 64 positions one ballot and a popcount prefix give cum[p] to lane p % 64,
// slot p / 64, which accumulates it as an integer and cum[p] / max(n_true, 1) as an IEEE fp64 quotient.
//
// Reduction, a function of the inputs only: wavefront w takes the rows [w * R, (w + 1) * R) in ascending order, R = R(rows) =
// 64 * max(1, ceil(rows / 262144)) (at most 4096 wavefronts), and stores ONE partial; metrics_reduce_kernel (one workgroup, one thread
// per position) adds the partials in ascending w.  No atomics: the sums do not depend on the CU count or the launch order, and for
// rows <= R the fp64 sum is the reference's own row-order sum, bit for bit.
// The wavefront's integer accumulator is 32 bits wide: R <= 64 * ceil((2^32 - 1) / 262144) = 2^20 rows of cum <= 1024 = 2^10 sum to at
// most 2^30.  The partials and the totals are 64 bits.
#include <hip/hip_runtime.h>

#include "xrl_device.h"
#include "xrl_kernels.h"

namespace xrl {

constexpr int kMetricsWaves = 4;         // wavefronts per workgroup
constexpr uint32_t kMetricsRowsPerStep = 262144;

template <int NS>
__global__ void __launch_bounds__(kMetricsWaves * 64)
metrics_kernel(MetricsArgs A, uint32_t R, uint32_t n_waves, uint64_t* __restrict__ part_m, double* __restrict__ part_r) {
    __shared__ uint2 lds[kMetricsWaves][NS * 64];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
    const uint32_t w = blockIdx.x * (uint32_t)kMetricsWaves + (uint32_t)wave;
    if (w >= n_waves) return;                                          // (whole wavefronts; no workgroup barrier below)
    uint2* sc = lds[wave];
    uint32_t* fl = reinterpret_cast<uint32_t*>(sc);                    // the match flags by rank reuse the list's first 4 bytes x T
    const uint32_t topk = A.topk;
    const uint32_t r_begin = w * R;                                    // < rows
    const uint32_t r_end = A.rows - r_begin > R ? r_begin + R : A.rows;

    uint32_t accm[NS];                                                 // <= 2^20 rows x 2^10 (see the head of the file)
    double accr[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) { accm[i] = 0u; accr[i] = 0.0; }

    for (uint32_t r = r_begin; r < r_end; ++r) {
        const uint32_t T = min(A.cnt[r], A.stride);                    // <= NS * 64 (host check)
        if (T == 0) continue;                                          // len(cum_matched) == 0: nothing, whatever the true row holds
        const uint64_t tb = A.true_ptr[r], t1 = A.true_ptr[r + 1], te = t1 > tb ? t1 : tb;
        const double n_true = (double)(te > tb ? te - tb : (uint64_t)1);   // len(truth), duplicates included; max(.., 1)

        // ---- load and publish (key, label)
        uint32_t lab[NS];
        uint64_t key[NS];                                              // (ordering key << 32 | ~label): larger = earlier, one comparison
        const uint32_t* __restrict__ pi = A.idx + (uint64_t)r * A.stride;
        const float* __restrict__ pv = A.val + (uint64_t)r * A.stride;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
            lab[i] = 0; key[i] = 0;
            if (j < T) {
                lab[i] = pi[j];
                const uint32_t k = ensemble_key(pv[j]);
                key[i] = (uint64_t)k << 32 | (uint64_t)~lab[i];
                sc[j] = make_uint2(~lab[i], k);
            }
        }
        wave_sync_lds();

        // ---- rank = pairs that order before mine (key descending, label ascending); an empty slot's key 0 is below every pair
        uint32_t rank[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) rank[i] = 0;
#pragma unroll 2
        for (uint32_t jj = 0; jj < T; ++jj) {
            const uint2 e = sc[jj];
            const uint64_t ek = (uint64_t)e.y << 32 | (uint64_t)e.x;
#pragma unroll
            for (int i = 0; i < NS; ++i) rank[i] += ek > key[i] ? 1u : 0u;
        }
        wave_sync_lds();                                               // every lane has read the list: the flags overwrite it below

        // ---- match: binary search of the sorted true row, one label per lane and slot.  The steps depend on the row's length only, so the
        // loop is wave-uniform and branch-free: the last true label <= mine (or the first of the row) is in [at, at + n) throughout, every
        // probe stays inside [tb, te) -- also for the lanes and slots past the row's end, which search for label 0 (one broadcast load per slot)
        // and store nothing.
        uint64_t at[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) at[i] = tb;
        for (uint64_t n = te - tb; n > 1; n -= n >> 1) {
            const uint64_t half = n >> 1;
#pragma unroll
            for (int i = 0; i < NS; ++i) at[i] = A.true_idx[at[i] + half] <= lab[i] ? at[i] + half : at[i];
        }
        // flag to LDS by rank (rank < T: an entry does not count itself)
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const uint32_t j = (uint32_t)i * 64u + (uint32_t)lane;
            if (j < T) fl[rank[i]] = (te > tb && A.true_idx[at[i]] == lab[i]) ? 1u : 0u;
        }
        wave_sync_lds();

        // ---- cumulate and accumulate: position p = i * 64 + lane; past the row the flags are none, so cum carries cum[T - 1]
        uint32_t base = 0;
#pragma unroll
        for (int i = 0; i < NS; ++i) {                                 // (every slot, also those past topk, which are never stored)
            const uint32_t p = (uint32_t)i * 64u + (uint32_t)lane;
            const bool f = p < T && fl[p] != 0u;
            const unsigned long long b = __ballot(f);
            const uint32_t cum = base + lanes_below(b) + (f ? 1u : 0u);
            base += (uint32_t)__popcll(b);
            accm[i] += cum;
            accr[i] = accr[i] + (double)cum / n_true;
        }
        wave_sync_lds();                                               // the flags are read: the next row's list may take their place
    }

#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const uint32_t p = (uint32_t)i * 64u + (uint32_t)lane;
        if (p < topk) {
            part_m[(uint64_t)w * topk + p] = (uint64_t)accm[i];
            part_r[(uint64_t)w * topk + p] = accr[i];
        }
    }
}

// the partials in ascending wavefront order, one thread per position
__global__ void __launch_bounds__(1024)
metrics_reduce_kernel(const uint64_t* __restrict__ part_m, const double* __restrict__ part_r, uint32_t n_waves, uint32_t topk,
                      uint64_t* __restrict__ matched, double* __restrict__ recall_sum) {
    const uint32_t p = threadIdx.x;
    if (p >= topk) return;
    uint64_t m = 0;
    double s = 0.0;
    for (uint32_t w = 0; w < n_waves; ++w) {
        m += part_m[(uint64_t)w * topk + p];
        s = s + part_r[(uint64_t)w * topk + p];
    }
    matched[p] = m;
    recall_sum[p] = s;
}

uint32_t metrics_rows_per_wave(uint32_t rows) {
    const uint32_t steps = rows / kMetricsRowsPerStep + (rows % kMetricsRowsPerStep ? 1u : 0u);
    return 64u * (steps ? steps : 1u);
}

uint32_t metrics_waves(uint32_t rows) {
    const uint32_t R = metrics_rows_per_wave(rows);
    return rows / R + (rows % R ? 1u : 0u);
}

size_t metrics_scratch_bytes(uint32_t rows, uint32_t topk) { return (size_t)metrics_waves(rows) * topk * (sizeof(uint64_t) + sizeof(double)); }

template <int NS>
static void launch_metrics_ns(const MetricsArgs& A, uint32_t R, uint32_t n_waves, uint64_t* part_m, double* part_r, hipStream_t s) {
    const dim3 grid((n_waves + (uint32_t)kMetricsWaves - 1u) / (uint32_t)kMetricsWaves), block(kMetricsWaves * 64);
    hipLaunchKernelGGL((metrics_kernel<NS>), grid, block, 0, s, A, R, n_waves, part_m, part_r);
    XRL_LAUNCH_CHECK();
}

void launch_metrics(const MetricsArgs& A, void* scratch, hipStream_t s) {
    if (A.rows == 0) return;
    if (A.stride == 0 || A.stride > kMetricsMax || A.topk == 0 || A.topk > kMetricsMax) fail("metrics: shape outside the kernel's capacity");
    if (!scratch) fail("metrics: the partial sums need their scratch");
    const uint32_t R = metrics_rows_per_wave(A.rows), n_waves = metrics_waves(A.rows);
    uint64_t* part_m = static_cast<uint64_t*>(scratch);
    double* part_r = reinterpret_cast<double*>(part_m + (size_t)n_waves * A.topk);
    switch (ensemble_slots(A.stride > A.topk ? A.stride : A.topk)) {
    case 1: launch_metrics_ns<1>(A, R, n_waves, part_m, part_r, s); break;
    case 2: launch_metrics_ns<2>(A, R, n_waves, part_m, part_r, s); break;
    case 4: launch_metrics_ns<4>(A, R, n_waves, part_m, part_r, s); break;
    case 8: launch_metrics_ns<8>(A, R, n_waves, part_m, part_r, s); break;
    default: launch_metrics_ns<16>(A, R, n_waves, part_m, part_r, s); break;
    }
    hipLaunchKernelGGL(metrics_reduce_kernel, dim3(1), dim3((A.topk + 63u) / 64u * 64u), 0, s, part_m, part_r, n_waves, A.topk, A.matched, A.recall_sum);
    XRL_LAUNCH_CHECK();
}

}  // namespace xrl
