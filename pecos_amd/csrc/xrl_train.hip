// K13: ranker training.  One (cluster, label) job of the reference's multilabel_train_with_codes (linear_solver.hpp:797-860) is the dual
// coordinate descent of solve_l2r_l1l2_svc (:420-528) over the instances init_worker (:667-712) lists, and its weights pass the emission
// of SVMJob::solve (:718-779).  The rule is stated in include/xrl_abi.h.
//   k13_check        ids of a CSR below a bound, optionally strictly ascending per row, row pointers monotone
//   k13_same         two row pointers / id arrays are the same (R against Y)
//   k13_labels       a label listed twice in C
//   k13_sizes        the longest M and Y columns and the largest sums of feature-row lengths over them: the sizes of a slot and of a staging row
//   k13_solve        ONE WAVEFRONT OWNS ONE JOB AT A TIME and takes the next from a counter by an atomic add; no wavefront waits on another.
//                    Its slot of scratch: the dense w [cols] with a bitmap of the features its instances touch, and index / alpha / QD /
//                    cost / y per instance.  Per coordinate the lanes load the row 64 pairs a step, gather w, round the fp32 products and
//                    add them as ONE chain in stored order; every lane computes the same fp64 scalars; the lanes apply the axpy in parallel
//                    (a row's ids are strictly ascending, so no two lanes meet).  The shuffle and the order of the coordinates are serial
//                    by the rule: lane 0 shuffles, reading the shared table of mt19937(0) outputs through the job's own cursor.  A job that
//                    reaches the table's end cleans its slot, is put on the redo list and ends; the host extends the table and the listed
//                    jobs run again from their start.  Loop bounds: a sweep visits at most `active` coordinates (each visit advances or
//                    shrinks), sweeps <= max_iter, a draw's rejections end with the table.
//   k13_label_counts, k13_place   the jobs' staged rows -> W^T by label
// A job's set-up and emission are xrl_train_job.h's, shared with K16 (xrl_newton.hip); train_layer below drives a layer for either solver.
#include <cstdlib>
#include <random>

#include "xrl_device.h"
#include "xrl_devprim.h"
#include "xrl_newton.h"
#include "xrl_train.h"
#include "xrl_train_job.h"

namespace xrl {

namespace {

constexpr const char* kWhat = "K13";

__global__ void __launch_bounds__(256)
k13_check(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ idx, uint32_t rows, uint64_t nnz, uint32_t bound, int sorted, uint32_t* __restrict__ flags) {
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (r >= rows) return;
    const uint64_t b = ptr[r], e = ptr[r + 1];
    uint32_t bad = 0;
    if (b > e || e > nnz || (r == 0 && b != 0) || (r + 1 == rows && e != nnz)) bad |= kBadPtr;
    else
        for (uint64_t x = b + lane; x < e; x += 64u) {
            const uint32_t f = idx[x];
            if (f >= bound) bad |= kBadId;
            if (sorted && x > b && idx[x - 1] >= f) bad |= kUnsorted;
        }
    if (bad) atomicOr(flags, bad);
}

__global__ void __launch_bounds__(256)
k13_same(const uint64_t* __restrict__ pa, const uint64_t* __restrict__ pb, uint64_t np, const uint32_t* __restrict__ ia, const uint32_t* __restrict__ ib, uint64_t ni,
         uint32_t* __restrict__ flags) {
    const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if ((x < np && pa[x] != pb[x]) || (x < ni && ia[x] != ib[x])) atomicOr(flags, (uint32_t)kDiffers);
}

__global__ void __launch_bounds__(256) k13_labels(const uint32_t* __restrict__ c_idx, uint64_t n, uint32_t* __restrict__ seen, uint32_t* __restrict__ flags) {
    const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (x < n && atomicAdd(&seen[c_idx[x]], 1u)) atomicOr(flags, (uint32_t)kTwice);
}

// rows [0, m_rows) of M^T then rows of Y^T: out[0] / out[2] <- the longest row, out[1] / out[3] <- the largest sum of the feature-row lengths of a row's instances
__global__ void __launch_bounds__(256)
k13_sizes(const uint64_t* __restrict__ m_ptr, const uint32_t* __restrict__ m_idx, uint32_t m_rows, const uint64_t* __restrict__ y_ptr, const uint32_t* __restrict__ y_idx,
          uint32_t y_rows, const uint64_t* __restrict__ x_ptr, unsigned long long* __restrict__ out) {
    const uint32_t r0 = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (r0 >= m_rows + y_rows) return;
    const bool isy = r0 >= m_rows;
    const uint32_t r = isy ? r0 - m_rows : r0;
    const uint64_t* ptr = isy ? y_ptr : m_ptr;
    const uint32_t* idx = isy ? y_idx : m_idx;
    const uint64_t b = ptr[r], e = ptr[r + 1];
    unsigned long long sum = 0;
    for (uint64_t x = b + lane; x < e; x += 64u) { const uint32_t i = idx[x]; sum += x_ptr[i + 1] - x_ptr[i]; }
    for (int d = 1; d < 64; d <<= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) { atomicMax(&out[isy ? 2 : 0], (unsigned long long)(e - b)); atomicMax(&out[isy ? 3 : 1], sum); }
}

struct K13Args : TrainJobArgs {
    int l2loss; uint64_t max_iter;
    // the rest of a slot's scratch, [slot * its size]
    float* alpha; float* qd;
    const uint32_t* table; uint64_t table_n;
    const uint32_t* job_list; uint32_t n_jobs; uint32_t* next;            // job_list null: jobs job0 .. job0 + n_jobs - 1
    uint32_t* redo; uint32_t* n_redo;
    unsigned long long* counters;                                          // iters, shrinks, reactivations, max_iter stops, clipped, lane rows, wave rows
};

// one uniform draw in [0, range), 1 <= range < 2^32: libstdc++'s uniform_int_distribution over a 32-bit generator (_S_nd: Lemire's
// multiply with the (-range) % range rejection).  false: the table ended.
__device__ __forceinline__ bool k13_draw(const uint32_t* __restrict__ table, uint64_t tn, uint64_t& cur, uint32_t range, uint32_t& out) {
    if (cur >= tn) return false;
    uint64_t prod = (uint64_t)table[cur++] * range;
    uint32_t low = (uint32_t)prod;
    if (low < range) {
        const uint32_t thr = (0u - range) % range;
        while (low < thr) {
            if (cur >= tn) return false;
            prod = (uint64_t)table[cur++] * range;
            low = (uint32_t)prod;
        }
    }
    out = (uint32_t)(prod >> 32);
    return true;
}

__device__ __forceinline__ bool k13_not_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

__device__ __forceinline__ void k13_swap(uint32_t* a, uint32_t i, uint32_t j) { const uint32_t t = a[i]; a[i] = a[j]; a[j] = t; }

// libstdc++'s std::shuffle (bits/stl_algo.h) of a[0, n) by one lane
__device__ bool k13_shuffle(uint32_t* a, uint32_t n, const uint32_t* __restrict__ table, uint64_t tn, uint64_t& cur) {
    if (n < 2) return true;
    uint32_t r;
    if (n <= 65535u) {
        uint32_t i = 1;
        if ((n & 1u) == 0) {
            if (!k13_draw(table, tn, cur, 2u, r)) return false;
            k13_swap(a, 1, r);
            i = 2;
        }
        for (; i < n; i += 2) {
            const uint32_t sr = i + 1u;
            if (!k13_draw(table, tn, cur, sr * (sr + 1u), r)) return false;
            k13_swap(a, i, r / (sr + 1u));
            k13_swap(a, i + 1, r % (sr + 1u));
        }
        return true;
    }
    for (uint32_t i = 1; i < n; ++i) {
        if (!k13_draw(table, tn, cur, i + 1u, r)) return false;
        k13_swap(a, i, r);
    }
    return true;
}

__device__ void k13_job(const K13Args& a, uint32_t job, uint32_t slot, uint32_t lane, unsigned long long (&ctr)[7]) {
    uint32_t* index = a.index + (uint64_t)slot * a.index_cap;
    float* alpha = a.alpha + (uint64_t)slot * a.N;
    float* qd = a.qd + (uint64_t)slot * a.N;
    float* cost = a.cost + (uint64_t)slot * a.N;
    signed char* ysg = a.ysg + (uint64_t)slot * a.N;
    float* w = a.w + (uint64_t)slot * a.d;
    uint32_t* touched = a.touched + (uint64_t)slot * a.dw;
    const double bias2 = a.bias > 0 ? a.bias * a.bias : 0.0;
    unsigned long long before[7];
    for (int k = 0; k < 7; ++k) before[k] = ctr[k];

    uint32_t label = job, code = 0;
    if (a.c_ptr) { label = a.c_idx[job]; code = segment_of(a.c_ptr, a.K, (uint64_t)job); }

    const uint32_t n = train_job_setup(a, label, code, lane, index, cost, ysg);

    // ---- QD = diag + x'x + bias^2, alpha = 0, and the features the job can touch.  The reference also adds y * alpha = (+-)0 times the row
    //      to w and (+-)0 * bias to b here (:444-446): nothing for a finite entry (w is +0), a NaN where X stores an inf or a NaN and, with an
    //      infinite bias, in b.  Every lane that meets such an entry stores the same quiet NaN, so no order shows; a NaN is never emitted and
    //      every comparison reads any NaN alike.
    const float kNaN = __uint_as_float(0x7FC00000u);
    for (uint32_t s0 = 0; s0 < n; s0 += 64u) {
        const uint32_t s = s0 + lane;
        const bool have = s < n;
        uint32_t i = 0;
        uint64_t b = 0, e = 0;
        if (have) { i = index[s]; row_span(a.x_ptr, i, a.x_nnz, b, e); }
        const bool wide = have && e - b >= kTrainWaveRow;
        float acc = 0.0f;
        if (have && !wide)
            for (uint64_t j = b; j < e; ++j) {
                const float v = a.x_val[j];
                const uint32_t f = a.x_idx[j];
                acc = __fadd_rn(acc, __fmul_rn(v, v));
                atomicOr(&touched[f >> 5], 1u << (f & 31u));
                if (k13_not_finite(v)) w[f] = kNaN;
            }
        unsigned long long wm = __ballot(wide);
        ctr[5] += (unsigned long long)__popcll(__ballot(have && !wide));
        ctr[6] += (unsigned long long)__popcll(wm);
        while (wm) {                                                   // at most 64 turns
            const int l = __builtin_ctzll(wm);
            wm &= wm - 1;
            const uint64_t bb = __shfl(b, l), ee = __shfl(e, l);
            float ws = 0.0f;
            for (uint64_t x0 = bb; x0 < ee; x0 += 64u) {
                const uint64_t x = x0 + lane;
                float p = 0.0f;
                if (x < ee) {
                    const float v = a.x_val[x];
                    const uint32_t f = a.x_idx[x];
                    p = __fmul_rn(v, v);
                    atomicOr(&touched[f >> 5], 1u << (f & 31u));
                    if (k13_not_finite(v)) w[f] = kNaN;
                }
                ws = wave_chain(ws, p, (uint32_t)min((uint64_t)64u, ee - x0));
            }
            if ((int)lane == l) acc = ws;
        }
        if (have) {
            const double cc = (ysg[i] > 0 ? a.Cp : a.Cn) * (double)cost[i];
            float q = a.l2loss ? (float)(0.5 / cc) : 0.0f;
            q = (float)__dadd_rn((double)q, __dadd_rn((double)acc, bias2));
            qd[i] = q; alpha[i] = 0.0f;
        }
    }
    wave_sync_hbm();

    // ---- the sweeps
    const double kInf = HUGE_VAL;
    double pgmax_old = kInf, pgmin_old = -kInf;
    uint32_t active = n;
    uint64_t iter = 0, cur = 0;
    float bw = (n && a.bias == kInf) ? kNaN : 0.0f;                   // (+-)0 * inf of the set-up, once an instance exists
    bool table_end = false, converged = false;
    while (iter < a.max_iter) {
        double pgmax_new = -kInf, pgmin_new = kInf;
        uint32_t ok = 1;
        if (lane == 0) ok = k13_shuffle(index, active, a.table, a.table_n, cur) ? 1u : 0u;
        if (!first_lane(ok)) { table_end = true; break; }
        for (uint32_t s = 0; s < active;) {                            // every turn advances s or lowers active
            uint32_t i = 0, ab = 0;
            if (lane == 0) { i = index[s]; ab = __float_as_uint(alpha[i]); }
            i = first_lane(i);
            const float al = __uint_as_float(first_lane(ab));
            const int yi = ysg[i];
            uint64_t rb, re;
            row_span(a.x_ptr, i, a.x_nnz, rb, re);
            float acc = 0.0f;
            for (uint64_t x0 = rb; x0 < re; x0 += 64u) {
                const uint64_t x = x0 + lane;
                float p = 0.0f;
                if (x < re) p = __fmul_rn(w[a.x_idx[x]], a.x_val[x]);
                acc = wave_chain(acc, p, (uint32_t)min((uint64_t)64u, re - x0));
            }
            const double cc = (yi > 0 ? a.Cp : a.Cn) * (double)cost[i];
            const double diag = a.l2loss ? 0.5 / cc : 0.0, C = a.l2loss ? kInf : cc;
            double G = __dadd_rn(__dmul_rn((double)yi, __dadd_rn((double)acc, a.bias > 0 ? __dmul_rn((double)bw, a.bias) : 0.0)), -1.0);
            G = __dadd_rn(G, __dmul_rn((double)al, diag));
            double PG = 0.0;
            bool shrink = false;
            if (al == 0.0f) {
                if (G > pgmax_old) shrink = true;
                else if (G < 0.0) PG = G;
            } else if ((double)al == C) {
                if (G < pgmin_old) shrink = true;
                else if (G > 0.0) PG = G;
            } else {
                PG = G;
            }
            if (shrink) {
                --active;
                if (lane == 0) k13_swap(index, s, active);
                ++ctr[1];
                continue;
            }
            pgmax_new = pgmax_new < PG ? PG : pgmax_new;              // std::max(a, b) = a < b ? b : a
            pgmin_new = PG < pgmin_new ? PG : pgmin_new;              // std::min(a, b) = b < a ? b : a
            if (fabs(PG) > 1.0e-12) {
                const double ao = (double)al;
                double t = __dadd_rn(ao, -(G / (double)qd[i]));
                t = t < 0.0 ? 0.0 : t;
                if (C < t) { t = C; ++ctr[4]; }
                const float an = (float)t;
                const double dd = __dmul_rn(__dadd_rn((double)an, -ao), (double)yi);
                for (uint64_t x = rb + lane; x < re; x += 64u) {
                    const uint32_t f = a.x_idx[x];
                    w[f] = (float)__dadd_rn((double)w[f], __dmul_rn(dd, (double)a.x_val[x]));
                }
                if (a.bias > 0) bw = (float)__dadd_rn((double)bw, __dmul_rn(dd, a.bias));
                if (lane == 0) alpha[i] = an;
                wave_sync_hbm();
            }
            ++s;
        }
        ++iter;
        if (pgmax_new - pgmin_new <= a.eps) {
            if (active == n) { converged = true; break; }
            active = n; pgmax_old = kInf; pgmin_old = -kInf;
            ++ctr[2];
            continue;
        }
        pgmax_old = pgmax_new; pgmin_old = pgmin_new;
        if (pgmax_old <= 0) pgmax_old = kInf;
        if (pgmin_old >= 0) pgmin_old = -kInf;
    }
    ctr[0] += iter;
    if (!converged && !table_end) ++ctr[3];
    wave_sync_hbm();                                                   // lane 0's last swaps of index, and the last axpy, before every lane reads them below

    // ---- emission; a job the table failed stages nothing and runs again from its start: this attempt is not counted
    if (!train_job_emit(a, job, label, lane, w, touched, cost, index, n, bw, table_end)) {
        if (lane == 0) a.redo[atomicAdd(a.n_redo, 1u)] = job;
        for (int k = 0; k < 7; ++k) ctr[k] = before[k];
    }
}

__global__ void __launch_bounds__(64) k13_solve(K13Args a) {
    const uint32_t lane = threadIdx.x, slot = blockIdx.x;
    unsigned long long ctr[7] = {0, 0, 0, 0, 0, 0, 0};
    for (;;) {                                                         // at most n_jobs + 1 turns
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(a.next, 1u);
        t = first_lane(t);
        if (t >= a.n_jobs) break;
        k13_job(a, a.job_list ? a.job_list[t] : a.job0 + t, slot, lane, ctr);
    }
    if (lane == 0)
        for (int k = 0; k < 7; ++k)
            if (ctr[k]) atomicAdd(&a.counters[k], ctr[k]);
}

__global__ void __launch_bounds__(256)
k13_label_counts(const unsigned long long* __restrict__ cnt, const uint32_t* __restrict__ job_label, uint32_t jobs, uint32_t labels, unsigned long long* __restrict__ by_label) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < jobs && job_label[j] < labels) by_label[job_label[j]] = cnt[j];
}

// one wavefront per job of a chunk: its row, compacted at src[j] .. src[j + 1], goes to the row of its label
__global__ void __launch_bounds__(256)
k13_place(const unsigned long long* __restrict__ src, const uint32_t* __restrict__ job_label, uint32_t n, uint32_t labels, const uint32_t* __restrict__ c_idx,
          const float* __restrict__ c_val, const unsigned long long* __restrict__ out_ptr, uint32_t* __restrict__ idx, float* __restrict__ val) {
    const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (j >= n || job_label[j] >= labels) return;
    const unsigned long long b = src[j], len = src[j + 1] - b, dst = out_ptr[job_label[j]];
    for (unsigned long long x = threadIdx.x & 63u; x < len; x += 64u) { idx[dst + x] = c_idx[b + x]; val[dst + x] = c_val[b + x]; }
}

uint64_t env_u64(const char* name, uint64_t dflt) {
    if (const char* e = std::getenv(name)) { const uint64_t v = std::strtoull(e, nullptr, 10); if (v) return v; }
    return dflt;
}

uint32_t read_flags(const DevBuf& flags, hipStream_t s) {
    uint32_t f = 0;
    XRL_HIP(hipMemcpyAsync(&f, flags.p, 4, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    return f;
}

void check_csr(const std::string& what, const char* name, const QueriesDev& m, uint32_t bound, bool sorted, DevBuf& flags, hipStream_t s) {
    if (!m.rows) { if (m.nnz) fail(what + name + " has stored entries and no rows"); return; }
    hipLaunchKernelGGL(k13_check, dim3(blocks_of(m.rows, 4, kWhat)), dim3(256), 0, s, m.row_ptr, m.col_idx, m.rows, m.nnz, bound, sorted ? 1 : 0, flags.as<uint32_t>());
    XRL_LAUNCH_CHECK();
    const uint32_t f = read_flags(flags, s);
    if (f & kBadPtr) fail(what + name + "'s row pointer does not ascend from 0 to its count of stored entries");
    if (f & kBadId) fail(what + name + " holds an id that is not below " + std::to_string(bound));
    if (f & kUnsorted) fail(what + name + " has a row whose column ids are not strictly ascending");
}

struct Chunk { DevBuf ptr, idx, val; uint32_t job0 = 0, n = 0; };

}  // namespace

void same_pattern_device(const char* what, const QueriesDev& A, const QueriesDev& B, hipStream_t s) {
    DevBuf flags;
    flags.reserve(4);
    XRL_HIP(hipMemsetAsync(flags.p, 0, 4, s));
    const uint64_t np = (uint64_t)A.rows + 1, n = std::max(np, A.nnz);
    hipLaunchKernelGGL(k13_same, dim3(blocks_of(n, 256, kWhat)), dim3(256), 0, s, A.row_ptr, B.row_ptr, np, A.col_idx, B.col_idx, A.nnz, flags.as<uint32_t>());
    XRL_LAUNCH_CHECK();
    if (read_flags(flags, s) & kDiffers) fail(std::string(what) + ": Rt does not share Yt's pattern (row pointer and column ids)");
}

void check_train_params(const std::string& what, const TrainParams& p) {
    if (p.solver_type == 7) fail(what + "solver L2R_LR_DUAL is not served on the device (its Newton steps and logarithms are not part of K13)");
    if (p.solver_type == 2) fail(what + "solver L2R_L2LOSS_SVC_PRIMAL is not served on the device (its Newton method is not part of K13)");
    if (p.solver_type != kSolverL2LossDual && p.solver_type != kSolverL1LossDual)
        fail(what + "unknown solver_type " + std::to_string(p.solver_type) + " (1 = L2R_L2LOSS_SVC_DUAL, 3 = L2R_L1LOSS_SVC_DUAL)");
}

namespace {

// One layer, whichever solver: the checks, the sizes of a slot and of a staging row, the batches under the scratch budget, and W^T by
// label.  newton (NT) or the dual coordinate descent (T); the caller has refused the solvers its entry point does not serve.
void train_layer(const char* what_c, const QueriesDev& X, const QueriesDev& Yt, const float* r_val, const QueriesDev* Ct, const QueriesDev* Mt,
                 const TrainParams& p, hipStream_t s, DevCsr& out, TrainCounters& T, NewtonCounters* NT) {
    const std::string what = std::string(what_c) + ": ";
    const bool newton = NT != nullptr;
    const bool coded = Ct && Mt;
    const uint32_t N = X.rows, d = X.cols, L = Yt.rows;
    const uint64_t jobs64 = coded ? Ct->nnz : L;
    if (jobs64 >= 0xFFFFFFFFull) fail(what + "2^32 - 1 jobs or more");
    const uint32_t jobs = (uint32_t)jobs64;

    DevBuf flags, tmp;
    flags.reserve(4);
    XRL_HIP(hipMemsetAsync(flags.p, 0, 4, s));
    check_csr(what, "X", X, d, true, flags, s);
    if (newton) newton_check_finite(what, X, s);
    check_csr(what, "Y", Yt, N, false, flags, s);
    if (coded) {
        check_csr(what, "C", *Ct, L, false, flags, s);
        check_csr(what, "M", *Mt, N, false, flags, s);
        DevBuf seen;
        seen.reserve((size_t)L * 4 + 4);
        XRL_HIP(hipMemsetAsync(seen.p, 0, (size_t)L * 4 + 4, s));
        if (Ct->nnz) {
            hipLaunchKernelGGL(k13_labels, dim3(blocks_of(Ct->nnz, 256, kWhat)), dim3(256), 0, s, Ct->col_idx, Ct->nnz, seen.as<uint32_t>(), flags.as<uint32_t>());
            XRL_LAUNCH_CHECK();
        }
        if (read_flags(flags, s) & kTwice) fail(what + "a label is listed under two columns of C (or twice in one); a label has one weight vector");
    }

    // sizes of a slot and of a staging row
    DevBuf sizes;
    sizes.reserve(32);
    XRL_HIP(hipMemsetAsync(sizes.p, 0, 32, s));
    {
        const uint32_t mr = coded ? Mt->rows : 0u;
        if (mr + L) {
            hipLaunchKernelGGL(k13_sizes, dim3(blocks_of((uint64_t)mr + L, 4, kWhat)), dim3(256), 0, s, coded ? Mt->row_ptr : nullptr, coded ? Mt->col_idx : nullptr, mr,
                               Yt.row_ptr, Yt.col_idx, L, X.row_ptr, sizes.as<unsigned long long>());
            XRL_LAUNCH_CHECK();
        }
    }
    uint64_t sz[4];
    XRL_HIP(hipMemcpyAsync(sz, sizes.p, 32, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    // a stored position of Y appends its row when the row is not listed at that moment: with R a listed row can become unlisted (a cost
    // of 0), so in the pure form too every stored position of the longest Y column may append
    const uint64_t index_cap64 = coded ? sz[0] + sz[2] : (uint64_t)N + (r_val ? sz[2] : 0);
    if (index_cap64 >= (1ull << 31)) fail(what + "a job of 2^31 instances or more");
    const uint32_t index_cap = (uint32_t)(index_cap64 ? index_cap64 : 1);
    const uint64_t touched_max = coded ? sz[1] + sz[3] : X.nnz;
    const uint64_t stride64 = (p.threshold <= 0.0 ? (uint64_t)d : std::min<uint64_t>(d, touched_max)) + 1;
    const uint32_t stride = (uint32_t)stride64;
    const uint32_t dw = (d + 31u) / 32u;

    const uint64_t budget = env_u64("XRL_TRAIN_SCRATCH_BYTES", kTrainScratchBytes);
    const uint64_t slot_bytes = (uint64_t)index_cap * 4 + (uint64_t)N * (newton ? 5 : 13) + (uint64_t)d * 4 + (uint64_t)dw * 4 + (newton ? newton_slot_bytes(N, d, index_cap) : 0);
    const uint32_t slots = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({budget / std::max<uint64_t>(slot_bytes, 1), kTrainMaxSlots, std::max<uint32_t>(jobs, 1)}));
    const uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(budget / (stride64 * 8), std::max<uint32_t>(jobs, 1)));
    T.jobs = jobs; T.slots = slots; T.stride = stride;

    DevBuf b_index, b_alpha, b_qd, b_cost, b_y, b_w, b_touched, b_next, b_stidx, b_stval, b_cnt, b_label, b_redo, b_ctr, b_table, b_list;
    b_index.reserve((size_t)slots * index_cap * 4);
    if (!newton) { b_alpha.reserve((size_t)slots * N * 4); b_qd.reserve((size_t)slots * N * 4); }
    b_cost.reserve((size_t)slots * N * 4); b_y.reserve((size_t)slots * N);
    b_w.reserve((size_t)slots * d * 4); b_touched.reserve((size_t)slots * dw * 4);
    // a slot is clean between jobs: cost, w and the bitmap are zero (every job leaves them so)
    if (N) XRL_HIP(hipMemsetAsync(b_cost.p, 0, (size_t)slots * N * 4, s));
    if (d) XRL_HIP(hipMemsetAsync(b_w.p, 0, (size_t)slots * d * 4, s));
    if (d) XRL_HIP(hipMemsetAsync(b_touched.p, 0, (size_t)slots * dw * 4, s));
    b_next.reserve(8);                                                 // {next job, redo count}
    b_stidx.reserve((size_t)batch * stride * 4); b_stval.reserve((size_t)batch * stride * 4);
    b_cnt.reserve(((size_t)jobs + 1) * 8); b_label.reserve(((size_t)jobs + 1) * 4);
    XRL_HIP(hipMemsetAsync(b_cnt.p, 0, ((size_t)jobs + 1) * 8, s));
    XRL_HIP(hipMemsetAsync(b_label.p, 0xFF, ((size_t)jobs + 1) * 4, s));
    b_redo.reserve((size_t)batch * 4); b_list.reserve((size_t)batch * 4);
    b_ctr.reserve(7 * 8);
    XRL_HIP(hipMemsetAsync(b_ctr.p, 0, 7 * 8, s));

    // the one stream every job reads: std::mt19937(0), filled and extended by the host
    std::mt19937 gen(0);
    std::vector<uint32_t> table;
    auto grow_table = [&](uint64_t words) {
        const size_t from = table.size();
        table.resize((size_t)words);
        for (size_t k = from; k < table.size(); ++k) table[k] = (uint32_t)gen();
        b_table.release();
        b_table.upload(table);
    };
    if (!newton) grow_table(env_u64("XRL_TRAIN_RANDOM_WORDS", kTrainRandomWords));
    NewtonScratch nsc;
    if (newton) newton_reserve(nsc, slots, N, d, index_cap, s);

    K13Args a{};
    a.x_ptr = X.row_ptr; a.x_idx = X.col_idx; a.x_val = X.val; a.x_nnz = X.nnz; a.N = N; a.d = d;
    a.y_ptr = Yt.row_ptr; a.y_idx = Yt.col_idx; a.r_val = r_val; a.y_nnz = Yt.nnz;
    if (coded) { a.c_ptr = Ct->row_ptr; a.c_idx = Ct->col_idx; a.K = Ct->rows; a.m_ptr = Mt->row_ptr; a.m_idx = Mt->col_idx; a.m_nnz = Mt->nnz; }
    a.threshold = p.threshold; a.Cp = p.Cp; a.Cn = p.Cn; a.eps = p.eps; a.bias = p.bias;
    a.max_nz = p.max_nonzeros; a.l2loss = p.solver_type == kSolverL2LossDual; a.max_iter = p.max_iter;
    a.index = b_index.as<uint32_t>(); a.index_cap = index_cap; a.alpha = b_alpha.as<float>(); a.qd = b_qd.as<float>(); a.cost = b_cost.as<float>();
    a.ysg = b_y.as<signed char>(); a.w = b_w.as<float>(); a.touched = b_touched.as<uint32_t>(); a.dw = dw;
    a.next = b_next.as<uint32_t>(); a.n_redo = b_next.as<uint32_t>() + 1;
    a.st_idx = b_stidx.as<uint32_t>(); a.st_val = b_stval.as<float>(); a.stride = stride;
    a.cnt = b_cnt.as<unsigned long long>(); a.job_label = b_label.as<uint32_t>();
    a.redo = b_redo.as<uint32_t>(); a.flags = flags.as<uint32_t>(); a.counters = b_ctr.as<unsigned long long>();

    std::vector<Chunk> chunks;
    for (uint32_t j0 = 0; j0 < jobs; j0 += batch) {
        const uint32_t nb = std::min(batch, jobs - j0);
        ++T.batches;
        a.job0 = j0; a.n_jobs = nb; a.job_list = nullptr;
        if (newton) {
            XRL_HIP(hipMemsetAsync(b_next.p, 0, 8, s));
            newton_launch(a, nsc, nb, a.next, std::min(slots, nb), s);
            const uint32_t bad = newton_bad_job(nsc, s);
            if (bad != 0xFFFFFFFFu) {
                uint32_t label = 0;
                XRL_HIP(hipMemcpy(&label, a.job_label + bad, 4, hipMemcpyDeviceToHost));
                fail(what + "label " + std::to_string(label) + ": the conjugate-gradient steps met a step length that is not finite; the reference then puts NaNs into " +
                     "features that no instance of the label stores, which this form does not cover");
            }
        }
        for (uint32_t ext = 0; !newton; ++ext) {
            a.table = b_table.as<uint32_t>(); a.table_n = table.size();
            XRL_HIP(hipMemsetAsync(b_next.p, 0, 8, s));
            hipLaunchKernelGGL(k13_solve, dim3(std::min(slots, a.n_jobs)), dim3(64), 0, s, a);
            XRL_LAUNCH_CHECK();
            uint32_t nr[2];
            XRL_HIP(hipMemcpyAsync(nr, b_next.p, 8, hipMemcpyDeviceToHost, s));
            XRL_HIP(hipStreamSynchronize(s));
            if (!nr[1]) break;
            if (ext >= kTrainMaxExtensions) fail(what + "the table of random words was extended " + std::to_string(ext) + " times and a job still reached its end");
            grow_table((uint64_t)table.size() * 4);
            ++T.extensions; T.reruns += nr[1];
            XRL_HIP(hipMemcpyAsync(b_list.p, b_redo.p, (size_t)nr[1] * 4, hipMemcpyDeviceToDevice, s));
            a.job_list = b_list.as<uint32_t>(); a.n_jobs = nr[1];
        }
        if (read_flags(flags, s) & kStageFull) fail(what + "a job emitted more entries than its staging row holds");
        // the batch's rows, compacted in job order
        Chunk c;
        c.job0 = j0; c.n = nb;
        c.ptr.reserve(((size_t)nb + 1) * 8);
        const uint64_t total = scan_total(tmp, reinterpret_cast<const uint64_t*>(a.cnt + j0), c.ptr.as<uint64_t>(), nb, s);
        c.idx.reserve(total * 4); c.val.reserve(total * 4);
        launch_copy_rows(c.ptr.as<uint64_t>(), nb, nullptr, stride, a.st_idx, a.st_val, c.idx.as<uint32_t>(), c.val.as<float>(), kWhat, s);
        XRL_HIP(hipStreamSynchronize(s));
        chunks.push_back(std::move(c));
    }

    // W^T by label
    DevBuf by_label;
    by_label.reserve(((size_t)L + 1) * 8);
    XRL_HIP(hipMemsetAsync(by_label.p, 0, ((size_t)L + 1) * 8, s));
    if (jobs) {
        hipLaunchKernelGGL(k13_label_counts, dim3(blocks_of(jobs, 256, kWhat)), dim3(256), 0, s, a.cnt, a.job_label, jobs, L, by_label.as<unsigned long long>());
        XRL_LAUNCH_CHECK();
    }
    out.ptr.reserve(((size_t)L + 1) * 8);
    out.nnz = scan_total(tmp, by_label.as<uint64_t>(), out.ptr.as<uint64_t>(), L, s);
    out.idx.reserve(out.nnz * 4); out.val.reserve(out.nnz * 4);
    for (const Chunk& c : chunks) {
        hipLaunchKernelGGL(k13_place, dim3(blocks_of(c.n, 4, kWhat)), dim3(256), 0, s, c.ptr.as<unsigned long long>(), a.job_label + c.job0, c.n, L, c.idx.as<uint32_t>(),
                           c.val.as<float>(), out.ptr.as<unsigned long long>(), out.idx.as<uint32_t>(), out.val.as<float>());
        XRL_LAUNCH_CHECK();
    }
    if (newton) {
        NT->jobs = T.jobs; NT->batches = T.batches; NT->slots = T.slots; NT->stride = T.stride;
        newton_read_counters(nsc, *NT, s);
        return;
    }
    uint64_t ctr[7];
    XRL_HIP(hipMemcpyAsync(ctr, b_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    T.iters = ctr[0]; T.shrinks = ctr[1]; T.reactivations = ctr[2]; T.max_iter_stops = ctr[3]; T.clipped = ctr[4]; T.lane_rows = ctr[5]; T.wave_rows = ctr[6];
}

}  // namespace

void train_layer_device(const char* what, const QueriesDev& X, const QueriesDev& Yt, const float* r_val, const QueriesDev* Ct, const QueriesDev* Mt,
                        const TrainParams& p, hipStream_t s, DevCsr& out, TrainCounters& T) {
    check_train_params(std::string(what) + ": ", p);
    train_layer(what, X, Yt, r_val, Ct, Mt, p, s, out, T, nullptr);
}

void train_layer_newton_device(const char* what, const QueriesDev& X, const QueriesDev& Yt, const float* r_val, const QueriesDev* Ct, const QueriesDev* Mt,
                               const TrainParams& p, hipStream_t s, DevCsr& out, NewtonCounters& NT) {
    check_newton_params(std::string(what) + ": ", p);
    TrainCounters T;
    train_layer(what, X, Yt, r_val, Ct, Mt, p, s, out, T, &NT);
}

}  // namespace xrl
