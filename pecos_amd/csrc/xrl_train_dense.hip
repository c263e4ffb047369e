// K13D: ranker training over a dense row-major X in HBM -- K13's jobs (xrl_train.hip: the same launch shape, slots, table of mt19937(0)
// outputs with its redo list, lane 0's shuffle, fp64 scalars, set-up and emission of xrl_train_job.h) with a data path of its own for rows
// that store every column.  The rule is R13D in include/xrl_abi.h: K13's on the CSR of all rows * cols entries, zeros included.
//   Ownership.  A step is 256 columns; lane l owns columns 256 s + 4 l .. + 3 of every step s and loads them as one float4 (scalar loads
//     with the same ownership when the rows are not 16-byte aligned, and in the lane that holds the row's end).  No index is loaded,
//     nothing is gathered, the set-up keeps no bitmap and uses no atomic.
//   w never leaves the lane that owns it.  k13d_solve<STEPS>, STEPS = 1 .. 4 (cols <= 256 STEPS): w is 4 STEPS registers and the current
//     row another 4 STEPS, kept from the dot product to the axpy: a row is read once per coordinate.  k13d_solve<0> (up to 16384 columns):
//     w is in the workgroup's LDS, each float4 read and written by its owning lane only -- no cross-lane LDS traffic, so no barrier inside
//     a sweep; the row streams through a ring of 4 steps and is read again for the axpy.
//   The chain.  ONE fp32 chain in column order: per step, lane j = 0 .. 63, component c = 0 .. 3, acc = fl32(acc + fl32(w * x)) from lane
//     broadcasts with a uniform lane number, eight lanes (32 broadcasts) unrolled so that they run ahead of the dependent adds.  cols
//     dependent adds per coordinate are the floor of this kernel; x'x of the set-up takes the same walk.
//   In flight under the chain of position s: the row (LDS form: its first 4 steps) of position s + 1, whose id comes from a window of 64
//     positions of index held in registers -- no dependent load ahead of the row's.  A shrink swaps index, so the window is read again;
//     the row in flight is then the one after next and is kept.  The order of the coordinates is the rule's.
//   Hand-off.  A job that stages stores w to its slot's w in HBM, sets the bitmap to every column when it has an instance, and calls
//     train_job_emit as it is: cols stores a job against cols adds a coordinate.
#include <algorithm>
#include <atomic>

#include "xrl_device.h"
#include "xrl_train.h"
#include "xrl_train_job.h"

namespace xrl {

namespace {

constexpr int kRing = (int)kTrainDenseRegSteps;                        // steps of a row in registers: all of it (register form) or a ring (LDS form)

struct K13DArgs : K13Args {
    const float* X; uint64_t row_stride;
    uint32_t nst;                                                      // steps of a row: ceil(d / 256)
    int vec;                                                           // every row starts 16-byte aligned
};

__device__ __forceinline__ float4 k13d_mul(const float4& a, const float4& b) {
    return make_float4(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y), __fmul_rn(a.z, b.z), __fmul_rn(a.w, b.w));
}

// acc + p(column 0) + p(column 1) + ... over the first cnt <= 256 columns of a step, one rounded addition after the other; every lane
// computes the same sum
__device__ __forceinline__ float k13d_chain(float acc, const float4& p, uint32_t cnt) {
    const uint32_t full = cnt >> 2, rem = cnt & 3u;
    uint32_t j = 0;
    for (; j + 8u <= full; j += 8u) {
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) {
            const float a0 = lane_f32(p.x, j + u), a1 = lane_f32(p.y, j + u), a2 = lane_f32(p.z, j + u), a3 = lane_f32(p.w, j + u);
            acc = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(acc, a0), a1), a2), a3);
        }
    }
    for (; j < full; ++j) {                                            // at most 7 turns
        const float a0 = lane_f32(p.x, j), a1 = lane_f32(p.y, j), a2 = lane_f32(p.z, j), a3 = lane_f32(p.w, j);
        acc = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(acc, a0), a1), a2), a3);
    }
    if (rem) {                                                         // the lane that holds the row's end
        acc = __fadd_rn(acc, lane_f32(p.x, full));
        if (rem > 1u) acc = __fadd_rn(acc, lane_f32(p.y, full));
        if (rem > 2u) acc = __fadd_rn(acc, lane_f32(p.z, full));
    }
    return acc;
}

__device__ __forceinline__ uint32_t k13d_step_cols(uint32_t d, uint32_t st) { return d > st * kTrainDenseStep ? min(kTrainDenseStep, d - st * kTrainDenseStep) : 0u; }

// the set-up's (+-)0 * x: a NaN where x is an inf or a NaN
__device__ __forceinline__ void k13d_poison(float4& w, const float4& x) {
    const float kNaN = __uint_as_float(0x7FC00000u);
    if (k13_not_finite(x.x)) w.x = kNaN;
    if (k13_not_finite(x.y)) w.y = kNaN;
    if (k13_not_finite(x.z)) w.z = kNaN;
    if (k13_not_finite(x.w)) w.w = kNaN;
}

// w + dd * x: an fp64 product and an fp64 add, rounded on the store
__device__ __forceinline__ void k13d_axpy(float4& w, double dd, const float4& x) {
    w.x = (float)__dadd_rn((double)w.x, __dmul_rn(dd, (double)x.x));
    w.y = (float)__dadd_rn((double)w.y, __dmul_rn(dd, (double)x.y));
    w.z = (float)__dadd_rn((double)w.z, __dmul_rn(dd, (double)x.z));
    w.w = (float)__dadd_rn((double)w.w, __dmul_rn(dd, (double)x.w));
}

// What a form keeps of w and of the current row.  STEPS 1 .. 4: both whole, in registers.  STEPS 0: w in LDS (wl[st * 64 + lane]), of the row a
// ring of kRing steps that holds its first steps on entry to a walk.
template <int STEPS> struct K13DState {
    static constexpr int R = STEPS ? STEPS : kRing;
    float4 w[STEPS ? STEPS : 1];
    float4 x[R];
    float4* wl;
};

// the first R steps of a row
template <int R> __device__ __forceinline__ void k13d_head(const K13DArgs& a, const float* __restrict__ row, uint32_t lane, float4 (&x)[R]) {
#pragma unroll
    for (int u = 0; u < R; ++u) x[u] = k13d_load(row, (uint32_t)u * kTrainDenseStep + 4u * lane, a.d, a.vec);
}

// The walk of a row in column order: SQ: the chain of fl32(x * x), and the set-up's poison into w; else the chain of fl32(w * x).
template <int STEPS, bool SQ> __device__ __forceinline__ float k13d_walk(const K13DArgs& a, const float* __restrict__ row, uint32_t lane, K13DState<STEPS>& st) {
    float acc = 0.0f;
    if constexpr (STEPS != 0) {
#pragma unroll
        for (int u = 0; u < STEPS; ++u) {
            if (SQ) k13d_poison(st.w[u], st.x[u]);
            acc = k13d_chain(acc, k13d_mul(SQ ? st.x[u] : st.w[u], st.x[u]), k13d_step_cols(a.d, (uint32_t)u));
        }
    } else {
        for (uint32_t s0 = 0; s0 < a.nst; s0 += (uint32_t)kRing) {
#pragma unroll
            for (int u = 0; u < kRing; ++u) {
                const uint32_t s = s0 + (uint32_t)u;
                if (s < a.nst) {
                    const float4 x = st.x[u];
                    float4 w = st.wl[s * 64u + lane];
                    if (SQ) {
                        const float4 before = w;
                        k13d_poison(w, x);
                        if (__float_as_uint(w.x) != __float_as_uint(before.x) || __float_as_uint(w.y) != __float_as_uint(before.y) ||
                            __float_as_uint(w.z) != __float_as_uint(before.z) || __float_as_uint(w.w) != __float_as_uint(before.w))
                            st.wl[s * 64u + lane] = w;
                    }
                    if (s + (uint32_t)kRing < a.nst) st.x[u] = k13d_load(row, (s + (uint32_t)kRing) * kTrainDenseStep + 4u * lane, a.d, a.vec);   // in flight under the chain
                    acc = k13d_chain(acc, k13d_mul(SQ ? x : w, x), k13d_step_cols(a.d, s));
                }
            }
        }
    }
    return acc;
}

template <int STEPS> __device__ __forceinline__ void k13d_update(const K13DArgs& a, const float* __restrict__ row, uint32_t lane, K13DState<STEPS>& st, double dd) {
    if constexpr (STEPS != 0) {
#pragma unroll
        for (int u = 0; u < STEPS; ++u) k13d_axpy(st.w[u], dd, st.x[u]);
    } else {
        for (uint32_t s0 = 0; s0 < a.nst; s0 += (uint32_t)kRing) {     // the row again, kRing loads in flight
            float4 x[kRing];
#pragma unroll
            for (int u = 0; u < kRing; ++u) x[u] = k13d_load(row, (s0 + (uint32_t)u) * kTrainDenseStep + 4u * lane, a.d, a.vec);   // (past the row: zeros, nothing loaded)
#pragma unroll
            for (int u = 0; u < kRing; ++u) {
                const uint32_t s = s0 + (uint32_t)u;
                if (s < a.nst) { float4 w = st.wl[s * 64u + lane]; k13d_axpy(w, dd, x[u]); st.wl[s * 64u + lane] = w; }
            }
        }
    }
}

template <int STEPS> __device__ void k13d_job(const K13DArgs& a, uint32_t job, uint32_t slot, uint32_t lane, float4* wl, unsigned long long (&ctr)[7]) {
    constexpr int R = K13DState<STEPS>::R;
    uint32_t* index = a.index + (uint64_t)slot * a.index_cap;
    float* alpha = a.alpha + (uint64_t)slot * a.N;
    float* qd = a.qd + (uint64_t)slot * a.N;
    float* cost = a.cost + (uint64_t)slot * a.N;
    signed char* ysg = a.ysg + (uint64_t)slot * a.N;
    float* w = a.w + (uint64_t)slot * a.d;
    uint32_t* touched = a.touched + (uint64_t)slot * a.dw;
    const double bias2 = a.bias > 0 ? a.bias * a.bias : 0.0;
    const float kNaN = __uint_as_float(0x7FC00000u);
    unsigned long long before[7];
    for (int k = 0; k < 7; ++k) before[k] = ctr[k];

    uint32_t label = job, code = 0;
    if (a.c_ptr) { label = a.c_idx[job]; code = segment_of(a.c_ptr, a.K, (uint64_t)job); }

    K13DState<STEPS> st;
    st.wl = wl;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (STEPS != 0) {
#pragma unroll
        for (int u = 0; u < STEPS; ++u) st.w[u] = zero4;
    } else {
        for (uint32_t s = 0; s < a.nst; ++s) wl[s * 64u + lane] = zero4;
    }

    const uint32_t n = train_job_setup(a, label, code, lane, index, cost, ysg);

    // ---- QD = diag + x'x + bias^2, alpha = 0, and the set-up's poison (see k13_job): one listed position after the other, the next row in flight
    float4 xn[R];
    uint32_t idw = 0;
    ctr[a.d >= kTrainWaveRow ? 6 : 5] += n;
    for (uint32_t t = 0; t < n; ++t) {
        const uint32_t k = t & 63u;
        if (k == 0) idw = t + lane < n ? index[t + lane] : 0u;
        const uint32_t i = lane_u32(idw, k);
        const float* row = a.X + (uint64_t)i * a.row_stride;
        if (k == 0) k13d_head<R>(a, row, lane, st.x);
        else {
#pragma unroll
            for (int u = 0; u < R; ++u) st.x[u] = xn[u];
        }
        if (k + 1u < 64u && t + 1u < n) k13d_head<R>(a, a.X + (uint64_t)lane_u32(idw, k + 1u) * a.row_stride, lane, xn);
        const int yi = ysg[i];
        const float ci = cost[i];
        const float acc = k13d_walk<STEPS, true>(a, row, lane, st);
        const double cc = (yi > 0 ? a.Cp : a.Cn) * (double)ci;
        float q = a.l2loss ? (float)(0.5 / cc) : 0.0f;
        q = (float)__dadd_rn((double)q, __dadd_rn((double)acc, bias2));
        if (lane == 0) { qd[i] = q; alpha[i] = 0.0f; }
    }
    wave_sync_hbm();

    // ---- the sweeps (k13_job's, the scalars of a coordinate unchanged)
    const double kInf = HUGE_VAL;
    double pgmax_old = kInf, pgmin_old = -kInf;
    uint32_t active = n;
    uint64_t iter = 0, cur = 0;
    float bw = (n && a.bias == kInf) ? kNaN : 0.0f;
    bool table_end = false, converged = false;
    bool have_next = false;                                            // xn holds the first R steps of row nid
    uint32_t nid = 0;
    while (iter < a.max_iter) {
        double pgmax_new = -kInf, pgmin_new = kInf;
        uint32_t ok = 1;
        if (lane == 0) ok = k13_shuffle(index, active, a.table, a.table_n, cur) ? 1u : 0u;
        if (!first_lane(ok)) { table_end = true; break; }
        wave_sync_hbm();                                               // lane 0's shuffle, before every lane reads its part of the window
        bool reload = true;
        uint32_t s0 = 0;
        for (uint32_t s = 0; s < active;) {                            // every turn advances s or lowers active
            if (reload || s - s0 >= 64u) { idw = s + lane < active ? index[s + lane] : 0u; s0 = s; reload = false; }
            const uint32_t i = lane_u32(idw, s - s0);
            const float* row = a.X + (uint64_t)i * a.row_stride;
            if (have_next && nid == i) {
#pragma unroll
                for (int u = 0; u < R; ++u) st.x[u] = xn[u];
            } else {
                k13d_head<R>(a, row, lane, st.x);
            }
            if (s + 1u < active && s + 1u - s0 < 64u) {
                const uint32_t ni = lane_u32(idw, s + 1u - s0);
                if (!(have_next && nid == ni)) k13d_head<R>(a, a.X + (uint64_t)ni * a.row_stride, lane, xn);
                nid = ni; have_next = true;
            }
            const float al = alpha[i];
            const int yi = ysg[i];
            const float ci = cost[i];
            const float q = qd[i];
            const float acc = k13d_walk<STEPS, false>(a, row, lane, st);
            const double cc = (yi > 0 ? a.Cp : a.Cn) * (double)ci;
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
                wave_sync_hbm();                                       // the window is read again from the swapped order
                reload = true;
                ++ctr[1];
                continue;
            }
            pgmax_new = pgmax_new < PG ? PG : pgmax_new;              // std::max(a, b) = a < b ? b : a
            pgmin_new = PG < pgmin_new ? PG : pgmin_new;              // std::min(a, b) = b < a ? b : a
            if (fabs(PG) > 1.0e-12) {
                const double ao = (double)al;
                double t = __dadd_rn(ao, -(G / (double)q));
                t = t < 0.0 ? 0.0 : t;
                if (C < t) { t = C; ++ctr[4]; }
                const float an = (float)t;
                const double dd = __dmul_rn(__dadd_rn((double)an, -ao), (double)yi);
                k13d_update<STEPS>(a, row, lane, st, dd);
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

    // ---- the hand-off: w to the slot's (zero) w in HBM, every column marked once an instance exists.  A job the table failed stages
    //      nothing: its slot stays clean, and it runs again from its start.
    if (!table_end) {
        for (uint32_t s = 0; s < a.nst; ++s) {
            float4 v = zero4;
            if constexpr (STEPS != 0) {
#pragma unroll
                for (int u = 0; u < STEPS; ++u) if ((uint32_t)u == s) v = st.w[u];
            } else {
                v = wl[s * 64u + lane];
            }
            const uint32_t c0 = s * kTrainDenseStep + 4u * lane;
            if (c0 < a.d) w[c0] = v.x;
            if (c0 + 1u < a.d) w[c0 + 1u] = v.y;
            if (c0 + 2u < a.d) w[c0 + 2u] = v.z;
            if (c0 + 3u < a.d) w[c0 + 3u] = v.w;
        }
        if (n)
            for (uint32_t wd = lane; wd < a.dw; wd += 64u) touched[wd] = k13_word_mask(wd, a.d);
    }
    wave_sync_hbm();                                                   // lane 0's last swaps of index, w and the bitmap, before every lane reads them below
    if (!train_job_emit(a, job, label, lane, w, touched, cost, index, n, bw, table_end)) {
        if (lane == 0) a.redo[atomicAdd(a.n_redo, 1u)] = job;
        for (int k = 0; k < 7; ++k) ctr[k] = before[k];
    }
}

template <int STEPS> __global__ void __launch_bounds__(64) k13d_solve(K13DArgs a) {
    extern __shared__ float4 k13d_w[];                                 // STEPS == 0: 64 * a.nst float4
    const uint32_t lane = threadIdx.x, slot = blockIdx.x;
    unsigned long long ctr[7] = {0, 0, 0, 0, 0, 0, 0};
    for (;;) {                                                         // at most n_jobs + 1 turns
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(a.next, 1u);
        t = first_lane(t);
        if (t >= a.n_jobs) break;
        k13d_job<STEPS>(a, a.job_list ? a.job_list[t] : a.job0 + t, slot, lane, k13d_w, ctr);
    }
    if (lane == 0)
        for (int k = 0; k < 7; ++k)
            if (ctr[k]) atomicAdd(&a.counters[k], ctr[k]);
}

std::atomic<uint64_t> g_reg_jobs{0}, g_lds_jobs{0};

uint32_t lds_bytes(uint32_t cols) { return cols <= kTrainDenseRegCols ? 0u : (cols + kTrainDenseStep - 1) / kTrainDenseStep * kTrainDenseStep * 4u; }

}  // namespace

uint32_t train_dense_max_slots(uint32_t cols) {
    const uint32_t lds = lds_bytes(cols);
    if (!lds) return kTrainMaxSlots;
    int dev = 0, cus = 0;
    XRL_HIP(hipGetDevice(&dev));
    XRL_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    return (uint32_t)std::min<uint64_t>(kTrainMaxSlots, (uint64_t)std::max(cus, 1) * (kTrainDenseLdsPerCu / lds));
}

void train_dense_launch(const K13Args& base, const TrainDenseX& X, uint32_t blocks, bool first, hipStream_t s) {
    if (X.cols > kTrainDenseMaxCols) fail("K13D: " + std::to_string(X.cols) + " columns are more than " + std::to_string(kTrainDenseMaxCols));
    K13DArgs a{};
    static_cast<K13Args&>(a) = base;
    a.X = X.val; a.row_stride = X.row_stride;
    a.nst = (X.cols + kTrainDenseStep - 1) / kTrainDenseStep;
    a.vec = (reinterpret_cast<uintptr_t>(X.val) % 16 == 0 && X.row_stride % 4 == 0) ? 1 : 0;
    const uint32_t lds = lds_bytes(X.cols);
    switch (lds ? 0u : std::max(a.nst, 1u)) {
        case 1: hipLaunchKernelGGL(k13d_solve<1>, dim3(blocks), dim3(64), 0, s, a); break;
        case 2: hipLaunchKernelGGL(k13d_solve<2>, dim3(blocks), dim3(64), 0, s, a); break;
        case 3: hipLaunchKernelGGL(k13d_solve<3>, dim3(blocks), dim3(64), 0, s, a); break;
        case 4: hipLaunchKernelGGL(k13d_solve<4>, dim3(blocks), dim3(64), 0, s, a); break;
        default: hipLaunchKernelGGL(k13d_solve<0>, dim3(blocks), dim3(64), lds, s, a); break;
    }
    if (first) (lds ? g_lds_jobs : g_reg_jobs) += base.n_jobs;
}

void train_dense_forms(uint64_t (&out)[4]) {
    out[0] = kTrainDenseRegCols; out[1] = kTrainDenseMaxCols; out[2] = g_reg_jobs.load(); out[3] = g_lds_jobs.load();
}

}  // namespace xrl
