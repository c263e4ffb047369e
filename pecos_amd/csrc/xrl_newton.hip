// K16: ranker training with the reference's primal solver for the L2-loss SVC.  One (cluster, label) job is the Newton method of
// solve_l2r_l2_svc_primal (linear_solver.hpp:407-417): l2r_l2_svc_fun's fun / grad / Hv / get_diag_preconditioner / linesearch_and_update
// (:62-323) under NEWTON::newton / pcg / norm (utils/newton.hpp:98-273), over the instances init_worker lists, and its weights pass the
// emission of SVMJob::solve (both in xrl_train_job.h, shared with K13).  The rule is stated in include/xrl_abi.h.
//   k16_finite       a non-finite value stored in X
//   k16_solve        ONE WAVEFRONT OWNS ONE JOB AT A TIME and takes the next from a counter by an atomic add; no wavefront waits on another.
//                    Its slot of scratch: K13's index / cost / y / dense w [cols] / bitmap of touched features, and wx, tmp by row, I and
//                    what grad compacts by listed position, the ascending list of the touched features, and g, M, s, r, d, Hd, z by
//                    feature.  THE COMPRESSED FORM: a feature no instance of the job stores stays (+-)0 in every vector and 1 in M, so
//                    every vector-vector step walks the touched list only, 64 features a step, dots and norm as ONE chain each.
//                    Per instance the lanes gather and multiply a row's entries and add them as one chain in stored order; every lane
//                    computes the same fp64 scalars; the lanes apply a row's axpy in parallel (its ids are strictly ascending) and the
//                    instances go ONE AFTER ANOTHER, because rows share features.  Loop bounds: 1000 Newton iterations, max(d + (bias > 0),
//                    5) CG steps, 20 halvings, as in the reference.
#include "xrl_device.h"
#include "xrl_devprim.h"
#include "xrl_newton.h"
#include "xrl_train_job.h"

namespace xrl {

namespace {

constexpr const char* kWhat = "K16";

struct K16Args : TrainJobArgs {
    float* wx; float* tmp; uint32_t* I; float* tq; float* dots; uint32_t* tlist; float* vec;
    uint32_t n_jobs; uint32_t* next;
    unsigned long long* counters; uint32_t* bad_job;
};

enum { cNewton, cCg, cHv, cHalvings, cBefore, cGradient, cLine, cActred, cCap, cgDhd, cgQ, cgPositive, cgCap, cLaneRows, cWaveRows, cNonfinite, kCtr };
static_assert(kCtr == (int)kNewtonDeviceCounters, "the counters");

__global__ void __launch_bounds__(256) k16_finite(const float* __restrict__ val, uint64_t nnz, uint32_t* __restrict__ flag) {
    const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (x < nnz && (__float_as_uint(val[x]) & 0x7F800000u) == 0x7F800000u) atomicOr(flag, 1u);
}

__device__ __forceinline__ bool k16_finite_d(double v) { return (__double_as_longlong(v) & 0x7FF0000000000000ll) != 0x7FF0000000000000ll; }

// one job's view of its slot and the solver's state that outlives a step
struct K16Job {
    const K16Args& a;
    const uint32_t lane;
    uint32_t* index; float* cost; signed char* ysg; float* w; float* wx; float* tmp; uint32_t* I; float* tq; float* dots; const uint32_t* tl;
    float *g, *M, *s, *r, *dv, *Hd, *z;
    uint32_t n, nt, sizeI;
    bool has_b;
    float b, bg, bM, bs, br, bd, bHd, bz;
    double wTw;
    unsigned long long (&ctr)[kCtr];

    __device__ __forceinline__ float get_c(uint32_t i) const { return (float)__dmul_rn((double)cost[i], ysg[i] > 0 ? a.Cp : a.Cn); }

    // dots[p] <- u . x_{list[p]}, p < cnt: an fp32 chain from +0 in stored order; rows below kTrainWaveRow entries one per lane, longer ones by the wavefront
    __device__ void rows_dot(const float* u, const uint32_t* list, uint32_t cnt) {
        for (uint32_t s0 = 0; s0 < cnt; s0 += 64u) {
            const uint32_t p = s0 + lane;
            const bool have = p < cnt;
            uint64_t rb = 0, re = 0;
            if (have) row_span(a.x_ptr, list[p], a.x_nnz, rb, re);
            const bool wide = have && re - rb >= kTrainWaveRow;
            float acc = 0.0f;
            if (have && !wide)
                for (uint64_t j = rb; j < re; ++j) acc = __fadd_rn(acc, __fmul_rn(u[a.x_idx[j]], a.x_val[j]));
            unsigned long long wm = __ballot(wide);
            while (wm) {                                               // at most 64 turns
                const int l = __builtin_ctzll(wm);
                wm &= wm - 1;
                const uint64_t bb = __shfl(rb, l), ee = __shfl(re, l);
                float ws = 0.0f;
                for (uint64_t x0 = bb; x0 < ee; x0 += 64u) {
                    const uint64_t x = x0 + lane;
                    float pr = 0.0f;
                    if (x < ee) pr = __fmul_rn(u[a.x_idx[x]], a.x_val[x]);
                    ws = wave_chain(ws, pr, (uint32_t)min((uint64_t)64u, ee - x0));
                }
                if ((int)lane == l) acc = ws;
            }
            if (have) dots[p] = acc;
        }
        wave_sync_hbm();
    }

    // The rows of I one after another: per row every lane gets coef(p, i) -> (cd, cf) of its listed position p, row(cd, cf) runs once
    // (uniform), entry(cd, cf, f, x) once per stored entry, the lanes in parallel; a row's stores are visible before the next row reads.
    template <class Coef, class Row, class Entry> __device__ __forceinline__ void rows_serial(Coef coef, Row row, Entry entry) {
        for (uint32_t s0 = 0; s0 < sizeI; s0 += 64u) {
            const uint32_t p = s0 + lane;
            uint64_t rb = 0, re = 0;
            double cd = 0.0;
            float cf = 0.0f;
            if (p < sizeI) { const uint32_t i = I[p]; row_span(a.x_ptr, i, a.x_nnz, rb, re); coef(p, i, cd, cf); }
            const uint32_t m = min(64u, sizeI - s0);
            for (uint32_t l = 0; l < m; ++l) {
                const uint64_t bb = __shfl(rb, (int)l), ee = __shfl(re, (int)l);
                const double qd = __shfl(cd, (int)l);
                const float qf = __shfl(cf, (int)l);
                row(qd, qf);
                for (uint64_t x = bb + lane; x < ee; x += 64u) entry(qd, qf, a.x_idx[x], a.x_val[x]);
                wave_sync_hbm();
            }
        }
    }

    // u . v over the touched features: an fp32 chain from +0 in ascending feature order
    __device__ float dot(const float* u, const float* v) const {
        float acc = 0.0f;
        for (uint32_t t0 = 0; t0 < nt; t0 += 64u) {
            const uint32_t t = t0 + lane;
            float p = 0.0f;
            if (t < nt) { const uint32_t f = tl[t]; p = __fmul_rn(u[f], v[f]); }
            acc = wave_chain(acc, p, min(64u, nt - t0));
        }
        return acc;
    }

    // sum_i C_times_loss(i, wx[i] + alpha * tmp[i]) over index, an fp64 chain (with_step false: at wx itself)
    __device__ double loss(double alpha, bool with_step) const {
        double acc = 0.0;
        for (uint32_t s0 = 0; s0 < n; s0 += 64u) {
            const uint32_t sx = s0 + lane;
            double term = 0.0;
            if (sx < n) {
                const uint32_t i = index[sx];
                const double v = with_step ? __dadd_rn(__dmul_rn((double)tmp[i], alpha), (double)wx[i]) : (double)wx[i];
                const double dd = __dadd_rn(1.0, -__dmul_rn((double)ysg[i], v));
                if (dd > 0) term = __dmul_rn(__dmul_rn((double)get_c(i), dd), dd);
            }
            acc = wave_chain(acc, term, min(64u, n - s0));
        }
        return acc;
    }

    // grad: I and the compacted values, then g = w + 2 X_I' v.  The reference compacts INTO tmp, the array it has just written by row id:
    // an instance whose row id is below the count of active instances at its turn overwrites that compacted slot with its raw wx * y
    // (tmp[i] is stored before tmp[sizeI]).  Here the compacted values have an array of their own, tq, and exactly those overwrites are
    // applied to it, after the step's compacted stores: a slot is compacted once, before any turn that can overwrite it.
    __device__ void grad() {
        sizeI = 0;
        for (uint32_t s0 = 0; s0 < n; s0 += 64u) {
            const uint32_t sx = s0 + lane;
            const bool have = sx < n;
            uint32_t i = 0;
            float t = 0.0f, v = 0.0f;
            bool act = false;
            if (have) {
                i = index[sx];
                const float y = (float)ysg[i];
                t = __fmul_rn(wx[i], y);
                act = t < 1.0f;
                if (act) v = __fmul_rn(__fmul_rn(get_c(i), y), __fadd_rn(t, -1.0f));
            }
            const unsigned long long m = __ballot(act);
            const uint32_t before = sizeI + lanes_below(m);
            if (act) { tq[before] = v; I[before] = i; }
            wave_sync_hbm();
            if (have && i < before) tq[i] = t;
            sizeI += (uint32_t)__popcll(m);
            wave_sync_hbm();
        }
        for (uint32_t t = lane; t < nt; t += 64u) g[tl[t]] = 0.0f;
        bg = 0.0f;
        wave_sync_hbm();
        const double bias = a.bias;
        rows_serial([&](uint32_t p, uint32_t, double&, float& cf) { cf = tq[p]; },
                    [&](double, float cf) { if (has_b) bg = (float)__dadd_rn((double)bg, __dmul_rn(bias, (double)cf)); },
                    [&](double, float cf, uint32_t f, float x) { g[f] = __fadd_rn(g[f], __fmul_rn(cf, x)); });
        for (uint32_t t = lane; t < nt; t += 64u) { const uint32_t f = tl[t]; g[f] = __fadd_rn(w[f], __fmul_rn(2.0f, g[f])); }
        if (has_b) bg = __fadd_rn(b, __fmul_rn(2.0f, bg));
        wave_sync_hbm();
    }

    __device__ double norm() const {
        double acc = 0.0;
        for (uint32_t t0 = 0; t0 < nt; t0 += 64u) {
            const uint32_t t = t0 + lane;
            double p = 0.0;
            if (t < nt) { const double v = (double)g[tl[t]]; p = __dmul_rn(v, v); }
            acc = wave_chain(acc, p, min(64u, nt - t0));
        }
        return sqrt(__dadd_rn(acc, __dmul_rn((double)bg, (double)bg)));
    }

    // M = 0.99 + 0.01 * (1 + sum_I 2 c x^2)
    __device__ void preconditioner() {
        for (uint32_t t = lane; t < nt; t += 64u) M[tl[t]] = 1.0f;
        bM = 1.0f;
        wave_sync_hbm();
        const double b2 = __dmul_rn(__dmul_rn(a.bias, a.bias), 2.0);
        rows_serial([&](uint32_t, uint32_t i, double& cd, float& cf) { const float c = get_c(i); cd = (double)c; cf = __fmul_rn(2.0f, c); },
                    [&](double cd, float) { if (has_b) bM = (float)__dadd_rn((double)bM, __dmul_rn(b2, cd)); },
                    [&](double, float cf, uint32_t f, float x) { M[f] = __fadd_rn(M[f], __fmul_rn(__fmul_rn(x, x), cf)); });
        for (uint32_t t = lane; t < nt; t += 64u) { const uint32_t f = tl[t]; M[f] = (float)__dadd_rn(0.99, __dmul_rn(0.01, (double)M[f])); }
        bM = (float)__dadd_rn(0.99, __dmul_rn(0.01, (double)bM));
        wave_sync_hbm();
    }

    // Hd = d + 2 X_I' (c .* (X_I d))
    __device__ void hv() {
        ++ctr[cHv];
        rows_dot(dv, I, sizeI);
        for (uint32_t t = lane; t < nt; t += 64u) Hd[tl[t]] = 0.0f;
        bHd = 0.0f;
        wave_sync_hbm();
        const double bias = a.bias;
        rows_serial([&](uint32_t p, uint32_t i, double& cd, float&) {
                        double xts = (double)dots[p];
                        if (has_b) xts = __dadd_rn(xts, __dmul_rn(bias, (double)bd));
                        cd = __dmul_rn((double)get_c(i), xts);
                    },
                    [&](double cd, float) { if (has_b) bHd = (float)__dadd_rn((double)bHd, __dmul_rn(cd, bias)); },
                    [&](double cd, float, uint32_t f, float x) { Hd[f] = (float)__dadd_rn((double)Hd[f], __dmul_rn(cd, (double)x)); });
        for (uint32_t t = lane; t < nt; t += 64u) { const uint32_t f = tl[t]; Hd[f] = __fadd_rn(dv[f], __fmul_rn(2.0f, Hd[f])); }
        bHd = __fadd_rn(bd, __fmul_rn(2.0f, bHd));
        wave_sync_hbm();
    }

    // z = r / M, correctly rounded: the fp64 quotient of two fp32 values rounds to the fp32 quotient (53 >= 2 * 24 + 2)
    __device__ __forceinline__ static float div32(float x, float y) { return (float)((double)x / (double)y); }

    // false: a non-finite alpha or beta
    __device__ bool pcg(uint32_t max_cg) {
        for (uint32_t t = lane; t < nt; t += 64u) {
            const uint32_t f = tl[t];
            const float rr = -g[f], zz = div32(rr, M[f]);
            s[f] = 0.0f; r[f] = rr; z[f] = zz; dv[f] = zz;
        }
        bd = 0.0f; bHd = 0.0f; bz = 0.0f;
        if (has_b) { bs = 0.0f; br = -bg; bz = div32(br, bM); bd = bz; }
        wave_sync_hbm();
        double zTr = (double)dot(z, r);
        if (has_b) zTr = __dadd_rn(zTr, __dmul_rn((double)bz, (double)br));
        const double rt = sqrt(sqrt(zTr));
        const double cgtol = 0.5 < rt ? 0.5 : rt;
        double Q = 0.0;
        uint32_t it = 0;
        int how = cgCap;
        while (it < max_cg) {
            ++it;
            hv();
            double dHd = (double)dot(dv, Hd);
            if (has_b) dHd = __dadd_rn(dHd, __dmul_rn((double)bd, (double)bHd));
            if (dHd <= 1.0e-16) { how = cgDhd; break; }
            double alpha = zTr / dHd;
            if (!k16_finite_d(alpha)) { ctr[cCg] += it; return false; }
            const double nalpha = -alpha;
            for (uint32_t t = lane; t < nt; t += 64u) {
                const uint32_t f = tl[t];
                s[f] = (float)__dadd_rn((double)s[f], __dmul_rn(alpha, (double)dv[f]));
                r[f] = (float)__dadd_rn((double)r[f], __dmul_rn(nalpha, (double)Hd[f]));
            }
            if (has_b) {
                bs = (float)__dadd_rn((double)bs, __dmul_rn(alpha, (double)bd));
                br = (float)__dadd_rn((double)br, __dmul_rn(nalpha, (double)bHd));
            }
            wave_sync_hbm();
            double newQ = __dmul_rn(-0.5, (double)__fadd_rn(dot(s, r), -dot(s, g)));
            if (has_b) newQ = __dadd_rn(newQ, -__dmul_rn(0.5, (double)__fadd_rn(__fmul_rn(bs, br), -__fmul_rn(bs, bg))));
            const double Qdiff = __dadd_rn(newQ, -Q);
            if (newQ <= 0 && Qdiff <= 0) {
                if (__dmul_rn((double)it, Qdiff) >= __dmul_rn(cgtol, newQ)) { how = cgQ; break; }
            } else { how = cgPositive; break; }
            Q = newQ;
            for (uint32_t t = lane; t < nt; t += 64u) { const uint32_t f = tl[t]; z[f] = div32(r[f], M[f]); }
            if (has_b) bz = div32(br, bM);
            wave_sync_hbm();
            double znew = (double)dot(z, r);
            if (has_b) znew = __dadd_rn(znew, __dmul_rn((double)bz, (double)br));
            const double beta = znew / zTr;
            if (!k16_finite_d(beta)) { ctr[cCg] += it; return false; }
            const double bm1 = __dadd_rn(beta, -1.0);
            for (uint32_t t = lane; t < nt; t += 64u) {
                const uint32_t f = tl[t];
                const float d1 = (float)__dadd_rn((double)dv[f], __dmul_rn(bm1, (double)dv[f]));
                dv[f] = (float)__dadd_rn((double)d1, (double)z[f]);
            }
            if (has_b) { bd = (float)__dmul_rn((double)bd, beta); bd = (float)__dadd_rn((double)bd, (double)bz); }
            wave_sync_hbm();
            zTr = znew;
        }
        ctr[cCg] += it;
        ++ctr[how];
        return true;
    }

    // -> the step taken (0: none); f <- the objective there
    __device__ double linesearch(double& f) {
        const double fold = f;
        rows_dot(s, index, n);                                         // Xv(s, tmp, bs)
        for (uint32_t sx = lane; sx < n; sx += 64u) {                  // (a row id listed twice gets the same value twice)
            const float rd = dots[sx];
            tmp[index[sx]] = has_b ? (float)__dadd_rn((double)rd, __dmul_rn(a.bias, (double)bs)) : rd;
        }
        wave_sync_hbm();
        double sTs = (double)dot(s, s), wTs = (double)dot(s, w), gTs = (double)dot(s, g);
        if (has_b) {
            sTs = __dadd_rn(sTs, __dmul_rn((double)bs, (double)bs));
            wTs = __dadd_rn(wTs, __dmul_rn((double)bs, (double)b));
            gTs = __dadd_rn(gTs, __dmul_rn((double)bs, (double)bg));
        }
        double alpha = 1.0;
        uint32_t k = 0;
        for (; k < kNewtonMaxHalvings; ++k) {
            const double ls = loss(alpha, true);
            f = __dadd_rn(__dadd_rn(ls, __dadd_rn(__dmul_rn(__dmul_rn(alpha, alpha), sTs), wTw) / 2.0), __dmul_rn(alpha, wTs));
            if (__dadd_rn(f, -fold) <= __dmul_rn(__dmul_rn(0.01, alpha), gTs)) break;
            alpha = __dmul_rn(alpha, 0.5);
        }
        ctr[cHalvings] += k;
        if (k >= kNewtonMaxHalvings) { f = fold; return 0.0; }
        // wx[i] += alpha * tmp[i] once per listed position, in listed order: inside a step of 64 the first lane that holds a row id applies
        // the update as often as the step lists it; the steps follow one another
        for (uint32_t s0 = 0; s0 < n; s0 += 64u) {
            const uint32_t sx = s0 + lane;
            const bool have = sx < n;
            const uint32_t i = have ? index[sx] : 0u;
            const uint32_t m = min(64u, n - s0);
            uint32_t times = 0;
            bool first = true;
            for (uint32_t l = 0; l < m; ++l) {
                const uint32_t il = (uint32_t)__builtin_amdgcn_readlane((int)i, (int)l);
                if (have && il == i) { if (l < lane) first = false; ++times; }
            }
            if (have && first) {
                float v = wx[i];
                const double st = __dmul_rn(alpha, (double)tmp[i]);
                for (uint32_t q = 0; q < times; ++q) v = (float)__dadd_rn((double)v, st);
                wx[i] = v;
            }
            wave_sync_hbm();
        }
        for (uint32_t t = lane; t < nt; t += 64u) { const uint32_t f2 = tl[t]; w[f2] = (float)__dadd_rn((double)w[f2], __dmul_rn(alpha, (double)s[f2])); }
        b = (float)__dadd_rn((double)b, __dmul_rn(alpha, (double)bs));
        wTw = __dadd_rn(wTw, __dadd_rn(__dmul_rn(__dmul_rn(alpha, alpha), sTs), __dmul_rn(__dmul_rn(2.0, alpha), wTs)));
        wave_sync_hbm();
        return alpha;
    }
};

__device__ void k16_job(const K16Args& a, uint32_t job, uint32_t slot, uint32_t lane, unsigned long long (&ctr)[kCtr]) {
    float* vec = a.vec + (uint64_t)slot * 7u * a.d;
    K16Job J{a, lane,
             a.index + (uint64_t)slot * a.index_cap, a.cost + (uint64_t)slot * a.N, a.ysg + (uint64_t)slot * a.N, a.w + (uint64_t)slot * a.d,
             a.wx + (uint64_t)slot * a.N, a.tmp + (uint64_t)slot * a.N, a.I + (uint64_t)slot * a.index_cap, a.tq + (uint64_t)slot * a.index_cap,
             a.dots + (uint64_t)slot * a.index_cap, a.tlist + (uint64_t)slot * a.d,
             vec, vec + a.d, vec + 2ull * a.d, vec + 3ull * a.d, vec + 4ull * a.d, vec + 5ull * a.d, vec + 6ull * a.d,
             0u, 0u, 0u, a.bias > 0, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0, ctr};
    uint32_t* touched = a.touched + (uint64_t)slot * a.dw;
    uint32_t* tlw = a.tlist + (uint64_t)slot * a.d;

    uint32_t label = job, code = 0;
    if (a.c_ptr) { label = a.c_idx[job]; code = segment_of(a.c_ptr, a.K, (uint64_t)job); }
    const uint32_t n = train_job_setup(a, label, code, lane, J.index, J.cost, J.ysg);
    J.n = n;

    // ---- wx = X w = +0 (w = 0 and X is finite), and the features the job touches
    for (uint32_t s0 = 0; s0 < n; s0 += 64u) {
        const uint32_t sx = s0 + lane;
        const bool have = sx < n;
        uint64_t rb = 0, re = 0;
        if (have) { const uint32_t i = J.index[sx]; row_span(a.x_ptr, i, a.x_nnz, rb, re); J.wx[i] = 0.0f; }
        const bool wide = have && re - rb >= kTrainWaveRow;
        if (have && !wide)
            for (uint64_t j = rb; j < re; ++j) { const uint32_t f = a.x_idx[j]; atomicOr(&touched[f >> 5], 1u << (f & 31u)); }
        unsigned long long wm = __ballot(wide);
        ctr[cLaneRows] += (unsigned long long)__popcll(__ballot(have && !wide));
        ctr[cWaveRows] += (unsigned long long)__popcll(wm);
        while (wm) {                                                   // at most 64 turns
            const int l = __builtin_ctzll(wm);
            wm &= wm - 1;
            const uint64_t bb = __shfl(rb, l), ee = __shfl(re, l);
            for (uint64_t x = bb + lane; x < ee; x += 64u) { const uint32_t f = a.x_idx[x]; atomicOr(&touched[f >> 5], 1u << (f & 31u)); }
        }
    }
    wave_sync_hbm();
    uint32_t nt = 0;
    for (uint32_t w0 = 0; w0 < a.dw; w0 += 64u) {
        const uint32_t wd = w0 + lane;
        const uint32_t bits = wd < a.dw ? touched[wd] : 0u;
        const uint32_t mine = (uint32_t)__popc(bits);
        uint32_t incl = mine;
        for (int dlt = 1; dlt < 64; dlt <<= 1) { const uint32_t t = __shfl_up(incl, dlt, 64); if ((int)lane >= dlt) incl += t; }
        uint32_t at = nt + incl - mine;
        for (uint32_t bb = bits; bb; bb &= bb - 1u) tlw[at++] = wd * 32u + (uint32_t)__builtin_ctz(bb);
        nt += (uint32_t)__shfl(incl, 63);
    }
    J.nt = nt;
    wave_sync_hbm();

    // ---- newton: w0 == w == 0, so the two evaluations at the start are one
    double f = J.loss(0.0, false);                                     // + 0.5 * wTw = +0
    J.grad();
    const double gnorm0 = J.norm();
    double gnorm = gnorm0;
    const uint64_t cap64 = (uint64_t)a.d + (J.has_b ? 1u : 0u);
    const uint32_t max_cg = (uint32_t)(cap64 < 5u ? 5u : (cap64 > 0x7FFFFFFFull ? 0x7FFFFFFFull : cap64));
    bool search = !(gnorm <= __dmul_rn(a.eps, gnorm0)), ended = false, finite = true;
    if (!search) { ++ctr[cBefore]; ended = true; }
    uint32_t iter = 1;
    while (iter <= kNewtonMaxIter && search) {
        ++ctr[cNewton];
        J.preconditioner();
        if (!J.pcg(max_cg)) { finite = false; break; }
        const double fold = f;
        const double step = J.linesearch(f);
        if (step == 0) { ++ctr[cLine]; ended = true; break; }
        J.grad();
        gnorm = J.norm();
        if (gnorm <= __dmul_rn(a.eps, gnorm0)) { ++ctr[cGradient]; ended = true; break; }
        if (f < -1.0e32) { ++ctr[cActred]; ended = true; break; }      // (a sum of squares: not met; counted with the next)
        if (fabs(__dadd_rn(fold, -f)) <= __dmul_rn(1.0e-12, fabs(f))) { ++ctr[cActred]; ended = true; break; }
        ++iter;
    }
    if (finite && !ended) ++ctr[cCap];
    if (!finite) {
        ++ctr[cNonfinite];
        if (lane == 0) atomicMin(a.bad_job, job);
    }
    wave_sync_hbm();
    train_job_emit(a, job, label, lane, J.w, touched, J.cost, J.index, n, J.b, false);
}

__global__ void __launch_bounds__(64) k16_solve(K16Args a) {
    const uint32_t lane = threadIdx.x, slot = blockIdx.x;
    unsigned long long ctr[kCtr];
    for (int k = 0; k < kCtr; ++k) ctr[k] = 0;
    for (;;) {                                                         // at most n_jobs + 1 turns
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(a.next, 1u);
        t = first_lane(t);
        if (t >= a.n_jobs) break;
        k16_job(a, a.job0 + t, slot, lane, ctr);
    }
    if (lane == 0)
        for (int k = 0; k < kCtr; ++k)
            if (ctr[k]) atomicAdd(&a.counters[k], ctr[k]);
}

}  // namespace

uint64_t newton_slot_bytes(uint32_t N, uint32_t d, uint32_t index_cap) { return (uint64_t)N * 8 + (uint64_t)index_cap * 12 + (uint64_t)d * 4 * 8; }

void newton_reserve(NewtonScratch& sc, uint32_t slots, uint32_t N, uint32_t d, uint32_t index_cap, hipStream_t s) {
    sc.N = N; sc.d = d; sc.index_cap = index_cap;
    sc.wx.reserve((size_t)slots * N * 4); sc.tmp.reserve((size_t)slots * N * 4);
    sc.I.reserve((size_t)slots * index_cap * 4); sc.tq.reserve((size_t)slots * index_cap * 4); sc.dots.reserve((size_t)slots * index_cap * 4);
    sc.tlist.reserve((size_t)slots * d * 4); sc.vec.reserve((size_t)slots * d * 4 * 7);
    sc.ctr.reserve(kNewtonDeviceCounters * 8); sc.bad.reserve(4);
    XRL_HIP(hipMemsetAsync(sc.ctr.p, 0, kNewtonDeviceCounters * 8, s));
    XRL_HIP(hipMemsetAsync(sc.bad.p, 0xFF, 4, s));
}

void newton_launch(const TrainJobArgs& base, const NewtonScratch& sc, uint32_t n_jobs, uint32_t* next, uint32_t blocks, hipStream_t s) {
    K16Args a{};
    static_cast<TrainJobArgs&>(a) = base;
    a.wx = sc.wx.as<float>(); a.tmp = sc.tmp.as<float>(); a.I = sc.I.as<uint32_t>(); a.tq = sc.tq.as<float>(); a.dots = sc.dots.as<float>();
    a.tlist = sc.tlist.as<uint32_t>(); a.vec = sc.vec.as<float>();
    a.n_jobs = n_jobs; a.next = next; a.counters = sc.ctr.as<unsigned long long>(); a.bad_job = sc.bad.as<uint32_t>();
    hipLaunchKernelGGL(k16_solve, dim3(blocks), dim3(64), 0, s, a);
    XRL_LAUNCH_CHECK();
}

uint32_t newton_bad_job(const NewtonScratch& sc, hipStream_t s) {
    uint32_t j = 0;
    XRL_HIP(hipMemcpyAsync(&j, sc.bad.p, 4, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    return j;
}

void newton_read_counters(const NewtonScratch& sc, NewtonCounters& c, hipStream_t s) {
    uint64_t v[kNewtonDeviceCounters];
    XRL_HIP(hipMemcpyAsync(v, sc.ctr.p, sizeof(v), hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    c.newton_iters = v[cNewton]; c.cg_iters = v[cCg]; c.hv_calls = v[cHv]; c.halvings = v[cHalvings];
    c.end_before_first = v[cBefore]; c.end_gradient = v[cGradient]; c.end_linesearch = v[cLine]; c.end_actred = v[cActred]; c.end_cap = v[cCap];
    c.cg_dhd = v[cgDhd]; c.cg_q = v[cgQ]; c.cg_positive = v[cgPositive]; c.cg_cap = v[cgCap];
    c.lane_rows = v[cLaneRows]; c.wave_rows = v[cWaveRows]; c.nonfinite_jobs = v[cNonfinite];
}

void newton_check_finite(const std::string& what, const QueriesDev& X, hipStream_t s) {
    if (!X.nnz) return;
    DevBuf flag;
    flag.reserve(4);
    XRL_HIP(hipMemsetAsync(flag.p, 0, 4, s));
    hipLaunchKernelGGL(k16_finite, dim3(blocks_of(X.nnz, 256, kWhat)), dim3(256), 0, s, X.val, X.nnz, flag.as<uint32_t>());
    XRL_LAUNCH_CHECK();
    uint32_t f = 0;
    XRL_HIP(hipMemcpyAsync(&f, flag.p, 4, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    if (f) fail(what + "X stores a value that is not finite (a NaN or an infinity); the primal solver's features that no instance stores would become NaNs, which this form does not cover");
}

void check_newton_params(const std::string& what, const TrainParams& p) {
    if (p.solver_type == kSolverL2LossDual || p.solver_type == kSolverL1LossDual)
        fail(what + "solver " + (p.solver_type == kSolverL2LossDual ? "L2R_L2LOSS_SVC_DUAL" : "L2R_L1LOSS_SVC_DUAL") +
             " is served by the entry point without `newton` in its name (xrl_single_layer_train_{csr,drm}_f32, xrl_train_layer_device)");
    if (p.solver_type == 7)
        fail(what + "solver L2R_LR_DUAL is not served on the device: its inner Newton steps call log in fp64, and the device's log is not the host library's, so its weights could not be the reference's bit for bit");
    if (p.solver_type != kSolverL2LossPrimal)
        fail(what + "unknown solver_type " + std::to_string(p.solver_type) + " (2 = L2R_L2LOSS_SVC_PRIMAL)");
}

}  // namespace xrl
