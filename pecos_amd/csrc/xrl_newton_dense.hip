// K16D: the primal L2-loss SVC over a dense row-major X in HBM -- K16's jobs and solver (xrl_newton.hip: one job at a time per owner from
// the atomic counter, xrl_train_job.h's set-up and emission, the fp64 scalars every lane computes, the Newton / pcg / line-search control
// flow, grad's tmp aliasing, the non-finite flags) with a data path of its own for rows that store every column.  The rule is R16D in
// include/xrl_abi.h: K16's on the CSR of all rows * cols entries, zeros included; the touched features are 0 .. cols - 1.
//   Ownership.  ONE WAVEFRONT OWNS ONE JOB, K16's launch shape: a layer has jobs by the thousand, so the device fills with independent
//     jobs and a job needs neither a barrier nor a broadcast of its scalars; what bounds the wavefronts on a CU is the LDS a job keeps.
//   Row passes (X v: fun's wx = +0 needs none; Hv's X_I d, the line search's X s).  The chains of different instances are independent, so
//     64 listed instances go at once: lane i continues instance i's fp32 chain, in column order, in one register across the panels.  A
//     panel is 32 columns: the wavefront loads it as 32 row segments per half (lanes 0 .. 31 one row, 32 .. 63 the next: 128 contiguous
//     bytes each, rows gathered by the job's list) into 32 registers, stores them to an LDS tile at a pitch of 33 floats -- lane i then reads
//     tile[i][c], 64 distinct banks -- next to v's panel, which every lane reads from one address.  The next panel's loads are issued
//     before the current panel's chain and land under it.  A tail of fewer than 64 instances leaves lanes idle.
//   Column passes (X' u and the diagonal: grad's g, Hv's X_I' (c .* xTs), the preconditioner's M).  A feature's value is one chain over I's
//     order.  Per 256-column step lane l owns columns 256 s + 4 l .. + 3 (k13d_load: one float4 where rows are 16-byte aligned), keeps
//     the four running values in registers while the instances go by, eight rows' loads in flight ahead of the serial adds; a row's
//     factor is computed by the lane of its listed position and read by all.  No atomics, no inter-lane traffic, no index.
//   The by-feature vectors w, g, M, s, r, d, Hd, z live in LDS behind the tile up to kNewtonDenseLdsCols columns (k16d_solve<true>; w is
//     handed to the slot's w for the emission), above in the slot's scratch as K16 keeps them (k16d_solve<false>).  Vector-vector steps
//     are K16's over 0 .. cols - 1 without a list: ONE chain each through wave_chain.
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "xrl_device.h"
#include "xrl_devprim.h"
#include "xrl_newton.h"
#include "xrl_newton_job.h"
#include "xrl_train_job.h"

namespace xrl {

namespace {

constexpr const char* kWhat = "K16D";
constexpr uint32_t kPanel = kNewtonDensePanel, kPitch = kNewtonDensePitch;
constexpr uint32_t kAhead = 8;                                         // rows whose loads are in flight in a column pass

struct K16DArgs : K16Args {
    const float* X; uint64_t row_stride;
    int aligned;                                                         // every row starts 16-byte aligned
};

__global__ void __launch_bounds__(256) k16d_finite(const float* __restrict__ X, uint64_t n, uint32_t cols, uint64_t row_stride, uint32_t* __restrict__ flag) {
    const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (x < n && (__float_as_uint(X[x / cols * row_stride + x % cols]) & 0x7F800000u) == 0x7F800000u) atomicOr(flag, 1u);
}

__device__ __forceinline__ double lane_f64(double v, uint32_t l) {     // l is uniform
    const long long b = __double_as_longlong(v);
    return __longlong_as_double((long long)(((unsigned long long)lane_u32((uint32_t)((unsigned long long)b >> 32), l) << 32) | lane_u32((uint32_t)b, l)));
}

typedef __attribute__((address_space(3))) float lds_float;

// one job's view of its slot and of the workgroup's LDS, and the solver's state that outlives a step.  LDS: the by-feature vectors are in
// the workgroup's LDS (V is an LDS pointer, so every access is a DS instruction), else in the slot's scratch.
template <bool LDS> struct K16DJob {
    typedef typename std::conditional<LDS, lds_float, float>::type* V;
    const K16DArgs& a;
    const uint32_t lane, d;
    uint32_t* index; float* cost; signed char* ysg; float* wx; float* tmp; uint32_t* I; float* tq; float* dots;
    lds_float* tile; lds_float* vp;
    V w, g, M, s, r, dv, Hd, z;
    uint32_t n, sizeI;
    bool has_b;
    float b, bg, bM, bs, br, bd, bHd, bz;
    double wTw;
    unsigned long long (&ctr)[kCtr];

    __device__ __forceinline__ float get_c(uint32_t i) const { return (float)__dmul_rn((double)cost[i], ysg[i] > 0 ? a.Cp : a.Cn); }

    // dots[p] <- u . x_{list[p]}, p < cnt: an fp32 chain from +0 over columns 0 .. d - 1, 64 listed rows a tile
    __device__ __forceinline__ void rows_dot(const V u, const uint32_t* list, uint32_t cnt) {
        const uint32_t half = lane >> 5, cl = lane & 31u;
        for (uint32_t s0 = 0; s0 < cnt; s0 += 64u) {
            const uint32_t m = min(64u, cnt - s0);
            const uint32_t rid = lane < m ? list[s0 + lane] : 0u;
            float xr[kPanel], vr = 0.0f;
            auto fetch = [&](uint32_t c0) {                            // the panel at c0: row 2 k + half, column c0 + cl; past the tile or the row: +0, not loaded
                const uint32_t c = c0 + cl;
                const bool in = c < d;
                vr = in ? u[c] : 0.0f;
#pragma unroll
                for (uint32_t k = 0; k < kPanel; ++k) {
                    const uint32_t r0 = lane_u32(rid, 2u * k), r1 = lane_u32(rid, 2u * k + 1u);
                    xr[k] = (in && 2u * k + half < m) ? a.X[(uint64_t)(half ? r1 : r0) * a.row_stride + c] : 0.0f;
                }
            };
            fetch(0u);
            float acc = 0.0f;
            const lds_float* mine = tile + lane * kPitch;
            for (uint32_t c0 = 0; c0 < d; c0 += kPanel) {
#pragma unroll
                for (uint32_t k = 0; k < kPanel; ++k) tile[(2u * k + half) * kPitch + cl] = xr[k];
                if (lane < kPanel) vp[lane] = vr;
                wave_sync_hbm();
                if (c0 + kPanel < d) fetch(c0 + kPanel);               // in flight under the chain
                if (d - c0 >= kPanel) {
#pragma unroll
                    for (uint32_t c = 0; c < kPanel; ++c) acc = __fadd_rn(acc, __fmul_rn(vp[c], mine[c]));
                } else {
                    for (uint32_t c = 0; c < d - c0; ++c) acc = __fadd_rn(acc, __fmul_rn(vp[c], mine[c]));
                }
                wave_sync_hbm();                                       // every lane has read the tile before the next panel is stored
            }
            if (lane < m) dots[s0 + lane] = acc;
        }
        wave_sync_hbm();
    }

    // The rows of I one after another, a 256-column step at a time: the lane of listed position p computes coef(p, i) -> (cd, cf); per
    // row, row(cd, cf) runs once (in the first step), entry(acc, cd, cf, x) once per step on the lane's four columns, whose running
    // values start at `init` and go to done(c0, acc) after the last row.
    template <class Coef, class Row, class Entry, class Done> __device__ __forceinline__ void cols_serial(float init, Coef coef, Row row, Entry entry, Done done) {
        for (uint32_t st = 0; st == 0 || st * 256u < d; ++st) {        // (no column: the rows' bias parts still go by)
            const uint32_t c0 = st * 256u + 4u * lane;
            float4 acc = make_float4(init, init, init, init);
            for (uint32_t s0 = 0; s0 < sizeI; s0 += 64u) {
                const uint32_t p = s0 + lane;
                uint32_t rid = 0;
                double cd = 0.0;
                float cf = 0.0f;
                if (p < sizeI) { rid = I[p]; coef(p, rid, cd, cf); }
                const uint32_t m = min(64u, sizeI - s0);
                for (uint32_t l0 = 0; l0 < m; l0 += kAhead) {
                    float4 x[kAhead];                                  // (past the last row: the last row again, not used)
#pragma unroll
                    for (uint32_t q = 0; q < kAhead; ++q) x[q] = k13d_load(a.X + (uint64_t)lane_u32(rid, min(l0 + q, m - 1u)) * a.row_stride, c0, d, a.aligned);
#pragma unroll
                    for (uint32_t q = 0; q < kAhead; ++q)
                        if (l0 + q < m) {
                            const double qd = lane_f64(cd, l0 + q);
                            const float qf = lane_f32(cf, l0 + q);
                            if (st == 0) row(qd, qf);
                            entry(acc, qd, qf, x[q]);
                        }
                }
            }
            done(c0, acc);
        }
        wave_sync_hbm();
    }

    // the lane's four values of a step into a by-feature vector
    template <class F> __device__ __forceinline__ void put4(V v, uint32_t c0, const float4& t, F f) const {
        if (c0 < d) v[c0] = f(c0, t.x);
        if (c0 + 1u < d) v[c0 + 1u] = f(c0 + 1u, t.y);
        if (c0 + 2u < d) v[c0 + 2u] = f(c0 + 2u, t.z);
        if (c0 + 3u < d) v[c0 + 3u] = f(c0 + 3u, t.w);
    }

    // u . v: an fp32 chain from +0 in ascending feature order
    __device__ __forceinline__ float dot(const V u, const V v) const {
        float acc = 0.0f;
        for (uint32_t t0 = 0; t0 < d; t0 += 64u) {
            const uint32_t t = t0 + lane;
            const float p = t < d ? __fmul_rn(u[t], v[t]) : 0.0f;
            acc = wave_chain(acc, p, min(64u, d - t0));
        }
        return acc;
    }

    // sum_i C_times_loss(i, wx[i] + alpha * tmp[i]) over index, an fp64 chain (with_step false: at wx itself)
    __device__ __forceinline__ double loss(double alpha, bool with_step) const {
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

    // grad: I and the compacted values with the reference's overwrites (see K16Job::grad), then g = w + 2 X_I' v
    __device__ __forceinline__ void grad() {
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
        bg = 0.0f;
        const double bias = a.bias;
        cols_serial(0.0f, [&](uint32_t p, uint32_t, double&, float& cf) { cf = tq[p]; },
                    [&](double, float cf) { if (has_b) bg = (float)__dadd_rn((double)bg, __dmul_rn(bias, (double)cf)); },
                    [&](float4& acc, double, float cf, const float4& x) {
                        acc.x = __fadd_rn(acc.x, __fmul_rn(cf, x.x)); acc.y = __fadd_rn(acc.y, __fmul_rn(cf, x.y));
                        acc.z = __fadd_rn(acc.z, __fmul_rn(cf, x.z)); acc.w = __fadd_rn(acc.w, __fmul_rn(cf, x.w));
                    },
                    [&](uint32_t c0, const float4& acc) { put4(g, c0, acc, [&](uint32_t f, float t) { return __fadd_rn(w[f], __fmul_rn(2.0f, t)); }); });
        if (has_b) bg = __fadd_rn(b, __fmul_rn(2.0f, bg));
    }

    __device__ __forceinline__ double norm() const {
        double acc = 0.0;
        for (uint32_t t0 = 0; t0 < d; t0 += 64u) {
            const uint32_t t = t0 + lane;
            double p = 0.0;
            if (t < d) { const double v = (double)g[t]; p = __dmul_rn(v, v); }
            acc = wave_chain(acc, p, min(64u, d - t0));
        }
        return sqrt(__dadd_rn(acc, __dmul_rn((double)bg, (double)bg)));
    }

    // M = 0.99 + 0.01 * (1 + sum_I 2 c x^2)
    __device__ __forceinline__ void preconditioner() {
        bM = 1.0f;
        const double b2 = __dmul_rn(__dmul_rn(a.bias, a.bias), 2.0);
        cols_serial(1.0f, [&](uint32_t, uint32_t i, double& cd, float& cf) { const float c = get_c(i); cd = (double)c; cf = __fmul_rn(2.0f, c); },
                    [&](double cd, float) { if (has_b) bM = (float)__dadd_rn((double)bM, __dmul_rn(b2, cd)); },
                    [&](float4& acc, double, float cf, const float4& x) {
                        acc.x = __fadd_rn(acc.x, __fmul_rn(__fmul_rn(x.x, x.x), cf)); acc.y = __fadd_rn(acc.y, __fmul_rn(__fmul_rn(x.y, x.y), cf));
                        acc.z = __fadd_rn(acc.z, __fmul_rn(__fmul_rn(x.z, x.z), cf)); acc.w = __fadd_rn(acc.w, __fmul_rn(__fmul_rn(x.w, x.w), cf));
                    },
                    [&](uint32_t c0, const float4& acc) { put4(M, c0, acc, [&](uint32_t, float t) { return (float)__dadd_rn(0.99, __dmul_rn(0.01, (double)t)); }); });
        bM = (float)__dadd_rn(0.99, __dmul_rn(0.01, (double)bM));
    }

    // Hd = d + 2 X_I' (c .* (X_I d))
    __device__ __forceinline__ void hv() {
        ++ctr[cHv];
        rows_dot(dv, I, sizeI);
        bHd = 0.0f;
        const double bias = a.bias;
        cols_serial(0.0f,
                    [&](uint32_t p, uint32_t i, double& cd, float&) {
                        double xts = (double)dots[p];
                        if (has_b) xts = __dadd_rn(xts, __dmul_rn(bias, (double)bd));
                        cd = __dmul_rn((double)get_c(i), xts);
                    },
                    [&](double cd, float) { if (has_b) bHd = (float)__dadd_rn((double)bHd, __dmul_rn(cd, bias)); },
                    [&](float4& acc, double cd, float, const float4& x) {
                        acc.x = (float)__dadd_rn((double)acc.x, __dmul_rn(cd, (double)x.x)); acc.y = (float)__dadd_rn((double)acc.y, __dmul_rn(cd, (double)x.y));
                        acc.z = (float)__dadd_rn((double)acc.z, __dmul_rn(cd, (double)x.z)); acc.w = (float)__dadd_rn((double)acc.w, __dmul_rn(cd, (double)x.w));
                    },
                    [&](uint32_t c0, const float4& acc) { put4(Hd, c0, acc, [&](uint32_t f, float t) { return __fadd_rn(dv[f], __fmul_rn(2.0f, t)); }); });
        bHd = __fadd_rn(bd, __fmul_rn(2.0f, bHd));
    }

    // z = r / M, correctly rounded: the fp64 quotient of two fp32 values rounds to the fp32 quotient (53 >= 2 * 24 + 2)
    __device__ __forceinline__ static float div32(float x, float y) { return (float)((double)x / (double)y); }

    // false: a non-finite alpha or beta
    __device__ __forceinline__ bool pcg(uint32_t max_cg) {
        for (uint32_t f = lane; f < d; f += 64u) {
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
            for (uint32_t f = lane; f < d; f += 64u) {
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
            for (uint32_t f = lane; f < d; f += 64u) z[f] = div32(r[f], M[f]);
            if (has_b) bz = div32(br, bM);
            wave_sync_hbm();
            double znew = (double)dot(z, r);
            if (has_b) znew = __dadd_rn(znew, __dmul_rn((double)bz, (double)br));
            const double beta = znew / zTr;
            if (!k16_finite_d(beta)) { ctr[cCg] += it; return false; }
            const double bm1 = __dadd_rn(beta, -1.0);
            for (uint32_t f = lane; f < d; f += 64u) {
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
    __device__ __forceinline__ double linesearch(double& f) {
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
        // wx[i] += alpha * tmp[i] once per listed position, in listed order (see K16Job::linesearch)
        for (uint32_t s0 = 0; s0 < n; s0 += 64u) {
            const uint32_t sx = s0 + lane;
            const bool have = sx < n;
            const uint32_t i = have ? index[sx] : 0u;
            const uint32_t m = min(64u, n - s0);
            uint32_t times = 0;
            bool first = true;
            for (uint32_t l = 0; l < m; ++l) {
                const uint32_t il = lane_u32(i, l);
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
        for (uint32_t f2 = lane; f2 < d; f2 += 64u) w[f2] = (float)__dadd_rn((double)w[f2], __dmul_rn(alpha, (double)s[f2]));
        b = (float)__dadd_rn((double)b, __dmul_rn(alpha, (double)bs));
        wTw = __dadd_rn(wTw, __dadd_rn(__dmul_rn(__dmul_rn(alpha, alpha), sTs), __dmul_rn(__dmul_rn(2.0, alpha), wTs)));
        wave_sync_hbm();
        return alpha;
    }
};

// lds: the workgroup's LDS behind the tile and v's panel holds the eight vectors, d floats each
template <bool LDS> __device__ __forceinline__ void k16d_job(const K16DArgs& a, uint32_t job, uint32_t slot, uint32_t lane, lds_float* lds, unsigned long long (&ctr)[kCtr]) {
    const uint32_t d = a.d;
    float* w_slot = a.w + (uint64_t)slot * d;
    typedef typename K16DJob<LDS>::V V;
    V w0, g0;                                                          // LDS: w, then g ..; scratch: the slot's w, and g .. in the slot's vec
    if constexpr (LDS) { w0 = lds + kNewtonDenseTileFloats; g0 = w0 + d; }
    else { w0 = w_slot; g0 = a.vec + (uint64_t)slot * 7u * d; }
    K16DJob<LDS> J{a, lane, d,
              a.index + (uint64_t)slot * a.index_cap, a.cost + (uint64_t)slot * a.N, a.ysg + (uint64_t)slot * a.N,
              a.wx + (uint64_t)slot * a.N, a.tmp + (uint64_t)slot * a.N, a.I + (uint64_t)slot * a.index_cap, a.tq + (uint64_t)slot * a.index_cap,
              a.dots + (uint64_t)slot * a.index_cap, lds, lds + 64u * kPitch,
              w0, g0, g0 + d, g0 + 2u * d, g0 + 3u * d, g0 + 4u * d, g0 + 5u * d, g0 + 6u * d,
              0u, 0u, a.bias > 0, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0, ctr};
    uint32_t* touched = a.touched + (uint64_t)slot * a.dw;

    uint32_t label = job, code = 0;
    if (a.c_ptr) { label = a.c_idx[job]; code = segment_of(a.c_ptr, a.K, (uint64_t)job); }
    const uint32_t n = train_job_setup(a, label, code, lane, J.index, J.cost, J.ysg);
    J.n = n;

    // ---- wx = X w = +0 (w = 0 and X is finite); every listed row stores d entries
    for (uint32_t sx = lane; sx < n; sx += 64u) J.wx[J.index[sx]] = 0.0f;
    if (LDS)
        for (uint32_t f = lane; f < d; f += 64u) J.w[f] = 0.0f;       // (the slot's w is zero between jobs)
    ctr[d >= kTrainWaveRow ? cWaveRows : cLaneRows] += n;
    wave_sync_hbm();

    // ---- newton: w0 == w == 0, so the two evaluations at the start are one
    double f = J.loss(0.0, false);                                     // + 0.5 * wTw = +0
    J.grad();
    const double gnorm0 = J.norm();
    double gnorm = gnorm0;
    const uint32_t max_cg = max(d + (J.has_b ? 1u : 0u), 5u);
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

    // ---- the hand-off: w to the slot's (zero) w in HBM, every column marked once an instance exists
    if (LDS)
        for (uint32_t f2 = lane; f2 < d; f2 += 64u) w_slot[f2] = J.w[f2];
    if (n)
        for (uint32_t wd = lane; wd < a.dw; wd += 64u) touched[wd] = k13_word_mask(wd, d);
    wave_sync_hbm();
    train_job_emit(a, job, label, lane, w_slot, touched, J.cost, J.index, n, J.b, false);
}

template <bool LDS> __global__ void __launch_bounds__(64) k16d_solve(K16DArgs a) {
    extern __shared__ float k16d_lds[];                                // the tile, v's panel, and (LDS) 8 * a.d floats
    const uint32_t lane = threadIdx.x, slot = blockIdx.x;
    unsigned long long ctr[kCtr];
    for (int k = 0; k < kCtr; ++k) ctr[k] = 0;
    for (;;) {                                                         // at most n_jobs + 1 turns
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(a.next, 1u);
        t = first_lane(t);
        if (t >= a.n_jobs) break;
        k16d_job<LDS>(a, a.job0 + t, slot, lane, (lds_float*)k16d_lds, ctr);
    }
    if (lane == 0)
        for (int k = 0; k < kCtr; ++k)
            if (ctr[k]) atomicAdd(&a.counters[k], ctr[k]);
}

std::atomic<uint64_t> g_lds_jobs{0}, g_scratch_jobs{0};

uint32_t lds_bytes(uint32_t cols) { return (kNewtonDenseTileFloats + (cols <= kNewtonDenseLdsCols ? kNewtonDenseVectors * cols : 0u)) * 4u; }

}  // namespace

uint32_t newton_dense_max_slots(uint32_t cols) {
    int dev = 0, cus = 0;
    XRL_HIP(hipGetDevice(&dev));
    XRL_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    return (uint32_t)std::min<uint64_t>(kTrainMaxSlots, (uint64_t)std::max(cus, 1) * std::min(16u, kTrainDenseLdsPerCu / lds_bytes(cols)));
}

void newton_dense_launch(const TrainJobArgs& base, const NewtonScratch& sc, const TrainDenseX& X, uint32_t n_jobs, uint32_t* next, uint32_t blocks, hipStream_t s) {
    if (X.cols > kTrainDenseMaxCols) fail(std::string(kWhat) + ": " + std::to_string(X.cols) + " columns are more than " + std::to_string(kTrainDenseMaxCols));
    K16DArgs a{};
    static_cast<K16Args&>(a) = newton_args(base, sc, n_jobs, next);
    a.X = X.val; a.row_stride = X.row_stride;
    a.aligned = (reinterpret_cast<uintptr_t>(X.val) % 16 == 0 && X.row_stride % 4 == 0) ? 1 : 0;
    const bool lds = X.cols <= kNewtonDenseLdsCols;
    if (lds) hipLaunchKernelGGL(k16d_solve<true>, dim3(blocks), dim3(64), lds_bytes(X.cols), s, a);
    else hipLaunchKernelGGL(k16d_solve<false>, dim3(blocks), dim3(64), lds_bytes(X.cols), s, a);
    XRL_LAUNCH_CHECK();
    (lds ? g_lds_jobs : g_scratch_jobs) += n_jobs;
}

void newton_dense_check_finite(const std::string& what, const TrainDenseX& X, hipStream_t s) {
    const uint64_t n = (uint64_t)X.rows * X.cols;
    if (!n) return;
    DevBuf flag;
    flag.reserve(4);
    XRL_HIP(hipMemsetAsync(flag.p, 0, 4, s));
    hipLaunchKernelGGL(k16d_finite, dim3(blocks_of(n, 256, kWhat)), dim3(256), 0, s, X.val, n, X.cols, X.row_stride, flag.as<uint32_t>());
    XRL_LAUNCH_CHECK();
    uint32_t f = 0;
    XRL_HIP(hipMemcpyAsync(&f, flag.p, 4, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    if (f) newton_fail_not_finite(what);
}

void newton_dense_forms(uint64_t (&out)[4]) {
    out[0] = kNewtonDenseLdsCols; out[1] = kTrainDenseMaxCols; out[2] = g_lds_jobs.load(); out[3] = g_scratch_jobs.load();
}

}  // namespace xrl
