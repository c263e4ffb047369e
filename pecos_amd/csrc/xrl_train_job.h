// What one training job is, whichever solver runs it (K13's dual coordinate descent in xrl_train.hip, K16's Newton method in
// xrl_newton.hip): the instances init_worker lists (linear_solver.hpp:667-712) and the emission of SVMJob::solve (:718-779), as __device__
// functions of ONE WAVEFRONT over its slot of scratch.  The rule is stated in include/xrl_abi.h at xrl_train_layer_device.
#pragma once
#include "xrl_device.h"

namespace xrl {

enum : uint32_t { kBadPtr = 1u, kBadId = 2u, kUnsorted = 4u, kDiffers = 8u, kTwice = 16u, kStageFull = 32u };

// What a wavefront's lanes wrote to HBM is visible to its other lanes afterwards.  A slot is touched by ONE wavefront, so workgroup scope
// is all that is needed: the workgroup's CU has one vector L1, write-through, which its own stores and atomics keep coherent, so the fence
// is a drain of the memory counters and no cache is invalidated.  Nothing in a slot is ever read by another workgroup during the launch.
__device__ __forceinline__ void wave_sync_hbm() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t first_lane(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the operands, the emission's parameters, and the part of a slot's scratch ([slot * its size]) that the set-up and the emission use
struct TrainJobArgs {
    const uint64_t* x_ptr; const uint32_t* x_idx; const float* x_val; uint64_t x_nnz; uint32_t N, d;
    const uint64_t* y_ptr; const uint32_t* y_idx; const float* r_val; uint64_t y_nnz;
    const uint64_t* c_ptr; const uint32_t* c_idx; uint32_t K;            // null: job j is label j, its instances are all rows
    const uint64_t* m_ptr; const uint32_t* m_idx; uint64_t m_nnz;
    double threshold, Cp, Cn, eps, bias;
    uint32_t max_nz;
    uint32_t* index; uint32_t index_cap; float* cost; signed char* ysg; float* w; uint32_t* touched; uint32_t dw;
    uint32_t job0;
    uint32_t* st_idx; float* st_val; uint32_t stride;                     // staging row of job j: (j - job0) * stride
    unsigned long long* cnt; uint32_t* job_label;                         // per job
    uint32_t* flags;
};

__device__ __forceinline__ uint32_t k13_word_mask(uint32_t wd, uint32_t d) { return (uint64_t)wd * 32u + 32u <= d ? 0xFFFFFFFFu : (1u << (d - wd * 32u)) - 1u; }

// (|w| bits, lower feature first) of a staged entry: the larger key is kept first
__device__ __forceinline__ uint64_t k13_key(float v, uint32_t f) { return ((uint64_t)(__float_as_uint(v) & 0x7FFFFFFFu) << 32) | (0xFFFFFFFFu - f); }

// ---- the instances (init_worker): M's column as stored, then Y's positives that are not among them, as stored.  -> their count; index,
//      cost and ysg (by row id) are written and visible to every lane
__device__ __forceinline__ uint32_t train_job_setup(const TrainJobArgs& a, uint32_t label, uint32_t code, uint32_t lane, uint32_t* index, float* cost, signed char* ysg) {
    uint32_t n = 0;
    if (a.m_ptr) {
        uint64_t mb, me;
        row_span(a.m_ptr, code, a.m_nnz, mb, me);
        for (uint64_t x = mb + lane; x < me; x += 64u) {
            const uint32_t i = a.m_idx[x];
            index[x - mb] = i; cost[i] = 1.0f; ysg[i] = -1;
        }
        n = (uint32_t)(me - mb);
    } else {
        for (uint32_t i = lane; i < a.N; i += 64u) { index[i] = i; cost[i] = 1.0f; ysg[i] = -1; }
        n = a.N;
    }
    wave_sync_hbm();
    {
        uint64_t yb, ye;
        row_span(a.y_ptr, label, a.y_nnz, yb, ye);
        // The reference walks the column one stored position after the other: a position appends its row when the row's cost is 0 at
        // that moment ("not listed"), then stores its own cost.  A row id stored twice is therefore appended once per occurrence that
        // meets a cost of 0, and the LAST stored cost stays.  Here 64 positions go per step, and the order is made the stored order BY
        // LANE NUMBER, never by the order in which the memory serves the lanes: every lane finds the nearest lower lane with its row id
        // (the cost that lane carries is the cost this lane meets) and whether a higher lane has it too; a lane without a lower twin
        // reads cost[i] as the steps before left it, and only the lane without a higher twin stores -- one writer per address, no atomic.
        for (uint64_t x0 = yb; x0 < ye; x0 += 64u) {
            const uint64_t x = x0 + lane;
            const bool have = x < ye;
            const uint32_t cnt = (uint32_t)min((uint64_t)64u, ye - x0);
            uint32_t i = 0;
            float c = 1.0f;
            if (have) { i = a.y_idx[x]; if (a.r_val) c = a.r_val[x]; }
            bool lower = false, higher = false;
            float met = 0.0f;
            for (uint32_t l = 0; l < cnt; ++l) {                       // l is uniform: two lane reads a turn, at most 64 turns
                const uint32_t il = (uint32_t)__builtin_amdgcn_readlane((int)i, (int)l);
                const float cl = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(c), (int)l));
                if (have && il == i) {
                    if (l < lane) { lower = true; met = cl; }
                    else if (l > lane) higher = true;
                }
            }
            if (have && !lower) met = cost[i];
            const bool fresh = have && met == 0.0f;                    // +0 and -0 both read as "not listed"; a NaN does not
            wave_sync_hbm();                                           // a first occurrence has read cost[i] before the last one stores to it
            if (have && !higher) cost[i] = c;
            if (have) ysg[i] = 1;
            const unsigned long long m = __ballot(fresh);
            const uint32_t at = n + lanes_below(m);
            if (fresh && at < a.index_cap) index[at] = i;
            n += (uint32_t)__popcll(m);
            wave_sync_hbm();                                           // the next step's lanes read the costs this step stored
        }
        if (n > a.index_cap) n = a.index_cap;                          // (cannot happen: a stored position of Y appends at most once, and the cap counts them all)
    }
    wave_sync_hbm();
    return n;
}

// ---- emission (SVMJob::solve): the entries with |w| >= threshold by ascending feature into the job's staging row; w and the bitmap
//      go back to zero on the way, and so do the instances' marks.  A job that is to run again (discard) stages nothing: false.
__device__ __forceinline__ bool train_job_emit(const TrainJobArgs& a, uint32_t job, uint32_t label, uint32_t lane, float* w, uint32_t* touched, float* cost,
                                               const uint32_t* index, uint32_t n, float bw, bool discard) {
    const uint32_t bj = job - a.job0;
    uint32_t* sidx = a.st_idx + (uint64_t)bj * a.stride;
    float* sval = a.st_val + (uint64_t)bj * a.stride;
    const bool every = a.threshold <= 0.0;
    uint32_t c = 0, full = 0;
    for (uint32_t w0 = 0; w0 < a.dw; w0 += 64u) {
        const uint32_t wd = w0 + lane;
        uint32_t bits = 0;
        if (wd < a.dw) {
            bits = touched[wd];
            if (bits) touched[wd] = 0u;
            if (every) bits = k13_word_mask(wd, a.d);
        }
        uint32_t mine = 0;
        if (!discard)
            for (uint32_t bb = bits; bb; bb &= bb - 1u) mine += (double)fabsf(w[wd * 32u + (uint32_t)__builtin_ctz(bb)]) >= a.threshold ? 1u : 0u;
        uint32_t incl = mine;
        for (int dlt = 1; dlt < 64; dlt <<= 1) { const uint32_t t = __shfl_up(incl, dlt, 64); if ((int)lane >= dlt) incl += t; }
        uint32_t at = c + incl - mine;
        for (uint32_t bb = bits; bb; bb &= bb - 1u) {
            const uint32_t f = wd * 32u + (uint32_t)__builtin_ctz(bb);
            const float v = w[f];
            w[f] = 0.0f;
            if (!discard && (double)fabsf(v) >= a.threshold) {
                if (at < a.stride) { sidx[at] = f; sval[at] = v; } else full = 1;
                ++at;
            }
        }
        c += (uint32_t)__shfl(incl, 63);
    }
    // the instances' marks
    for (uint32_t s = lane; s < n; s += 64u) cost[index[s]] = 0.0f;
    wave_sync_hbm();
    if (__ballot(full)) { if (lane == 0) atomicOr(a.flags, (uint32_t)kStageFull); c = min(c, a.stride); }
    if (discard) return false;
    bool push_bias = a.bias > 0 && (double)fabsf(bw) >= a.threshold;
    if (a.max_nz && c >= a.max_nz) {
        // the max_nz largest |w|, ties to the lower feature: T = the max_nz-th largest key, by bisection over the key's value (64 steps)
        unsigned long long lo = 0, hi = ~0ull;
        while (lo < hi) {
            const unsigned long long mid = lo + ((hi - lo) >> 1) + 1ull;
            uint32_t ge = 0;
            for (uint32_t x0 = 0; x0 < c; x0 += 64u) {
                const uint32_t x = x0 + lane;
                ge += (uint32_t)__popcll(__ballot(x < c && k13_key(sval[x], sidx[x]) >= mid));
            }
            if (ge >= a.max_nz) lo = mid; else hi = mid - 1ull;
        }
        // the bias competes with the least kept feature (:764-773)
        const float least = __uint_as_float((uint32_t)(lo >> 32));
        bool drop_least = false;
        if (a.bias > 0) {
            if (fabsf(bw) > least) drop_least = true; else push_bias = false;
        }
        uint32_t kept = 0;
        for (uint32_t x0 = 0; x0 < c; x0 += 64u) {
            const uint32_t x = x0 + lane;
            uint32_t f = 0;
            float v = 0.0f;
            bool keep = false;
            if (x < c) { f = sidx[x]; v = sval[x]; const unsigned long long k = k13_key(v, f); keep = drop_least ? k > lo : k >= lo; }
            const unsigned long long m = __ballot(keep);
            if (keep) { sidx[kept + lanes_below(m)] = f; sval[kept + lanes_below(m)] = v; }
            kept += (uint32_t)__popcll(m);
            wave_sync_hbm();
        }
        c = kept;
    }
    if (push_bias) {
        if (c < a.stride) { if (lane == 0) { sidx[c] = a.d; sval[c] = bw; } ++c; }
        else if (lane == 0) atomicOr(a.flags, (uint32_t)kStageFull);
    }
    if (lane == 0) { a.cnt[job] = c; a.job_label[job] = label; }
    return true;
}

}  // namespace xrl
