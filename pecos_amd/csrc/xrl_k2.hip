// Per-query top-k of a layer's candidates and the winners' child ids, on gfx950 (64-wide wavefronts).
//   K2 k2_topk_*       sorted_csr + reorder_prediction      inference.hpp:1223-1298, 1919-1923
#include <hip/hip_runtime.h>

#include <type_traits>

#include "xrl_device.h"
#include "xrl_kernels.h"

namespace xrl {

// ---------------------------------------------------------------------------------------------
// K2: one wavefront per query.  Candidates are scanned in POSITION order; the running top-k list
// is kept sorted by (value desc, position asc), which is the comparator of sorted_csr
// (inference.hpp:1265-1273): a later candidate only displaces the current k-th if it is
// STRICTLY greater, and is inserted after every element that is >= it.  "Greater" is a compare of
// score_key values (xrl_device.h), as in every other form of the top-k: one total order on the
// fp32 bit patterns, NaN scores included (a float compare would rank a NaN first while the list
// fills and drop it afterwards).
// ---------------------------------------------------------------------------------------------
struct K2Args {
    const uint32_t* chunk_col;
    const uint32_t* perm_inv;
    const uint32_t* p_idx; const uint32_t* p_cnt; uint32_t p_stride;
    const uint32_t* cand_off; const uint32_t* ncand; const float* cand;
    uint32_t* out_idx; float* out_val; uint32_t* out_cnt;
    uint32_t nrows, beam_in, cand_stride, k, out_stride;
    int implicit_root;
    // exact bound pruning (k2_topk_wave only): rank_limit > 0 restricts the selection to the candidates of the first rank_limit beam
    // slots and reports in done[q] whether that selection is already FINAL -- every candidate of a later slot scores at most its
    // parent's score (transform <= 1 times / <= 0 plus the parent's score) and would lose a tie by position, so once k selected
    // candidates score >= the next parent's score nothing can change.  skip_done: queries to leave untouched (second phase).
    const float* p_val;
    int mult;                    // the combiner multiplies (sigmoid, l{p}-hinge): a child of a parent with a NEGATIVE score (possible when an
                                 // earlier layer used another post-processor) lies in [score, 0], so the bound is max(score, 0); additive
                                 // combiners (log-*) add a transform <= 0: the bound is the score itself
    uint32_t rank_limit;
    uint32_t* done;
    const uint32_t* skip_done;
    const uint32_t* xok;         // [nrows] the pruning guard of every query (prune_guard_ok): 0 = never final before every candidate is scored
    // the list of the queries a first stage left unfinished (count *rest_cnt, any order): with `done` the launch APPENDS to it (one atomicAdd per
    // wavefront, i.e. per unfinished query), without it k2_topk_list ranks the listed queries only
    uint32_t* rest_q; uint32_t* rest_cnt;
};

__device__ __forceinline__ uint32_t k2_child_id(const K2Args& a, uint64_t q, uint32_t pos) {
    // position -> (beam slot, child) -> original child id (reorder_prediction, inference.hpp:1776-1784)
    uint32_t parent = 0, off = 0;
    if (!a.implicit_root) {
        const uint32_t cnt = min(a.p_cnt[q], a.beam_in);
        uint32_t jj = 0;
        for (uint32_t j = 1; j < cnt; ++j) if (a.cand_off[q * a.beam_in + j] <= pos) jj = j; else break;
        off = a.cand_off[q * a.beam_in + jj];
        parent = a.p_idx[q * a.p_stride + jj];
    }
    const uint32_t child = a.chunk_col[parent] + (pos - off);
    return a.perm_inv ? a.perm_inv[child] : child;
}

__global__ void __launch_bounds__(64) k2_topk_reg(K2Args a) {   // k <= 64: lane i holds the i-th best
    const uint64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t n = a.ncand[q], k = a.k;
    const float* __restrict__ cv = a.cand + q * a.cand_stride;
    float lv = -INFINITY;
    uint32_t th = 0u;         // key of the current k-th best once the list is full (0: not full; every candidate's key is >= 1)
    uint32_t lp = 0, m = 0;
    constexpr int KB = 4;     // candidate batches (64 each) fetched per iteration: KB loads in flight
    const uint32_t nlast = n ? n - 1 : 0;
    for (uint32_t base0 = 0; base0 < n; base0 += 64 * KB) {
        float vb[KB];
#pragma unroll
        for (int b = 0; b < KB; ++b) { const uint32_t p = base0 + b * 64 + lane; vb[b] = cv[p < n ? p : nlast]; }   // unconditional, clamped
#pragma unroll
        for (int b = 0; b < KB; ++b) {
            const uint32_t base = base0 + b * 64;
            const uint32_t p = base + lane;
            const bool valid = p < n;
            const float v = vb[b];
            unsigned long long mask = __ballot(valid && (m < k || score_key(v) > th));
            while (mask) {
                const int l = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const float vv = __shfl(v, l);
                const uint32_t kv = score_key(vv);
                if (m == k && !(kv > th)) continue;
                const int r = __popcll(__ballot((uint32_t)lane < m && score_key(lv) >= kv));
                const float uv = __shfl_up(lv, 1);
                const uint32_t up = __shfl_up(lp, 1);
                if (lane > r) { lv = uv; lp = up; }
                else if (lane == r) { lv = vv; lp = base + l; }
                if (m < k) ++m;
                th = (m == k) ? score_key(__shfl(lv, (int)k - 1)) : 0u;
            }
        }
    }
    if ((uint32_t)lane < m) {
        a.out_idx[q * a.out_stride + lane] = k2_child_id(a, q, lp);
        a.out_val[q * a.out_stride + lane] = lv;
    }
    if (lane == 0) a.out_cnt[q] = m;
}

__global__ void __launch_bounds__(64) k2_topk_lds(K2Args a) {   // any k that fits LDS: sorted list in LDS
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* lv = reinterpret_cast<float*>(smem);
    uint32_t* lp = reinterpret_cast<uint32_t*>(lv + a.k);
    const uint64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t n = a.ncand[q], k = a.k;
    const float* __restrict__ cv = a.cand + q * a.cand_stride;
    uint32_t th = 0u;         // key of the current k-th best once the list is full (0: not full)
    uint32_t m = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t p = base + lane;
        const bool valid = p < n;
        const float v = valid ? cv[p] : 0.f;
        unsigned long long mask = __ballot(valid && (m < k || score_key(v) > th));
        while (mask) {
            const int l = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const float vv = __shfl(v, l);
            const uint32_t kv = score_key(vv);
            if (m == k && !(kv > th)) continue;
            uint32_t r = 0;
            for (uint32_t i0 = 0; i0 < m; i0 += 64) {
                const uint32_t i = i0 + lane;
                r += (uint32_t)__popcll(__ballot(i < m && score_key(lv[i]) >= kv));
            }
            const uint32_t e = (m < k) ? m : k - 1;        // elements [r, e) move up by one
            for (uint32_t hi = e; hi > r;) {
                const uint32_t lo = (hi - r > 64) ? hi - 64 : r;
                const uint32_t i = lo + lane;
                const bool mv = i < hi;
                float tv = 0.f; uint32_t tp = 0;
                if (mv) { tv = lv[i]; tp = lp[i]; }
                wave_sync_lds();
                if (mv) { lv[i + 1] = tv; lp[i + 1] = tp; }
                wave_sync_lds();
                hi = lo;
            }
            if (lane == 0) { lv[r] = vv; lp[r] = base + l; }
            wave_sync_lds();
            if (m < k) ++m;
            th = (m == k) ? score_key(lv[k - 1]) : 0u;
        }
    }
    wave_sync_lds();
    for (uint32_t i = lane; i < m; i += 64) {
        a.out_idx[q * a.out_stride + i] = k2_child_id(a, q, lp[i]);
        a.out_val[q * a.out_stride + i] = lv[i];
    }
    if (lane == 0) a.out_cnt[q] = m;
}

// K2, register form (k <= 64, candidate rows of up to 64 * NS scores): the whole candidate row sits in registers
// (candidate p = r*64 + lane) and wave_topk (xrl_device.h) selects and ranks with ballot bisection instead of
// serial insertions.  Four queries (wavefronts) per workgroup.
template <int NS>
__device__ __forceinline__ void k2_wave_query(const K2Args& a, const uint64_t q, uint2* sc, const int lane) {
    uint32_t n = min(a.ncand[q], (uint32_t)(64 * NS));
    const uint32_t bcnt0 = a.implicit_root ? 1u : min(a.p_cnt[q], a.beam_in);
    // (both loads are issued up front, whether or not the query has that many parents: no dependent round trips later)
    const uint32_t rl = min(a.rank_limit, a.beam_in - 1u);
    const uint32_t lim_off = a.rank_limit ? a.cand_off[q * a.beam_in + rl] : 0u;
    const float ps_next = a.rank_limit ? a.p_val[q * a.p_stride + rl] : 0.0f;
    const bool limited = a.rank_limit != 0u && bcnt0 > a.rank_limit;
    if (limited) n = min(n, lim_off);
    const float* __restrict__ cv = a.cand + q * a.cand_stride;
    const uint32_t slast = a.cand_stride - 1u;                  // last float of the query's candidate row (the loads below do not wait for n)
    // the beam's block offsets and parents, one per lane (beams of up to 64 parents): in flight while the candidates are ranked,
    // so that mapping a winner's position back to its child needs no dependent loads afterwards
    const uint32_t bcnt = a.implicit_root ? 1u : min(a.p_cnt[q], a.beam_in);
    const bool lane_beam = !a.implicit_root && bcnt <= 64u;
    uint32_t b_off = 0xFFFFFFFFu, b_par = 0u, b_cc = 0u;
    if (lane_beam && (uint32_t)lane < bcnt) { b_off = a.cand_off[q * a.beam_in + lane]; b_par = a.p_idx[q * a.p_stride + lane]; b_cc = a.chunk_col[b_par]; }
    uint32_t key[NS], sbits[NS], pos[NS];
#pragma unroll
    for (int r = 0; r < NS; ++r) {
        const uint32_t p = (uint32_t)r * 64u + (uint32_t)lane;
        const float v = cv[min(p, slast)];                         // unconditional, clamped to the row (positions >= n are masked below)
        sbits[r] = __float_as_uint(v); pos[r] = p;
        key[r] = p < n ? score_key(v) : 0u;
    }
    if (a.done) {   // (before the selection: it consumes the keys)
        bool d = true;
        // the k-th best >= the best any later slot can reach (a NaN parent score proves nothing: no pruning)
        if (limited) d = a.xok[q] != 0u && ps_next == ps_next && wave_count_ge<NS>(key, score_key(a.mult ? fmaxf(ps_next, 0.0f) : ps_next)) >= a.k;
        if (lane == 0) {
            a.done[q] = d ? 1u : 0u;
            if (!d && a.rest_q) a.rest_q[atomicAdd(a.rest_cnt, 1u)] = (uint32_t)q;
        }
    }
    uint32_t rank, sb, pp;
    const uint32_t kk = wave_topk<NS>(key, sbits, pos, a.k, sc, lane, rank, sb, pp);
    uint32_t child;
    if (lane_beam) {
        uint32_t jj = 0;                                            // last beam slot whose block starts at or before the position
        for (uint32_t j = 1; j < bcnt; ++j) jj = ((uint32_t)__builtin_amdgcn_readlane((int)b_off, (int)j) <= pp) ? j : jj;
        const uint32_t off = (uint32_t)__shfl((int)b_off, (int)jj, 64), cc = (uint32_t)__shfl((int)b_cc, (int)jj, 64);
        child = cc + (pp - off);
        if ((uint32_t)lane < kk && a.perm_inv) child = a.perm_inv[child];
    } else {
        child = (uint32_t)lane < kk ? k2_child_id(a, q, pp) : 0u;
    }
    if ((uint32_t)lane < kk) {
        a.out_idx[q * a.out_stride + rank] = child;
        a.out_val[q * a.out_stride + rank] = __uint_as_float(sb);
    }
    if (lane == 0) a.out_cnt[q] = kk;
}

template <int NS>
__global__ void __launch_bounds__(256) k2_topk_wave(K2Args a) {
    __shared__ uint2 sc_all[4 * 64];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t q32 = blockIdx.x * 4u + wave;
    if (q32 >= a.nrows) return;
    if (a.skip_done && a.skip_done[q32]) return;
    k2_wave_query<NS>(a, q32, sc_all + wave * 64u, lane);
}

// (k2_topk_list re-reads the kernel arguments for every listed query, through a pointer the compiler cannot see through: with the argument words
//  hoisted out of its loop and kept live around the selection the instantiations lose an occupancy step -- NS = 13: 75 VGPRs against 50)
//  K2Args must stay k2_topk_list's ONLY kernel argument: it is read from offset 0 of the kernel-argument segment, word by word.
typedef const __attribute__((address_space(4))) uint32_t K2ArgWord;
static_assert(sizeof(K2Args) % 4 == 0 && alignof(K2Args) <= 8 && std::is_trivially_copyable<K2Args>::value, "k2_wave_query_reload copies K2Args as 32-bit words");
template <int NS>
__device__ __forceinline__ void k2_wave_query_reload(K2ArgWord* wp, const uint32_t q32, uint2* sc, const int lane) {
    constexpr int NW = (int)(sizeof(K2Args) / 4);
    union { K2Args a; uint32_t w[NW]; } u;
    asm volatile("" : "+s"(wp));
#pragma unroll
    for (int i = 0; i < NW; ++i) u.w[i] = wp[i];
    k2_wave_query<NS>(u.a, q32, sc, lane);
}

// The last stage of a bound-pruned layer on the LIST of unfinished queries: a small fixed grid, every wavefront takes the listed queries
// wave, wave + #wavefronts, ... of the device-side count (the batch-sized grid of k2_topk_wave would return on skip_done[q] almost everywhere).
template <int NS>
__global__ void __launch_bounds__(256) k2_topk_list(K2Args a) {
    __shared__ uint2 sc_all[4 * 64];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * 4u, nq = min(*a.rest_cnt, a.nrows);
    for (uint32_t i = blockIdx.x * 4u + wave; i < nq; i += n_waves) {
        const uint32_t q32 = __builtin_amdgcn_readfirstlane(a.rest_q[i]);
        if (q32 < a.nrows) k2_wave_query_reload<NS>((K2ArgWord*)__builtin_amdgcn_kernarg_segment_ptr(), q32, sc_all + wave * 64u, lane);
        wave_sync_lds();
    }
}

size_t k2_max_k() { return (160 * 1024) / 8; }

static bool k2_wave_shape(uint32_t k, uint32_t cand_stride) { return k <= 64 && cand_stride <= 64u * 32u; }
bool k2_wave_path(const LayerPlan& P) { return k2_wave_shape(P.k, P.cand_stride); }

K2Choice k2_form(uint32_t k, uint32_t cand_stride, int64_t big_min_k, int stage, uint32_t limited_cands) {
    if (k == 0) fail("k2: only_topk / beam_size resolved to 0");
    if (stage < 0 || stage > 2) fail("k2: stage is 0 (whole row), 1 (bound-pruning stage) or 2 (list of unfinished queries)");
    const bool wave = k2_wave_shape(k, cand_stride);
    if (stage != 0 && !wave) fail("k2: bound pruning needs the register top-k path");
    // beyond the LDS kernel's reach (or forced, tests: k2_big_min_k): the segmented sort of xrl_topk_big.hip
    if (stage == 0 && (k > k2_max_k() || (big_min_k > 0 && (int64_t)k >= big_min_k))) return {K2_FORM_BIG, 0u};
    if (wave) {
        // (a rank-limited selection looks at the first slots' candidates only: registers for that many)
        const uint32_t ns = ((limited_cands ? std::min(cand_stride, limited_cands) : cand_stride) + 63u) / 64u;
        static const uint32_t buckets[] = {1, 2, 4, 8, 13, 16, 24, 32};
        uint32_t nn = 32;
        for (const uint32_t b : buckets) if (ns <= b) { nn = b; break; }
        // (the looped instantiation for 16 candidate registers would lose an occupancy step -- 68 VGPRs against 60: those rows keep the
        //  batch-sized grid and skip on the done flags)
        return {stage == 2 && nn != 16 ? K2_FORM_LIST : K2_FORM_WAVE, nn};
    }
    if (k <= 64) return {K2_FORM_REG, 0u};
    return {K2_FORM_LDS, 0u};   // (k <= k2_max_k(): a whole-row launch beyond it went to the segmented sort above, a pruning stage was refused)
}

namespace {
// fills what every launch sets and runs the form k2_form names; `a` arrives with its bound-pruning words set (all zero: the whole row)
void k2_launch(const LayerDev& L, const LayerPlan& P, BeamDev prev, const uint32_t* cand_off, const uint32_t* ncand, const float* cand, BeamDev out,
               hipStream_t s, K2Args a, int stage, uint32_t limited_cands) {
    a.mult = (P.pp.kind == PP_SIGMOID || P.pp.kind == PP_LP_HINGE) ? 1 : 0;
    a.chunk_col = L.chunk_col; a.perm_inv = L.perm_inv;
    a.p_idx = prev.idx; a.p_cnt = prev.cnt; a.p_stride = prev.stride; a.p_val = prev.val;
    a.cand_off = cand_off; a.ncand = ncand; a.cand = cand;
    a.out_idx = out.idx; a.out_val = out.val; a.out_cnt = out.cnt;
    a.nrows = P.nrows; a.beam_in = P.beam_in; a.cand_stride = P.cand_stride; a.k = P.k; a.out_stride = out.stride;
    a.implicit_root = P.implicit_root;
    const K2Choice c = k2_form(P.k, P.cand_stride, P.tune.k2_big_min_k, stage, limited_cands);
    switch (c.form) {
    case K2_FORM_BIG:
        launch_k2_topk_big(L, P, prev, cand_off, ncand, cand, out.idx, out.val, out.cnt, out.stride, s);
        return;
    case K2_FORM_WAVE:
    case K2_FORM_LIST: {
        const bool walk = c.form == K2_FORM_LIST;
        const dim3 grid(walk ? std::min<uint32_t>((P.nrows + 3u) / 4u, 1024u) : (P.nrows + 3u) / 4u), block(256);
#define XRL_K2_WAVE(NN) case NN: if (walk) hipLaunchKernelGGL(k2_topk_list<NN>, grid, block, 0, s, a); else hipLaunchKernelGGL(k2_topk_wave<NN>, grid, block, 0, s, a); break
        switch (c.ns) {
        XRL_K2_WAVE(1); XRL_K2_WAVE(2); XRL_K2_WAVE(4); XRL_K2_WAVE(8); XRL_K2_WAVE(13); XRL_K2_WAVE(24); XRL_K2_WAVE(32);
        case 16: hipLaunchKernelGGL(k2_topk_wave<16>, grid, block, 0, s, a); break;     // (never the list form: k2_form)
        default: fail("k2: no instantiation for " + std::to_string(c.ns) + " candidate registers");
        }
#undef XRL_K2_WAVE
        break;
    }
    case K2_FORM_REG:
        hipLaunchKernelGGL(k2_topk_reg, dim3(P.nrows), dim3(64), 0, s, a);
        break;
    case K2_FORM_LDS: {
        const size_t lds = (size_t)P.k * 8;
        if (lds > 48 * 1024)   // per DEVICE attribute: set on every large launch
            XRL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k2_topk_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k2_topk_lds, dim3(P.nrows), dim3(64), lds, s, a);
        break;
    }
    }
    XRL_LAUNCH_CHECK();
}
}  // namespace

void launch_k2_topk(const LayerDev& L, const LayerPlan& P, BeamDev prev, const uint32_t* cand_off,
                    const uint32_t* ncand, const float* cand, BeamDev out, hipStream_t s) {
    if (P.nrows != 0) k2_launch(L, P, prev, cand_off, ncand, cand, out, s, K2Args{}, 0, 0u);
}

void launch_k2_stage(const LayerDev& L, const LayerPlan& P, BeamDev prev, const uint32_t* cand_off,
                     const uint32_t* ncand, const float* cand, BeamDev out, const Stage& st, hipStream_t s) {
    if (P.nrows == 0) return;
    const bool last = st.kind == STAGE_LAST, list = last && st.io.rest_q;
    st.io.check("k2", !last);
    if (st.kind == STAGE_MID && st.io.rest_q) fail("k2: a middle stage keeps the batch-sized grid (the list belongs to layers of two stages)");
    if (list && !k2_wave_path(P)) fail("k2: the list form serves the last stage of a bound-pruned layer");
    K2Args a{};
    if (!last) { a.rank_limit = st.slot_end; a.done = st.io.done; a.xok = st.io.xok; }
    if (st.kind != STAGE_FIRST) a.skip_done = st.io.done;   // (a middle stage skips the queries finished earlier and renews the flags: one buffer serves both)
    if (st.kind != STAGE_MID) { a.rest_q = st.io.rest_q; a.rest_cnt = st.io.rest_cnt; }   // FIRST (with done) appends, LAST (without) walks the list
    k2_launch(L, P, prev, cand_off, ncand, cand, out, s, a, list ? 2 : 1, last ? 0u : std::max(1u, st.cands));
}

}  // namespace xrl
