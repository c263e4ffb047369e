// K18: PairwiseANN in HBM.  One wavefront per (query row, label key) pair, pairs taken from an atomic counter (K13's and K17's launch shape), so
// short and long columns balance by themselves.  The rule is the reference's predict_single (ann/pairwise.hpp:265-288): every entry of the
// label's column is emplaced in stored order into a max-heap on the distance alone, the heap is popped down to only_topk, sort_heap runs.
//
// Phase A, parallel: the distances of the column's entries (K17's two rules, xrl_ann_device.h), the query staged once in LDS.
//   dense:  16 lanes per row, four rows a step;   sparse: one merge per lane, 64 rows a step
//   every distance becomes a 64-bit key (order-preserving image of the distance bits, position p in the column); a NaN takes image 0
// Phase B, the form.  The heap's history shows in the answer only where distances tie or are NaN.  With m = min(n, only_topk + 1):
//   sorted  n <= CAP: the wavefront sorts the keys in LDS (bitonic).  If the first m images are pairwise different under == and none is a NaN
//           (a NaN sorts first, so any NaN of the column is among them), the first min(n, only_topk) entries are the answer.
//   stream  n > CAP, only_topk + 1 <= KEEP: LDS keeps the best KEEP keys, each further chunk of CAP - KEEP is merged in by one sort; same test.
//   replay  everything else: lane 0 runs the reference's emplace / pop / sort_heap over all n distances in stored order -- in LDS for n <= CAP
//           (over the key array, the distances are kept beside it), else over per-slot HBM scratch after the distances are computed into it
//           (again, if the stream form came first: a second pass).
// Serial by the rule: the replay.  Every loop carries a bound (entries of the column, heap depth, log^2 sort stages); there are no spin waits.
// No MFMA: a matrix instruction cannot produce the avx512f clone's rounding sequence.
#include <algorithm>

#include "xrl_ann_device.h"
#include "xrl_pairwise.h"

namespace xrl {
namespace {

enum : uint32_t { kPairInternal = 128u };

struct PairArgs {
    PairDev g;
    const float* q_val; uint64_t q_stride; const uint64_t* q_ptr; const uint32_t* q_idx; uint64_t q_nnz;
    const uint32_t* keys; uint32_t pairs, topk; int same_input;
    uint32_t* out_I; uint32_t* out_M; float* out_D; float* out_V; uint64_t out_stride;
    float* scratch; uint32_t col_cap;
    uint32_t* next; uint32_t* flags; unsigned long long* counters;
};

// the header of the work buffer
struct WorkHead { uint32_t next, flags, pad0, pad1; unsigned long long counters[6]; };

struct PairQuery { const float* q; const uint32_t* qi; const float* qv; uint64_t qb, qe; };

constexpr unsigned long long kPadKey = ~0ull;             // above every key: an image is at most 0xFFFFFFFF and a position is below n

__device__ __forceinline__ unsigned long long pair_key(float d, uint32_t p) {
    const uint32_t b = __float_as_uint(d);
    const uint32_t o = d != d ? 0u : ((b & 0x80000000u) ? ~b : (b | 0x80000000u));   // -inf is 0x007FFFFF: 0 is a NaN's alone
    return ((unsigned long long)o << 32) | p;
}
__device__ __forceinline__ float key_dist(unsigned long long k) {                    // (of a number, never of a NaN)
    const uint32_t o = (uint32_t)(k >> 32);
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// the query row in LDS (dense: feat_dim floats; sparse: ids at sq[0 ..), values at sq[kPairQueryLds / 2 ..)) up to the cap, else where it lies in HBM
__device__ __forceinline__ PairQuery stage_query(const PairArgs& a, uint32_t row, uint32_t* sq, uint32_t lane) {
    PairQuery r{nullptr, nullptr, nullptr, 0, 0};
    if (a.g.dense) {
        const float* src = a.q_val + (uint64_t)row * a.q_stride;
        r.q = src;
        if (a.g.feat_dim <= kPairQueryLds) {
            for (uint32_t i = lane; i < a.g.feat_dim; i += 64u) sq[i] = __float_as_uint(src[i]);
            r.q = reinterpret_cast<const float*>(sq);
        }
    } else {
        row_span(a.q_ptr, row, a.q_nnz, r.qb, r.qe);
        r.qi = a.q_idx; r.qv = a.q_val;
        const uint64_t len = r.qe - r.qb;
        if (len <= kPairQueryLds / 2u) {
            for (uint32_t i = lane; i < (uint32_t)len; i += 64u) {
                sq[i] = a.q_idx[r.qb + i];
                sq[kPairQueryLds / 2u + i] = __float_as_uint(a.q_val[r.qb + i]);
            }
            r.qi = sq; r.qv = reinterpret_cast<const float*>(sq + kPairQueryLds / 2u);
            r.qb = 0; r.qe = len;
        }
    }
    wave_sync_mem();
    return r;
}

// store(p, distance(query, X_trn[row of entry p])) for the entries p0 <= p < p0 + cnt of the column that starts at cb; called by all lanes
template <class F>
__device__ __forceinline__ void pair_dists(const PairArgs& a, const PairQuery& r, uint64_t cb, uint32_t p0, uint32_t cnt, uint32_t lane, F&& store) {
    if (a.g.dense) {
        for (uint32_t k0 = 0; k0 < cnt; k0 += 4u) {
            const uint32_t k = k0 + (lane >> 4);
            const uint32_t node = a.g.y_idx[cb + p0 + (k < cnt ? k : cnt - 1u)];
            const float d = dense_dist(a.g.feat, a.g.feat_dim, 0, r.q, node, lane);
            if (k < cnt && (lane & 15u) == 0u) store(p0 + k, d);
        }
    } else {
        for (uint32_t k0 = 0; k0 < cnt; k0 += 64u) {
            const uint32_t k = k0 + lane;
            if (k < cnt) store(p0 + k, sparse_dist(a.g.row_ptr, a.g.idx, a.g.val, 0, r.qi, r.qv, r.qb, r.qe, a.g.y_idx[cb + p0 + k]));
        }
    }
}

// ascending bitonic sort of keys[0, P), P a power of two; the keys are pairwise different (their positions are)
__device__ __forceinline__ void wave_sort_keys(unsigned long long* keys, uint32_t P, uint32_t lane) {
    for (uint32_t k = 2u; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t t = lane; t < P / 2u; t += 64u) {
                const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), x = i | j;
                const unsigned long long u = keys[i], v = keys[x];
                if ((u > v) == ((i & k) == 0u)) { keys[i] = v; keys[x] = u; }
            }
            wave_sync_mem();
        }
    }
}
__device__ __forceinline__ uint32_t pow2_at_least(uint32_t n) { uint32_t p = 2u; while (p < n) p <<= 1; return p; }

// the first m sorted keys are totally ordered: no NaN (it would be the first), no two images equal under == (-0 ties with +0)
__device__ __forceinline__ bool first_ordered(const unsigned long long* keys, uint32_t m, uint32_t lane) {
    bool bad = false;
    for (uint32_t t = lane; t < m; t += 64u) {
        const uint32_t o = (uint32_t)(keys[t] >> 32);
        if (o == 0u) bad = true;
        if (t + 1u < m) {
            const uint32_t o2 = (uint32_t)(keys[t + 1u] >> 32);
            if (o == o2 || (o == 0x7FFFFFFFu && o2 == 0x80000000u)) bad = true;
        }
    }
    return __ballot(bad) == 0ull;
}

// the reference's predict_single over dist[0, n) in stored order, by one lane; the heap entry's id is the position.  -> entries left, ascending
__device__ __forceinline__ uint32_t pair_replay(float* hd, uint32_t* hi, const float* dist, uint32_t n, uint32_t topk) {
    for (uint32_t p = 0; p < n; ++p) heap_push_at<true>(hd, hi, (int)p, 0, dist[p], p);
    uint32_t size = n;
    if (topk < n)
        while (size > topk) { heap_pop<true>(hd, hi, (int)size); --size; }
    for (uint32_t s = size; s > 1u; --s) heap_pop<true>(hd, hi, (int)s);
    return size;
}

__device__ __forceinline__ void pair_write(const PairArgs& a, uint32_t b, uint32_t t, uint64_t cb, uint32_t p, float d) {
    const uint64_t at = (uint64_t)b * a.out_stride + t;
    a.out_I[at] = a.g.y_idx[cb + p]; a.out_M[at] = 1u; a.out_D[at] = d; a.out_V[at] = a.g.y_val[cb + p];
}

// ctr: sorted, stream, replay, distance evaluations, second passes, longest column
__device__ void pair_one(const PairArgs& a, uint32_t b, uint32_t slot, uint32_t lane, const PairQuery& r, unsigned long long* s_key, float* s_dist,
                         unsigned long long* ctr) {
    const uint32_t label = a.keys[b];
    const uint64_t cb = a.g.y_ptr[label];
    const uint32_t n = (uint32_t)(a.g.y_ptr[label + 1] - cb), topk = a.topk;
    if (n > ctr[5]) ctr[5] = n;
    if (n == 0u) { ++ctr[0]; return; }
    const uint32_t m = topk < n ? topk + 1u : n, n_out = min(n, topk);
    wave_sync_mem();                                                   // (the pair before this one has read its LDS)
    if (n <= kPairCap) {
        pair_dists(a, r, cb, 0u, n, lane, [&](uint32_t p, float d) { s_dist[p] = d; s_key[p] = pair_key(d, p); });
        ctr[3] += n;
        const uint32_t P = pow2_at_least(n);
        for (uint32_t t = n + lane; t < P; t += 64u) s_key[t] = kPadKey;
        wave_sync_mem();
        wave_sort_keys(s_key, P, lane);
        if (first_ordered(s_key, m, lane)) {
            for (uint32_t t = lane; t < n_out; t += 64u) { const uint32_t p = (uint32_t)s_key[t]; pair_write(a, b, t, cb, p, s_dist[p]); }
            ++ctr[0];
            return;
        }
        wave_sync_mem();
        float* hd = reinterpret_cast<float*>(s_key);                   // the heap takes the key array's place: CAP distances, then CAP positions
        uint32_t* hi = reinterpret_cast<uint32_t*>(s_key) + kPairCap;
        uint32_t size = 0;
        if (lane == 0) size = pair_replay(hd, hi, s_dist, n, topk);
        size = lane0(size);
        wave_sync_mem();
        for (uint32_t t = lane; t < size; t += 64u) pair_write(a, b, t, cb, hi[t], hd[t]);
        ++ctr[2];
        return;
    }
    bool second = false;
    if ((unsigned long long)topk + 1ull <= kPairKeep) {
        pair_dists(a, r, cb, 0u, kPairCap, lane, [&](uint32_t p, float d) { s_key[p] = pair_key(d, p); });
        wave_sync_mem();
        wave_sort_keys(s_key, kPairCap, lane);
        for (uint32_t p0 = kPairCap; p0 < n;) {                        // at most n / (CAP - KEEP) + 1 turns
            const uint32_t c = min(n - p0, kPairCap - kPairKeep);
            pair_dists(a, r, cb, p0, c, lane, [&](uint32_t p, float d) { s_key[kPairKeep + (p - p0)] = pair_key(d, p); });
            for (uint32_t t = kPairKeep + c + lane; t < kPairCap; t += 64u) s_key[t] = kPadKey;
            wave_sync_mem();
            wave_sort_keys(s_key, kPairCap, lane);
            p0 += c;
        }
        ctr[3] += n;
        if (first_ordered(s_key, m, lane)) {
            for (uint32_t t = lane; t < n_out; t += 64u) { const unsigned long long k = s_key[t]; pair_write(a, b, t, cb, (uint32_t)k, key_dist(k)); }
            ++ctr[1];
            return;
        }
        second = true;
    }
    if (n > a.col_cap) {                                               // (never: the scratch is sized from the index's longest column)
        if (lane == 0) atomicOr(a.flags, kPairInternal);
        return;
    }
    float* dist = a.scratch + (uint64_t)slot * 3u * a.col_cap;
    float* hd = dist + a.col_cap;
    uint32_t* hi = reinterpret_cast<uint32_t*>(hd + a.col_cap);
    pair_dists(a, r, cb, 0u, n, lane, [&](uint32_t p, float d) { dist[p] = d; });
    ctr[3] += n;
    if (second) ++ctr[4];
    wave_sync_mem();
    uint32_t size = 0;
    if (lane == 0) size = pair_replay(hd, hi, dist, n, topk);
    size = lane0(size);
    wave_sync_mem();
    for (uint32_t t = lane; t < size; t += 64u) pair_write(a, b, t, cb, hi[t], hd[t]);
    ++ctr[2];
}

__global__ void __launch_bounds__(64) k18_pairs(PairArgs a) {
    __shared__ unsigned long long s_key[kPairCap];
    __shared__ float s_dist[kPairCap];
    __shared__ uint32_t s_q[kPairQueryLds];
    if (*a.flags) return;                                              // refused queries or keys: the outputs stay as they are
    const uint32_t lane = threadIdx.x, slot = blockIdx.x;
    unsigned long long ctr[6] = {0, 0, 0, 0, 0, 0};
    uint32_t staged = 0xFFFFFFFFu;                                     // (a row index is below 2^32 - 1)
    PairQuery r{};
    for (;;) {                                                         // at most pairs + 1 turns
        uint32_t b = 0;
        if (lane == 0) b = atomicAdd(a.next, 1u);
        b = lane0(b);
        if (b >= a.pairs) break;
        const uint32_t row = a.same_input ? 0u : b;
        if (row != staged) {
            wave_sync_mem();
            r = stage_query(a, row, s_q, lane);
            staged = row;
        }
        pair_one(a, b, slot, lane, r, s_key, s_dist, ctr);
    }
    if (lane == 0) {
        for (int k = 0; k < 5; ++k)
            if (ctr[k]) atomicAdd(&a.counters[k], ctr[k]);
        atomicMax(&a.counters[5], ctr[5]);
    }
}

// ---- checks
__global__ void __launch_bounds__(256)
k18_check_csr(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const float* __restrict__ val, uint32_t rows, uint32_t cols, uint64_t nnz,
              uint32_t* __restrict__ flags) {
    const uint32_t f = check_csr_rows(ptr, idx, val, rows, cols, nnz);
    if (f) atomicOr(flags, f);
}
__global__ void __launch_bounds__(256)
k18_check_drm(const float* __restrict__ val, uint32_t rows, uint32_t cols, uint64_t stride, uint32_t* __restrict__ flags) {
    const uint32_t f = check_drm_rows(val, rows, cols, stride);
    if (f) atomicOr(flags, f);
}
__global__ void __launch_bounds__(256) k18_check_keys(const uint32_t* __restrict__ keys, uint32_t pairs, uint32_t num_label, uint32_t* __restrict__ flags) {
    uint32_t f = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x; b < pairs; b += (uint64_t)gridDim.x * 256u)
        if (keys[b] >= num_label) f = kPairBadLabel;
    if (f) atomicOr(flags, f);
}
// Y_csc: column pointers ascending within nnz, a column of fewer than 2^32 - 1 entries; out[0] the flags, out[1] the longest column
__global__ void __launch_bounds__(256) k18_check_y_ptr(const uint64_t* __restrict__ ptr, uint32_t cols, uint64_t nnz, uint32_t* __restrict__ out) {
    uint32_t f = 0, longest = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x; c < cols; c += (uint64_t)gridDim.x * 256u) {
        const uint64_t b = ptr[c], e = ptr[c + 1];
        if (b > e || e > nnz || e - b >= 0xFFFFFFFFull) f = kPairBadYPtr;
        else longest = max(longest, (uint32_t)(e - b));
    }
    if (f) atomicOr(&out[0], f);
    if (longest) atomicMax(&out[1], longest);
}
__global__ void __launch_bounds__(256) k18_check_y_idx(const uint32_t* __restrict__ idx, uint64_t nnz, uint32_t rows, uint32_t* __restrict__ out) {
    uint32_t f = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < nnz; p += (uint64_t)gridDim.x * 256u)
        if (idx[p] >= rows) f = kPairBadYRow;
    if (f) atomicOr(&out[0], f);
}

uint32_t grid_of(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 4096)); }

void launch_check_x(const QueriesDev& X, uint64_t stride, uint32_t rows, uint32_t* flags, hipStream_t s) {
    if (X.dense) {
        if ((uint64_t)rows * X.cols) hipLaunchKernelGGL(k18_check_drm, dim3(grid_of((uint64_t)rows * X.cols)), dim3(256), 0, s, X.val, rows, X.cols, stride, flags);
    } else if (rows) {
        hipLaunchKernelGGL(k18_check_csr, dim3(grid_of(rows)), dim3(256), 0, s, X.row_ptr, X.col_idx, X.val, rows, X.cols, X.nnz, flags);
    }
    XRL_LAUNCH_CHECK();
}

}  // namespace

uint32_t pairwise_check_index(PairIndex& ix, hipStream_t s) {
    PairDev& d = ix.d;
    DevBuf out;
    out.reserve(8);
    XRL_HIP(hipMemsetAsync(out.p, 0, 8, s));
    QueriesDev X{};
    X.val = d.dense ? d.feat : d.val; X.row_ptr = d.row_ptr; X.col_idx = d.idx; X.rows = d.num_input; X.cols = d.feat_dim; X.dense = d.dense; X.nnz = d.dense ? 0 : ix.nnz_x;
    launch_check_x(X, d.feat_dim, d.num_input, out.as<uint32_t>(), s);
    hipLaunchKernelGGL(k18_check_y_ptr, dim3(grid_of(d.num_label)), dim3(256), 0, s, d.y_ptr, d.num_label, ix.nnz_y, out.as<uint32_t>());
    XRL_LAUNCH_CHECK();
    uint32_t h[2] = {0, 0};
    XRL_HIP(hipMemcpyAsync(h, out.p, 8, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    if (!(h[0] & kPairBadYPtr) && ix.nnz_y) {                          // (the row ids are read only once the pointers are known to lie within them)
        hipLaunchKernelGGL(k18_check_y_idx, dim3(grid_of(ix.nnz_y)), dim3(256), 0, s, d.y_idx, ix.nnz_y, d.num_input, out.as<uint32_t>());
        XRL_LAUNCH_CHECK();
        XRL_HIP(hipMemcpyAsync(h, out.p, 4, hipMemcpyDeviceToHost, s));
        XRL_HIP(hipStreamSynchronize(s));
    }
    d.max_col = h[1];
    return h[0];
}

std::string pairwise_refusal(const std::string& what, uint32_t f, const PairIndex& ix, const char* of) {
    const std::string m = std::string(of);
    if (f & kPairBadYPtr) return what + "the column pointers of Y are not ascending within its stored entries";
    if (f & kPairBadYRow) return what + "Y has a row id at or above X_trn.rows = " + std::to_string(ix.d.num_input);
    if (f & kPairBadLabel) return what + "a label key is at or above num_label_keys = " + std::to_string(ix.d.num_label);
    if (f & kBadPtr) return what + "the row pointers of " + m + " are not ascending within its stored entries";
    if (f & kBadRange) return what + "a row of " + m + " has a column id at or above feat_dim = " + std::to_string(ix.d.feat_dim);
    if (f & kBadOrder) return what + "a row of " + m + " has unsorted or repeated column ids";
    if (f & kBadValue) return what + "a value of " + m + " is not finite";
    return what + "internal: a column is longer than the searchers' scratch";
}

uint32_t pairwise_default_slots(const PairIndex& ix, uint32_t pairs) {
    const uint64_t per_slot = ix.d.max_col > kPairCap ? 12ull * ix.d.max_col : 0;
    const uint64_t by_budget = per_slot ? std::max<uint64_t>(1, kPairSlotBudget / per_slot) : kPairMaxSlots;
    return (uint32_t)std::min<uint64_t>({by_budget, kPairMaxSlots, std::max<uint32_t>(pairs, 1)});
}

void pairwise_searchers_reserve(PairSearchers& sc, const PairIndex& ix, uint32_t slots) {
    sc.owner = &ix; sc.device = ix.device;
    sc.col_cap = ix.d.max_col > kPairCap ? ix.d.max_col : 0;
    sc.slots = std::min(slots, pairwise_default_slots(ix, slots));     // (cut to the byte budget)
    sc.scratch.reserve((size_t)sc.slots * sc.col_cap * 12);
    sc.work.reserve(sizeof(WorkHead));
}

void pairwise_search(const char* name, const PairIndex& ix, const QueriesDev& Q, uint64_t q_stride, const uint32_t* d_keys, uint32_t pairs, uint32_t only_topk,
                     bool same_input, uint32_t* d_I, uint32_t* d_M, float* d_D, float* d_V, uint64_t out_stride, PairSearchers* sc, hipStream_t s, PairCounters& c) {
    const std::string what = std::string(name) + ": ";
    if (!pairs || !only_topk) return;
    PairSearchers own;
    if (!sc) { pairwise_searchers_reserve(own, ix, pairwise_default_slots(ix, pairs)); sc = &own; }
    if (sc->owner != &ix || sc->device != ix.device) fail(what + "the searchers belong to another index");
    if (sc->busy.exchange(true)) fail(what + "the searchers are in use by another call; a searchers handle serves one call at a time");
    struct Release { std::atomic<bool>& b; ~Release() { b = false; } } release{sc->busy};   // (every path below ends after the stream's synchronisation, or by an exception)
    WorkHead* wh = sc->work.as<WorkHead>();
    XRL_HIP(hipMemsetAsync(wh, 0, sizeof(WorkHead), s));
    PairArgs a{};
    a.g = ix.d;
    a.q_val = Q.val; a.q_stride = q_stride; a.q_ptr = Q.row_ptr; a.q_idx = Q.col_idx; a.q_nnz = Q.nnz;
    a.keys = d_keys; a.pairs = pairs; a.topk = only_topk; a.same_input = same_input ? 1 : 0;
    a.out_I = d_I; a.out_M = d_M; a.out_D = d_D; a.out_V = d_V; a.out_stride = out_stride;
    a.scratch = sc->scratch.as<float>(); a.col_cap = sc->col_cap;
    a.next = &wh->next; a.flags = &wh->flags; a.counters = wh->counters;
    launch_check_x(Q, q_stride, same_input ? 1u : pairs, &wh->flags, s);
    hipLaunchKernelGGL(k18_check_keys, dim3(grid_of(pairs)), dim3(256), 0, s, d_keys, pairs, ix.d.num_label, &wh->flags);
    XRL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k18_pairs, dim3(std::min(sc->slots, pairs)), dim3(64), 0, s, a);
    XRL_LAUNCH_CHECK();
    WorkHead h{};
    XRL_HIP(hipMemcpyAsync(&h, wh, sizeof(WorkHead), hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));                                  // the one synchronisation: the refusals and the counters
    if (h.flags) fail(pairwise_refusal(what, h.flags, ix, "the queries"));
    c.sorted += h.counters[0]; c.stream += h.counters[1]; c.replay += h.counters[2]; c.dist += h.counters[3]; c.second_pass += h.counters[4];
    c.max_col = std::max<uint64_t>(c.max_col, h.counters[5]);
}

}  // namespace xrl
