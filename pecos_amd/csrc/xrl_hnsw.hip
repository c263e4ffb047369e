// K17: HNSW search in HBM.  One wavefront per query, queries taken from an atomic counter (K13's launch shape); the traversal is the
// reference's predict_single / search_level (hnsw.hpp:850-971) step for step, the queues are libstdc++'s push_heap / pop_heap / sort_heap
// restated (the comparator reads the distance only, so __push_heap / __adjust_heap decide which of two equal distances leaves first).
//
// Parallel: the distances of a popped node's unvisited neighbours (they do not depend on the admissions).  A step marks the neighbours by lane
// and compacts the fresh ones in j order, computes every distance, then lane 0 replays the reference's j-ascending admission loop.
//   dense:  16 lanes per neighbour, lane l owns acc[l] of the avx512f clone's statement, four neighbours per step
//   sparse: one lane per neighbour merges two ascending rows; the chain is serial by the rule
// Serial by the rule: the heap sifts, the admission order, the upper-level passes.
// Every loop carries a bound: pops <= num_node, sifts <= heap depth, passes <= num_node + 1 per level.  There are no spin waits.
#include <algorithm>
#include <cstdlib>

#include "xrl_device.h"
#include "xrl_hnsw.h"

namespace xrl {
namespace {

enum : uint32_t { kBadOrder = 1u, kBadRange = 2u, kBadValue = 4u, kBadPtr = 8u };

struct HnswArgs {
    HnswDev g;
    const float* x_val; uint64_t x_stride; const uint64_t* x_ptr; const uint32_t* x_idx; uint64_t x_nnz;
    uint32_t efS, topk, ef;
    uint32_t* out_idx; float* out_dist; uint32_t* out_count; uint64_t out_stride;
    uint32_t* visited; uint32_t* token;
    float* cand_d; uint32_t* cand_i; uint32_t cand_cap;
    float* top_d; uint32_t* top_i; uint32_t top_cap;      // null: the LDS form
    float* nbr_d; uint32_t* nbr_i; uint32_t nbr_cap;      // null: the LDS form
    uint32_t* next; uint32_t n_jobs; const uint32_t* job_list; uint32_t* redo; uint32_t* n_redo; const uint32_t* flags;
    unsigned long long* counters;
};

__device__ __forceinline__ void wave_sync_mem() {          // LDS and HBM written by one lane, read by another of the same wavefront
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ uint32_t lane0(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ float lane0(float v) { return __uint_as_float(lane0(__float_as_uint(v))); }

// ---- libstdc++'s heaps (bits/stl_heap.h), over a pair of arrays; MAX: std::less (the topk queue), else std::greater (the cand queue)
template <bool MAX> __device__ __forceinline__ bool heap_comp(float a, float b) { return MAX ? a < b : a > b; }

template <bool MAX> __device__ __forceinline__ void heap_push_at(float* d, uint32_t* id, int hole, int top, float vd, uint32_t vi) {   // __push_heap
    int parent = (hole - 1) / 2;
    while (hole > top && heap_comp<MAX>(d[parent], vd)) {              // hole halves: at most the heap's depth
        d[hole] = d[parent]; id[hole] = id[parent];
        hole = parent; parent = (hole - 1) / 2;
    }
    d[hole] = vd; id[hole] = vi;
}
template <bool MAX> __device__ __forceinline__ void heap_adjust(float* d, uint32_t* id, int hole, int len, float vd, uint32_t vi) {    // __adjust_heap
    const int top = hole;
    int child = hole;
    while (child < (len - 1) / 2) {                                    // child doubles: at most the heap's depth
        child = 2 * (child + 1);
        if (heap_comp<MAX>(d[child], d[child - 1])) --child;
        d[hole] = d[child]; id[hole] = id[child];
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        d[hole] = d[child - 1]; id[hole] = id[child - 1];
        hole = child - 1;
    }
    heap_push_at<MAX>(d, id, hole, top, vd, vi);
}
// std::pop_heap over [0, n): the top goes to position n - 1
template <bool MAX> __device__ __forceinline__ void heap_pop(float* d, uint32_t* id, int n) {
    if (n > 1) {
        const float vd = d[n - 1]; const uint32_t vi = id[n - 1];
        d[n - 1] = d[0]; id[n - 1] = id[0];
        heap_adjust<MAX>(d, id, 0, n - 1, vd, vi);
    }
}

// ---- distances
// A NaN distance carries the host's default NaN.  The loader and the check kernels admit finite values only, so no operand of either rule is
// ever a NaN of the caller's: every NaN is born of an invalid operation on finite or infinite values (inf + -inf), which an x86 host answers
// with 0xFFC00000 -- sign bit set -- and then carries unchanged through the later additions and the final (float)(1.0 - (double)s) or
// -2 * dot.  The device's default NaN is 0x7FC00000, and a negated operand flips a NaN's sign, so the bits are set once, at the end.  (K10's
// host_nan in xrl_spgemm.hip also hands on a caller's NaN payload; there is none to hand on here.)  The comparisons stay the reference's.
__device__ __forceinline__ float host_default_nan(float d) { return d == d ? d : __uint_as_float(0xFFC00000u); }
// Dense, the avx512f clone: called by all 64 lanes, the 16 lanes of a group share `node`; every lane of the group returns the distance.
__device__ __forceinline__ float dense_dist(const HnswDev& g, const float* __restrict__ q, uint32_t node, uint32_t lane) {
    const float* __restrict__ v = g.feat + (uint64_t)node * g.feat_dim;
    const uint32_t len = g.feat_dim, n16 = len / 16u, l = lane & 15u, jj = lane & 3u;
    const int base = (int)(lane & ~15u);
    float acc = 0.0f;
    for (uint32_t i = 0; i < n16; ++i) {                               // fused, lane l owns acc[l]
        const float x = q[16u * i + l], y = v[16u * i + l];
        if (g.l2) { const float df = __fsub_rn(x, y); acc = __fmaf_rn(df, df, acc); }
        else acc = __fmaf_rn(x, y, acc);
    }
    const float a0 = __shfl(acc, base + (int)jj), a1 = __shfl(acc, base + 4 + (int)jj), a2 = __shfl(acc, base + 8 + (int)jj), a3 = __shfl(acc, base + 12 + (int)jj);
    float qj = __fadd_rn(__fadd_rn(a0, a1), __fadd_rn(a2, a3));
    uint32_t k = n16 * 16u;
    for (; k + 4u <= len; k += 4u) {                                   // every further whole group of 4: NOT fused
        const float x = q[k + jj], y = v[k + jj];
        float p;
        if (g.l2) { const float df = __fsub_rn(x, y); p = __fmul_rn(df, df); }
        else p = __fmul_rn(x, y);
        qj = __fadd_rn(qj, p);
    }
    const float q0 = __shfl(qj, base), q1 = __shfl(qj, base + 1), q2 = __shfl(qj, base + 2), q3 = __shfl(qj, base + 3);
    float s = __fadd_rn(__fadd_rn(__fadd_rn(q0, q1), q2), q3);
    for (; k < len; ++k) {                                             // the last len % 4 elements: fused
        const float x = q[k], y = v[k];
        if (g.l2) { const float df = __fsub_rn(x, y); s = __fmaf_rn(df, df, s); }
        else s = __fmaf_rn(x, y, s);
    }
    return host_default_nan(g.l2 ? s : (float)(1.0 - (double)s));
}

// Sparse: one lane merges the query's row [qb, qe) with the item's; the products of the matching ids are added one by one in ascending id order.
// l2 is the reference's x_sq + y_sq - 2 * dot with both squares 0 (it measures each vector against itself): -2 * dot.
__device__ __forceinline__ float sparse_dist(const HnswArgs& a, uint64_t qb, uint64_t qe, uint32_t node) {
    uint64_t ib = a.g.row_ptr[node];
    const uint64_t ie = a.g.row_ptr[node + 1];
    float dot = 0.0f;
    while (qb < qe && ib < ie) {                                       // at most the two rows' lengths
        const uint32_t x = a.x_idx[qb], y = a.g.idx[ib];
        if (x == y) { dot = __fadd_rn(dot, __fmul_rn(a.x_val[qb], a.g.val[ib])); ++qb; ++ib; }
        else if (x < y) ++qb;
        else ++ib;
    }
    return host_default_nan(a.g.l2 ? (float)((double)__fadd_rn(0.0f, 0.0f) - 2.0 * (double)dot) : (float)(1.0 - (double)dot));
}

struct QueryRow { const float* q; uint64_t qb, qe; };

// cd[k] <- distance(query, cn[k]) for k < n; called by all lanes, the buffers are synchronised by the caller
__device__ __forceinline__ void dist_many(const HnswArgs& a, const QueryRow& r, const uint32_t* cn, float* cd, uint32_t n, uint32_t lane) {
    if (a.g.dense) {
        for (uint32_t k0 = 0; k0 < n; k0 += 4u) {
            const uint32_t k = k0 + (lane >> 4);
            const float d = dense_dist(a.g, r.q, cn[k < n ? k : n - 1u], lane);
            if (k < n && (lane & 15u) == 0u) cd[k] = d;
        }
    } else {
        for (uint32_t k0 = 0; k0 < n; k0 += 64u) {
            const uint32_t k = k0 + lane;
            if (k < n) cd[k] = sparse_dist(a, r.qb, r.qe, cn[k]);
        }
    }
}
__device__ __forceinline__ float dist_one(const HnswArgs& a, const QueryRow& r, uint32_t node, uint32_t lane) {
    return a.g.dense ? dense_dist(a.g, r.q, node, lane) : sparse_dist(a, r.qb, r.qe, node);
}

// One query.  false: the cand heap overflowed; nothing was written and the query is to run again with more entries.
__device__ bool hnsw_query(const HnswArgs& a, uint32_t qi, uint32_t slot, uint32_t lane, float* tk_d, uint32_t* tk_i, float* cd, uint32_t* cn,
                           unsigned long long* ctr) {
    const HnswDev& g = a.g;
    uint32_t* vis = a.visited + (uint64_t)slot * g.num_node;
    float* ca_d = a.cand_d + (uint64_t)slot * a.cand_cap;
    uint32_t* ca_i = a.cand_i + (uint64_t)slot * a.cand_cap;
    // a clean visited set: this query's token differs from every mark the slot holds
    uint32_t tok = a.token[slot] + 1u;
    if (tok == 0u) {
        for (uint32_t i = lane; i < g.num_node; i += 64u) vis[i] = 0u;
        tok = 1u;
    }
    wave_sync_mem();
    if (lane == 0) a.token[slot] = tok;

    QueryRow r{nullptr, 0, 0};
    if (g.dense) r.q = a.x_val + (uint64_t)qi * a.x_stride;
    else row_span(a.x_ptr, qi, a.x_nnz, r.qb, r.qe);

    unsigned long long n_dist = 1, n_pops = 0, n_adm = 0, n_pass = 0, max_cand = 1;
    // ---- the upper levels: a pass walks the neighbour list fetched at its start, and takes the first j of the strict minimum below curr_dist
    uint32_t curr = g.init_node;
    float curr_dist = dist_one(a, r, curr, lane);
    for (uint32_t level = g.max_level; level >= 1u; --level) {
        bool changed = true;
        for (uint32_t pass = 0; changed && pass <= g.num_node; ++pass) {
            changed = false;
            ++n_pass;
            const uint64_t at = (uint64_t)curr * g.l1_levels + (level - 1u);
            const uint32_t deg = min(g.l1_deg[at], g.maxM);
            wave_sync_mem();
            for (uint32_t j = lane; j < deg; j += 64u) cn[j] = g.l1_nbr[at * g.maxM + j];
            wave_sync_mem();
            dist_many(a, r, cn, cd, deg, lane);
            wave_sync_mem();
            n_dist += deg;
            for (uint32_t j = 0; j < deg; ++j) {
                const float d = cd[j];
                if (d < curr_dist) { curr_dist = d; curr = cn[j]; changed = true; }
            }
        }
    }
    // ---- level 0: best-first search with efS' = max(efS, topk)
    ++n_dist;                                                          // (search_level measures its entry point again)
    uint32_t n_top = 1, n_cand = 1, overflow = 0;
    float ub = curr_dist;
    wave_sync_mem();
    if (lane == 0) {
        tk_d[0] = ub; tk_i[0] = curr;
        ca_d[0] = ub; ca_i[0] = curr;
        vis[curr] = tok;
    }
    wave_sync_mem();
    for (uint32_t pops = 0; n_cand > 0u && pops < g.num_node; ++pops) {
        const float c_d = ca_d[0];
        const uint32_t c_i = ca_i[0];
        if (c_d > ub) break;
        wave_sync_mem();
        if (lane == 0) heap_pop<false>(ca_d, ca_i, (int)n_cand);
        --n_cand;
        ++n_pops;
        const uint32_t deg = min(g.l0_deg[c_i], g.maxM0);
        const uint32_t* nbr = g.l0_nbr + (uint64_t)c_i * g.maxM0;
        uint32_t nf = 0;
        for (uint32_t j0 = 0; j0 < deg; j0 += 64u) {                   // test and mark by lane (a neighbourhood lists no node twice: the loader checks)
            const uint32_t j = j0 + lane;
            bool fresh = false;
            uint32_t nb = 0;
            if (j < deg) {
                nb = nbr[j];
                fresh = vis[nb] != tok;
                if (fresh) vis[nb] = tok;
            }
            const unsigned long long m = __ballot(fresh);
            if (fresh) cn[nf + lanes_below(m)] = nb;
            nf += (uint32_t)__popcll(m);
        }
        wave_sync_mem();
        dist_many(a, r, cn, cd, nf, lane);
        wave_sync_mem();
        n_dist += nf;
        if (lane == 0) {                                               // the reference's admission loop, j ascending
            for (uint32_t k = 0; k < nf; ++k) {
                const float d = cd[k];
                if (n_top < a.ef || d < ub) {
                    if (n_cand >= a.cand_cap) { overflow = 1; break; }
                    heap_push_at<false>(ca_d, ca_i, (int)n_cand, 0, d, cn[k]);
                    ++n_cand;
                    if (n_cand > max_cand) max_cand = n_cand;
                    heap_push_at<true>(tk_d, tk_i, (int)n_top, 0, d, cn[k]);
                    ++n_top;
                    if (n_top > a.ef) { heap_pop<true>(tk_d, tk_i, (int)n_top); --n_top; }
                    ub = tk_d[0];
                    ++n_adm;
                }
            }
        }
        n_top = lane0(n_top); n_cand = lane0(n_cand); ub = lane0(ub); overflow = lane0(overflow);
        wave_sync_mem();
        if (overflow) return false;
    }
    // ---- pop down to topk only if topk < efS, then sort_heap
    if (lane == 0) {
        if (a.topk < a.efS)
            while (n_top > a.topk) { heap_pop<true>(tk_d, tk_i, (int)n_top); --n_top; }
        for (uint32_t n = n_top; n > 1u; --n) heap_pop<true>(tk_d, tk_i, (int)n);
    }
    n_top = lane0(n_top);
    wave_sync_mem();
    for (uint32_t k = lane; k < n_top; k += 64u) {
        a.out_idx[(uint64_t)qi * a.out_stride + k] = tk_i[k];
        a.out_dist[(uint64_t)qi * a.out_stride + k] = tk_d[k];
    }
    if (lane == 0) {
        a.out_count[qi] = n_top;
        ctr[0] += n_dist; ctr[1] += n_pops; ctr[2] += n_adm; ctr[3] += n_pass;
        if (max_cand > ctr[4]) ctr[4] = max_cand;
    }
    wave_sync_mem();
    return true;
}

__global__ void __launch_bounds__(64) k17_search(HnswArgs a) {
    __shared__ float s_tk_d[kHnswCap + 1];
    __shared__ uint32_t s_tk_i[kHnswCap + 1];
    __shared__ float s_cd[kHnswLdsDegree];
    __shared__ uint32_t s_cn[kHnswLdsDegree];
    if (*a.flags) return;                                              // a refused X: the outputs stay as they are
    const uint32_t lane = threadIdx.x, slot = blockIdx.x;
    float* tk_d = a.top_d ? a.top_d + (uint64_t)slot * a.top_cap : s_tk_d;
    uint32_t* tk_i = a.top_i ? a.top_i + (uint64_t)slot * a.top_cap : s_tk_i;
    float* cd = a.nbr_d ? a.nbr_d + (uint64_t)slot * a.nbr_cap : s_cd;
    uint32_t* cn = a.nbr_i ? a.nbr_i + (uint64_t)slot * a.nbr_cap : s_cn;
    unsigned long long ctr[5] = {0, 0, 0, 0, 0};
    for (;;) {                                                         // at most n_jobs + 1 turns
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(a.next, 1u);
        t = lane0(t);
        if (t >= a.n_jobs) break;
        const uint32_t qi = a.job_list ? a.job_list[t] : t;
        if (!hnsw_query(a, qi, slot, lane, tk_d, tk_i, cd, cn, ctr) && lane == 0) a.redo[atomicAdd(a.n_redo, 1u)] = qi;
    }
    if (lane == 0) {
        for (int k = 0; k < 4; ++k)
            if (ctr[k]) atomicAdd(&a.counters[k], ctr[k]);
        atomicMax(&a.counters[4], ctr[4]);
    }
}

// the query rows: ids strictly ascending and below cols, values finite, row pointers ascending and within nnz
__global__ void __launch_bounds__(256)
k17_check_csr(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const float* __restrict__ val, uint32_t rows, uint32_t cols, uint64_t nnz,
              uint32_t* __restrict__ flags) {
    uint32_t f = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * 256u) {
        const uint64_t b = ptr[r], e = ptr[r + 1];
        if (b > e || e > nnz) { f |= kBadPtr; continue; }
        for (uint64_t p = b; p < e; ++p) {
            if (idx[p] >= cols) f |= kBadRange;
            if (p > b && idx[p] <= idx[p - 1]) f |= kBadOrder;
            if ((__float_as_uint(val[p]) & 0x7F800000u) == 0x7F800000u) f |= kBadValue;
        }
    }
    if (f) atomicOr(flags, f);
}
__global__ void __launch_bounds__(256)
k17_check_drm(const float* __restrict__ val, uint32_t rows, uint32_t cols, uint64_t stride, uint32_t* __restrict__ flags) {
    const uint64_t n = (uint64_t)rows * cols;
    uint32_t f = 0;
    for (uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x; x < n; x += (uint64_t)gridDim.x * 256u) {
        const uint64_t r = x / cols, c = x % cols;
        if ((__float_as_uint(val[r * stride + c]) & 0x7F800000u) == 0x7F800000u) f |= kBadValue;
    }
    if (f) atomicOr(flags, f);
}

uint32_t cand_cap_of(uint32_t num_node) {
    uint64_t cap = kHnswCandCap;
    if (const char* e = std::getenv("XRL_HNSW_CAND_CAP")) { const uint64_t v = std::strtoull(e, nullptr, 10); if (v) cap = v; }   // (tests: a small capacity makes queries run again)
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cap, num_node));
}

// the header of the work buffer: next, n_redo, flags, pad (u32 each), then 5 u64 counters
struct WorkHead { uint32_t next, n_redo, flags, pad; unsigned long long counters[5]; };

}  // namespace

uint32_t hnsw_default_slots(const HnswIndex& ix, uint32_t rows) {
    const uint64_t per_slot = (uint64_t)ix.d.num_node * 4 + (uint64_t)cand_cap_of(ix.d.num_node) * 8;
    const uint64_t by_budget = std::max<uint64_t>(1, kHnswSlotBudget / std::max<uint64_t>(per_slot, 1));
    return (uint32_t)std::min<uint64_t>({by_budget, kHnswMaxSlots, std::max<uint32_t>(rows, 1)});
}

void hnsw_searchers_reserve(HnswSearchers& sc, const HnswIndex& ix, uint32_t slots, hipStream_t s) {
    sc.owner = &ix; sc.device = ix.device; sc.slots = slots; sc.num_node = ix.d.num_node;
    sc.cand_cap = cand_cap_of(ix.d.num_node);
    const size_t vb = (size_t)slots * ix.d.num_node * 4;
    sc.visited.reserve(vb); sc.token.reserve((size_t)slots * 4);
    XRL_HIP(hipMemsetAsync(sc.visited.p, 0, vb, s));                  // (on the stream that searches next, or synchronised by the caller)
    XRL_HIP(hipMemsetAsync(sc.token.p, 0, (size_t)slots * 4, s));
    sc.cand_d.reserve((size_t)slots * sc.cand_cap * 4); sc.cand_i.reserve((size_t)slots * sc.cand_cap * 4);
}

void hnsw_search(const char* name, const HnswIndex& ix, const QueriesDev& X, uint64_t x_stride, uint32_t efS, uint32_t topk, uint32_t* d_idx, float* d_dist,
                 uint32_t* d_count, uint64_t out_stride, HnswSearchers* sc, hipStream_t s, HnswCounters& c) {
    const std::string what = std::string(name) + ": ";
    const uint32_t rows = X.rows;
    if (!rows) return;
    HnswSearchers own;
    if (!sc) { hnsw_searchers_reserve(own, ix, hnsw_default_slots(ix, rows), s); sc = &own; }
    if (sc->owner != &ix || sc->num_node != ix.d.num_node || sc->device != ix.device) fail(what + "the searchers belong to another index");
    if (sc->busy.exchange(true)) fail(what + "the searchers are in use by another call; a searchers handle serves one call at a time");
    struct Release { std::atomic<bool>& b; ~Release() { b = false; } } release{sc->busy};   // (every path below ends after the stream's last synchronisation, or by an exception)
    const uint32_t ef = std::max(efS, topk);
    const uint32_t max_deg = std::max(ix.d.maxM0, ix.d.maxM);
    HnswArgs a{};
    a.g = ix.d;
    a.x_val = X.val; a.x_stride = x_stride; a.x_ptr = X.row_ptr; a.x_idx = X.col_idx; a.x_nnz = X.nnz;
    a.efS = efS; a.topk = topk; a.ef = ef;
    a.out_idx = d_idx; a.out_dist = d_dist; a.out_count = d_count; a.out_stride = out_stride;
    a.visited = sc->visited.as<uint32_t>(); a.token = sc->token.as<uint32_t>();
    a.cand_d = sc->cand_d.as<float>(); a.cand_i = sc->cand_i.as<uint32_t>(); a.cand_cap = sc->cand_cap;
    if (ef > kHnswCap) {                                               // the HBM form of the topk heap: the same code over scratch
        const uint32_t cap = std::min(ef, ix.d.num_node) + 1u;        // (the heap never holds more than the nodes there are, plus the one about to leave)
        if (cap > sc->top_cap) { sc->top_d.reserve((size_t)sc->slots * cap * 4); sc->top_i.reserve((size_t)sc->slots * cap * 4); sc->top_cap = cap; }
        a.top_d = sc->top_d.as<float>(); a.top_i = sc->top_i.as<uint32_t>(); a.top_cap = sc->top_cap;
    }
    if (max_deg > kHnswLdsDegree) {
        if (max_deg > sc->nbr_cap) { sc->nbr_d.reserve((size_t)sc->slots * max_deg * 4); sc->nbr_i.reserve((size_t)sc->slots * max_deg * 4); sc->nbr_cap = max_deg; }
        a.nbr_d = sc->nbr_d.as<float>(); a.nbr_i = sc->nbr_i.as<uint32_t>(); a.nbr_cap = sc->nbr_cap;
    }
    sc->work.reserve(sizeof(WorkHead) + (size_t)rows * 8);
    XRL_HIP(hipMemsetAsync(sc->work.p, 0, sizeof(WorkHead), s));
    WorkHead* wh = sc->work.as<WorkHead>();
    uint32_t* redo0 = reinterpret_cast<uint32_t*>(wh + 1);
    a.next = &wh->next; a.n_redo = &wh->n_redo; a.flags = &wh->flags; a.counters = wh->counters;
    a.n_jobs = rows; a.job_list = nullptr; a.redo = redo0;

    if (X.dense) {
        const uint64_t n = (uint64_t)rows * X.cols;
        if (n) hipLaunchKernelGGL(k17_check_drm, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, s, X.val, rows, X.cols, x_stride, &wh->flags);
    } else {
        hipLaunchKernelGGL(k17_check_csr, dim3((uint32_t)std::min<uint64_t>(((uint64_t)rows + 255) / 256, 4096)), dim3(256), 0, s, X.row_ptr, X.col_idx, X.val, rows,
                           X.cols, X.nnz, &wh->flags);
    }
    XRL_LAUNCH_CHECK();
    hipLaunchKernelGGL(k17_search, dim3(std::min(sc->slots, rows)), dim3(64), 0, s, a);
    XRL_LAUNCH_CHECK();
    WorkHead h{};
    XRL_HIP(hipMemcpyAsync(&h, wh, sizeof(WorkHead), hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));                                  // the one synchronisation: the overflow flag (and the refusals of X)
    if (h.flags & kBadPtr) fail(what + "the row pointers of X are not ascending within its stored entries");
    if (h.flags & kBadRange) fail(what + "a query row has a column id at or above feat_dim = " + std::to_string(ix.d.feat_dim));
    if (h.flags & kBadOrder) fail(what + "a query row has unsorted or repeated column ids");
    if (h.flags & kBadValue) fail(what + "a query value is not finite");
    if (h.n_redo) {                                                    // queries whose cand heap overflowed: again, with an entry per node
        const uint32_t n_redo = h.n_redo;
        const uint32_t cap2 = std::max<uint32_t>(ix.d.num_node, 1);
        const uint32_t slots2 = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)sc->slots, (uint64_t)n_redo, kHnswSlotBudget / ((uint64_t)cap2 * 8)}));
        DevBuf cd2, ci2;
        cd2.reserve((size_t)slots2 * cap2 * 4); ci2.reserve((size_t)slots2 * cap2 * 4);
        a.cand_d = cd2.as<float>(); a.cand_i = ci2.as<uint32_t>(); a.cand_cap = cap2;
        a.job_list = redo0; a.redo = redo0 + rows; a.n_jobs = n_redo;
        XRL_HIP(hipMemsetAsync(&wh->next, 0, 8, s));                   // next and n_redo; the counters go on
        hipLaunchKernelGGL(k17_search, dim3(slots2), dim3(64), 0, s, a);
        XRL_LAUNCH_CHECK();
        XRL_HIP(hipMemcpyAsync(&h, wh, sizeof(WorkHead), hipMemcpyDeviceToHost, s));
        XRL_HIP(hipStreamSynchronize(s));
        if (h.n_redo) fail(what + "internal: a cand heap with an entry per node overflowed");
        c.rerun += n_redo;
    }
    c.dist += h.counters[0]; c.pops += h.counters[1]; c.admissions += h.counters[2]; c.passes += h.counters[3];
    c.max_cand = std::max<uint64_t>(c.max_cand, h.counters[4]);
    (ef > kHnswCap ? c.hbm_queries : c.lds_queries) += rows;
}

}  // namespace xrl
