// K19: HNSW graph construction in HBM, the reference's HNSW::train at threads = 1 (hnsw.hpp:555-846) step for step.
//
// k19_insert: ONE workgroup of four wavefronts builds one index; insertions are serial by the rule, a launch inserts a bounded run of
// consecutive nodes (kHnswTrainRun, a first guess) and the host loops over the runs.  Inside an insertion:
//   search at efC, greedy descent   the distances of a popped node's unvisited neighbours by the whole workgroup (dense: 16 lanes per neighbour,
//                                   16 neighbours per step; sparse: one merge per thread), then thread 0 replays the admissions and the heap
//                                   sifts in j order -- K17's serial part, over the same device functions (xrl_ann_device.h)
//   get_neighbors_heuristic         keep / drop is serial in the candidate; the distances of one candidate to every node kept so far in parallel,
//                                   a workgroup-wide OR of `<` decides (the reference's early break only saves work)
//   the reverse links               the add_link(dst, q) of one level touch disjoint lists and read only features: one wavefront each, with its
//                                   Mcurmax + 1 distances, its candidate heaps and its heuristic in its own part of LDS
// LDS: the topk heap (efC <= CAP), the cand heap (a node enters it at most once: up to kHnswTrainCandLds nodes in LDS, above in HBM), the
// staged query row, one neighbourhood, the kept list.  After a search the cand heap's space serves the heuristic's min-heap, then the
// per-wavefront heaps of the reverse links.  The visited marks are one token-stamped array in HBM.
// Lists written in one phase and read in the next are separated by workgroup barriers (__syncthreads: fence + barrier); vector stores only.
// Every loop carries the reference's bound: pops <= num_node, passes <= num_node + 1, sifts <= heap depth, candidates <= heap size.
//
// k19_sort_neighbours: one wavefront per node.  Distances in parallel; a list whose distances are pairwise different and not NaN is placed by
// rank (every correct sort agrees), any other by one lane's replay of libstdc++'s std::sort (bits/stl_algo.h).
#include <algorithm>
#include <cmath>
#include <random>

#include "xrl_ann_device.h"
#include "xrl_hnsw_train.h"

namespace xrl {
namespace {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kWaveSlots = kHnswTrainCandLds / kWaves;          // a reverse link's share of the arena: three lists of up to kHnswLdsDegree + 1
constexpr uint32_t kLinkMin = 260, kLinkKept = 520;                  // offsets of its min-heap and kept list; its max-heap is at 0
static_assert(kLinkKept + kHnswLdsDegree <= kWaveSlots && kHnswCap <= kHnswTrainCandLds && 2 * kHnswTrainMaxM <= kHnswLdsDegree, "the LDS plan");

struct TrainArgs {
    uint32_t num_node, feat_dim, maxM, maxM0, efC, l1_levels;
    int dense, l2;
    uint32_t* l0_deg; uint32_t* l0_nbr; uint32_t* l1_deg; uint32_t* l1_nbr;
    const float* feat; const uint64_t* row_ptr; const uint32_t* idx; const float* val; uint64_t nnz;
    const uint32_t* level;              // [num_node]
    uint32_t* state;                    // init_node, max_level, the visited token: carried from launch to launch
    uint32_t* visited;                  // [num_node]
    float* cand_d; uint32_t* cand_i;    // null: the LDS form
    unsigned long long* counters;       // HnswTrainCounters
    uint32_t first, last;               // the run [first, last)
};

struct Shared {
    float top_d[kHnswCap + 1]; uint32_t top_i[kHnswCap + 1];
    float arena_d[kHnswTrainCandLds]; uint32_t arena_i[kHnswTrainCandLds];
    float row_v[kHnswTrainRowLds]; uint32_t row_i[kHnswTrainRowLds / 2];
    uint32_t cn[kHnswLdsDegree]; float cd[kHnswLdsDegree];
    uint32_t kept_i[kHnswTrainMaxM]; float kept_d[kHnswTrainMaxM];
    uint32_t wcnt[kWaves];
    uint32_t n_top, n_cand, curr, changed;
    float ub, curr_dist;
};

// one side of a distance: a dense row, or the entries [qb, qe) of (qi, qv)
struct Row { const float* q; const uint32_t* qi; const float* qv; uint64_t qb, qe; };

__device__ __forceinline__ Row row_of(const TrainArgs& a, uint32_t node) {
    Row r{nullptr, a.idx, a.val, 0, 0};
    if (a.dense) r.q = a.feat + (uint64_t)node * a.feat_dim;
    else row_span(a.row_ptr, node, a.nnz, r.qb, r.qe);
    return r;
}
__device__ __forceinline__ uint32_t* deg_ptr(const TrainArgs& a, uint32_t node, uint32_t level) {
    return level ? a.l1_deg + ((uint64_t)node * a.l1_levels + (level - 1u)) : a.l0_deg + node;
}
__device__ __forceinline__ uint32_t* nbr_ptr(const TrainArgs& a, uint32_t node, uint32_t level) {
    return level ? a.l1_nbr + ((uint64_t)node * a.l1_levels + (level - 1u)) * a.maxM : a.l0_nbr + (uint64_t)node * a.maxM0;
}

// a group is the workgroup (WG) or one wavefront
template <bool WG> __device__ __forceinline__ void group_sync() { if (WG) __syncthreads(); else wave_sync_mem(); }
template <bool WG> __device__ __forceinline__ bool group_any(bool p) { return WG ? __syncthreads_or(p ? 1 : 0) != 0 : __ballot(p) != 0ull; }

// cd[k] <- distance(r, cn[k]) for k < n, by the nt threads of a group (whole wavefronts) of which the caller is thread t
__device__ __forceinline__ void dist_many(const TrainArgs& a, const Row& r, const uint32_t* cn, float* cd, uint32_t n, uint32_t t, uint32_t nt) {
    if (a.dense) {
        for (uint32_t k0 = 0; k0 < n; k0 += nt >> 4) {
            const uint32_t k = k0 + (t >> 4);
            const float d = dense_dist(a.feat, a.feat_dim, a.l2, r.q, cn[k < n ? k : n - 1u], t & 63u);
            if (k < n && (t & 15u) == 0u) cd[k] = d;
        }
    } else {
        for (uint32_t k = t; k < n; k += nt) cd[k] = sparse_dist(a.row_ptr, a.idx, a.val, a.l2, r.qi, r.qv, r.qb, r.qe, cn[k]);
    }
}
// is some kept[k], k < n, strictly closer to r than dq -- the heuristic's test, every distance evaluated
template <bool WG> __device__ __forceinline__ bool any_closer(const TrainArgs& a, const Row& r, const uint32_t* kept, uint32_t n, float dq, uint32_t t, uint32_t nt) {
    bool p = false;
    if (a.dense) {
        for (uint32_t k0 = 0; k0 < n; k0 += nt >> 4) {
            const uint32_t k = k0 + (t >> 4);
            const float d = dense_dist(a.feat, a.feat_dim, a.l2, r.q, kept[k < n ? k : n - 1u], t & 63u);
            p = p || (k < n && d < dq);
        }
    } else {
        for (uint32_t k = t; k < n; k += nt) p = p || sparse_dist(a.row_ptr, a.idx, a.val, a.l2, r.qi, r.qv, r.qb, r.qe, kept[k]) < dq;
    }
    return group_any<WG>(p);
}

// get_neighbors_heuristic over the max-heap (hd, hi) of n entries, by a group: untouched when n < M; else drained into the min-heap (md, mi)
// in pop order, a candidate kept unless some kept one is strictly closer to it than the query is, at most M kept, and the kept ones emplaced
// back in that order.  n is the same in every thread.  n_dist: the leader's count of distances.
template <bool WG> __device__ __forceinline__ void heuristic(const TrainArgs& a, float* hd, uint32_t* hi, uint32_t& n, uint32_t M, float* md, uint32_t* mi, float* kd,
                                                             uint32_t* ki, uint32_t t, uint32_t nt, unsigned long long& n_dist) {
    if (n < M) return;
    const bool leader = t == 0u;
    group_sync<WG>();
    if (leader)
        for (uint32_t left = n, m = 0; left > 0u; --left, ++m) {
            const float vd = hd[0]; const uint32_t vi = hi[0];
            heap_pop<true>(hd, hi, (int)left);
            heap_push_at<false>(md, mi, (int)m, 0, vd, vi);
        }
    uint32_t left = n, nk = 0;
    for (; left > 0u && nk < M; --left) {                              // at most n candidates
        group_sync<WG>();
        const float cur_d = md[0]; const uint32_t cur_i = mi[0];
        group_sync<WG>();
        if (leader) heap_pop<false>(md, mi, (int)left);
        const bool closer = nk ? any_closer<WG>(a, row_of(a, cur_i), ki, nk, cur_d, t, nt) : false;
        if (!closer) {
            if (leader) { kd[nk] = cur_d; ki[nk] = cur_i; }
            ++nk;
        }
        if (leader) n_dist += nk - (closer ? 0u : 1u);
    }
    group_sync<WG>();
    if (leader)
        for (uint32_t k = 0; k < nk; ++k) heap_push_at<true>(hd, hi, (int)k, 0, kd[k], ki[k]);
    n = nk;
    group_sync<WG>();
}

// search_level at efC from `entry` on `level`, by the workgroup: the topk heap is left in S.top_* with S.n_top entries
__device__ void search_level(const TrainArgs& a, Shared& S, const Row& q, uint32_t entry, uint32_t level, uint32_t& tok, float* ca_d, uint32_t* ca_i, uint32_t t,
                             unsigned long long& n_dist) {
    const uint32_t lane = t & 63u, w = t >> 6, cap = level ? a.maxM : a.maxM0;
    ++tok;                                                             // a clean visited set: the token differs from every mark
    if (tok == 0u) {
        for (uint32_t i = t; i < a.num_node; i += kThreads) a.visited[i] = 0u;
        tok = 1u;
    }
    if (t == 0) S.cn[0] = entry;
    __syncthreads();
    dist_many(a, q, S.cn, S.cd, 1u, t, kThreads);
    __syncthreads();
    if (t == 0) {
        const float d = S.cd[0];
        S.top_d[0] = d; S.top_i[0] = entry; ca_d[0] = d; ca_i[0] = entry;
        a.visited[entry] = tok;
        S.n_top = 1u; S.n_cand = 1u; S.ub = d;
        ++n_dist;
    }
    __syncthreads();
    for (uint32_t pops = 0; pops < a.num_node; ++pops) {
        const uint32_t n_cand = S.n_cand;
        if (n_cand == 0u) break;
        const float c_d = ca_d[0];
        const uint32_t c_i = ca_i[0];
        if (c_d > S.ub) break;
        __syncthreads();
        if (t == 0) { heap_pop<false>(ca_d, ca_i, (int)n_cand); S.n_cand = n_cand - 1u; }
        const uint32_t deg = min(*deg_ptr(a, c_i, level), cap);
        const uint32_t* nbr = nbr_ptr(a, c_i, level);
        bool fresh = false;                                            // test and mark by thread: a neighbourhood lists no node twice
        uint32_t nb = 0;
        if (t < deg) {
            nb = nbr[t];
            fresh = a.visited[nb] != tok;
            if (fresh) a.visited[nb] = tok;
        }
        const unsigned long long m = __ballot(fresh);
        if (lane == 0) S.wcnt[w] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = 0, nf = 0;                                      // the fresh ones compacted in j order
        for (uint32_t i = 0; i < kWaves; ++i) { if (i < w) off += S.wcnt[i]; nf += S.wcnt[i]; }
        if (fresh) S.cn[off + lanes_below(m)] = nb;
        __syncthreads();
        dist_many(a, q, S.cn, S.cd, nf, t, kThreads);
        __syncthreads();
        if (t == 0) {                                                  // the reference's admission loop, j ascending
            uint32_t n_top = S.n_top, nc = S.n_cand;
            float ub = S.ub;
            for (uint32_t k = 0; k < nf; ++k) {
                const float d = S.cd[k];
                if (n_top < a.efC || d < ub) {
                    heap_push_at<false>(ca_d, ca_i, (int)nc, 0, d, S.cn[k]);
                    ++nc;
                    heap_push_at<true>(S.top_d, S.top_i, (int)n_top, 0, d, S.cn[k]);
                    ++n_top;
                    if (n_top > a.efC) { heap_pop<true>(S.top_d, S.top_i, (int)n_top); --n_top; }
                    ub = S.top_d[0];
                }
            }
            S.n_top = n_top; S.n_cand = nc; S.ub = ub;
            n_dist += nf;
        }
        __syncthreads();
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kThreads) k19_insert(TrainArgs a) {
    __shared__ Shared S;
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    float* ca_d = a.cand_d ? a.cand_d : S.arena_d;
    uint32_t* ca_i = a.cand_i ? a.cand_i : S.arena_i;
    uint32_t init_node = a.state[0], max_level = a.state[1], tok = a.state[2];
    unsigned long long n_search = 0, n_select = 0, n_reverse = 0, n_rewritten = 0;
    __syncthreads();
    for (uint32_t q = a.first; q < a.last; ++q) {
        const uint32_t ql = a.level[q];
        if (q == 0u) { init_node = 0u; max_level = ql; continue; }
        // ---- the query row, staged when it fits
        Row qr = row_of(a, q);
        __syncthreads();
        if (a.dense) {
            if (a.feat_dim <= kHnswTrainRowLds) {
                for (uint32_t k = t; k < a.feat_dim; k += kThreads) S.row_v[k] = qr.q[k];
                qr.q = S.row_v;
            }
        } else if (qr.qe - qr.qb <= kHnswTrainRowLds / 2) {
            const uint32_t len = (uint32_t)(qr.qe - qr.qb);
            for (uint32_t k = t; k < len; k += kThreads) { S.row_i[k] = a.idx[qr.qb + k]; S.row_v[k] = a.val[qr.qb + k]; }
            qr.qi = S.row_i; qr.qv = S.row_v; qr.qb = 0; qr.qe = len;
        }
        __syncthreads();
        // ---- the greedy descent from max_level to above the query's level: a pass walks the list fetched at its start
        uint32_t curr = init_node;
        if (ql < max_level) {
            if (t == 0) S.cn[0] = curr;
            __syncthreads();
            dist_many(a, qr, S.cn, S.cd, 1u, t, kThreads);
            __syncthreads();
            if (t == 0) { S.curr = curr; S.curr_dist = S.cd[0]; ++n_search; }
            __syncthreads();
            for (uint32_t level = max_level; level > ql; --level) {
                for (uint32_t pass = 0; pass <= a.num_node; ++pass) {
                    curr = S.curr;
                    const uint32_t deg = min(*deg_ptr(a, curr, level), a.maxM);
                    const uint32_t* nbr = nbr_ptr(a, curr, level);
                    if (t < deg) S.cn[t] = nbr[t];
                    __syncthreads();
                    dist_many(a, qr, S.cn, S.cd, deg, t, kThreads);
                    __syncthreads();
                    if (t == 0) {
                        float cdist = S.curr_dist;
                        uint32_t c = curr, changed = 0;
                        for (uint32_t j = 0; j < deg; ++j)
                            if (S.cd[j] < cdist) { cdist = S.cd[j]; c = S.cn[j]; changed = 1u; }
                        S.curr = c; S.curr_dist = cdist; S.changed = changed;
                        n_search += deg;
                    }
                    __syncthreads();
                    if (!S.changed) break;
                }
            }
            curr = S.curr;
        }
        // ---- per level: search at efC, select, connect both ways
        for (uint32_t level = min(ql, max_level);; --level) {
            const uint32_t cap = level ? a.maxM : a.maxM0;
            search_level(a, S, qr, curr, level, tok, ca_d, ca_i, t, n_search);
            uint32_t n = S.n_top;
            heuristic<true>(a, S.top_d, S.top_i, n, a.maxM, S.arena_d, S.arena_i, S.kept_d, S.kept_i, t, kThreads, n_select);
            if (t == 0)                                                // the selected neighbours, farthest first
                for (uint32_t k = 0; k < n; ++k) { S.cn[k] = S.top_i[0]; heap_pop<true>(S.top_d, S.top_i, (int)(n - k)); }
            __syncthreads();
            uint32_t* q_nbr = nbr_ptr(a, q, level);                    // add_link(q, dst): the new node's list has room
            if (t < n) q_nbr[t] = S.cn[t];
            if (t == 0) *deg_ptr(a, q, level) = n;
            curr = S.cn[n - 1u];
            // add_link(dst, q), one wavefront each
            float* hd = S.arena_d + w * kWaveSlots;
            uint32_t* hi = S.arena_i + w * kWaveSlots;
            for (uint32_t j = w; j < n; j += kWaves) {
                const uint32_t dst = S.cn[j];
                uint32_t* dp = deg_ptr(a, dst, level);
                uint32_t* nb = nbr_ptr(a, dst, level);
                const uint32_t deg = min(*dp, cap);
                if (deg < cap) {
                    if (lane == 0) { nb[deg] = q; *dp = deg + 1u; }
                    continue;
                }
                float* ld = hd + kLinkMin;                             // (the candidates as a list, where the min-heap will be)
                uint32_t* li = hi + kLinkMin;
                wave_sync_mem();
                for (uint32_t k = lane; k <= deg; k += 64u) li[k] = k ? nb[k - 1u] : q;
                wave_sync_mem();
                dist_many(a, row_of(a, dst), li, ld, deg + 1u, lane, 64u);
                wave_sync_mem();
                if (lane == 0) {
                    for (uint32_t k = 0; k <= deg; ++k) heap_push_at<true>(hd, hi, (int)k, 0, ld[k], li[k]);
                    n_reverse += deg + 1u;
                    ++n_rewritten;
                }
                uint32_t m = deg + 1u;
                heuristic<false>(a, hd, hi, m, cap, hd + kLinkMin, hi + kLinkMin, hd + kLinkKept, hi + kLinkKept, lane, 64u, n_reverse);
                if (lane == 0) {
                    for (uint32_t k = 0; k < m; ++k) { nb[k] = hi[0]; heap_pop<true>(hd, hi, (int)(m - k)); }
                    *dp = m;
                }
                wave_sync_mem();
            }
            __syncthreads();
            if (level == 0u) break;
        }
        if (ql > max_level) { max_level = ql; init_node = q; }
    }
    __syncthreads();
    if (t == 0) {
        a.state[0] = init_node; a.state[1] = max_level; a.state[2] = tok;
        if (n_search) atomicAdd(&a.counters[0], n_search);
        if (n_select) atomicAdd(&a.counters[1], n_select);
    }
    if (lane == 0) {
        if (n_reverse) atomicAdd(&a.counters[2], n_reverse);
        if (n_rewritten) atomicAdd(&a.counters[3], n_rewritten);
    }
}

// ---- libstdc++'s std::sort (bits/stl_algo.h) over (d, id) under `<` on the distance, by one lane.  The bounds on the unguarded scans never
// bind on distances that order; they keep a list with a NaN inside its array (its order is not pinned).
__device__ __forceinline__ void swap_at(float* d, uint32_t* id, int x, int y) {
    const float td = d[x]; const uint32_t ti = id[x];
    d[x] = d[y]; id[x] = id[y]; d[y] = td; id[y] = ti;
}
__device__ __forceinline__ void linear_insert(float* d, uint32_t* id, int last, int lo) {   // __unguarded_linear_insert
    const float vd = d[last]; const uint32_t vi = id[last];
    int next = last - 1;
    while (next >= lo && vd < d[next]) { d[last] = d[next]; id[last] = id[next]; last = next; --next; }
    d[last] = vd; id[last] = vi;
}
__device__ __forceinline__ void insertion_sort(float* d, uint32_t* id, int first, int last) {   // __insertion_sort
    for (int i = first + 1; i < last; ++i) {
        if (d[i] < d[first]) {
            const float vd = d[i]; const uint32_t vi = id[i];
            for (int k = i; k > first; --k) { d[k] = d[k - 1]; id[k] = id[k - 1]; }
            d[first] = vd; id[first] = vi;
        } else linear_insert(d, id, i, first);
    }
}
__device__ void std_sort(float* d, uint32_t* id, int n) {
    if (n < 2) return;
    int depth = 2 * (31 - __clz(n));
    int st_f[48], st_l[48], st_d[48], sp = 0;                          // (the ranges of the recursion are disjoint: their order is free)
    st_f[0] = 0; st_l[0] = n; st_d[0] = depth; sp = 1;
    while (sp > 0) {
        --sp;
        const int first = st_f[sp];
        int last = st_l[sp], dep = st_d[sp];
        while (last - first > 16) {
            if (dep == 0) {                                            // __partial_sort(first, last, last): make_heap, sort_heap
                const int len = last - first;
                for (int parent = (len - 2) / 2; parent >= 0; --parent) heap_adjust<true>(d + first, id + first, parent, len, d[first + parent], id[first + parent]);
                for (int m = len; m > 1; --m) heap_pop<true>(d + first, id + first, m);
                break;
            }
            --dep;
            const int mid = first + (last - first) / 2, x = first + 1, z = last - 1;   // __move_median_to_first(first, x, mid, z)
            if (d[x] < d[mid]) {
                if (d[mid] < d[z]) swap_at(d, id, first, mid);
                else if (d[x] < d[z]) swap_at(d, id, first, z);
                else swap_at(d, id, first, x);
            } else if (d[x] < d[z]) swap_at(d, id, first, x);
            else if (d[mid] < d[z]) swap_at(d, id, first, z);
            else swap_at(d, id, first, mid);
            int lo = first + 1, hi = last;                             // __unguarded_partition(first + 1, last, first)
            const float pv = d[first];
            for (;;) {
                while (lo < last && d[lo] < pv) ++lo;
                --hi;
                while (hi > first && pv < d[hi]) --hi;
                if (!(lo < hi)) break;
                swap_at(d, id, lo, hi);
                ++lo;
            }
            if (sp < 48) { st_f[sp] = lo; st_l[sp] = last; st_d[sp] = dep; ++sp; }
            last = lo;
        }
    }
    if (n > 16) {                                                      // __final_insertion_sort
        insertion_sort(d, id, 0, 16);
        for (int i = 16; i < n; ++i) linear_insert(d, id, i, 0);
    } else insertion_sort(d, id, 0, n);
}

__global__ void __launch_bounds__(64) k19_sort_neighbours(TrainArgs a) {
    __shared__ float sd[kHnswLdsDegree];
    __shared__ uint32_t si[kHnswLdsDegree], so[kHnswLdsDegree];
    const uint32_t lane = threadIdx.x;
    unsigned long long n_rank = 0, n_replay = 0;
    for (uint32_t node = blockIdx.x; node < a.num_node; node += gridDim.x) {
        const Row r = row_of(a, node);
        const uint32_t top = min(a.level[node], a.l1_levels);
        for (uint32_t level = 0; level <= top; ++level) {
            const uint32_t deg = min(*deg_ptr(a, node, level), level ? a.maxM : a.maxM0);
            if (deg == 0u) break;                                      // the reference returns: the node's higher levels stay as they are
            uint32_t* nb = nbr_ptr(a, node, level);
            wave_sync_mem();
            for (uint32_t k = lane; k < deg; k += 64u) si[k] = nb[k];
            wave_sync_mem();
            dist_many(a, r, si, sd, deg, lane, 64u);
            wave_sync_mem();
            bool tie = false;
            for (uint32_t k = lane; k < deg; k += 64u) {
                const float d = sd[k];
                uint32_t rank = 0;
                if (d != d) tie = true;
                for (uint32_t j = 0; j < deg; ++j) {
                    const float e = sd[j];
                    if (e < d) ++rank;
                    else if (e == d && j != k) tie = true;
                }
                so[k] = rank;
            }
            if (__ballot(tie) != 0ull) {
                if (lane == 0) { std_sort(sd, si, (int)deg); ++n_replay; }
                wave_sync_mem();
                for (uint32_t k = lane; k < deg; k += 64u) nb[k] = si[k];
            } else {
                for (uint32_t k = lane; k < deg; k += 64u) nb[so[k]] = si[k];
                if (lane == 0) ++n_rank;
            }
        }
    }
    if (lane == 0) {
        if (n_rank) atomicAdd(&a.counters[4], n_rank);
        if (n_replay) atomicAdd(&a.counters[5], n_replay);
    }
}

__global__ void __launch_bounds__(256)
k19_check_csr(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const float* __restrict__ val, uint32_t rows, uint32_t cols, uint64_t nnz,
              uint32_t* __restrict__ flags) {
    const uint32_t f = check_csr_rows(ptr, idx, val, rows, cols, nnz);
    if (f) atomicOr(flags, f);
}
__global__ void __launch_bounds__(256) k19_check_drm(const float* __restrict__ val, uint32_t rows, uint32_t cols, uint64_t stride, uint32_t* __restrict__ flags) {
    const uint32_t f = check_drm_rows(val, rows, cols, stride);
    if (f) atomicOr(flags, f);
}

}  // namespace

std::vector<uint32_t> hnsw_level_plan(uint32_t n, uint32_t M, int max_level_upper_bound) {
    std::vector<uint32_t> level(n);
    const float mult_l = 1.0 / log(1.0 * M);
    std::mt19937 rng(0);                                               // random_number_generator<>'s default seed
    for (uint32_t i = 0; i < n; ++i) {
        level[i] = (uint32_t)(-log(std::uniform_real_distribution<double>(0.0, 1.0)(rng)) * mult_l);
        if (max_level_upper_bound >= 0) level[i] = std::min<uint32_t>(level[i], (uint32_t)max_level_upper_bound);
    }
    return level;
}

uint32_t hnsw_check_items(const QueriesDev& X, uint64_t x_stride, hipStream_t s) {
    DevBuf flags;
    flags.reserve(4);
    XRL_HIP(hipMemsetAsync(flags.p, 0, 4, s));
    if (X.dense) {
        const uint64_t n = (uint64_t)X.rows * X.cols;
        if (n) hipLaunchKernelGGL(k19_check_drm, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, s, X.val, X.rows, X.cols, x_stride, flags.as<uint32_t>());
    } else {
        hipLaunchKernelGGL(k19_check_csr, dim3((uint32_t)std::min<uint64_t>(((uint64_t)X.rows + 255) / 256, 4096)), dim3(256), 0, s, X.row_ptr, X.col_idx, X.val, X.rows, X.cols,
                           X.nnz, flags.as<uint32_t>());
    }
    XRL_LAUNCH_CHECK();
    uint32_t f = 0;
    XRL_HIP(hipMemcpyAsync(&f, flags.p, 4, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    return f;
}

void hnsw_train(HnswIndex& ix, const std::vector<uint32_t>& levels, hipStream_t s, HnswTrainCounters& c) {
    HnswDev& d = ix.d;
    const uint32_t N = d.num_node;
    d.l1_levels = *std::max_element(levels.begin(), levels.end());
    const size_t n0 = (size_t)N * d.maxM0, n1d = (size_t)N * d.l1_levels, n1 = n1d * d.maxM;
    ix.l0_deg.reserve((size_t)N * 4); ix.l0_nbr.reserve(n0 * 4); ix.l1_deg.reserve(n1d * 4); ix.l1_nbr.reserve(n1 * 4);
    XRL_HIP(hipMemsetAsync(ix.l0_deg.p, 0, (size_t)N * 4, s));
    XRL_HIP(hipMemsetAsync(ix.l0_nbr.p, 0, n0 * 4, s));
    if (n1d) XRL_HIP(hipMemsetAsync(ix.l1_deg.p, 0, n1d * 4, s));
    if (n1) XRL_HIP(hipMemsetAsync(ix.l1_nbr.p, 0, n1 * 4, s));
    DevBuf level, visited, work, cand_d, cand_i;                       // work: the three words of state, a pad, the six counters
    level.reserve((size_t)N * 4); visited.reserve((size_t)N * 4); work.reserve(16 + 6 * 8);
    XRL_HIP(hipMemcpyAsync(level.p, levels.data(), (size_t)N * 4, hipMemcpyHostToDevice, s));
    XRL_HIP(hipMemsetAsync(visited.p, 0, (size_t)N * 4, s));
    XRL_HIP(hipMemsetAsync(work.p, 0, 16 + 6 * 8, s));
    TrainArgs a{};
    a.num_node = N; a.feat_dim = d.feat_dim; a.maxM = d.maxM; a.maxM0 = d.maxM0; a.efC = ix.efC; a.l1_levels = d.l1_levels; a.dense = d.dense; a.l2 = d.l2;
    a.l0_deg = ix.l0_deg.as<uint32_t>(); a.l0_nbr = ix.l0_nbr.as<uint32_t>(); a.l1_deg = ix.l1_deg.as<uint32_t>(); a.l1_nbr = ix.l1_nbr.as<uint32_t>();
    a.feat = d.feat; a.row_ptr = d.row_ptr; a.idx = d.idx; a.val = d.val;
    if (!d.dense) XRL_HIP(hipMemcpyAsync(&a.nnz, d.row_ptr + N, 8, hipMemcpyDeviceToHost, s));
    a.level = level.as<uint32_t>(); a.state = work.as<uint32_t>(); a.visited = visited.as<uint32_t>();
    a.counters = reinterpret_cast<unsigned long long*>(work.as<char>() + 16);
    if (N > kHnswTrainCandLds) {
        cand_d.reserve((size_t)N * 4); cand_i.reserve((size_t)N * 4);
        a.cand_d = cand_d.as<float>(); a.cand_i = cand_i.as<uint32_t>();
    }
    XRL_HIP(hipStreamSynchronize(s));                                  // (nnz has arrived; the level plan may leave the host)
    for (uint32_t first = 0; first < N; first += kHnswTrainRun) {      // insertions are serial: one workgroup, one bounded run per launch
        a.first = first; a.last = std::min<uint64_t>((uint64_t)first + kHnswTrainRun, N);
        hipLaunchKernelGGL(k19_insert, dim3(1), dim3(kThreads), 0, s, a);
        XRL_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k19_sort_neighbours, dim3(std::min<uint32_t>(N, 4096)), dim3(64), 0, s, a);
    XRL_LAUNCH_CHECK();
    struct { uint32_t state[4]; unsigned long long ctr[6]; } h{};
    XRL_HIP(hipMemcpyAsync(&h, work.p, sizeof(h), hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    d.init_node = h.state[0]; d.max_level = h.state[1];
    d.l0_deg = a.l0_deg; d.l0_nbr = a.l0_nbr; d.l1_deg = a.l1_deg; d.l1_nbr = a.l1_nbr;
    ix.bytes += 4ull * ((uint64_t)N + n0 + n1d + n1);
    c.dist_search += h.ctr[0]; c.dist_select += h.ctr[1]; c.dist_reverse += h.ctr[2]; c.rewritten += h.ctr[3]; c.sort_rank += h.ctr[4]; c.sort_replay += h.ctr[5];
}

}  // namespace xrl
