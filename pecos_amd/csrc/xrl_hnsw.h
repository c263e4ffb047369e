// HNSW search in HBM (K17, xrl_hnsw.hip): a folder saved by the reference's HNSW.save, split into arrays that suit the GPU, and the
// reference's predict_single / search_level (hnsw.hpp:850-971) run by one wavefront per query.  DESIGN.md section 9 has the contract.
#pragma once
#include <atomic>

#include "xrl_common.h"
#include "xrl_predict.h"

namespace xrl {

constexpr uint32_t kHnswCap = 1024;          // CAP: the topk heap of efS' <= CAP lives in LDS (CAP + 1 entries of 8 bytes), a larger one in HBM scratch
constexpr uint32_t kHnswCandCap = 4096;      // default capacity of a slot's cand heap; a query that overflows it runs again with num_node entries
constexpr uint32_t kHnswLdsDegree = 256;     // a neighbourhood of up to this many nodes is staged in LDS, a larger one in HBM scratch
constexpr uint32_t kHnswMaxSlots = 2048;     // wavefronts (= slots) of one launch
constexpr uint64_t kHnswSlotBudget = 1ull << 30;   // bytes of per-slot scratch a launch may hold

// the index as the kernel reads it
struct HnswDev {
    uint32_t num_node, feat_dim, maxM, maxM0, max_level, init_node, l1_levels;
    int dense, l2;
    const uint32_t* l0_deg;  const uint32_t* l0_nbr;     // [num_node], [num_node * maxM0]
    const uint32_t* l1_deg;  const uint32_t* l1_nbr;     // [num_node * l1_levels], [num_node * l1_levels * maxM]; level l is column l - 1
    const float* feat;                                   // dense: [num_node * feat_dim]
    const uint64_t* row_ptr; const uint32_t* idx; const float* val;   // sparse: the items as a CSR
};

struct HnswIndex {
    int device = 0;
    HnswDev d{};
    uint32_t efC = 0;
    uint64_t bytes = 0;
    DevBuf l0_deg, l0_nbr, l1_deg, l1_nbr, feat, row_ptr, idx, val;
};

// device scratch of `slots` wavefronts, for ONE call at a time (a second call that finds them in use is refused, never queued): the visited marks (clean: every mark differs from the slot's next token), the cand heaps, and what
// the larger forms need
struct HnswSearchers {
    const void* owner = nullptr;               // the index they were made for; no other is served
    std::atomic<bool> busy{false};             // one call at a time: a call regrows and reuses work / top / nbr, and its kernels read them until its last synchronisation
    int device = 0;
    uint32_t slots = 0, num_node = 0;
    DevBuf visited, token;                     // u32 [slots * num_node], u32 [slots]
    DevBuf cand_d, cand_i; uint32_t cand_cap = 0;
    DevBuf top_d, top_i; uint32_t top_cap = 0;     // HBM form of the topk heap, entries per slot
    DevBuf nbr_d, nbr_i; uint32_t nbr_cap = 0;     // neighbourhoods above kHnswLdsDegree
    DevBuf work;                               // next, n_redo, check flags, counters, the redo list
};

struct HnswCounters { uint64_t dist = 0, pops = 0, admissions = 0, passes = 0, max_cand = 0, rerun = 0, lds_queries = 0, hbm_queries = 0; };

// Queries X (dense with row stride x_stride, or a CSR) against the index; row r writes its count[r] <= topk entries at r * out_stride and leaves
// the rest untouched.  Checks X on the device first (name: the entry point, for the refusals); a refused X leaves the outputs unchanged.
// One synchronisation of `s`, at the end.  sc: the caller's searchers, or null (scratch of this call).
void hnsw_search(const char* name, const HnswIndex& ix, const QueriesDev& X, uint64_t x_stride, uint32_t efS, uint32_t topk, uint32_t* d_idx, float* d_dist,
                 uint32_t* d_count, uint64_t out_stride, HnswSearchers* sc, hipStream_t s, HnswCounters& c);
void hnsw_searchers_reserve(HnswSearchers& sc, const HnswIndex& ix, uint32_t slots, hipStream_t s);   // the marks are cleared on s
uint32_t hnsw_default_slots(const HnswIndex& ix, uint32_t rows);

}  // namespace xrl
