// PairwiseANN in HBM (K18, xrl_pairwise.hip): the reference's pecos::ann::PairwiseANN (ann/pairwise.hpp) over a resident X_trn and Y_csc.
// One wavefront per (query row, label key) pair: an exact scan of the label's column, the `only_topk` nearest kept as the reference's heap
// keeps them.  DESIGN.md section 9 has the contract and the three forms.
#pragma once
#include <atomic>

#include "xrl_common.h"
#include "xrl_predict.h"

namespace xrl {

constexpr uint32_t kPairCap = 1024;          // CAP: a column of up to CAP entries is sorted (and, if need be, replayed) in LDS
constexpr uint32_t kPairKeep = 512;          // KEEP: the stream form keeps the best KEEP keys and merges CAP - KEEP new ones per sort
constexpr uint32_t kPairQueryLds = 1024;     // a dense query of up to this many floats, a sparse one of up to half as many entries, is staged in LDS
constexpr uint32_t kPairMaxSlots = 2048;     // wavefronts (= slots) of one launch
constexpr uint64_t kPairSlotBudget = 1ull << 30;   // bytes of per-slot HBM scratch (12 per entry of the longest column) a searchers handle may hold

// the index as the kernel reads it
struct PairDev {
    uint32_t num_input, num_label, feat_dim, max_col;    // max_col: the longest column of Y
    int dense;
    const uint64_t* y_ptr; const uint32_t* y_idx; const float* y_val;      // Y_csc: [num_label + 1], row ids and values in stored order
    const float* feat;                                                      // dense X_trn: [num_input * feat_dim]
    const uint64_t* row_ptr; const uint32_t* idx; const float* val;        // sparse X_trn as a CSR
};

struct PairIndex {
    int device = 0;
    PairDev d{};
    uint64_t nnz_y = 0, nnz_x = 0;
    DevBuf y_ptr, y_idx, y_val, feat, row_ptr, idx, val;
};

// device scratch of `slots` wavefronts, for ONE call at a time (a second call that finds them in use is refused, never queued)
struct PairSearchers {
    const void* owner = nullptr;
    std::atomic<bool> busy{false};
    int device = 0;
    uint32_t slots = 0, col_cap = 0;           // col_cap: entries of scratch per slot (0: the index has no column above CAP)
    DevBuf scratch;                            // per slot: float dist[col_cap], float heap_d[col_cap], u32 heap_i[col_cap]
    DevBuf work;                               // next, check flags, counters
};

struct PairCounters { uint64_t sorted = 0, stream = 0, replay = 0, dist = 0, second_pass = 0, max_col = 0; };

// What a build found wrong, as kBad* flags of xrl_ann_device.h plus these
enum : uint32_t { kPairBadYRow = 16u, kPairBadYPtr = 32u, kPairBadLabel = 64u };

// After the arrays of ix are in HBM: checks X_trn and Y_csc on the device, finds the longest column.  Returns the flags (0: fine).  Synchronises s.
uint32_t pairwise_check_index(PairIndex& ix, hipStream_t s);
// The message of the first flag set; `what` is the entry point's prefix, `of` names the matrix ("X_trn" / "the queries")
std::string pairwise_refusal(const std::string& what, uint32_t flags, const PairIndex& ix, const char* of);

void pairwise_searchers_reserve(PairSearchers& sc, const PairIndex& ix, uint32_t slots);
uint32_t pairwise_default_slots(const PairIndex& ix, uint32_t pairs);

// Pair b: query row (same_input ? 0 : b) of Q against column keys[b]; writes its min(n, only_topk) entries at b * out_stride in the four outputs
// (Imat row id, Mmat 1, Dmat distance, Vmat the Y value) and leaves the rest untouched.  Checks Q and the keys on the device first; a refusal
// leaves the outputs unchanged.  One synchronisation of s, at the end.
void pairwise_search(const char* name, const PairIndex& ix, const QueriesDev& Q, uint64_t q_stride, const uint32_t* d_keys, uint32_t pairs, uint32_t only_topk,
                     bool same_input, uint32_t* d_I, uint32_t* d_M, float* d_D, float* d_V, uint64_t out_stride, PairSearchers* sc, hipStream_t s, PairCounters& c);

}  // namespace xrl
