// HNSW graph construction in HBM (K19, xrl_hnsw_train.hip): the reference's HNSW::train at threads = 1 (hnsw.hpp:555-846) over items that are
// already the index's own arrays.  One workgroup inserts the nodes one after the other (k19_insert, a bounded run of nodes per launch), then one
// wavefront per node sorts its neighbour lists (k19_sort_neighbours).  DESIGN.md section 9 has the contract.
#pragma once
#include <vector>

#include "xrl_hnsw.h"

namespace xrl {

constexpr uint32_t kHnswTrainMaxM = 128;      // maxM0 = 2 M <= kHnswLdsDegree: a neighbourhood and a reverse link's candidates are staged in LDS
constexpr uint32_t kHnswTrainRun = 256;       // nodes inserted by one launch of k19_insert: a first guess, nothing was tuned
constexpr uint32_t kHnswTrainCandLds = 4096;  // the cand heap of a search holds a node at most once: up to this many nodes it lives in LDS, above in HBM
constexpr uint32_t kHnswTrainRowLds = 2048;   // floats of a staged query row (dense), or half as many stored entries (sparse); a longer row is read from HBM

// distance evaluations of the searches and descents, of the heuristic over a search's result, of the reverse links; neighbour lists rewritten by a
// reverse link; lists sorted by the parallel rank form, by the replay of libstdc++'s std::sort
struct HnswTrainCounters { uint64_t dist_search = 0, dist_select = 0, dist_reverse = 0, rewritten = 0, sort_rank = 0, sort_replay = 0; };

// The level of every node as the reference's train draws them (mt19937 seeded 0, the host's log), capped by max_level_upper_bound >= 0.
std::vector<uint32_t> hnsw_level_plan(uint32_t n, uint32_t M, int max_level_upper_bound);

// Flags (xrl_ann_device.h) of the check kernels K17 runs on its queries, here on the items about to be trained; synchronises s.
uint32_t hnsw_check_items(const QueriesDev& X, uint64_t x_stride, hipStream_t s);

// ix holds the items (d.feat, or d.row_ptr / d.idx / d.val), num_node, feat_dim, dense, l2 and maxM / maxM0; this allocates the graph arrays,
// builds them, and sets max_level, init_node and l1_levels.  Synchronises s.
void hnsw_train(HnswIndex& ix, const std::vector<uint32_t>& levels, hipStream_t s, HnswTrainCounters& c);

}  // namespace xrl
