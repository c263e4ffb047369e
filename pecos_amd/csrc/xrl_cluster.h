// K11 (xrl_cluster.hip) and its host plan (xrl_cluster_plan.cpp): the balanced hierarchical 2-means of the reference (Tree::run_clustering,
// pecos/core/utils/clustering.hpp:403-503) on the device, with the reference's answer for threads = 1 -- the rule is stated in
// include/xrl_abi.h at xrl_run_clustering_device.
#pragma once
#include "../../include/xrl_abi.h"
#include "xrl_kernels.h"

namespace xrl {

constexpr uint32_t kClusterNoSwitch = 0xFFFFFFFFu;
// a run (node, feature) of this many entries or more is one wavefront's chain; shorter runs are served one per lane
constexpr uint32_t kClusterWaveRun = 64;

// Everything random in a clustering is independent of the data: the plan holds it, level by level.  Positions index `elements`.
struct ClusterLevel {
    bool sampled = false;            // rate < 1: the nodes shuffle their ranges and work on a prefix
    bool first_touch = false;        // the SKMEANS norm walks the features in the order of first touch (the reference's sdvec mode)
    std::vector<uint32_t> beg;       // [nodes + 1]: node i of the level owns the positions [beg[i], beg[i + 1])
    std::vector<uint32_t> work_end;  // [nodes]: the node works on [beg[i], work_end[i])
    std::vector<uint32_t> r_pos, l_pos;   // [nodes]: the two positions whose difference is the first centre (max_iter > 0)
    std::vector<uint32_t> perm;      // sampled: [rows], elements'[p] = elements[perm[p]]
};

struct ClusterPlan {
    uint32_t rows = 0, depth = 0;
    uint32_t switch_level = kClusterNoSwitch;   // the first level in first-touch mode
    std::vector<uint32_t> node_seed;            // [2^(depth + 1)], by node id
    std::vector<ClusterLevel> levels;
    std::vector<uint32_t> leaf_beg;             // [2^depth + 1]
};

// Checks the arguments that need no data (messages start with `what`) and draws the plan.  nnz: stored entries (rows * cols for a
// dense matrix).
ClusterPlan make_cluster_plan(const char* what, uint64_t rows, uint64_t cols, uint64_t nnz, uint64_t depth, const ClusteringParam* param);

struct ClusterForms {
    uint64_t lane_runs = 0, wave_runs = 0, seg_sorts = 0;
    uint32_t switch_level = kClusterNoSwitch;
    std::vector<uint32_t> iters;                // per level
};

// X: a CSR view in HBM.  d_codes [rows], d_scores nullptr or [depth * rows].  Enqueues on s and synchronises it at least once per
// iteration.  Fails on a row whose column ids are not strictly ascending or reach X.cols.
void cluster_device(const char* what, const QueriesDev& X, const ClusterPlan& plan, const ClusteringParam& param, uint32_t* d_codes, float* d_scores,
                    hipStream_t s, ClusterForms& forms);

}  // namespace xrl
