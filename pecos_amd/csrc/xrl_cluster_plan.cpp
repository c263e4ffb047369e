// The host plan of a clustering (K11): node seeds, ranges, sample counts, shuffles and the first centres' two rows, none of which depends
// on the feature values.  Drawn with std::mt19937, std::uniform_int_distribution and std::shuffle, as the reference draws them
// (pecos/core/utils/random.hpp:24-43, clustering.hpp:195-199, 307-308, 411-414): the draws are those of the reference compiled with the
// same C++ standard library.
#include <algorithm>
#include <numeric>
#include <random>

#include "xrl_cluster.h"

namespace xrl {

ClusterPlan make_cluster_plan(const char* what_c, uint64_t rows, uint64_t cols, uint64_t nnz, uint64_t depth, const ClusteringParam* param) {
    const std::string what = std::string(what_c) + ": ";
    if (!param) fail(what + "null ClusteringParam");
    const ClusteringParam& P = *param;
    if (P.partition_algo != 0 && P.partition_algo != 5) fail(what + "partition_algo must be 0 (KMEANS) or 5 (SKMEANS), got " + std::to_string(P.partition_algo));
    // the reference's three invalid_argument cases and its fourth, on the warm-up (clustering.hpp:59-70)
    if (!(P.min_sample_rate > 0 && P.min_sample_rate <= 1)) fail(what + "expect 0 < min_sample_rate <= 1.0");
    if (!(P.max_sample_rate > 0 && P.max_sample_rate <= 1)) fail(what + "expect 0 < max_sample_rate <= 1.0");
    if (P.min_sample_rate > P.max_sample_rate) fail(what + "expect min_sample_rate <= max_sample_rate");
    if (!(P.warmup_ratio >= 0 && P.warmup_ratio <= 1)) fail(what + "expect 0 <= warmup_ratio <= 1.0");
    if (depth > 30) fail(what + "depth " + std::to_string(depth) + " is above 30");
    if (rows > 0xFFFFFFF0ull) fail(what + "too many rows");
    if ((1ull << depth) > rows) fail(what + "2^depth = " + std::to_string(1ull << depth) + " leaves need at least as many rows, got " + std::to_string(rows));

    ClusterPlan plan;
    plan.rows = (uint32_t)rows; plan.depth = (uint32_t)depth;
    std::mt19937 seeds((unsigned)P.seed);
    plan.node_seed.resize((size_t)2 << depth);
    for (uint32_t& v : plan.node_seed) v = std::uniform_int_distribution<unsigned>(0, std::numeric_limits<unsigned>::max())(seeds);

    const size_t warmup_layers = size_t(depth * P.warmup_ratio);
    std::vector<uint32_t> beg{0u, (uint32_t)rows};
    bool first_touch = false;
    std::vector<size_t> iota;
    for (uint32_t d = 0; d < depth; ++d) {
        const uint32_t nodes = 1u << d;
        ClusterLevel lv;
        // the level's rate, in float as the reference writes it (clustering.hpp:160-167)
        float rate = P.min_sample_rate;
        if (d >= warmup_layers) rate = P.min_sample_rate + (P.max_sample_rate - P.min_sample_rate) * (d + 1 - warmup_layers) / (depth - warmup_layers);
        lv.sampled = rate < 1.0;
        if (double(nnz) / (double(nodes) * double(cols)) < 1) first_touch = true;      // clustering.hpp:434-436: it never switches back
        if (first_touch && plan.switch_level == kClusterNoSwitch) plan.switch_level = d;
        lv.first_touch = first_touch;
        lv.beg = beg;
        lv.work_end.resize(nodes);
        if (P.kmeans_max_iter) { lv.r_pos.resize(nodes); lv.l_pos.resize(nodes); }
        if (lv.sampled) { lv.perm.resize(rows); std::iota(lv.perm.begin(), lv.perm.end(), 0u); }
        for (uint32_t i = 0; i < nodes; ++i) {
            std::mt19937 rng(plan.node_seed[nodes + i]);
            const size_t b = beg[i], size = beg[i + 1] - beg[i];
            size_t n = size;
            if (lv.sampled) {
                iota.resize(size);
                std::iota(iota.begin(), iota.end(), b);
                std::shuffle(iota.begin(), iota.end(), rng);
                std::copy(iota.begin(), iota.end(), lv.perm.begin() + b);
                n = size_t(rate * size);
                if (n < 2) fail(what + "level " + std::to_string(d) + " samples " + std::to_string(n) + " of a node's " + std::to_string(size) +
                                " elements; a node needs 2 to draw its first centre");
            }
            lv.work_end[i] = (uint32_t)(b + n);
            if (P.kmeans_max_iter) {
                const size_t r = std::uniform_int_distribution<size_t>(0, n - 1)(rng);
                const size_t l = (r + std::uniform_int_distribution<size_t>(1, n - 1)(rng)) % n;
                lv.r_pos[i] = (uint32_t)(b + r); lv.l_pos[i] = (uint32_t)(b + l);
            }
        }
        plan.levels.push_back(std::move(lv));
        std::vector<uint32_t> next(2 * (size_t)nodes + 1);
        for (uint32_t i = 0; i < nodes; ++i) { next[2 * i] = beg[i]; next[2 * i + 1] = (uint32_t)(((uint64_t)beg[i] + beg[i + 1]) >> 1); }
        next[2 * nodes] = (uint32_t)rows;
        beg.swap(next);
    }
    plan.leaf_beg = beg;
    return plan;
}

}  // namespace xrl
