// Launch interface of the HIP kernels (the xrl_*.hip units).  All pointers are device pointers.
#pragma once
#include "xrl_model.h"

namespace xrl {

// Device-resident query matrix (CSR with 32-bit offsets relative to the matrix, or dense row-major).
struct QueriesDev {
    const uint64_t* row_ptr;   // [rows+1] (CSR) or nullptr
    const uint32_t* col_idx;
    const float* val;          // CSR values, or the dense matrix
    uint32_t rows, cols;
    int dense;
    uint64_t nnz;              // CSR only
};

// Beam of the previous layer, fixed stride per query; idx == nullptr means the implicit root
// (one parent, id 0, score 1: HierarchicalMLModel::predict, inference.hpp:2462-2463).
struct BeamDev {
    uint32_t* idx;
    float* val;
    uint32_t* cnt;
    uint32_t stride;
};

struct K1Tune { int wpb = 1, lds_pad = 0, ablate = 0, k1g_variant = 0, pres_mode = 1, tile_rows = 1, k2_big_min_k = 0; };   // per-model tuning / debug knobs (xrl_set_option k1_wpb, k1_lds_pad, k1_ablate, k1g_variant, presence, tile_rows, k2_big_min_k), filled by make_plan (xrl_predict.cpp)

struct LayerPlan {
    uint32_t row0, nrows;       // query rows [row0, row0+nrows) of the query matrix
    uint32_t beam_in;           // max #parents per query entering the layer
    uint32_t k;                 // #survivors kept by this layer
    uint32_t cand_stride;       // floats reserved per query in `cand`
    PostProc pp;
    int first_layer;            // no combine (no_prev_pred)
    int implicit_root;          // previous beam is the implicit all-ones root
    int prune;                  // exact bound pruning allowed (option prune, and the layer not switched to unstaged by the pruning feedback)
    int bias_first;             // sparse X under weight_matrix_type HASH_CHUNKED: the bias row is applied BEFORE the query's features
                                // (chunk_ops<csr, hash>, inference.hpp:705-735); dense X is bias-first in every layout
    int layer;                  // index in the chain (profiling, feedback slot)
    K1Tune tune;
    uint32_t* fb_host = nullptr;  // pruning feedback (PruneFeedback::host), or nullptr
    uint32_t* fb_dev = nullptr;   // K1Q's sampled counters (PruneFeedback::dev)
};

// K0  prolongate: per query, offsets of every beam parent's child block + candidate count, and one
//     16-byte item descriptor per (query, beam slot, tile-in-parent) for K1.
void launch_k0_prolongate(const LayerDev& L, const LayerPlan& P, const QueriesDev& X, BeamDev prev, uint32_t* cand_off,
                          uint32_t* ncand, void* items, hipStream_t s, uint32_t item_ranks = 0xFFFFFFFFu /* beam slots that get item descriptors */);
// ---- Bound-pruned layers run in STAGES of beam slots (route_layer, xrl_predict.cpp).  What the stages hand to each other, per row batch
// (LaneWs::prune_done / x_ok / prune_cnt / rest_q):
//   done[q]     the top-k selected so far is final (exact bound, K2Args): FIRST writes it, MID skips on it and renews it, LAST skips on it
//   xok[q]      the per-query pruning guard (launch_xguard / K1Q's out_xok), read by whatever writes done
//   *n_items    the number of items launch_k0b_remaining compacted for the stage's sort and K1
//   rest_q      (nullptr: no list) the queries FIRST left unfinished, *rest_cnt of them in any order: whatever writes done in FIRST appends to it,
//               the launches of LAST walk it on small fixed grids instead of the batch
// Who zeroes *n_items: without a list launch_k0b_remaining does (a memset ahead of its kernel); with a list the CALLER zeroes it together with
// *rest_cnt before the first stage's launches (xrl_predict.cpp, "rest_list") -- the list's count has to be zero by then anyway.
struct StageLinks {
    uint32_t* done; const uint32_t* xok; uint32_t* n_items; uint32_t* rest_q; uint32_t* rest_cnt;
    void check(const char* who, bool writes_done) const {   // the one copy of what K2, K0b and K1T's selecting epilogue ask of them
        if (rest_q && !rest_cnt) fail(std::string(who) + ": the list of unfinished queries needs its count");
        if (!done || (writes_done && !xok)) fail(std::string(who) + ": bound pruning needs the done and the per-query guard flags");
    }
};
enum StageKind { STAGE_FIRST, STAGE_MID, STAGE_LAST };
struct Stage { StageKind kind; uint32_t slot_begin, slot_end /* its beam slots */; uint32_t cands /* FIRST, MID: cand_bound(slot_end), the most candidates K2 ranks */; StageLinks io; };
// a later stage's items: those of its beam slots of the queries with done[q] == 0 (list form: of the listed queries), compact; *io.n_items = their number
void launch_k0b_remaining(const LayerDev& L, const LayerPlan& P, const QueriesDev& X, BeamDev prev, const uint32_t* cand_off, const Stage& st, void* items, hipStream_t s);
bool k2_wave_path(const LayerPlan& P);   // the register top-k kernel serves this layer (what bound pruning needs)
size_t k0_item_bytes();
// K1  (query, tile) inner products + bias + post-processor + combine, one item per G lanes.
// list_grid > 0 (a compacted list, n_items != nullptr): a fixed grid of about this many workgroups walks the list (k1_list_kernel) where that form is
// compiled -- sparse queries, 16 or 32 lanes per item, post-processors of class 0 -- instead of a grid sized for n_slots.  Returns whether it ran.
bool launch_k1(const LayerDev& L, const LayerPlan& P, const QueriesDev& X, const void* items, const uint32_t* n_items,
               float* cand, int group, hipStream_t s, uint32_t list_grid = 0);
// one workgroup: exclusive scan of v[0, n) in place, v[n] = the total (xrl_devprim.hip); the caller checks the launch with its own
void launch_block_scan(uint32_t* v, uint32_t n, hipStream_t s);
// counting sort of the item descriptors by tile (LDS histograms, no global atomics); start[n_tiles] = #items
void launch_sort_items(const LayerDev& L, uint64_t n_slots, const void* items, void* sorted, uint32_t* H,
                       uint32_t* start, hipStream_t s,
                       const uint32_t* n_dev = nullptr);   // n_dev: device count of a compacted list (<= n_slots)
// counting sort of the QUERIES of a row batch by the best parent of their beam (slot 0), as a permutation: perm[slot] = query (K1Q's sorted launch)
void launch_sort_queries(BeamDev prev, uint32_t nrows, uint32_t n_keys, uint32_t* H, uint32_t* start, uint32_t* perm, hipStream_t s);
uint32_t qsort_max_keys();
size_t qsort_hist_bytes(uint32_t nrows, uint32_t n_keys);
void launch_step_marker(hipStream_t s);   // XRL_STEP_MARKER=1: an empty kernel at the start of every predict (step boundaries in kernel traces)
uint32_t sort_max_tiles();
size_t sort_hist_bytes(uint64_t n_slots, uint32_t n_tiles);
// K2  per-query top-k with (value desc, position asc) order; maps positions to original child ids.  The whole candidate row:
void launch_k2_topk(const LayerDev& L, const LayerPlan& P, BeamDev prev, const uint32_t* cand_off,
                    const uint32_t* ncand, const float* cand, BeamDev out, hipStream_t s);
// ... and one stage of a bound-pruned layer (see K2Args).  FIRST: the candidates of the slots [0, slot_end) only, writes done, appends the unfinished
// queries to the list if there is one.  MID: the same, skipping the queries that are done and renewing their flags (never with a list).  LAST: every
// candidate of the queries that are not done -- with a list: of the listed queries, on a fixed grid.
void launch_k2_stage(const LayerDev& L, const LayerPlan& P, BeamDev prev, const uint32_t* cand_off,
                     const uint32_t* ncand, const float* cand, BeamDev out, const Stage& st, hipStream_t s);
// stats: sum over (query, parent) of the reference chunk's algorithmic bytes, and of candidates
constexpr int kStatsPerLayer = 8;   // [0] reference-chunk bytes, [1] candidates, [2] items, [3] probes, [4] matched rows, [5] their entries,
                                    // [6] tile columns over the items, [7] query features x tile columns over the items
void launch_stats(const LayerDev& L, const LayerPlan& P, const QueriesDev& X, BeamDev prev, const uint32_t* ncand, const void* items,
                  double* out8, hipStream_t s, uint64_t item_slots = 0 /* slots of `items` (0: rows x beam x tiles per parent) */);
// K3  sparse_inner_products (pecos/core/utils/matrix.hpp:1049-1060), 4 layout combos
void launch_k3_inner_products(const uint64_t* x_ptr, const uint32_t* x_idx, const float* x_val, int x_dense,
                              const uint64_t* w_ptr, const uint32_t* w_idx, const float* w_val, int w_dense,
                              uint32_t dim, uint64_t len, const uint32_t* rows, const uint32_t* cols,
                              float* out, hipStream_t s);

unsigned long long* k1_phase_buffer();
void k1_phase_read(unsigned long long out[8], bool reset);   // debug: per-phase cycle totals of K1
// K4  predict_on_selected_outputs: one layer of (query, node) pairs against CSC W
void launch_k4_selected(const uint64_t* col_ptr, const uint32_t* row_idx, const float* val, uint32_t w_rows, float bias,
                        const QueriesDev& X, const uint32_t* pair_q, const uint32_t* node, const uint32_t* ppos,
                        const uint64_t* prev_off, const float* prev_val, float* out_val, uint64_t n_pairs,
                        const PostProc& pp, int first_layer, hipStream_t s);
// K1G (xrl_k1g.hip): dense queries against a dense-format layer as a tiled, k-ordered SGEMM over tile-sorted items
uint32_t k1g_cols(const LayerDev& L);                 // 0: the layer cannot be served by K1G
void launch_k1g(const LayerDev& L, const LayerPlan& P, const QueriesDev& X, const void* items_sorted, const uint32_t* start,
                uint32_t* blk_start, const uint32_t* x_ok, float* cand, hipStream_t s);
void launch_xguard(const QueriesDev& X, uint32_t row0, uint32_t nrows, float wmax, uint32_t* ok, hipStream_t s);   // per query row (CSR or dense): finite and too small to overflow any accumulator (prune_guard_ok)
// K1C (xrl_pairs.hip): the CSC route of a layer (w_ops<csc_t>, inference.hpp:1081-1149) over the candidates K0 laid out
void launch_k1c_csc(const LayerDev& L, const uint64_t* col_ptr, const uint32_t* row_idx, const float* val, const LayerPlan& P,
                    const QueriesDev& X, BeamDev prev, const uint32_t* cand_off, const uint32_t* ncand, float* cand, hipStream_t s);
// [X_feat | X_emb] -> one CSR on the device (concat_model's query form, matcher.py:864-890)
void launch_concat_csr(const uint64_t* in_ptr, const uint32_t* in_idx, const float* in_val, const float* emb, uint32_t rows,
                       uint32_t sparse_cols, uint32_t dense_cols, int normalize_emb, uint64_t* out_ptr, uint32_t* out_idx, float* out_val, hipStream_t s);
// xrl_features.hip: the weighting half of the reference's TF-IDF vectorizer (tfidf.hpp:798-822) on a device CSR of term counts
void launch_tfidf_weight(const uint64_t* row_ptr, const uint32_t* col_idx, const float* count, const float* idf, uint32_t rows, uint32_t cols,
                         int binary, int sublinear_tf, int norm_p, float* out, hipStream_t s,
                         uint32_t seg_stride = 1, uint32_t seg_off = 0, uint32_t* err = nullptr);   // rows = segments of row_ptr; *err = 1 on a column id >= cols
int k1_auto_group(const LayerDev& L, const Layer& host, int dense);
// K1T (xrl_k1t.hip): K1 on the densely held tile rows (LayerDev::wt), accumulators in registers; launch_k1 routes to it when k1t_serves
bool k1t_serves(const LayerDev& L, const QueriesDev& X);
// `sel` (option leaf_fuse): the FIRST stage of a bound-pruned layer in ONE launch -- one item per query (beam slot 0, query order), and the
// kernel's epilogue does what launch_k2_stage would do on the row it has just computed: top-k, child ids, done[q] for every query (and the list);
// the candidate row is stored for the queries that are not done.  P is the whole layer's plan.  items == nullptr (beam_in <= 32):
// the launch derives its items from the beam itself and writes cand_off / ncand of the unfinished queries -- no launch_k0_prolongate before it.
struct K1TSelect { BeamDev prev, out; uint32_t* cand_off; uint32_t* ncand; StageLinks io; };
bool k1t_selects(const LayerDev& L, const LayerPlan& P, const QueriesDev& X);   // one tile per parent, 32 lanes per item, k <= kTopkExtractMaxK, a combining layer
void launch_k1t(const LayerDev& L, const LayerPlan& P, const QueriesDev& X, const void* items, const uint32_t* n_items, float* cand, hipStream_t s,
                const K1TSelect* sel = nullptr);
// K1Q (xrl_k1q.hip): a whole layer -- prolongate, chunk products against the DENSE row format, post-processor,
// combine, top-k, child re-ordering -- in one query-stationary kernel: previous beam in, next beam out.
uint32_t k1q_regs(const LayerDev& L, uint32_t beam_in, uint32_t k, bool dense_x);   // 0: the layer / beam / k cannot (or should not) be served by K1Q
// n consecutive dense-format layers in ONE launch (the beam stays in LDS between them); n <= 8
void launch_k1q(const LayerDev* const* Ls, const LayerPlan* Ps, int n, const QueriesDev& X, BeamDev prev, BeamDev out,
                hipStream_t s, float prune_wmax, uint32_t* out_xok = nullptr,
                const uint32_t* qperm = nullptr /* launch slot -> query (launch_sort_queries); every XCD then takes a contiguous range of slots */);
                // prune_wmax / out_xok: the bound-pruning guard (prune_guard_ok, xrl_device.h); out_xok[q] receives every query's flag
size_t k2_max_k();
// Which K2 form serves a launch: pure host arithmetic, launch_k2_topk / launch_k2_stage dispatch on its result (xrl_debug_k2_form exports it for the tests).
// stage: 0 = the whole candidate row in one launch; 1 = a stage of the bound pruning on the batch-sized grid (rank-limited, sets or skips on the
// done flags); 2 = its last stage on the list of unfinished queries.  limited_cands: the most candidates a rank-limited stage looks at (0: the row).
enum K2Form : int { K2_FORM_WAVE = 0, K2_FORM_LIST = 1, K2_FORM_REG = 2, K2_FORM_LDS = 3, K2_FORM_BIG = 4 };
struct K2Choice { K2Form form; uint32_t ns; };   // ns: candidate registers per lane of the wave / list form (0 otherwise)
K2Choice k2_form(uint32_t k, uint32_t cand_stride, int64_t big_min_k, int stage, uint32_t limited_cands);
// xrl_topk_big.hip: top-k sizes beyond k2_max_k() -- one segmented radix sort over the batch's candidate rows (no cap, like the reference's sorted_csr)
void launch_k2_topk_big(const LayerDev& L, const LayerPlan& P, BeamDev prev, const uint32_t* cand_off, const uint32_t* ncand, const float* cand,
                        uint32_t* out_idx, float* out_val, uint32_t* out_cnt, uint32_t out_stride, hipStream_t s);

// xrl_ensemble.hip, K6: the result rows of n_models predicts (xrl_predict_device's output form, idx / val row stride stride[m]) merged
// into one fixed-stride result like CsrEnsembler's average, rank_average, sigmoid_average, softmax_average and round_robin or
// Text2Text.predict's tail do on the host, each but finish with an optional cut (A.only_topk) like
// TransformerMatcher.ensemble_prediction's.  One kernel serves every mode.  The pointer tables travel to the kernel by value.
// Capacity: n_models <= 8, sum of the strides <= 1024 (one wavefront holds a row).
constexpr int kEnsembleMaxModels = 8;
constexpr uint32_t kEnsembleMaxTotal = 1024;
constexpr int kEnsembleWaves = 4;                // wavefronts (= rows) per workgroup of K6
// modes 0-2 are xrl_ensemble_device's; xrl_ensemble_methods_device serves 0, 2 and 3-5
enum { kEnsembleAverage = 0, kEnsembleFinish = 1, kEnsembleRankAverage = 2, kEnsembleSigmoidAverage = 3, kEnsembleSoftmaxAverage = 4,
       kEnsembleRoundRobin = 5 };
struct EnsembleArgs {
    const uint32_t* idx[kEnsembleMaxModels];
    const float* val[kEnsembleMaxModels];
    const uint32_t* cnt[kEnsembleMaxModels];      // row lengths; a length above the stride counts as the stride
    uint32_t stride[kEnsembleMaxModels];
    uint32_t n_models, rows;
    int mode;
    int has_threshold;                            // finish only
    float threshold;
    uint32_t only_topk;                           // finish: the cut after the threshold; every other mode: the cut of xrl_ensemble_methods_device; 0 = all
    uint32_t* out_idx;
    float* out_val;
    uint32_t* out_cnt;
    uint32_t out_stride;                          // >= the longest possible output row (the caller checks)
};
uint32_t ensemble_slots(uint32_t stride_sum);     // entries per lane (1, 2, 4, 8 or 16) of the instantiation that serves this total
// mm_scratch: one device uint32 (rank_average and round_robin only: the call's largest row length, reduced on `s` ahead of K6)
void launch_ensemble(const EnsembleArgs& A, uint32_t* mm_scratch, hipStream_t s);

// xrl_metrics.hip, K8: the sums behind precision / recall at 1 .. topk (smat_util.Metrics.generate) of one fixed-stride result against the true
// labels as a device CSR pattern.  One wavefront per block of R(rows) consecutive rows writes one partial; a one-workgroup kernel adds the
// partials in block order.  Capacity: stride, topk <= 1024 (one wavefront holds a row).
constexpr uint32_t kMetricsMax = 1024;
struct MetricsArgs {
    const uint32_t* idx; const float* val; const uint32_t* cnt;   // the result; a count above the stride counts as the stride
    uint32_t stride, rows, topk;
    const uint64_t* true_ptr; const uint32_t* true_idx;           // [rows + 1] absolute offsets into true_idx; ascending inside a row
    uint64_t* matched; double* recall_sum;                        // [topk] each
};
uint32_t metrics_rows_per_wave(uint32_t rows);    // R(rows) = 64 * max(1, ceil(rows / 262144)): at most 4096 wavefronts, a function of rows only
uint32_t metrics_waves(uint32_t rows);            // ceil(rows / R(rows))
size_t metrics_scratch_bytes(uint32_t rows, uint32_t topk);   // the partials: per wavefront u64 matched[topk], then per wavefront f64 recall_sum[topk]
void launch_metrics(const MetricsArgs& A, void* scratch, hipStream_t s);

// xrl_select_plan.hip, K7: predict_on_selected_outputs on the device. One launch plans the reference's tree walk for every row of a batch
// (per layer: the row's nodes in the walk's order, the position of every node's parent in the previous layer's list, the count), then one
// K4 launch per layer scores the planned slots.  Rows are fixed-stride like xrl_predict_device's results; capacity kSelectMaxStride labels.
constexpr uint32_t kSelectMaxStride = 1024;
constexpr uint32_t kSelectNone = 0xFFFFFFFFu;
enum { kSelectOk = 0, kSelectOutOfRange = 1, kSelectTwice = 2, kSelectNoParent = 3 };
struct SelectTreeLayer {                          // one layer of the tree, ORIGINAL node ids (Model::d_sel_tree holds `depth` of them)
    const uint32_t* parent;                       // [c_rows] the node's parent, kSelectNone = none (layer 0: anything not under the root)
    const uint32_t* crank;                        // [c_rows] the node's position inside its parent's column of C, in stored order
    uint32_t c_rows, pad;
};
struct SelectPlanArgs {
    const uint32_t* sel_idx; const uint32_t* sel_cnt;   // the caller's rows (all of them; sel_cnt may be null = sel_stride each)
    uint32_t sel_stride;
    uint32_t row0, nrows;                         // the batch: rows [row0, row0 + nrows) of the caller's arrays = rows [0, nrows) of the scratch
    uint32_t depth, nr_labels;
    const SelectTreeLayer* tree;
    // scratch, layer l at l * layer_elems (node, ppos: rows of sel_stride) / l * layer_rows (cnt)
    uint32_t* node; uint32_t* ppos; uint32_t* cnt; uint64_t layer_elems, layer_rows;
    uint32_t* out_idx; uint32_t* out_cnt; uint32_t out_stride;   // the caller's buffers (all rows): the last layer's nodes and counts
    unsigned long long* status;                   // (row << 32 | code) of the lowest bad row, atomicMin; starts as 0xFFFFFFFF << 32
};
void launch_select_plan(const SelectPlanArgs& A, hipStream_t s);
// K4 on the planned slots of one layer: slot i = (row i / sel_stride, position i % sel_stride), live below cnt[row]; 16 lanes per slot
struct SelectScoreArgs {
    const uint64_t* col_ptr; const uint32_t* row_idx; const float* val; uint32_t w_rows; float bias;   // W, CSC, original column ids
    const uint32_t* node; uint32_t node_stride;   // the layer's ordered nodes (batch row 0): scratch rows, or the caller's d_out_idx
    const uint32_t* ppos; const uint32_t* cnt;    // scratch (batch rows)
    const float* prev_val;                        // [nrows * sel_stride] the previous layer's values, null on layer 0
    float* out_val; uint32_t out_stride;          // (batch row 0) scratch rows, or the caller's d_out_val
    uint32_t row0, nrows, sel_stride;
};
void launch_k4_selected_dev(const SelectScoreArgs& A, const QueriesDev& X, const PostProc& pp, hipStream_t s);

}  // namespace xrl
