// Host orchestrator: per-layer K0 -> K1 -> K2 launches on one HIP stream, ping-pong beam
// buffers, no host synchronisation inside the layer loop (grid sizes depend only on shapes).
//
// Reference driver being restated: HierarchicalMLModel::predict (inference.hpp:2446-2488) calling
// MLModel::predict_internal (:2029-2080) per layer.
//
// predict_device is an outline: resolve_layers (k / beam / candidate stride per layer) -> PruneFeedback::begin_predict -> reserve_scratch
// (walks the routes once) -> per row batch and layer: route_layer DECIDES (a Route, nothing launched), one of launch_csc_layer /
// launch_k1g_layer / launch_k1q_group / launch_tile_layer / launch_constrained_layer LAUNCHES what it says (launch_batch): the launch functions decide
// nothing.  A new way to run a layer is a Route field + a branch there.  Bound-pruned layers run in the stages the Route lists: Batch::stage builds
// the descriptor (Stage, xrl_kernels.h) every launch of a stage takes.  Tile format: launch_tile_layer is launch_tile_unstaged, or launch_tile_first
// -> rest_form -> launch_tile_later per later stage; rest_form is the one decision taken while a batch is being enqueued (between two equivalent
// forms of the later stages, from the pruning feedback's item count) -- it launches nothing.
#include "xrl_predict.h"
#include "xrl_constrain.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace xrl {

size_t profile_slot(Model& m, const char* name, uint32_t layer) {
    for (size_t i = 0; i < m.profile.size(); ++i)
        if (m.profile[i].layer == layer && m.profile[i].name == name) return i;
    m.profile.push_back(ProfileSlot{name, layer});
    return m.profile.size() - 1;
}

namespace {

// dense-X SGEMM layers, bound pruning: beam slots whose children fill about one candidate register (64) are scored first -- never all of
// them (the second stage must keep at least one slot)
uint32_t k1g_first_slots(const Layer& L, uint32_t beam_in, int forced = 0) {
    if (forced > 0) return (uint32_t)std::max<int64_t>(1, std::min<int64_t>(beam_in > 1 ? (int64_t)beam_in - 1 : 1, forced));
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(beam_in > 1 ? beam_in - 1 : 1, 64 / std::max<uint64_t>(1, L.cand_bound(1))));
}

struct LayerShape { uint32_t k, beam_in, cand_stride; PostProc pp; };   // resolve_layers: what a layer keeps, takes in and may evaluate per query

// Every decision about how layers [l, last] run on a batch of a given size (route_layer); the launch functions read it and decide nothing.
enum RouteKind { ROUTE_CSC, ROUTE_K1G, ROUTE_K1Q, ROUTE_TILE, ROUTE_CONSTRAINED };
struct Route {
    RouteKind kind;
    size_t last;             // K1Q: last layer of the group that shares the launch (every other kind: the layer itself) ...
    bool sorted_last;        // ... and that layer runs on its own, on queries sorted by their best beam parent (option qsort)
    int mode;                // items K1 walks: 0 = natural order, 1 = tile-sorted, 3 = K1G's tiled SGEMM over tile-sorted items (dense X)
    int group;               // tile format: lanes per item
    bool pruned;             // K1G, tile format: exact bound pruning in stages of beam slots
    uint32_t J;              // ... slots [0, J) are the first stage (K1G unpruned: the whole beam)
    uint32_t stage_end[3]; int n_stage;   // pruned: stage s scores the slots [stage_end[s-1], stage_end[s])
    bool fuse, fuse_k0;      // tile format (option leaf_fuse): K1T selects the first stage's top-k itself / derives its items too
    bool sorts_rest;         // tile format (option sort_rest): the later stages run on tile-sorted items, unless the feedback's item count says too few
    bool compact_rest;       // tile format, two stages (option leaf_tail): the first stage lists the unfinished queries, the later stage's launches walk that list
};

// What the launch functions share: the predict's constants and the row batch in flight (begin_batch).
struct Batch {
    Model& m; const Model::Options& opt; const QueriesDev& X; const PredictOpts& o; const std::vector<LayerShape>& shape;
    BeamDev result{}; uint32_t beam_stride = 1;   // the caller's output buffers (row 0); stride of the lanes' ping-pong beams
    bool has_init = false, csc = false, stats = false; double* stats_dev = nullptr;
    uint64_t nb = 1; int lanes = 1;      // rows per batch; batches alternate between this many lanes
    PruneFeedback::Plan fb{};
    float prune_wmax = 0.0f;             // the bound-pruning guard (prune_guard_ok, xrl_device.h) prices a query's largest |x| with the model's largest |weight| x max(1, |bias|)
    hipEvent_t k1_done = nullptr; size_t ev_next = 0;   // the most recent K1 launch (either lane); how many of m.events this predict has used
    // ---- the row batch in flight: rows [row0, row0 + nrows) on stream S, typed views of its lane's scratch
    uint64_t row0 = 0; uint32_t nrows = 0; hipStream_t S = nullptr;
    bool x_ok_done = false;              // x_ok[q] = the pruning guard of query q (also "all x finite" for K1G's fast loop) is written: by launch_xguard
                                         // or, for free, by a K1Q launch that runs before the first layer that needs it
    BeamDev beam[2]{};
    uint32_t *cand_off, *ncand, *sort_hist, *sort_start, *blk_start, *x_ok, *qperm, *qsort_hist, *qsort_start, *prune_done, *prune_cnt, *rest_q;
    float* cand; void *items, *items_sorted;

    void begin_batch(const LaneWs& lw, hipStream_t s, uint64_t r0, uint32_t n) {
        auto u32 = [](const DevBuf& d) { return d.as<uint32_t>(); };
        row0 = r0; nrows = n; S = s; x_ok_done = false;
        for (int i = 0; i < 2; ++i) beam[i] = BeamDev{u32(lw.beam_idx[i]), lw.beam_val[i].as<float>(), u32(lw.beam_cnt[i]), beam_stride};
        cand_off = u32(lw.cand_off); ncand = u32(lw.ncand); cand = lw.cand.as<float>(); items = lw.items.p; items_sorted = lw.items_sorted.p;
        sort_hist = u32(lw.sort_hist); sort_start = u32(lw.sort_start); blk_start = u32(lw.blk_start); x_ok = u32(lw.x_ok);
        qperm = u32(lw.qperm); qsort_hist = u32(lw.qsort_hist); qsort_start = u32(lw.qsort_start); prune_done = u32(lw.prune_done); prune_cnt = u32(lw.prune_cnt); rest_q = u32(lw.rest_q);
    }
    // What the stages of a bound-pruned layer hand to each other.  prune_cnt is two words -- [0] the later stage's item count, [1] the length of rest_q --
    // and only these two functions know: clear_list zeroes both in one memset, before the first stage (StageLinks, xrl_kernels.h: who zeroes *n_items).
    StageLinks links(const Route& r) const {
        StageLinks io{prune_done, x_ok, prune_cnt, nullptr, nullptr};
        if (r.compact_rest) { io.rest_q = rest_q; io.rest_cnt = prune_cnt + 1; }
        return io;
    }
    void clear_list() { XRL_HIP(hipMemsetAsync(prune_cnt, 0, 8, S)); }
    Stage stage(const Route& r, int st, const Layer& L) const {   // stage st of r.n_stage
        const bool last = st == r.n_stage - 1; const uint32_t end = r.stage_end[st];
        return Stage{st == 0 ? STAGE_FIRST : last ? STAGE_LAST : STAGE_MID, st ? r.stage_end[st - 1] : 0u, end, last ? 0u : (uint32_t)L.cand_bound(end), links(r)};
    }
    bool unstaged(size_t l) const { return l < (size_t)kFbLayers && fb.unstaged[l]; }   // pruning feedback: the layer scores everything in one pass this time
    // (route_layer reads the plan's shape and policy fields only: it is asked about batch sizes, not about a batch)
    LayerPlan make_plan(size_t l) const {
        LayerPlan P{};
        P.layer = (int)l; P.row0 = (uint32_t)row0; P.nrows = nrows;
        P.beam_in = shape[l].beam_in; P.k = shape[l].k; P.cand_stride = shape[l].cand_stride; P.pp = shape[l].pp;
        P.tune = K1Tune{opt.k1_wpb, opt.k1_lds_pad, opt.k1_ablate, opt.k1g_variant, opt.presence, opt.tile_rows, opt.k2_big_min_k};
        P.first_layer = (l == 0 && (!has_init || o.no_prev_pred)) ? 1 : 0; P.implicit_root = (l == 0 && !has_init) ? 1 : 0;   // no_prev_pred
        P.bias_first = (m.weight_matrix_type == 1 && !X.dense) ? 1 : 0; P.prune = (opt.prune && !unstaged(l)) ? 1 : 0;
        if (opt.prune && opt.adaptive && !stats && l < (size_t)kFbLayers) { P.fb_host = m.fb.host; P.fb_dev = m.fb.dev.as<uint32_t>(); }
        return P;
    }
    BeamDev beam_prev(size_t l) const {   // what layer l reads: the explicit initial beam, the implicit root (all null), or the lane's ping-pong buffer
        if (l > 0 || !has_init) return l > 0 ? beam[(l - 1) & 1] : BeamDev{};
        const BeamDev& i = *o.initial;
        return BeamDev{i.idx + row0 * i.stride, i.val + row0 * i.stride, i.cnt + row0, i.stride};
    }
    BeamDev beam_out(size_t l) const {    // what layer l writes: the other ping-pong buffer, or (last layer) the batch's rows of the caller's buffers
        if (l + 1 < shape.size()) return beam[l & 1];
        return BeamDev{result.idx + row0 * result.stride, result.val + row0 * result.stride, result.cnt + row0, result.stride};
    }
    hipEvent_t next_event() {
        if (ev_next == m.events.size()) { hipEvent_t e; XRL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); m.events.push_back(e); }
        return m.events[ev_next++];
    }
    void chain(hipStream_t from, hipStream_t to) { hipEvent_t e = next_event(); XRL_HIP(hipEventRecord(e, from)); XRL_HIP(hipStreamWaitEvent(to, e, 0)); }   // `to` continues after what `from` holds now
    static bool debug_sync() { static const bool on = [] { const char* e = std::getenv("XRL_DEBUG_SYNC"); return e && e[0] == '1'; }(); return on; }
    bool named() const { return m.profiling || debug_sync(); }   // somebody reads the launch names (K1Q composes its own only then)
    template <class F> void timed(const char* name, uint32_t layer, F&& fn) {
        if (debug_sync()) {   // XRL_DEBUG_SYNC=1: every launch group is announced and synchronised on its own, a device fault names the kernel family and the layer
            std::fprintf(stderr, "[xrl debug] %s layer %u rows %llu+%u\n", name, layer, (unsigned long long)row0, nrows); std::fflush(stderr);
            fn(); const hipError_t e = hipStreamSynchronize(S);
            if (e != hipSuccess) fail(std::string("device fault in ") + name + " (layer " + std::to_string(layer) + ", rows " + std::to_string(row0) + "+" + std::to_string(nrows) + "): " + hipGetErrorString(e));
            return;
        }
        profiled(m, S, name, layer, fn);
    }
    void need_x_ok() {   // once per row batch
        if (!x_ok_done) timed("xguard", 0, [&] { launch_xguard(X, (uint32_t)row0, nrows, prune_wmax, x_ok, S); });
        x_ok_done = true;
    }
};

// ---- resolve per-layer k / post-processor (inference.hpp:2471, 2055-2058)
std::vector<LayerShape> resolve_layers(const Model& m, const QueriesDev& X, const PredictOpts& o) {
    // MLModel::predict_internal's shape checks live in Python for the reference
    // (xmc/base.py:1603-1607); here a mismatch is a loud error instead of UB.
    if (!X.dense && X.cols != m.nr_features && X.cols != m.layers[0]->w_rows)
        fail("X.shape[1] (" + std::to_string(X.cols) + ") != nr_features (" + std::to_string(m.nr_features) + ")");
    if (X.dense && X.cols < m.nr_features)
        fail("dense X has fewer columns (" + std::to_string(X.cols) + ") than nr_features (" + std::to_string(m.nr_features) + ")");
    const size_t T = m.layers.size();
    const bool has_init = o.initial != nullptr;
    std::vector<LayerShape> shape(T);
    for (size_t l = 0; l < T; ++l) {
        const Layer& L = *m.layers[l]; LayerShape& s = shape[l];
        const uint32_t ov = (l == T - 1) ? o.only_topk : o.beam_size;
        s.k = ov ? ov : L.only_topk;
        if (s.k == 0) fail("layer " + std::to_string(l) + ": only_topk resolved to 0");
        s.pp = o.post_processor ? parse_post_processor(o.post_processor) : L.pp;
        uint64_t bin = (l == 0) ? (has_init ? std::max<uint32_t>(1, o.initial_max) : 1) : std::min<uint64_t>(shape[l - 1].k, shape[l - 1].cand_stride);
        if (!(l == 0 && has_init)) bin = std::min<uint64_t>(bin, L.c_cols ? L.c_cols : 1);   // explicit codes may list a parent more than once
        s.beam_in = (uint32_t)std::max<uint64_t>(1, bin);
        const uint64_t cb = std::max<uint64_t>(1, (l == 0 && has_init && o.initial_cand_bound) ? o.initial_cand_bound : L.cand_bound_kept(s.beam_in));
        if (cb > 0x7FFFFFFFull) fail("candidate row too long; lower beam_size");
        s.cand_stride = (uint32_t)cb;
    }
    return shape;
}

// ---- batch rows so that the candidate buffer stays bounded (default 6 GiB of 288)
void size_batches(Batch& b, uint64_t n_rows) {
    uint32_t cs_max = 1;
    for (const LayerShape& s : b.shape) cs_max = std::max(cs_max, s.cand_stride);
    uint64_t nb = std::min<uint64_t>(std::max<uint64_t>(1, kCandBudgetBytes / ((uint64_t)cs_max * 4)), 1u << 22);
    if (b.opt.max_batch_rows > 0) nb = std::min<uint64_t>(nb, (uint64_t)b.opt.max_batch_rows);
    nb = std::min<uint64_t>(nb, std::max<uint64_t>(1, std::max<uint64_t>(n_rows, b.o.reserve_rows)));   // reserve_rows: size the scratch for the caller's largest batch up front
    // two lanes: the row batches alternate between the caller's stream and an auxiliary one.  K1 launches are chained
    // across the lanes (one K1 at a time owns the memory system); a lane's K0 / sort / K2 run under the other lane's K1.
    b.lanes = (b.opt.overlap_min_rows > 0 && !b.stats && !b.m.profiling && n_rows >= (uint64_t)b.opt.overlap_min_rows) ? 2 : 1;
    b.nb = b.lanes == 2 ? std::min<uint64_t>(nb, (n_rows + 1) / 2) : nb;
}

// per layer: 0 = K1 on the items in natural order, 1 = K1 on tile-sorted items, 3 = K1G (dense X, tiled SGEMM over tile-sorted items)
int tile_mode(const Batch& b, size_t l, uint64_t rows) {
    const Layer& L = *b.m.layers[l];
    if (L.n_tiles > sort_max_tiles()) return 0;
    const uint64_t slots = rows * b.shape[l].beam_in * L.max_tiles_per_parent;
    // 3 = K1G: dense queries against a dense-format layer as a tiled SGEMM over tile-sorted items
    if (b.X.dense && b.opt.dense_layers && b.opt.k1g_min_items > 0 && !b.csc && k1g_cols(L.dev) != 0 && b.shape[l].k <= k2_max_k() &&
        slots / std::max<uint32_t>(1, L.n_tiles) >= (uint64_t)b.opt.k1g_min_items) return 3;
    return (b.opt.sort_min_tiles > 0 && L.n_tiles >= (uint32_t)b.opt.sort_min_tiles) ? 1 : 0;
}

// How layer l (and, for K1Q, the layers that share its launch) runs on a batch of `nrows` rows.  Launches nothing, reads no device-written word.
Route route_layer(const Batch& b, size_t l, uint64_t nrows) {
    const Model& m = b.m; const Model::Options& opt = b.opt; const Layer& L = *m.layers[l];
    const uint32_t beam_in = b.shape[l].beam_in;
    Route r{}; r.last = l; r.J = 1;
    // a handle under an output constraint (xrl_set_output_constraint): every layer scores the kept candidates of its view one pair at a time
    // (offsets -> K1P -> K2), whatever the layout -- no bound pruning, no feedback sampling, no sorted launch, no scratch beyond the candidate rows
    if (m.constrained) { r.kind = ROUTE_CONSTRAINED; return r; }
    r.mode = tile_mode(b, l, nrows);
    // the second phase of a bound-pruned tile-format layer runs on TILE-SORTED items (option sort_rest): what is left after the first phase
    // is, on a model that does not let the bound stop much, most of the layer's work, and in query order every (query, tile) item finds its
    // tile's lookup words and entries cold (Amazon-670K-hard: 7 % L2 hits, the fabric's request ceiling); tile-sorted, the items of a tile
    // run back to back on one XCD and share them
    r.sorts_rest = opt.sort_rest != 0 && !b.stats && L.n_tiles <= sort_max_tiles() && L.n_tiles >= 64u;
    // CSC route (weight_matrix_type CSC, single-layer API): one (query, child) dot product per candidate, bias first
    if (b.csc) { r.kind = ROUTE_CSC; return r; }
    const LayerPlan P = b.make_plan(l);
    // exact bound pruning needs a combiner (a child's score is then <= its parent's) and the register top-k kernel
    const bool boundable = !P.implicit_root && !P.first_layer && P.pp.kind != PP_NOOP && beam_in > 1 && k2_wave_path(P);
    if (!b.stats && r.mode == 3) {
        // ---- exact bound pruning (see the tile-format route below): the GEMM over the children of the J best beam parents first,
        //      then a second, tile-sorted GEMM over the remaining slots of the queries whose top-k is not final yet.  J covers about
        //      one candidate register (64 candidates), like K1Q's first stage.
        r.kind = ROUTE_K1G; r.pruned = opt.prune && boundable; r.J = r.pruned ? k1g_first_slots(L, beam_in, opt.k1g_first) : beam_in;
        if (r.pruned) { r.stage_end[0] = r.J; r.stage_end[1] = beam_in; r.n_stage = 2; }
        return r;
    }
    // layers held in the dense row format: the whole layer is one query-stationary kernel (beam in, beam out)
    const bool dense_x = b.X.dense != 0 || opt.dense_layers >= 2;
    auto regs = [&](size_t ll) { return k1q_regs(m.layers[ll]->dev, b.shape[ll].beam_in, b.shape[ll].k, dense_x); };
    auto runs_k1q = [&](size_t ll) { return opt.dense_layers && !b.stats && tile_mode(b, ll, nrows) != 3 && regs(ll) != 0; };
    if (runs_k1q(l)) {
        r.kind = ROUTE_K1Q;
        // consecutive dense-format layers run in ONE launch: the wavefront that owns a query carries its beam through them in LDS
        // (only narrow layers share a launch: a fused kernel is compiled for -- and holds the registers of -- its widest layer)
        auto narrow = [&](size_t ll) { return regs(ll) <= (uint32_t)std::min(3, opt.k1q_fuse); };
        while (opt.k1q_fuse && narrow(l) && r.last + 1 < b.shape.size() && r.last + 1 - l < 8 && runs_k1q(r.last + 1) && narrow(r.last + 1)) ++r.last;
        // SORTED launch of the group's last layer (option qsort): a layer of many parents whose matrix is far larger than the L2s is
        // request-bound -- one 64-byte fabric request per (feature, beam parent) and query -- and the queries that share beam
        // parents are scattered over the batch.  The layers before it run as usual; the queries are then counting-sorted by the best
        // parent of the beam they produced and the last layer runs in that order, every XCD on a contiguous range of it.
        const uint32_t nk = m.layers[r.last]->dev.n_parents;
        r.sorted_last = opt.qsort != 0 && !b.X.dense && r.last > 0 && nrows >= (uint64_t)std::max(1, opt.qsort_min_rows) &&
                        nk >= (uint32_t)std::max(2, opt.qsort_min_parents) && nk <= qsort_max_keys();
        return r;
    }
    r.kind = ROUTE_TILE; r.group = opt.k1_group > 0 ? opt.k1_group : k1_auto_group(L.dev, L, b.X.dense);
    if (b.unstaged(l) && r.mode == 0 && r.sorts_rest) r.mode = 1;    // pruning feedback: everything in one pass, on tile-sorted items
    // ---- exact bound pruning, tile format: score the children of the best beam parent first (K0 -> K1 -> K2 on one slot), then
    //      only the remaining slots of the queries whose top-k is not final yet (see K2Args).
    r.pruned = opt.prune && !b.unstaged(l) && boundable;
    if (b.stats) {
        // the stats pass walks the tile format whatever kernel the timed pass runs: stage it the way THAT kernel stages the layer, so
        // that the work it counts is the work the timed kernels evaluate (K1G: J parents first; K1Q: the parents of candidate
        // register 0 first, nothing skipped when the whole beam fits one register)
        if (r.mode == 3) r.J = k1g_first_slots(L, beam_in, opt.k1g_first);      // (the SAME staging the timed K1G path uses: ADVICE r3)
        else if (opt.dense_layers && regs(l) != 0) {
            if (regs(l) <= 1) r.pruned = false;
            else r.J = std::max<uint32_t>(1, (64u >> L.dev.d_gp_log2) / std::max<uint32_t>(1, L.dev.d_max_tiles));
        }
        if (r.J >= beam_in) r.pruned = false;
    } else if (r.mode != 0) r.pruned = false;
    if (!r.pruned) return r;
    // stages of beam slots: [0, J) first, then -- wide beams only (>= 16 parents: Wiki10-31K's 20) -- a MIDDLE stage [J, J2) before
    // "everything else": with 20 parents of ~60 children and k = 20 the first parent alone rarely settles the top-k, the first
    // five usually do, and the last stage then sees few queries.
    r.stage_end[r.n_stage++] = r.J;
    if (opt.prune_mid != 0 && beam_in >= 16u && !b.stats) r.stage_end[r.n_stage++] = std::min<uint32_t>(beam_in - 1u, r.J + 4u);
    r.stage_end[r.n_stage++] = beam_in;
    // option leaf_fuse: with one tile per parent, K1T's lanes end up holding every candidate of slot 0 -- its epilogue selects the top-k
    // and sets the done flags itself (xrl_k1t.hip, SEL): no k2_topk launch, and no candidate row stored for a query that is done.
    r.fuse = opt.leaf_fuse != 0 && r.J == 1 && !b.stats && k1t_selects(L.dev, P, b.X);
    // ... and (beams of up to 32 parents) derives its items from the beam: K0 is not launched either.  leaf_fuse = 2 keeps K0 (A/B runs).
    r.fuse_k0 = r.fuse && opt.leaf_fuse != 2 && beam_in <= 32u;
    // option leaf_tail: narrow beams (two stages) -- whatever writes done[q] in the first stage also appends the unfinished queries to a list, and
    // k0b_remaining / K1 / k2_topk_rest are pointed at that list instead of the batch (Amazon-670K: 1.6 % of the queries).  Wide beams with a
    // middle stage and the stats pass keep the batch-sized launches.
    r.compact_rest = opt.leaf_tail != 0 && r.n_stage == 2 && !b.stats;
    return r;
}

// Everything the routes of this predict's batch sizes (nb rows, and the remainder) touch, reserved once, before the first launch.
void reserve_scratch(const Batch& b, Workspace& ws, uint64_t n_rows) {
    const Model& m = b.m; const size_t T = b.shape.size(); const uint64_t nb = b.nb;
    uint32_t bin_max = 1, cs_max = 1; uint64_t slots_max = 1;
    for (size_t l = 0; l < T; ++l) {
        bin_max = std::max(bin_max, b.shape[l].beam_in); cs_max = std::max(cs_max, b.shape[l].cand_stride); slots_max = std::max<uint64_t>(slots_max, nb * b.shape[l].beam_in * m.layers[l]->max_tiles_per_parent);
    }
    // bytes per lane of the buffers only some routes use (0: none does, nothing is allocated)
    size_t sorted = 0, hist = 0, starts = 0, x_ok = 0, done = 0, cnt = 0, rest = 0, qperm = 0, qhist = 0, qstarts = 0;
    for (const uint64_t rows : {nb, n_rows % nb}) {
        // (every layer is asked, also the inner ones of a K1Q group: they answer like the group does)
        for (size_t l = 0; l < T && rows; ++l) {
            const Route r = route_layer(b, l, rows); const Layer& L = *m.layers[l];
            const bool staged_tile = r.kind == ROUTE_TILE && r.pruned;
            if (r.mode != 0 || (b.opt.prune && r.sorts_rest)) { hist = std::max(hist, sort_hist_bytes(nb * b.shape[l].beam_in * L.max_tiles_per_parent, L.n_tiles)); starts = std::max(starts, ((size_t)L.n_tiles + 1) * 4); }
            if (starts || staged_tile) sorted = slots_max * k0_item_bytes();   // (the compacted items of the later stages go to items_sorted, sorted or not)
            if (staged_tile || (r.kind == ROUTE_K1G && r.pruned)) { done = (size_t)nb * 4; cnt = 256; }
            if (staged_tile && r.compact_rest) rest = (size_t)nb * 4;
            // (a later layer of a batch that is NOT served by K1Q decides its pruning in K2 and needs the guard flags: the K1Q launch writes them)
            if (r.kind == ROUTE_K1G || staged_tile || (r.kind == ROUTE_K1Q && b.opt.prune && r.last + 1 < T)) x_ok = (size_t)nb * 4;
            const uint32_t nk = m.layers[r.last]->dev.n_parents;
            if (r.kind == ROUTE_K1Q && r.sorted_last) { qperm = (size_t)nb * 4; qhist = std::max(qhist, qsort_hist_bytes((uint32_t)nb, nk)); qstarts = std::max(qstarts, ((size_t)nk + 1) * 4); }
        }
    }
    for (int ln = 0; ln < b.lanes; ++ln) {
        LaneWs& lw = ws.lane[ln];
        for (int i = 0; i < 2; ++i) { lw.beam_idx[i].reserve(nb * b.beam_stride * 4); lw.beam_val[i].reserve(nb * b.beam_stride * 4); lw.beam_cnt[i].reserve(nb * 4); }
        lw.items.reserve(slots_max * k0_item_bytes());
        lw.cand_off.reserve(nb * bin_max * 4); lw.ncand.reserve(nb * 4); lw.cand.reserve(nb * (uint64_t)cs_max * 4);
        lw.items_sorted.reserve(sorted); lw.sort_hist.reserve(hist); lw.sort_start.reserve(starts); lw.blk_start.reserve(starts);
        lw.x_ok.reserve(x_ok); lw.prune_done.reserve(done); lw.prune_cnt.reserve(cnt); lw.rest_q.reserve(rest);
        lw.qperm.reserve(qperm); lw.qsort_hist.reserve(qhist); lw.qsort_start.reserve(qstarts);
    }
    if (b.stats) m.ws->stats.reserve(T * kStatsPerLayer * sizeof(double));
}

void launch_csc_layer(Batch& b, size_t l) {
    Layer& L = *b.m.layers[l]; const LayerPlan P = b.make_plan(l); const BeamDev prev = b.beam_prev(l);
    ensure_device_csc(L);
    b.timed("k0_prolongate", l, [&] { launch_k0_prolongate(L.dev, P, b.X, prev, b.cand_off, b.ncand, b.items, b.S); });
    b.timed("k1c_csc", l, [&] { launch_k1c_csc(L.dev, L.d_csc_ptr.as<uint64_t>(), L.d_csc_idx.as<uint32_t>(), L.d_csc_val.as<float>(), P, b.X, prev, b.cand_off, b.ncand, b.cand, b.S); });
    b.timed("k2_topk", l, [&] { launch_k2_topk(L.dev, P, prev, b.cand_off, b.ncand, b.cand, b.beam_out(l), b.S); });
}

// the constrained route: K0 and K2 as they are, on a copy of the layer's view of itself whose chunk_col / perm_inv are the constraint's (layers above
// the rule's early stop keep their own); K0 writes offsets and counts only (no item descriptors: item_ranks = 0); K1P scores with the handle's arithmetic
void launch_constrained_layer(Batch& b, size_t l) {
    Layer& L = *b.m.layers[l]; LayerPlan P = b.make_plan(l); const BeamDev prev = b.beam_prev(l);
    P.fb_host = nullptr; P.fb_dev = nullptr; P.prune = 0;   // (the CSC copy of W is there: the setter uploads it before it sets Model::constrained)
    LayerDev V = L.dev;
    if (L.view.active) { V.chunk_col = L.view.d_chunk_col.as<uint32_t>(); V.perm_inv = L.view.d_perm_inv.as<uint32_t>(); }
    const int chain = (b.csc || b.X.dense) ? kChainCsc : kChainChunked;
    b.timed("k0_constrained", l, [&] { launch_k0_prolongate(V, P, b.X, prev, b.cand_off, b.ncand, b.items, b.S, 0); });
    b.timed("k1p_constrained", l, [&] { launch_k1p_constrained(V, L.d_csc_ptr.as<uint64_t>(), L.d_csc_idx.as<uint32_t>(), L.d_csc_val.as<float>(), P, chain, b.X, prev, b.cand_off, b.ncand, b.cand, b.S); });
    b.timed("k2_constrained", l, [&] { launch_k2_topk(V, P, prev, b.cand_off, b.ncand, b.cand, b.beam_out(l), b.S); });
}

// K0 -> sort -> K1G -> K2 over the first r.J beam slots (unpruned: all of them, and that is the layer); pruned: the same over the remaining
// slots of the queries K2 did not mark done
void launch_k1g_layer(Batch& b, size_t l, const Route& r) {
    const Layer& L = *b.m.layers[l]; const QueriesDev& X = b.X; hipStream_t S = b.S;
    const LayerPlan P = b.make_plan(l); const BeamDev prev = b.beam_prev(l), out = b.beam_out(l);
    b.need_x_ok();   // once per row batch: which dense query rows are finite (K1G's fast loop needs it on layers with missing cells) + the pruning guard
    LayerPlan PA = P; PA.beam_in = r.J;
    b.timed("k0_prolongate", l, [&] { launch_k0_prolongate(L.dev, P, X, prev, b.cand_off, b.ncand, b.items, S, r.J); });
    b.timed("k1_sort_items", l, [&] { launch_sort_items(L.dev, (uint64_t)b.nrows * r.J * L.max_tiles_per_parent, b.items, b.items_sorted, b.sort_hist, b.sort_start, S); });
    b.timed("k1g_dense_x", l, [&] { launch_k1g(L.dev, PA, X, b.items_sorted, b.sort_start, b.blk_start, b.x_ok, b.cand, S); });
    if (!r.pruned) { b.timed("k2_topk", l, [&] { launch_k2_topk(L.dev, P, prev, b.cand_off, b.ncand, b.cand, out, S); }); return; }
    const Stage first = b.stage(r, 0, L), rest = b.stage(r, 1, L);
    LayerPlan PB = P; PB.beam_in = rest.slot_end - rest.slot_begin;
    b.timed("k2_topk", l, [&] { launch_k2_stage(L.dev, P, prev, b.cand_off, b.ncand, b.cand, out, first, S); });
    b.timed("k0b_remaining", l, [&] { launch_k0b_remaining(L.dev, P, X, prev, b.cand_off, rest, b.items, S); });
    b.timed("k1_sort_items_rest", l, [&] { launch_sort_items(L.dev, (uint64_t)b.nrows * PB.beam_in * L.max_tiles_per_parent, b.items, b.items_sorted, b.sort_hist, b.sort_start, S, rest.io.n_items); });
    b.timed("k1g_dense_x_rest", l, [&] { launch_k1g(L.dev, PB, X, b.items_sorted, b.sort_start, b.blk_start, b.x_ok, b.cand, S); });
    b.timed("k2_topk_rest", l, [&] { launch_k2_stage(L.dev, P, prev, b.cand_off, b.ncand, b.cand, out, rest, S); });
}

// layers [l, r.last] in one K1Q launch; with r.sorted_last the last one in a launch of its own, after the queries were sorted by the beam it reads
void launch_k1q_group(Batch& b, size_t l, const Route& r) {
    const QueriesDev& X = b.X; hipStream_t S = b.S; const LayerDev* Ls[8]; LayerPlan Ps[8];
    for (size_t ll = l; ll <= r.last; ++ll) {
        Ls[ll - l] = &b.m.layers[ll]->dev; Ps[ll - l] = b.make_plan(ll);
        Ps[ll - l].fb_host = Ps[0].fb_host; Ps[ll - l].fb_dev = Ps[0].fb_dev;   // (a launch samples through the feedback words of its group's first layer)
    }
    const BeamDev prev = b.beam_prev(l);
    const size_t n_shared = r.last - l + (r.sorted_last ? 0 : 1), ls = r.last;   // layers [l, l + n_shared) share a launch
    const char* const single = X.dense ? "k1q_dense_x" : "k1q_dense";
    char fused[48] = "";   // profile / trace name of a launch of several layers; composed only when somebody reads it
    if (n_shared > 1 && b.named()) std::snprintf(fused, sizeof fused, "k1q_fused_%s%zu_%zu", X.dense ? "x_" : "", l, l + n_shared - 1);
    // (a later layer of this batch that is NOT served by K1Q decides its pruning in K2 and needs the guard flags: this launch writes them)
    uint32_t* xok_out = nullptr;
    if (!b.x_ok_done && b.opt.prune && r.last + 1 < b.shape.size()) { xok_out = b.x_ok; b.x_ok_done = true; }
    BeamDev pv = prev;
    if (n_shared) {
        pv = b.beam_out(l + n_shared - 1);
        b.timed(n_shared > 1 ? fused : single, l, [&] { launch_k1q(Ls, Ps, (int)n_shared, X, prev, pv, S, b.prune_wmax, xok_out); });
        xok_out = nullptr;
    }
    if (!r.sorted_last) return;
    b.timed("k1_sort_queries", ls, [&] { launch_sort_queries(pv, b.nrows, Ls[ls - l]->n_parents, b.qsort_hist, b.qsort_start, b.qperm, S); });
    b.timed(single, ls, [&] { launch_k1q(Ls + (ls - l), Ps + (ls - l), 1, X, pv, b.beam_out(ls), S, b.prune_wmax, xok_out, b.qperm); });
}

const char* const kK1Name[2][3] = {{"k1_sparse", "k1_sparse_mid", "k1_sparse_rest"}, {"k1_dense", "k1_dense_mid", "k1_dense_rest"}};   // [dense X][first / middle / last stage]

// What the passes of a tile-format layer share
struct TileLayer { size_t l; const Layer& L; LayerPlan P; BeamDev prev, out; const char* const* k1_name; double* stats; };

// tile-format layer in one pass: K0 -> (sort) -> K1 -> K2
void launch_tile_unstaged(Batch& b, const TileLayer& t, const Route& r) {
    const Layer& L = t.L; const LayerPlan& P = t.P; const QueriesDev& X = b.X; hipStream_t S = b.S; const size_t l = t.l;
    b.timed("k0_prolongate", l, [&] { launch_k0_prolongate(L.dev, P, X, t.prev, b.cand_off, b.ncand, b.items, S); });
    if (r.mode != 0) b.timed("k1_sort_items", l, [&] { launch_sort_items(L.dev, (uint64_t)b.nrows * P.beam_in * L.max_tiles_per_parent, b.items, b.items_sorted, b.sort_hist, b.sort_start, S); });
    if (b.lanes == 2 && b.k1_done) XRL_HIP(hipStreamWaitEvent(S, b.k1_done, 0));   // K1 launches take turns across the lanes
    LayerPlan PU = P; PU.fb_host = nullptr;   // (an unstaged pass's item count is not a feedback sample: a probe's outcome may be pending)
    b.timed(t.k1_name[0], l, [&] { launch_k1(L.dev, PU, X, r.mode == 1 ? b.items_sorted : b.items, r.mode == 1 ? b.sort_start + L.n_tiles : nullptr, b.cand, r.group, S); });
    if (b.lanes == 2) { b.k1_done = b.next_event(); XRL_HIP(hipEventRecord(b.k1_done, S)); }
    b.timed("k2_topk", l, [&] { launch_k2_topk(L.dev, P, t.prev, b.cand_off, b.ncand, b.cand, t.out, S); });
    if (t.stats) launch_stats(L.dev, P, X, t.prev, b.ncand, b.items, t.stats, S);
}

// The first stage takes its items from K0 (K0 -> K1 -> K2 on its slots, + the done flags and the list for the later stages), or (r.fuse) is one K1T
// launch that keeps K1's profile name.
void launch_tile_first(Batch& b, const TileLayer& t, const Route& r, const Stage& st) {
    const Layer& L = t.L; const LayerPlan& P = t.P; const QueriesDev& X = b.X; hipStream_t S = b.S; const size_t l = t.l;
    b.need_x_ok();
    // (a profile slot of its own -- "rest_list", and "rest_list_grid" in the later stage: the three later launches keep their names, these say which form ran)
    if (st.io.rest_q) b.timed("rest_list", l, [&] { b.clear_list(); });
    if (!r.fuse_k0) b.timed("k0_prolongate", l, [&] { launch_k0_prolongate(L.dev, P, X, t.prev, b.cand_off, b.ncand, b.items, S, st.slot_end); });
    if (b.lanes == 2 && b.k1_done) XRL_HIP(hipStreamWaitEvent(S, b.k1_done, 0));
    if (r.fuse) {
        const K1TSelect sel{t.prev, t.out, b.cand_off, b.ncand, st.io};
        b.timed("k1_sparse", l, [&] { launch_k1t(L.dev, P, X, r.fuse_k0 ? nullptr : b.items, nullptr, b.cand, S, &sel); });
    } else {
        LayerPlan PA = P; PA.beam_in = st.slot_end;        // (K1 sizes its grid from beam_in x tiles per parent)
        b.timed(t.k1_name[0], l, [&] { launch_k1(L.dev, PA, X, b.items, nullptr, b.cand, r.group, S); });
        b.timed("k2_topk", l, [&] { launch_k2_stage(L.dev, P, t.prev, b.cand_off, b.ncand, b.cand, t.out, st, S); });
    }
    // the stats pass walks the whole list of the later stage: unused slots read as "no tile"
    if (t.stats) XRL_HIP(hipMemsetAsync(b.items_sorted, 0xFF, (uint64_t)b.nrows * (P.beam_in - st.slot_end) * L.max_tiles_per_parent * k0_item_bytes(), S));
}

// Which of two equivalent forms the later stages of a bound-pruned tile-format layer take: decided from the item count the pruning feedback already samples
// (the last stage's K1 launch writes it to a host-visible word), read while the batch is being enqueued -- after the first stage's launches, the device
// may have written it since the predict began.  Launches nothing; results never depend on either answer.
struct RestForm { bool srt; uint32_t list_grid; };   // the items are tile-sorted before K1; > 0: K1 walks the compacted list on a fixed grid of about this many workgroups
RestForm rest_form(const Batch& b, const TileLayer& t, const Route& r) {
    const Layer& L = t.L; RestForm f{r.sorts_rest, 0};
    const uint32_t seen = t.P.fb_host ? b.m.fb.word(fb_items_word((int)t.l)) : kFbPending;
    // srt, unless the previous predicts left (almost) nothing for the later stages: four tiny launches of the sort then cost more than
    // the locality buys (a 61 250-row shard of Amazon-670K: 0.99 -> 0.93 ms per step, profiles/r05_k1q/README.md).
    if (f.srt && t.P.fb_host && b.opt.sort_rest_min > 0) {
        // (measured, Amazon-670K shape, 8192 leaf tiles: 78 k items = 9.5 per tile -- K1 runs 0.295 ms sorted, 0.298 unsorted, the sort costs 0.062;
        //  4.4 M items = 537 per tile on the hard model -- unsorted K1 finds 7 % of its lines in the L2, sorted 94 %: the sort pays once
        //  a tile's lookup words and entries are re-used a few dozen times)
        const uint64_t need = std::max<uint64_t>((uint64_t)b.opt.sort_rest_min, 32ull * L.n_tiles);
        if (seen != kFbPending && (uint64_t)seen < need) f.srt = false;
    }
    if (r.compact_rest) {
        // K1 on the compacted list: a fixed grid that walks it, when the feedback's last item count says that the list fills a small part of a LARGE
        // worst-case grid (measured, profiles/r06_leaf.md section 7: Amazon-670K's 78 k items of 4.4 M slots 0.297 -> 0.239 ms with 6144 workgroups;
        // a 61 250-row shard's 551 k slots 0.053 -> 0.057 ms: not there).  Either kernel is right for any count.
        const uint64_t slots_s = (uint64_t)b.nrows * (r.stage_end[1] - r.stage_end[0]) * L.max_tiles_per_parent;   // (a list: two stages)
        if (b.opt.leaf_tail >= 2) f.list_grid = (uint32_t)b.opt.leaf_tail;
        else if (seen != kFbPending && slots_s >= (1ull << 21) && (uint64_t)seen * 8u <= slots_s) f.list_grid = 6144;
    }
    return f;
}

// One later stage: k0b (the unfinished queries' items of its slots) -> (sort) -> K1 -> K2 over the candidates of all slots scored so far (a middle
// stage: + the done flags for the next one).  It finds done / cand_off / ncand / cand (unfinished queries) as the stage before left them.
void launch_tile_later(Batch& b, const TileLayer& t, const Route& r, const Stage& st, const RestForm& f) {
    const Layer& L = t.L; const LayerPlan& P = t.P; const QueriesDev& X = b.X; hipStream_t S = b.S; const size_t l = t.l;
    const bool last = st.kind == STAGE_LAST; const uint64_t mtp = L.max_tiles_per_parent;
    LayerPlan PB = P; PB.beam_in = st.slot_end - st.slot_begin; PB.tune.wpb = 4;   // a later stage's grid is sized for "nothing pruned": mostly empty wavefronts, 4 per workgroup to dispatch fewer groups
    // (sorted: the compacted list goes where the first phase's items were -- K1 has consumed them -- and is sorted into items_sorted)
    bool ran_list = false;
    b.timed(last ? "k0b_remaining" : "k0b_remaining_mid", l, [&] { launch_k0b_remaining(L.dev, P, X, t.prev, b.cand_off, st, f.srt ? b.items : b.items_sorted, S); });
    if (f.srt) b.timed(last ? "k1_sort_items_rest" : "k1_sort_items_mid", l, [&] { launch_sort_items(L.dev, (uint64_t)b.nrows * PB.beam_in * mtp, b.items, b.items_sorted, b.sort_hist, b.sort_start, S, st.io.n_items); });
    b.timed(t.k1_name[last ? 2 : 1], l, [&] { ran_list = launch_k1(L.dev, PB, X, b.items_sorted, f.srt ? b.sort_start + L.n_tiles : st.io.n_items, b.cand, r.group, S, f.list_grid); });
    if (ran_list && b.named()) b.timed("rest_list_grid", l, [] {});   // (an empty slot: K1 ran its fixed-grid form)
    if (b.lanes == 2 && last) { b.k1_done = b.next_event(); XRL_HIP(hipEventRecord(b.k1_done, S)); }
    b.timed(last ? "k2_topk_rest" : "k2_topk_mid", l, [&] { launch_k2_stage(L.dev, P, t.prev, b.cand_off, b.ncand, b.cand, t.out, st, S); });
    if (t.stats && last) {   // (the stats pass has two stages)
        launch_stats(L.dev, P, X, t.prev, b.ncand, b.items, t.stats, S, (uint64_t)b.nrows * st.slot_begin * mtp);
        launch_stats(L.dev, PB, X, t.prev, nullptr, b.items_sorted, t.stats, S, (uint64_t)b.nrows * PB.beam_in * mtp);
    }
}

// tile-format layer: one pass, or bound-pruned in r.n_stage stages of beam slots
void launch_tile_layer(Batch& b, size_t l, const Route& r) {
    const LayerPlan P = b.make_plan(l);
    const TileLayer t{l, *b.m.layers[l], P, b.beam_prev(l), b.beam_out(l), kK1Name[b.X.dense ? 1 : 0], b.stats ? b.stats_dev + kStatsPerLayer * l : nullptr};
    if (!r.pruned) { launch_tile_unstaged(b, t, r); return; }
    launch_tile_first(b, t, r, b.stage(r, 0, t.L));
    const RestForm f = rest_form(b, t, r);
    if (P.fb_host) b.m.fb.tile_slots[l] = (uint64_t)b.nrows * (P.beam_in - r.stage_end[r.n_stage - 2]) * t.L.max_tiles_per_parent;
    for (int st = 1; st < r.n_stage; ++st) launch_tile_later(b, t, r, b.stage(r, st, t.L), f);
}

void launch_batch(Batch& b) {   // every layer of the row batch in flight
    for (size_t l = 0; l < b.shape.size(); ++l) {
        const Route r = route_layer(b, l, b.nrows);
        switch (r.kind) {
            case ROUTE_CSC: launch_csc_layer(b, l); break;
            case ROUTE_K1G: launch_k1g_layer(b, l, r); break;
            case ROUTE_K1Q: launch_k1q_group(b, l, r); break;
            case ROUTE_TILE: launch_tile_layer(b, l, r); break;
            case ROUTE_CONSTRAINED: launch_constrained_layer(b, l); break;
        }
        l = r.last;
    }
}
}  // namespace

// ---- pruning feedback: which layers run UNSTAGED this time because their first stage settled (almost) no query the last times
PruneFeedback::Plan PruneFeedback::begin_predict(size_t n_layers, bool sample) {
    Plan plan;
    if (!host) {
        XRL_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), kFbHostWords * 4, hipHostMallocDefault));
        for (int i = 0; i < kFbHostWords; ++i) host[i] = i < kFbCounterWords ? 0u : kFbPending;
        dev.reserve(kFbCounterWords * 4); XRL_HIP(hipMemset(dev.p, 0, kFbCounterWords * 4));
    }
    for (int l = 0; l < (int)std::min<size_t>(n_layers, kFbLayers); ++l) {
        if (sample && unstaged[l]) {
            // An unstaged layer is PROBED every kReprobe predicts: that one predict stages it, the following ones keep running
            // unstaged until the probe's counters arrive (a caller that queues predicts without synchronising is many predicts
            // ahead of the device: waiting for the outcome in the staged state would run all of them staged).
            bool decided = false, stage_again = false;
            if (probing[l]) {
                const uint32_t sn = word(fb_seen_word(l)), sec = word(fb_second_word(l)), dseen = sn - seen[l], dsec = sec - second[l];
                const uint32_t cnt = word(fb_items_word(l));
                if (dseen >= kMinSamples) { decided = true; stage_again = !((double)dsec > kSecondShare * (double)dseen); seen[l] = sn; second[l] = sec; }
                else if (cnt != kFbPending && tile_slots[l] > 0) { decided = true; stage_again = !((double)cnt > kItemShare * (double)tile_slots[l]); }
                if (decided) { probing[l] = 0; unstaged_calls[l] = 0; if (stage_again) unstaged[l] = 0; }
            }
            if (unstaged[l] && ++unstaged_calls[l] >= kReprobe) {    // (an undecided probe -- a batch too small to sample 256 queries -- is repeated)
                unstaged_calls[l] = 0; probing[l] = 1; plan.probed[l] = true;
                // (advisor, round 6: re-basing the counters after an UNDECIDED probe drops the samples it did collect -- kept as it is here)
                if (!decided) { seen[l] = word(fb_seen_word(l)); second[l] = word(fb_second_word(l)); }
                host[fb_items_word(l)] = kFbPending; tile_slots[l] = 0;
            }
        } else if (sample) {
            // query-stationary layers: of the sampled queries that ran staged, how many needed the second pass
            const uint32_t sn = word(fb_seen_word(l)), sec = word(fb_second_word(l)), dseen = sn - seen[l], dsec = sec - second[l];
            if (dseen >= kMinSamples) {
                if ((double)dsec > kSecondShare * (double)dseen) { unstaged[l] = 1; unstaged_calls[l] = 0; probing[l] = 0; }
                seen[l] = sn; second[l] = sec;
            }
            // tile-format layers: the item count of the last stage against the slots it was sized for
            const uint32_t cnt = word(fb_items_word(l));
            if (cnt != kFbPending && tile_slots[l] > 0 && (double)cnt > kItemShare * (double)tile_slots[l]) { unstaged[l] = 1; unstaged_calls[l] = 0; probing[l] = 0; }
        }
        plan.unstaged[l] = unstaged[l] != 0 && !plan.probed[l];
    }
    return plan;
}

uint32_t effective_topk(const Model& m, uint32_t only_topk) { return only_topk ? only_topk : m.layers.back()->only_topk; }   // inference.hpp:2055

void predict_device(Model& m, const QueriesDev& X, const PredictOpts& o, uint32_t* d_out_idx, float* d_out_val,
                    uint32_t* d_out_cnt, uint32_t out_stride, hipStream_t stream, bool sync, uint32_t row_begin, uint32_t row_count) {
    const size_t T = m.layers.size();
    // rows [row_begin, row_end) of X (results land at the same rows of the output buffers); default: all rows
    if (row_begin > X.rows) fail("predict: row range outside X");
    const uint64_t row_end = std::min<uint64_t>(X.rows, (uint64_t)row_begin + row_count), n_rows = row_end - row_begin;
    if (!m.ws) m.ws = std::make_unique<Workspace>();
    if (!stream) stream = m.stream;
    // the scratch buffers are shared by every predict of the handle: an asynchronous predict still running on another stream must finish first
    if (m.ws_done && m.ws_stream != stream) XRL_HIP(hipStreamWaitEvent(stream, m.ws_done, 0));
    static const bool step_marker = [] { const char* e = std::getenv("XRL_STEP_MARKER"); return e && e[0] == '1'; }();
    if (step_marker && !o.stats_out) launch_step_marker(stream);

    const std::vector<LayerShape> shape = resolve_layers(m, X, o);
    if (shape[T - 1].k > out_stride) fail("out_stride smaller than the effective only_topk");
    Batch b{m, m.opt, X, o, shape, BeamDev{d_out_idx, d_out_val, d_out_cnt, out_stride}};
    b.has_init = o.initial != nullptr; b.csc = o.csc_route || m.csc_route; b.stats = o.stats_out != nullptr;
    for (size_t l = 0; l < T; ++l) {
        if (l + 1 < T) b.beam_stride = std::max(b.beam_stride, shape[l].k);
        b.prune_wmax = std::max(b.prune_wmax, m.layers[l]->w_absmax);
    }
    if (!(b.prune_wmax <= 3.0e38f)) b.prune_wmax = INFINITY;
    size_batches(b, n_rows);
    if (m.opt.prune && m.opt.adaptive && !m.constrained) b.fb = m.fb.begin_predict(T, !b.stats);
    reserve_scratch(b, *m.ws, n_rows);
    if (b.stats) { b.stats_dev = m.ws->stats.as<double>(); XRL_HIP(hipMemsetAsync(m.ws->stats.p, 0, T * kStatsPerLayer * sizeof(double), stream)); }

    // ---- streams and cross-stream ordering
    hipStream_t lane_stream[2] = {stream, stream};
    if (b.lanes == 2) {
        if (!m.aux_stream) XRL_HIP(hipStreamCreateWithFlags(&m.aux_stream, hipStreamNonBlocking));
        lane_stream[1] = m.aux_stream;
        b.chain(stream, m.aux_stream);                                 // the auxiliary lane starts after everything queued so far
    }

    uint64_t batch = 0;
    for (uint64_t row0 = row_begin; row0 < row_end; row0 += b.nb, ++batch) {
        const int ln = (int)(batch % (uint64_t)b.lanes);
        b.begin_batch(m.ws->lane[ln], lane_stream[ln], row0, (uint32_t)std::min<uint64_t>(b.nb, row_end - row0));
        launch_batch(b);
    }
    if (b.lanes == 2) b.chain(m.aux_stream, stream);                    // the caller's stream continues after the auxiliary lane

    if (!m.ws_done) XRL_HIP(hipEventCreateWithFlags(&m.ws_done, hipEventDisableTiming));
    XRL_HIP(hipEventRecord(m.ws_done, stream)); m.ws_stream = stream;

    if (o.stats_out || sync) XRL_HIP(hipStreamSynchronize(stream));
    // per layer (kStatsPerLayer doubles): [0] algorithmic bytes of the reference chunks streamed (8E + 4R + 4(R+1) each,
    // SURVEY.md 8d), [1] candidates evaluated, [2..7] matched work of the (query, tile) items (launch_stats)
    if (o.stats_out) XRL_HIP(hipMemcpy(o.stats_out, m.ws->stats.p, T * kStatsPerLayer * sizeof(double), hipMemcpyDeviceToHost));
}

void resolve_profile(Model& m) {
    if (m.pending.empty()) return;
    XRL_HIP(hipSetDevice(m.device));
    XRL_HIP(hipDeviceSynchronize());
    for (auto& ev : m.pending) {
        float ms = 0.f;
        XRL_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
        m.profile[ev.slot].ms += ms;
        m.profile[ev.slot].launches += 1;
        (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b);
    }
    m.pending.clear();
}

}  // namespace xrl
