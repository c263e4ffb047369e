// predict_on_selected_outputs: score a given (query, label) sparsity pattern through the tree.
//
// Reference: HierarchicalMLModel::predict_on_selected_outputs (inference.hpp:2507-2571):
//   * per-layer patterns bottom-up, S_{l-1} = pattern(S_l x C_l) with sorted indices (:2527-2541);
//   * per layer top-down, prolongate_sparse_predictions (:1302-1358) walks the previous layer's
//     entries IN THEIR ORDER and appends, for each, the children (in C's stored order) that belong to
//     this layer's pattern -- that walk defines the order of the output row;
//   * scores come from the CSC route (vector_ops::inner_product, :1018-1078), K4 in xrl_pairs.hip.
// Two forms.  predict_selected (the c_xlinear_predict_on_selected_outputs_* entry points, csr_codes, the single-layer API): the pattern
// bookkeeping runs on the host, the inner products, transform and combine on the GPU, one launch and one synchronisation per layer.
// predict_selected_device (xrl_predict_selected_device): the labels are fixed-stride rows in HBM, K7 (xrl_select_plan.hip) plans the same walk on
// the device and the layers are scored without a visit to the host.
#include <algorithm>

#include "xrl_predict.h"

namespace xrl {

namespace {
// what a bad row is told, by the host walk below and by the device form's synchronous return alike
const char* const kFeatureDimMsg = "Feature dimension of query matrix does not match weight matrix";
const char* const kOutOfRangeMsg = "selected_outputs_csr holds a label id out of range";
std::string twice_msg(uint64_t row) { return "selected_outputs_csr row " + std::to_string(row) + " holds a label twice"; }
std::string no_parent_msg(uint32_t node, size_t layer) { return "selected label " + std::to_string(node) + " has no parent in layer " + std::to_string(layer) + " (pruned tree)"; }
}  // namespace

void predict_selected(Model& m, const QueriesDev& X, uint32_t s_rows, uint32_t s_cols, const uint64_t* s_ptr,
                      const uint32_t* s_idx, const char* post_processor, std::vector<uint32_t>& out_idx,
                      std::vector<float>& out_val, const SelectedInit* init) {
    const size_t T = m.layers.size();
    const Layer& last = *m.layers.back();
    const uint32_t out_cols = last.reordered ? last.c_rows : last.w_cols;
    if (s_rows != X.rows) fail("Instance dimension of query and selected output matrix do not match");
    if (s_cols != out_cols) fail("Label dimension of selected output matrix does not match");
    if (!X.dense && X.cols != m.nr_features && X.cols != m.layers[0]->w_rows) fail(kFeatureDimMsg);
    const uint32_t N = s_rows;
    const uint64_t nnz = s_ptr[N];

    // ---- patterns, bottom-up (sorted unique per query)
    std::vector<std::vector<uint64_t>> pat_ptr(T, std::vector<uint64_t>(N + 1, 0));
    std::vector<std::vector<uint32_t>> pat(T);
    pat[T - 1].assign(s_idx, s_idx + nnz);
    for (uint32_t q = 0; q <= N; ++q) pat_ptr[T - 1][q] = s_ptr[q];
    for (uint32_t q = 0; q < N; ++q) {
        auto b = pat[T - 1].begin() + s_ptr[q], e = pat[T - 1].begin() + s_ptr[q + 1];
        std::sort(b, e);
        if (std::adjacent_find(b, e) != e) fail(twice_msg(q));
        if (b != e && *(e - 1) >= out_cols) fail(kOutOfRangeMsg);
    }
    for (size_t l = T - 1; l > 0; --l) {
        const Layer& L = *m.layers[l];
        std::vector<uint32_t> tmp;
        for (uint32_t q = 0; q < N; ++q) {
            tmp.clear();
            for (uint64_t i = pat_ptr[l][q]; i < pat_ptr[l][q + 1]; ++i) {
                const uint32_t pr = L.h_parent[pat[l][i]];
                if (pr == 0xFFFFFFFFu) fail(no_parent_msg(pat[l][i], l));
                tmp.push_back(pr);
            }
            std::sort(tmp.begin(), tmp.end());
            tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
            pat[l - 1].insert(pat[l - 1].end(), tmp.begin(), tmp.end());
            pat_ptr[l - 1][q + 1] = pat[l - 1].size();
        }
    }

    // ---- traversal order, top-down (prolongate_sparse_predictions)
    std::vector<std::vector<uint32_t>> node(T), ppos(T), pair_q(T);
    std::vector<uint32_t> mark;
    // previous-layer predictions entering layer 0: the implicit root (ones(N x 1)), explicit csr_codes, or
    // ones(N x C.cols) without combine (single-layer API, libpecos.cpp:237-274)
    std::vector<uint64_t> init_ptr; std::vector<uint32_t> init_node; std::vector<float> init_val;
    const bool has_init = init != nullptr;
    if (has_init) {
        const uint32_t P0 = m.layers[0]->c_cols;
        init_ptr.assign(N + 1, 0);
        if (init->codes) {
            if (init->codes->rows != N) fail("Instance dimension of query and prev_layer_pred matrix do not match");
            if (init->codes->cols != P0) fail("Label dimension of prev_layer_pred and C matrix do not match");
            const uint64_t cn = init->codes->row_ptr[N];
            init_ptr.assign(init->codes->row_ptr, init->codes->row_ptr + N + 1);
            init_node.assign(init->codes->col_idx, init->codes->col_idx + cn);
            init_val.assign(init->codes->val, init->codes->val + cn);
        } else {
            init_node.resize((size_t)N * P0); init_val.assign((size_t)N * P0, 1.0f);
            for (uint32_t q = 0; q < N; ++q) { init_ptr[q + 1] = (uint64_t)(q + 1) * P0; for (uint32_t p = 0; p < P0; ++p) init_node[(size_t)q * P0 + p] = p; }
        }
    }
    for (size_t l = 0; l < T; ++l) {
        const Layer& L = *m.layers[l];
        mark.assign((size_t)L.c_rows + 1, 0u);
        node[l].reserve(pat[l].size()); ppos[l].reserve(pat[l].size()); pair_q[l].reserve(pat[l].size());
        for (uint32_t q = 0; q < N; ++q) {
            const uint32_t stamp = q + 1;
            for (uint64_t i = pat_ptr[l][q]; i < pat_ptr[l][q + 1]; ++i) mark[pat[l][i]] = stamp;
            const uint64_t before = node[l].size();
            const uint64_t pb = l ? pat_ptr[l - 1][q] : (has_init ? init_ptr[q] : 0), pe = l ? pat_ptr[l - 1][q + 1] : (has_init ? init_ptr[q + 1] : 1);
            for (uint64_t i = pb; i < pe; ++i) {
                const uint32_t parent = l ? node[l - 1][i] : (has_init ? init_node[i] : 0u);   // previous layer's ORDERED list
                if (parent >= L.c_cols) fail("selected-output walk left the tree");
                for (uint64_t c = L.h_c_ptr[parent]; c < L.h_c_ptr[parent + 1]; ++c) {
                    const uint32_t j = L.h_c_idx[c];
                    if (mark[j] == stamp) { node[l].push_back(j); ppos[l].push_back((uint32_t)(i - pb)); pair_q[l].push_back(q); }
                }
            }
            if (node[l].size() - before != pat_ptr[l][q + 1] - pat_ptr[l][q]) fail("selected-output pattern is inconsistent with the cluster chain");
        }
    }

    // ---- device: one K4 launch per layer
    if (!m.ws) m.ws = std::make_unique<Workspace>();
    hipStream_t stream = m.stream;
    DevBuf d_node, d_ppos, d_q, d_off[2], d_val[2];
    if (has_init) { d_off[1].upload(init_ptr); d_val[1].upload(init_val); }   // plays "layer -1" (prv of layer 0)
    for (size_t l = 0; l < T; ++l) {
        Layer& L = *m.layers[l];
        ensure_device_csc(L);
        const uint64_t np = node[l].size();
        d_node.upload(node[l]); d_ppos.upload(ppos[l]); d_q.upload(pair_q[l]);
        const int cur = (int)(l & 1), prv = cur ^ 1;
        d_off[cur].upload(pat_ptr[l]);
        d_val[cur].reserve(np * 4);
        const PostProc pp = post_processor ? parse_post_processor(post_processor) : L.pp;
        launch_k4_selected(L.d_csc_ptr.as<uint64_t>(), L.d_csc_idx.as<uint32_t>(), L.d_csc_val.as<float>(), L.w_rows, L.bias, X,
                           d_q.as<uint32_t>(), d_node.as<uint32_t>(), d_ppos.as<uint32_t>(),
                           (l || has_init) ? d_off[prv].as<uint64_t>() : nullptr, (l || has_init) ? d_val[prv].as<float>() : nullptr,
                           d_val[cur].as<float>(), np, pp, (l == 0 && (!has_init || init->no_prev_pred)) ? 1 : 0, stream);
        XRL_HIP(hipStreamSynchronize(stream));   // the upload buffers are reused by the next layer
    }
    out_idx = std::move(node[T - 1]);
    out_val.resize(out_idx.size());
    if (!out_val.empty())
        XRL_HIP(hipMemcpy(out_val.data(), d_val[(T - 1) & 1].p, out_val.size() * 4, hipMemcpyDeviceToHost));
}

// ---------------------------------------------------------------------------------------------
// The device form: labels in fixed-stride rows in HBM, the walk planned by K7 (xrl_select_plan.hip), one K4 launch per layer on the planned slots,
// nothing visits the host between the launches.
// ---------------------------------------------------------------------------------------------
void check_selected_inputs(const Model& m, const QueriesDev& X) {
    if (!X.dense && X.cols != m.nr_features && X.cols != m.layers[0]->w_rows) fail(kFeatureDimMsg);
    for (const auto& L : m.layers)
        if (!L->csc_ready && !L->w_host && L->w_path.empty()) fail("predict_on_selected_outputs: the layer's CSC weights are not available");
}

namespace {
// the host path's message for the bad row the status word names: the row's labels come back and the host checks them the way predict_selected does
std::string bad_row_message(const Model& m, uint32_t code, uint32_t row, const uint32_t* d_sel_idx, const uint32_t* d_sel_cnt, uint32_t sel_stride) {
    if (code == kSelectOutOfRange) return kOutOfRangeMsg;
    if (code == kSelectTwice) return twice_msg(row);
    uint32_t n = sel_stride;
    if (d_sel_cnt) XRL_HIP(hipMemcpy(&n, d_sel_cnt + row, 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> cur(std::min(n, sel_stride)), up;
    if (!cur.empty()) XRL_HIP(hipMemcpy(cur.data(), d_sel_idx + (uint64_t)row * sel_stride, cur.size() * 4, hipMemcpyDeviceToHost));
    for (size_t l = m.layers.size(); l-- > 0;) {
        const Layer& L = *m.layers[l];
        std::sort(cur.begin(), cur.end());
        cur.erase(std::unique(cur.begin(), cur.end()), cur.end());
        up.clear();
        for (uint32_t v : cur) {
            const uint32_t pr = v < L.h_parent.size() ? L.h_parent[v] : kSelectNone;
            if (pr == kSelectNone || (l == 0 && pr != 0)) return no_parent_msg(v, l);
            up.push_back(pr);
        }
        cur.swap(up);
    }
    return "selected-output pattern is inconsistent with the cluster chain";
}
}  // namespace

void predict_selected_device(Model& m, const QueriesDev& X, const char* post_processor, const uint32_t* d_sel_idx, const uint32_t* d_sel_cnt,
                             uint32_t sel_stride, uint32_t* d_out_idx, float* d_out_val, uint32_t* d_out_cnt, uint32_t out_stride,
                             uint32_t* d_status, hipStream_t stream, bool sync) {
    const size_t T = m.layers.size();
    const Layer& last = *m.layers.back();
    const uint32_t N = X.rows;
    if (!m.ws) m.ws = std::make_unique<Workspace>();
    Workspace& ws = *m.ws;
    if (!stream) stream = m.stream;
    for (auto& L : m.layers) ensure_device_csc(*L);
    ensure_device_tree(m);
    // the scratch buffers are shared by every predict of the handle: an asynchronous one still running on another stream must finish first
    if (m.ws_done && m.ws_stream != stream) XRL_HIP(hipStreamWaitEvent(stream, m.ws_done, 0));

    // rows per batch: T rows of nodes and parent positions, two of values, T counts per query row, within the candidate budget; one K4 grid
    const uint64_t row_bytes = (uint64_t)sel_stride * 4 * (2 * T + 2) + 4 * T;
    uint64_t nb = std::max<uint64_t>(1, kCandBudgetBytes / row_bytes);
    nb = std::min<uint64_t>(nb, (0x7FFFFFFFull * 16) / sel_stride);
    if (m.opt.max_batch_rows > 0) nb = std::min<uint64_t>(nb, (uint64_t)m.opt.max_batch_rows);
    nb = std::min<uint64_t>(nb, N);
    const uint64_t layer_elems = nb * sel_stride;
    ws.sel_node.reserve(T * layer_elems * 4); ws.sel_ppos.reserve(T * layer_elems * 4); ws.sel_cnt.reserve(T * nb * 4);
    ws.sel_val[0].reserve(layer_elems * 4); ws.sel_val[1].reserve(layer_elems * 4);
    ws.sel_status.reserve(8);
    XRL_HIP(hipMemsetAsync(ws.sel_status.p, 0x00, 4, stream));                                 // {code 0, row 0xFFFFFFFF}: no bad row
    XRL_HIP(hipMemsetAsync(static_cast<char*>(ws.sel_status.p) + 4, 0xFF, 4, stream));

    for (uint64_t row0 = 0; row0 < N; row0 += nb) {
        const uint32_t nrows = (uint32_t)std::min<uint64_t>(nb, N - row0);
        SelectPlanArgs P{};
        P.sel_idx = d_sel_idx; P.sel_cnt = d_sel_cnt; P.sel_stride = sel_stride; P.row0 = (uint32_t)row0; P.nrows = nrows;
        P.depth = (uint32_t)T; P.nr_labels = last.reordered ? last.c_rows : last.w_cols; P.tree = m.d_sel_tree.as<SelectTreeLayer>();
        P.node = ws.sel_node.as<uint32_t>(); P.ppos = ws.sel_ppos.as<uint32_t>(); P.cnt = ws.sel_cnt.as<uint32_t>();
        P.layer_elems = layer_elems; P.layer_rows = nb;
        P.out_idx = d_out_idx; P.out_cnt = d_out_cnt; P.out_stride = out_stride; P.status = ws.sel_status.as<unsigned long long>();
        profiled(m, stream, "k7_select_plan", 0, [&] { launch_select_plan(P, stream); });
        for (size_t l = 0; l < T; ++l) {
            const Layer& L = *m.layers[l];
            const bool final_layer = l + 1 == T;
            const int cur = (int)(l & 1), prv = cur ^ 1;
            SelectScoreArgs S{};
            S.col_ptr = L.d_csc_ptr.as<uint64_t>(); S.row_idx = L.d_csc_idx.as<uint32_t>(); S.val = L.d_csc_val.as<float>(); S.w_rows = L.w_rows; S.bias = L.bias;
            S.node = final_layer ? d_out_idx + row0 * out_stride : P.node + l * layer_elems; S.node_stride = final_layer ? out_stride : sel_stride;
            S.ppos = P.ppos + l * layer_elems; S.cnt = P.cnt + l * nb;
            S.prev_val = l ? ws.sel_val[prv].as<float>() : nullptr;
            S.out_val = final_layer ? d_out_val + row0 * out_stride : ws.sel_val[cur].as<float>(); S.out_stride = final_layer ? out_stride : sel_stride;
            S.row0 = (uint32_t)row0; S.nrows = nrows; S.sel_stride = sel_stride;
            const PostProc pp = post_processor ? parse_post_processor(post_processor) : L.pp;
            profiled(m, stream, "k4_selected_dev", (uint32_t)l, [&] { launch_k4_selected_dev(S, X, pp, stream); });
        }
    }
    if (d_status) XRL_HIP(hipMemcpyAsync(d_status, ws.sel_status.p, 8, hipMemcpyDeviceToDevice, stream));
    if (!m.ws_done) XRL_HIP(hipEventCreateWithFlags(&m.ws_done, hipEventDisableTiming));
    XRL_HIP(hipEventRecord(m.ws_done, stream)); m.ws_stream = stream;
    if (!sync) return;
    uint32_t st[2] = {0, 0};
    XRL_HIP(hipMemcpyAsync(st, ws.sel_status.p, 8, hipMemcpyDeviceToHost, stream));
    XRL_HIP(hipStreamSynchronize(stream));
    if (st[0] != kSelectOk) fail(bad_row_message(m, st[0], st[1], d_sel_idx, d_sel_cnt, sel_stride));
}

}  // namespace xrl
