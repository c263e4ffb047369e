// In-memory models and the entry points around caller-owned weights: xrl_model_create, the single-layer API with its handle cache,
// predict-on-selected-outputs, and the sparse inner products -- with their extern "C" wrappers.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>

#include "xrl_host_pipeline.h"
#include "xrl_match.h"

using namespace xrl;

namespace {
HostCsc host_csc(const ScipyCscF32* M, const char* what) {
    if (!M) fail(std::string("null ") + what);
    HostCsc h; h.rows = M->rows; h.cols = M->cols;
    h.col_ptr.assign(M->col_ptr, M->col_ptr + M->cols + 1);
    const uint64_t nnz = h.col_ptr.back();
    h.row_idx.assign(M->row_idx, M->row_idx + nnz);
    h.val.assign(M->val, M->val + nnz);
    return h;
}

// labels x 1, every label in the one cluster: the C of a layer that is given none
HostCsc one_cluster(uint32_t labels) {
    HostCsc c; c.rows = labels; c.cols = 1; c.col_ptr = {0, labels};
    c.row_idx.resize(labels); c.val.assign(labels, 1.f);
    for (uint32_t i = 0; i < labels; ++i) c.row_idx[i] = i;
    return c;
}

std::unique_ptr<Model> model_from_arrays(uint32_t depth, const ScipyCscF32* const* W, const ScipyCscF32* const* C,
                                         const float* bias, const uint32_t* only_topk, const char* const* pp, bool csc_route = false) {
    auto m = std::make_unique<Model>();
    m->csc_route = csc_route;
    if (csc_route) m->weight_matrix_type = 0;
    m->device = g_device;
    for (uint32_t d = 0; d < depth; ++d) {
        HostCsc w = host_csc(W[d], "W");
        HostCsc c = (C && C[d]) ? host_csc(C[d], "C") : one_cluster(w.cols);
        m->layers.push_back(compile_layer(w, c, bias[d], only_topk[d], pp[d] ? pp[d] : "noop", nullptr, 0, csc_route));
        m->layers.back()->w_host = std::make_shared<HostCsc>(std::move(w));
    }
    finalize_model(*m);
    return m;
}

// ---- single-layer API (libpecos.cpp:201-274): the reference builds a temporary MLModel<csc_t> around the caller's W / C
// on every call.  Here the compiled one-layer handle (tree bookkeeping + W in CSC form on the device) is CACHED, keyed
// by the identity of the caller's arrays (pointers, shapes, nnz, bias) plus a fingerprint of their contents, so that
// loops which call the layer again and again with the same weights -- MAN negative mining (xmc/base.py:1562-1563), the
// matcher -> ranker hand-off -- pay the compile + upload once.  The fingerprint covers every byte of W and C, so an in-place
// edit is seen on the next call; xrl_single_layer_cache_clear() drops every entry (frees the device copies).
struct SlKey {
    // identity of the caller's VALUE arrays (the reference's Python binding hands over W.data / C.data as they are, while
    // the index arrays are re-cast to u32 / u64 copies on every call, pecos/core/base.py:235-239), shapes, nnz, bias,
    // and a fingerprint of the contents of all arrays
    const void *wv, *cv;
    uint32_t wr, wc, cr, cc; uint64_t wnnz, cnnz; float bias; uint64_t fp; int device;
    bool operator==(const SlKey& o) const {
        return wv == o.wv && cv == o.cv && wr == o.wr && wc == o.wc && cr == o.cr &&
               cc == o.cc && wnnz == o.wnnz && cnnz == o.cnnz && bias == o.bias && fp == o.fp && device == o.device;
    }
};
struct SlEntry { SlKey key; std::shared_ptr<Model> model; uint64_t stamp; };
std::mutex g_sl_mu;
std::vector<SlEntry> g_sl_cache;
uint64_t g_sl_clock = 0, g_sl_hits = 0, g_sl_misses = 0;
constexpr size_t kSlCacheCap = 8;

uint64_t fingerprint(uint64_t h, const void* data, size_t elems, size_t elem_bytes) {
    // 64-bit hash of EVERY byte (four independent multiply-xorshift lanes over 8-byte words, ~10 GB/s on one core): an in-place
    // edit of W / C anywhere, or a different matrix of the same shape at the same address, changes the key -- cheap next to the
    // compile + upload a hit saves
    const unsigned char* p = static_cast<const unsigned char*>(data);
    size_t n = elems * elem_bytes;
    if (!p || !n) return h ^ 0x9E3779B97F4A7C15ull;
    uint64_t l[4] = {h ^ 0x243F6A8885A308D3ull, h ^ 0x13198A2E03707344ull, h ^ 0xA4093822299F31D0ull, h ^ 0x082EFA98EC4E6C89ull};
    auto mix = [](uint64_t a, uint64_t w) { a = (a ^ w) * 0x9FB21C651E98DF25ull; return a ^ (a >> 29); };
    while (n >= 32) {
        uint64_t w[4]; std::memcpy(w, p, 32);
        l[0] = mix(l[0], w[0]); l[1] = mix(l[1], w[1]); l[2] = mix(l[2], w[2]); l[3] = mix(l[3], w[3]);
        p += 32; n -= 32;
    }
    uint64_t tail[4] = {0, 0, 0, 0}; std::memcpy(tail, p, n);
    for (int i = 0; i < 4; ++i) l[i] = mix(l[i], tail[i] + n);
    return mix(mix(mix(l[0], l[1]), l[2]), l[3]) ^ (uint64_t)(elems * elem_bytes);
}

std::shared_ptr<Model> single_layer_model(const ScipyCscF32* W, const ScipyCscF32* C, float bias) {
    if (!W) fail("null W");
    SlKey k{};
    k.wv = W->val; k.wr = W->rows; k.wc = W->cols; k.wnnz = W->cols ? W->col_ptr[W->cols] : 0;
    k.cv = C ? (const void*)C->val : nullptr;
    k.cr = C ? C->rows : 0; k.cc = C ? C->cols : 0; k.cnnz = (C && C->cols) ? C->col_ptr[C->cols] : 0;
    k.bias = bias; k.device = g_device;
    uint64_t h = 1469598103934665603ull;
    h = fingerprint(h, W->col_ptr, (size_t)W->cols + 1, 8);
    h = fingerprint(h, W->row_idx, k.wnnz, 4);
    h = fingerprint(h, W->val, k.wnnz, 4);
    if (C) { h = fingerprint(h, C->col_ptr, (size_t)C->cols + 1, 8); h = fingerprint(h, C->row_idx, k.cnnz, 4); h = fingerprint(h, C->val, k.cnnz, 4); }
    k.fp = h;
    {
        std::lock_guard<std::mutex> g(g_sl_mu);
        for (auto& e : g_sl_cache) if (e.key == k) { e.stamp = ++g_sl_clock; ++g_sl_hits; return e.model; }
        ++g_sl_misses;
    }
    const ScipyCscF32* Wp = W; const ScipyCscF32* Cp = C;
    const uint32_t topk = 0; const char* pps = "noop";     // per call: only_topk and the post-processor arrive through PredictOpts
    std::shared_ptr<Model> m = model_from_arrays(1, &Wp, &Cp, &bias, &topk, &pps, /*csc_route=*/true);
    m->ws = std::make_unique<Workspace>();
    ensure_device_csc(*m->layers[0]);
    std::lock_guard<std::mutex> g(g_sl_mu);
    if (g_sl_cache.size() >= kSlCacheCap) {
        size_t victim = 0;
        for (size_t i = 1; i < g_sl_cache.size(); ++i) if (g_sl_cache[i].stamp < g_sl_cache[victim].stamp) victim = i;
        g_sl_cache.erase(g_sl_cache.begin() + victim);
    }
    g_sl_cache.push_back(SlEntry{k, m, ++g_sl_clock});
    return m;
}

void single_layer_predict(const HostX& x, const ScipyCsrF32* csr_codes, ScipyCscF32* W, ScipyCscF32* C,
                          const char* pp, uint32_t only_topk, float bias, py_sparse_allocator_t alloc) {
    // libpecos.cpp:201-235: MLModel<csc_t> around caller-owned W / C -> the CSC arithmetic (K1C), bit for bit
    require_gpu();
    use_device(g_device);
    if (!alloc) fail("null allocator callback");
    const char* pps = pp ? pp : "noop";
    std::shared_ptr<Model> mp = single_layer_model(W, C, bias);
    Model& m = *mp;
    std::lock_guard<std::mutex> g(m.mu);
    Workspace& ws = *m.ws;
    QueriesDev X{};
    upload_x(x, ws.x_ptr, ws.x_idx, ws.x_val, X);
    PredictOpts o; o.only_topk = only_topk; o.post_processor = pps; o.csc_route = true;
    if (only_topk == 0) fail("only_topk must be positive");
    BeamDev init{};
    const Layer& L = *m.layers[0];
    const uint32_t P = L.c_cols;
    std::vector<uint32_t> hi, hc; std::vector<float> hv;
    uint32_t stride = 1;
    const bool with_codes = csr_codes != nullptr;
    if (with_codes) {
        if (csr_codes->rows != X.rows) fail("Instance dimension of query and prev_layer_pred matrix do not match");
        if (csr_codes->cols != P) fail("Label dimension of prev_layer_pred and C matrix do not match");
        // every parent id must exist; a row may list a parent more than once (a non-canonical CSR): the reference
        // prolongates each occurrence, so the candidate row is sized from the real per-row sum of chunk sizes
        uint64_t bound = 1;
        for (uint32_t r = 0; r < X.rows; ++r) {
            const uint64_t b = csr_codes->row_ptr[r], e = csr_codes->row_ptr[r + 1];
            if (e < b) fail("csr_codes: row_ptr is not monotone");
            stride = std::max<uint32_t>(stride, (uint32_t)(e - b));
            uint64_t sum = 0;
            for (uint64_t t = b; t < e; ++t) {
                const uint32_t p = csr_codes->col_idx[t];
                if (p >= P) fail("csr_codes: parent id " + std::to_string(p) + " out of range (C has " + std::to_string(P) + " columns)");
                sum += L.h_c_ptr[p + 1] - L.h_c_ptr[p];
            }
            bound = std::max(bound, sum);
        }
        o.initial_cand_bound = bound;
        hi.assign((size_t)X.rows * stride, 0); hv.assign((size_t)X.rows * stride, 0.f); hc.assign(X.rows, 0);
        for (uint32_t r = 0; r < X.rows; ++r) {
            const uint64_t b = csr_codes->row_ptr[r], e = csr_codes->row_ptr[r + 1];
            hc[r] = (uint32_t)(e - b);
            for (uint64_t t = b; t < e; ++t) { hi[(size_t)r * stride + (t - b)] = csr_codes->col_idx[t]; hv[(size_t)r * stride + (t - b)] = csr_codes->val[t]; }
        }
    } else if (P > 1) {   // fill_ones(X.rows, C->cols): every parent, score 1, and NO combine
        stride = P;
        hi.resize((size_t)X.rows * P); hv.assign((size_t)X.rows * P, 1.f); hc.assign(X.rows, P);
        for (uint32_t r = 0; r < X.rows; ++r) for (uint32_t p = 0; p < P; ++p) hi[(size_t)r * P + p] = p;
    }
    if (!hi.empty()) {
        ws.init_idx.upload(hi); ws.init_val.upload(hv); ws.init_cnt.upload(hc);
        init = BeamDev{ws.init_idx.as<uint32_t>(), ws.init_val.as<float>(), ws.init_cnt.as<uint32_t>(), stride};
        o.initial = &init; o.initial_max = stride;
    }
    o.no_prev_pred = !with_codes;   // combine only when csr_codes were given (libpecos.cpp:215-222)
    run_and_emit(m, X, o, alloc);
}

// The resident form (xrl_single_layer_predict_device): X, W^T and the codes are in HBM already.  The one-layer model is compiled around an
// EMPTY weight pattern (tree bookkeeping only, from a host copy of C: nr_labels entries) and W's CSC arrays -- the CSR arrays of W^T -- are
// copied device to device; then the same CSC route through the same predict_device as the host form.
void single_layer_predict_device(void* Xh, void* Wth, void* Cth, const uint32_t* d_ci, const float* d_cv, const uint32_t* d_cc, uint32_t c_stride, const char* pp,
                                 uint32_t only_topk, float bias, uint32_t* d_oi, float* d_ov, uint32_t* d_oc, uint32_t out_stride, hipStream_t s) {
    const std::string what = "xrl_single_layer_predict_device: ";
    const Queries& x = csr_handle(what, Xh, "X");
    const Queries& wt = csr_handle(what, Wth, "Wt");
    const Queries* ct = Cth ? &csr_handle(what, Cth, "Ct") : nullptr;
    if (only_topk == 0) fail(what + "only_topk must be positive");
    if (out_stride < only_topk) fail(what + "out_stride (" + std::to_string(out_stride) + ") is smaller than only_topk (" + std::to_string(only_topk) + ")");
    if (!d_oi || !d_ov || !d_oc) fail(what + "null output buffer");
    const bool with_codes = d_ci || d_cv || d_cc;
    if (with_codes && (!d_ci || !d_cv || !d_cc)) fail(what + "csr_codes: labels, scores and counts come together or not at all");
    if (with_codes && c_stride == 0) fail(what + "csr_codes: a stride of 0");
    const char* pps = pp ? pp : "noop";                    // (an unknown name is the identity, as in the host form and the reference)
    for (const Queries* o : {&wt, ct})
        if (o && o->device != x.device) fail(what + "the operands are on devices " + std::to_string(x.device) + " and " + std::to_string(o->device) + "; a predict needs all on one");
    const uint32_t w_rows = wt.dev.cols, labels = wt.dev.rows;
    if (x.dev.cols + (bias > 0 ? 1u : 0u) != w_rows)
        fail(what + "Feature dimension of query and W do not match (X has " + std::to_string(x.dev.cols) + " columns, bias " + (bias > 0 ? "adds one" : "adds none") + ", W has " +
             std::to_string(w_rows) + " rows)");
    if (ct && ct->dev.cols != labels) fail(what + "Label dimension of C and W do not match (" + std::to_string(ct->dev.cols) + " != " + std::to_string(labels) + ")");
    require_gpu();
    use_device(x.device);

    // the tree bookkeeping: C on the host (Ct's CSR arrays are C's CSC arrays), or one cluster that holds every label
    HostCsc c;
    if (!ct) c = one_cluster(labels);
    else {
        c.rows = labels; c.cols = ct->dev.rows;
        c.col_ptr.resize((size_t)c.cols + 1); c.row_idx.resize((size_t)ct->dev.nnz); c.val.resize((size_t)ct->dev.nnz);
        XRL_HIP(hipStreamSynchronize(s));
        download_csr(ct->dev, c.col_ptr.data(), c.row_idx.data(), c.val.data());
        if (c.col_ptr[c.cols] != ct->dev.nnz) fail(what + "Ct's row pointer does not end at its entry count");
        for (uint32_t p = 0; p < c.cols; ++p) if (c.col_ptr[p + 1] < c.col_ptr[p]) fail(what + "Ct's row pointer does not ascend");
        for (uint32_t l : c.row_idx) if (l >= labels) fail(what + "Ct holds an id that is not below " + std::to_string(labels));
    }
    HostCsc w;                                             // shape only: compile_layer(structure_only) reads no weight
    w.rows = w_rows; w.cols = labels; w.col_ptr.assign((size_t)labels + 1, 0);
    Model m;
    m.csc_route = true; m.weight_matrix_type = 0; m.device = x.device;
    m.layers.push_back(compile_layer(w, c, bias, 0, "noop", nullptr, 0, /*structure_only=*/true));
    Layer& L = *m.layers[0];
    L.w_absmax = INFINITY;                                 // the weights were never on the host: nothing is priced with them (the CSC route does not prune)
    finalize_model(m);
    if (!s) { XRL_HIP(hipStreamSynchronize(nullptr)); s = m.stream; }   // the default stream: what it holds is done, then the model's own (as the host form runs)
    L.d_csc_ptr.reserve(((size_t)labels + 1) * 8); L.d_csc_idx.reserve((size_t)wt.dev.nnz * 4); L.d_csc_val.reserve((size_t)wt.dev.nnz * 4);
    XRL_HIP(hipMemcpyAsync(L.d_csc_ptr.p, wt.dev.row_ptr, ((size_t)labels + 1) * 8, hipMemcpyDeviceToDevice, s));
    if (wt.dev.nnz) {
        XRL_HIP(hipMemcpyAsync(L.d_csc_idx.p, wt.dev.col_idx, (size_t)wt.dev.nnz * 4, hipMemcpyDeviceToDevice, s));
        XRL_HIP(hipMemcpyAsync(L.d_csc_val.p, wt.dev.val, (size_t)wt.dev.nnz * 4, hipMemcpyDeviceToDevice, s));
    }
    L.csc_ready = true;
    m.ws = std::make_unique<Workspace>();
    if (const char* e = std::getenv("XRL_SINGLE_LAYER_MAX_BATCH_ROWS")) m.opt.max_batch_rows = std::strtoll(e, nullptr, 10);   // (tests: few rows in several batches)

    PredictOpts o; o.only_topk = only_topk; o.post_processor = pps; o.csc_route = true;
    const uint32_t P = L.c_cols;
    BeamDev init{};
    if (with_codes) {
        // the codes are used in place; their parents are checked and the candidate row sized by one kernel and one 8-byte readback
        bool bad = false;
        const uint64_t bound = beam_cand_bound_device(d_ci, d_cc, c_stride, x.dev.rows, L.dev.chunk_col, P, s, bad);
        if (bad) fail(what + "csr_codes: parent id " + std::to_string(bound) + " out of range (C has " + std::to_string(P) + " columns)");
        note_cand_bound(std::max<uint64_t>(1, bound));
        o.initial_cand_bound = std::max<uint64_t>(1, bound);
        init = BeamDev{const_cast<uint32_t*>(d_ci), const_cast<float*>(d_cv), const_cast<uint32_t*>(d_cc), c_stride};
        o.initial = &init; o.initial_max = c_stride;
    } else if (P > 1) {   // fill_ones(X.rows, C->cols): every parent, score 1, and NO combine
        Workspace& ws = *m.ws;
        const size_t n = (size_t)x.dev.rows * P;
        ws.init_idx.reserve(n * 4); ws.init_val.reserve(n * 4); ws.init_cnt.reserve((size_t)x.dev.rows * 4);
        fill_ones_beam_device(ws.init_idx.as<uint32_t>(), ws.init_val.as<float>(), ws.init_cnt.as<uint32_t>(), x.dev.rows, P, s);
        init = BeamDev{ws.init_idx.as<uint32_t>(), ws.init_val.as<float>(), ws.init_cnt.as<uint32_t>(), P};
        o.initial = &init; o.initial_max = P;
        note_cand_bound(labels);
    } else note_cand_bound(labels);
    o.no_prev_pred = !with_codes;   // combine only when csr_codes were given (libpecos.cpp:215-222)
    if (x.dev.rows) predict_device(m, x.dev, o, d_oi, d_ov, d_oc, out_stride, s, /*sync=*/true);
    else XRL_HIP(hipStreamSynchronize(s));
}

// X to the device, the scores of S's pattern, and their hand-off through the allocator: S's row pointer, the scores in its order
void predict_selected_emit(Model& m, const HostX& x, const ScipyCsrF32* S, const char* pp, const SelectedInit* init, py_sparse_allocator_t alloc) {
    QueriesDev X{};
    upload_x(x, m.ws->x_ptr, m.ws->x_idx, m.ws->x_val, X);
    std::vector<uint32_t> oi; std::vector<float> ov;
    predict_selected(m, X, S->rows, S->cols, S->row_ptr, S->col_idx, pp, oi, ov, init);
    uint32_t* o_idx = nullptr; uint64_t* o_ptr = nullptr; float* o_val = nullptr;
    alloc(false, S->rows, S->cols, oi.size(), &o_idx, &o_ptr, &o_val);
    if (!o_ptr || (!oi.empty() && (!o_idx || !o_val))) fail("allocator callback returned null buffers");
    std::memcpy(o_ptr, S->row_ptr, ((size_t)S->rows + 1) * 8);
    if (!oi.empty()) { std::memcpy(o_idx, oi.data(), oi.size() * 4); std::memcpy(o_val, ov.data(), ov.size() * 4); }
}

void selected_host(void* ptr, const HostX& x, const ScipyCsrF32* S, const char* pp, py_sparse_allocator_t alloc) {
    // libpecos.cpp:179-198 (C_XLINEAR_PREDICT_ON_SELECTED_OUTPUTS)
    Model& m = *as_model(ptr);
    if (!alloc) fail("null allocator callback");
    if (!S) fail("null selected_outputs_csr");
    std::lock_guard<std::mutex> g(m.mu);
    use_device(m.device);
    if (!m.ws) m.ws = std::make_unique<Workspace>();
    predict_selected_emit(m, x, S, pp, nullptr, alloc);
}

void single_layer_selected(const HostX& x, const ScipyCsrF32* S, const ScipyCsrF32* csr_codes, ScipyCscF32* W,
                           ScipyCscF32* C, const char* pp, float bias, py_sparse_allocator_t alloc) {
    // libpecos.cpp:237-274: a temporary one-layer model around caller-owned W / C, selected outputs only
    require_gpu();
    use_device(g_device);
    if (!alloc) fail("null allocator callback");
    if (!S) fail("null selected_outputs_csr");
    std::shared_ptr<Model> m = single_layer_model(W, C, bias);
    std::lock_guard<std::mutex> g(m->mu);
    ScipyCsrF32View cv{};
    SelectedInit init{nullptr, true};
    if (csr_codes) { cv = ScipyCsrF32View{csr_codes->rows, csr_codes->cols, csr_codes->row_ptr, csr_codes->col_idx, csr_codes->val}; init.codes = &cv; init.no_prev_pred = false; }
    predict_selected_emit(*m, x, S, pp ? pp : "noop", &init, alloc);
}

// W is CSC (`Wc`) or dense column-major (`Wd`): one of the two is null
void inner_products(const HostX& x, const ScipyCscF32* Wc, const ScipyDcmF32* Wd, bool w_csc, uint64_t len, uint32_t* rows, uint32_t* cols, float* out) {
    require_gpu();
    use_device(g_device);
    if (!x.given || !(w_csc ? (const void*)Wc : (const void*)Wd)) fail("null matrix");
    DevBuf xp, xi, xv, wp, wi, wv, dr, dc, dout;
    QueriesDev X{};
    upload_x(x, xp, xi, xv, X);
    uint32_t dim = x.cols;
    if (w_csc) {
        const uint64_t nnz = Wc->cols ? Wc->col_ptr[Wc->cols] : 0;
        wp.upload_raw(Wc->col_ptr, ((size_t)Wc->cols + 1) * 8); wi.upload_raw(Wc->row_idx, nnz * 4); wv.upload_raw(Wc->val, nnz * 4);
    } else {
        wv.upload_raw(Wd->val, (size_t)Wd->rows * Wd->cols * 4);
        dim = Wd->rows;
    }
    dr.upload_raw(rows, len * 4); dc.upload_raw(cols, len * 4); dout.reserve(len * 4);
    launch_k3_inner_products(X.row_ptr, X.col_idx, xv.as<float>(), x.csr ? 0 : 1, wp.as<uint64_t>(), wi.as<uint32_t>(), wv.as<float>(), w_csc ? 0 : 1, dim, len,
                             dr.as<uint32_t>(), dc.as<uint32_t>(), dout.as<float>(), nullptr);
    XRL_HIP(hipDeviceSynchronize());
    if (len) XRL_HIP(hipMemcpy(out, dout.p, len * 4, hipMemcpyDeviceToHost));
}
}  // namespace

extern "C" {

void* xrl_model_create(uint32_t depth, const ScipyCscF32* const* W, const ScipyCscF32* const* C, const float* bias,
                       const uint32_t* only_topk, const char* const* post_processor) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        require_gpu();
        use_device(g_device);
        if (!depth || !W || !bias || !only_topk || !post_processor) fail("xrl_model_create: bad arguments");
        return model_from_arrays(depth, W, C, bias, only_topk, post_processor).release();
    });
}

void c_xlinear_predict_on_selected_outputs_csr_f32(void* ptr, const ScipyCsrF32* input_x, const ScipyCsrF32* selected_outputs_csr,
                                                   const char* overridden_post_processor_str, const int /*threads*/,
                                                   py_sparse_allocator_t pred_alloc) {
    guarded([&] { selected_host(ptr, HostX(input_x), selected_outputs_csr, overridden_post_processor_str, pred_alloc); });
}

void c_xlinear_predict_on_selected_outputs_drm_f32(void* ptr, const ScipyDrmF32* input_x, const ScipyCsrF32* selected_outputs_csr,
                                                   const char* overridden_post_processor_str, const int /*threads*/,
                                                   py_sparse_allocator_t pred_alloc) {
    guarded([&] { selected_host(ptr, HostX(input_x), selected_outputs_csr, overridden_post_processor_str, pred_alloc); });
}

void c_xlinear_single_layer_predict_csr_f32(const ScipyCsrF32* input_x, const ScipyCsrF32* csr_codes, ScipyCscF32* W,
                                            ScipyCscF32* C, const char* post_processor_str, const uint32_t only_topk,
                                            const int /*num_threads*/, const float bias, py_sparse_allocator_t pred_alloc) {
    guarded([&] { single_layer_predict(HostX(input_x), csr_codes, W, C, post_processor_str, only_topk, bias, pred_alloc); });
}

void c_xlinear_single_layer_predict_drm_f32(const ScipyDrmF32* input_x, const ScipyCsrF32* csr_codes, ScipyCscF32* W,
                                            ScipyCscF32* C, const char* post_processor_str, const uint32_t only_topk,
                                            const int /*num_threads*/, const float bias, py_sparse_allocator_t pred_alloc) {
    guarded([&] { single_layer_predict(HostX(input_x), csr_codes, W, C, post_processor_str, only_topk, bias, pred_alloc); });
}

void c_xlinear_single_layer_predict_on_selected_outputs_csr_f32(const ScipyCsrF32* input_x, const ScipyCsrF32* selected_outputs_csr,
                                                                const ScipyCsrF32* csr_codes, ScipyCscF32* W, ScipyCscF32* C,
                                                                const char* post_processor_str, const int /*num_threads*/,
                                                                const float bias, py_sparse_allocator_t pred_alloc) {
    guarded([&] { single_layer_selected(HostX(input_x), selected_outputs_csr, csr_codes, W, C, post_processor_str, bias, pred_alloc); });
}

void c_xlinear_single_layer_predict_on_selected_outputs_drm_f32(const ScipyDrmF32* input_x, const ScipyCsrF32* selected_outputs_csr,
                                                                const ScipyCsrF32* csr_codes, ScipyCscF32* W, ScipyCscF32* C,
                                                                const char* post_processor_str, const int /*num_threads*/,
                                                                const float bias, py_sparse_allocator_t pred_alloc) {
    guarded([&] { single_layer_selected(HostX(input_x), selected_outputs_csr, csr_codes, W, C, post_processor_str, bias, pred_alloc); });
}

int xrl_single_layer_predict_device(void* X, void* Wt, void* Ct_or_null, const uint32_t* d_codes_idx, const float* d_codes_val, const uint32_t* d_codes_cnt,
                                    uint32_t codes_stride, const char* post_processor, uint32_t only_topk, float bias, uint32_t* d_out_idx, float* d_out_val,
                                    uint32_t* d_out_cnt, uint32_t out_stride, void* hip_stream) {
    return guarded_value(-1, [&] {
        single_layer_predict_device(X, Wt, Ct_or_null, d_codes_idx, d_codes_val, d_codes_cnt, codes_stride, post_processor, only_topk, bias, d_out_idx, d_out_val,
                                    d_out_cnt, out_stride, static_cast<hipStream_t>(hip_stream));
        return 0;
    });
}

void xrl_single_layer_cache_clear(void) {
    guarded([&] { std::lock_guard<std::mutex> g(g_sl_mu); g_sl_cache.clear(); });
}
void xrl_single_layer_cache_stats(uint64_t* hits, uint64_t* misses, uint64_t* entries) {
    std::lock_guard<std::mutex> g(g_sl_mu);
    if (hits) *hits = g_sl_hits;
    if (misses) *misses = g_sl_misses;
    if (entries) *entries = g_sl_cache.size();
}

void c_sparse_inner_products_csr2csc_f32(const ScipyCsrF32* pX, const ScipyCscF32* pW, uint64_t len, uint32_t* r, uint32_t* c, float* val, int /*threads*/) {
    guarded([&] { inner_products(HostX(pX), pW, nullptr, true, len, r, c, val); });
}
void c_sparse_inner_products_drm2csc_f32(const ScipyDrmF32* pX, const ScipyCscF32* pW, uint64_t len, uint32_t* r, uint32_t* c, float* val, int /*threads*/) {
    guarded([&] { inner_products(HostX(pX), pW, nullptr, true, len, r, c, val); });
}
void c_sparse_inner_products_csr2dcm_f32(const ScipyCsrF32* pX, const ScipyDcmF32* pW, uint64_t len, uint32_t* r, uint32_t* c, float* val, int /*threads*/) {
    guarded([&] { inner_products(HostX(pX), nullptr, pW, false, len, r, c, val); });
}
void c_sparse_inner_products_drm2dcm_f32(const ScipyDrmF32* pX, const ScipyDcmF32* pW, uint64_t len, uint32_t* r, uint32_t* c, float* val, int /*threads*/) {
    guarded([&] { inner_products(HostX(pX), nullptr, pW, false, len, r, c, val); });
}

}  // extern "C"
