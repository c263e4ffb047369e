// extern "C" surface of libxrl_amd.so (include/xrl_abi.h): device selection, model load / destruct / attributes, the host-ABI predict
// wrappers, query handles (and the upload / download / free bodies they share with the matrix handles of xrl_smat_abi.cpp),
// device-resident predicts, profile, options and the debug entry points.  The host pipeline behind
// c_xlinear_predict_* is xrl_host_pipeline.cpp, the single-layer / selected-outputs / inner-product entry points are xrl_single_layer.cpp,
// the TF-IDF producer is xrl_tfidf_abi.cpp.  Every entry point catches all C++ exceptions and records them for xrl_last_error();
// nothing is ever thrown across the C boundary.
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>

#include "xrl_host_pipeline.h"

namespace xrl {
thread_local std::string g_err;
thread_local bool g_has_err = false;
thread_local int g_device = 0;

void set_err(const std::string& s) { g_err = s; g_has_err = true; }

Model* as_model(void* p) {
    if (!p) fail("null model handle");
    return static_cast<Model*>(p);
}

void use_device(int dev) { XRL_HIP(hipSetDevice(dev)); }

void require_gpu() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        fail("libxrl_amd: no HIP device visible -- this library has no CPU fallback");
}

void upload_x(const HostX& x, DevBuf& ptr, DevBuf& idx, DevBuf& val, QueriesDev& d) {
    if (!x.given) fail("null X");
    const uint64_t elems = x.elems();
    if (x.csr) {
        if (x.rows) ptr.upload_raw(x.row_ptr, ((size_t)x.rows + 1) * 8);
        else { ptr.reserve(8); XRL_HIP(hipMemset(ptr.p, 0, 8)); }
        idx.upload_raw(x.col_idx, elems * 4);
    }
    val.upload_raw(x.val, elems * 4);
    d = device_view(x, ptr, idx, val);
}

Queries* upload_handle(const HostX& x, int device) {
    use_device(device);
    auto q = std::make_unique<Queries>();
    QueriesDev d{};
    upload_x(x, q->own.ptr, q->own.idx, q->own.val, d);
    q->own.nnz = d.nnz;
    set_view(*q, device, d);
    return q.release();
}

void download_csr(const QueriesDev& v, uint64_t* row_ptr, uint32_t* col_idx, float* val) {
    XRL_HIP(hipMemcpy(row_ptr, v.row_ptr, ((size_t)v.rows + 1) * 8, hipMemcpyDeviceToHost));
    if (v.nnz) {
        XRL_HIP(hipMemcpy(col_idx, v.col_idx, (size_t)v.nnz * 4, hipMemcpyDeviceToHost));
        XRL_HIP(hipMemcpy(val, v.val, (size_t)v.nnz * 4, hipMemcpyDeviceToHost));
    }
}

void free_handle(void* h) {
    Queries* q = static_cast<Queries*>(h);
    if (!q) return;
    if (q->own.ptr.p || q->own.idx.p || q->own.val.p) (void)hipSetDevice(q->device);
    delete q;
}
}  // namespace xrl

using namespace xrl;

extern "C" {

const char* xrl_last_error(void) { return g_has_err ? g_err.c_str() : nullptr; }
void xrl_clear_error(void) { g_has_err = false; }
const char* xrl_version(void) { return "xrl_amd 0.1 (gfx950)"; }

int xrl_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int xrl_set_device(int device) {
    return guarded_value(-1, [&] { use_device(device); g_device = device; return 0; });
}

// a model folder in the npz (kind 0) or the mmap (kind 1) layout -> a warmed-up handle on the calling thread's device
static void* load_handle(const char* model_path, int kind, int weight_matrix_type) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        if (!model_path) fail("null model path");
        require_gpu();
        use_device(g_device);
        auto m = kind == 0 ? load_model_from_disk(model_path, weight_matrix_type) : load_mmap_model_from_disk(model_path);
        m->device = g_device; m->src_path = model_path; m->src_kind = kind;
        warm_handle(*m);
        return m.release();
    });
}

void* c_xlinear_load_model_from_disk_ext(const char* model_path, int weight_matrix_type) { return load_handle(model_path, 0, weight_matrix_type); }
void* c_xlinear_load_model_from_disk(const char* model_path) { return load_handle(model_path, 0, 2 /* DEFAULT_LAYER_TYPE = BINARY_SEARCH_CHUNKED */); }
// (lazy_load: the model is copied to HBM either way)
void* c_xlinear_load_mmap_model_from_disk(const char* model_path, const bool) { return load_handle(model_path, 1, 2); }

void c_xlinear_compile_mmap_model(const char* model_path, const char* mmap_model_path) {
    guarded([&] {
        if (!model_path || !mmap_model_path) fail("null path");
        compile_mmap_model(model_path, mmap_model_path);    // host-only: no GPU needed
    });
}

void c_xlinear_destruct_model(void* ptr) {
    guarded([&] {
        if (!ptr) return;
        Model* m = static_cast<Model*>(ptr);
        (void)hipSetDevice(m->device);
        delete m;                                     // (~Model releases the replicas, streams and events, each on its own device)
    });
}

uint32_t c_xlinear_get_int_attr(void* ptr, const char* attr) {
    uint32_t v = 0;
    guarded([&] {
        Model& m = *as_model(ptr);
        if (!attr) fail("null attr");
        if (!std::strcmp(attr, "depth")) v = (uint32_t)m.layers.size();
        else if (!std::strcmp(attr, "nr_features")) v = m.nr_features;
        else if (!std::strcmp(attr, "nr_labels")) v = m.nr_labels;
        else if (!std::strcmp(attr, "nr_codes")) v = m.nr_codes;
        else if (!std::strcmp(attr, "device")) v = (uint32_t)m.device;   // additive: the GPU the handle lives on
        else if (!std::strcmp(attr, "nr_pred_cols")) {   // additive: column count of predict()'s CSR
            const Layer& last = *m.layers.back();
            v = last.reordered ? last.c_rows : last.w_cols;
        }
        else if (!std::strcmp(attr, "nr_bucket_layers")) {   // additive: layers using the bucket row lookup instead of rank-bitmaps
            for (auto& l : m.layers) v += l->dev.bucket ? 1u : 0u;
        }
        else if (!std::strcmp(attr, "nr_bitmap64_layers")) {  // additive: layers using 64-feature bitmap words that carry the first row's extent
            for (auto& l : m.layers) v += l->dev.bitmap64 ? 1u : 0u;
        }
        else if (!std::strcmp(attr, "nr_dense_layers")) {    // additive: layers that also carry the dense row format (K1Q)
            for (auto& l : m.layers) v += l->dev.wd ? 1u : 0u;
        }
        else if (!std::strcmp(attr, "merged01")) v = m.layers[0]->dev.wd01 ? 1u : 0u;   // additive: the root carries levels 0 + 1 as one merged dense matrix (LayerDev::wd01)
        else if (!std::strcmp(attr, "nr_devices")) v = 1u + (uint32_t)m.replicas.size();   // additive: devices behind the handle (xrl_set_option "devices")
        else fail(std::string(attr) + " is not implemented in get_int_attr.");
    });
    return v;
}

int c_xlinear_get_layer_type(void* ptr, int layer_depth) {
    int v = -1;
    guarded([&] {
        Model& m = *as_model(ptr);
        if (layer_depth < 0 || (size_t)layer_depth >= m.layers.size()) fail("layer_depth out of range");
        v = m.weight_matrix_type;
    });
    return v;
}

void c_xlinear_predict_csr_f32(void* ptr, const ScipyCsrF32* input_x, const uint32_t overridden_beam_size,
                               const char* overridden_post_processor_str, const uint32_t overridden_only_topk,
                               const int /*threads*/, py_sparse_allocator_t pred_alloc) {
    guarded([&] { predict_host(ptr, HostX(input_x), overridden_beam_size, overridden_post_processor_str, overridden_only_topk, pred_alloc); });
}

void c_xlinear_predict_drm_f32(void* ptr, const ScipyDrmF32* input_x, const uint32_t overridden_beam_size,
                               const char* overridden_post_processor_str, const uint32_t overridden_only_topk,
                               const int /*threads*/, py_sparse_allocator_t pred_alloc) {
    guarded([&] { predict_host(ptr, HostX(input_x), overridden_beam_size, overridden_post_processor_str, overridden_only_topk, pred_alloc); });
}

int xrl_inspect_model(const char* model_path, uint64_t* out, uint32_t cap) {
    int depth = -1;
    guarded([&] {
        if (!model_path) fail("null model path");
        const std::string path(model_path);
        const JsonValue meta = parse_json_file(path + "/param.json");
        const JsonValue* dv = meta.get("depth");
        if (!dv || dv->type != JsonValue::NUMBER) fail(path + "/param.json: missing \"depth\"");
        const int d_n = (int)dv->num;
        for (int d = 0; d < d_n; ++d) {
            const std::string lp = path + "/" + std::to_string(d) + ".model";
            (void)parse_json_file(lp + "/param.json");
            HostCsc W, C;
            load_csc_npz(lp + "/W.npz", W);
            uint64_t c_rows = W.cols, c_cols = 1, c_nnz = W.cols;
            if (!(d == 0 && !file_exists(lp + "/C.npz"))) { load_csc_npz(lp + "/C.npz", C); c_rows = C.rows; c_cols = C.cols; c_nnz = C.nnz(); }
            const uint64_t rec[6] = {W.rows, W.cols, W.nnz(), c_rows, c_cols, c_nnz};
            for (int i = 0; i < 6; ++i) if (out && (uint32_t)(6 * d + i) < cap) out[6 * d + i] = rec[i];
        }
        depth = d_n;
    });
    return depth;
}

static void* queries_upload(void* model, const HostX& x) {
    return guarded_value((void*)nullptr, [&]() -> void* { return upload_handle(x, as_model(model)->device); });
}
void* xrl_queries_upload_csr(void* model, const ScipyCsrF32* X) { return queries_upload(model, HostX(X)); }
void* xrl_queries_upload_drm(void* model, const ScipyDrmF32* X) { return queries_upload(model, HostX(X)); }

void* xrl_queries_from_device_csr(void* model, uint32_t rows, uint32_t cols, const uint64_t* d_row_ptr, const uint32_t* d_col_idx,
                                  const float* d_val, uint64_t nnz) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        Model& m = *as_model(model);
        if (rows && (!d_row_ptr || (nnz && (!d_col_idx || !d_val)))) fail("xrl_queries_from_device_csr: null device pointer");
        auto q = std::make_unique<Queries>();
        set_view(*q, m.device, csr_view(rows, cols, d_row_ptr, d_col_idx, d_val, nnz));
        return q.release();
    });
}

void* xrl_queries_tfidf_device(void* model, uint32_t rows, uint32_t cols, const uint64_t* d_row_ptr, const uint32_t* d_col_idx,
                               const float* d_count, uint64_t nnz, const float* d_idf, int binary, int sublinear_tf, int norm_p, float* d_out,
                               void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        Model& m = *as_model(model);
        if (rows && (!d_row_ptr || (nnz && (!d_col_idx || !d_count)))) fail("xrl_queries_tfidf_device: null device pointer");
        use_device(m.device);
        auto q = std::make_unique<Queries>();
        if (!d_out) q->own.val.reserve(nnz * 4);         // the handle owns the weighted values unless the caller supplies the buffer; row pointers and column ids stay the caller's
        float* dst = d_out ? d_out : q->own.val.as<float>();
        hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : m.stream;
        DevBuf d_err; d_err.reserve(4);
        XRL_HIP(hipMemsetAsync(d_err.p, 0, 4, s));
        launch_tfidf_weight(d_row_ptr, d_col_idx, d_count, d_idf, rows, cols, binary, sublinear_tf, norm_p, dst, s, 1, 0, d_err.as<uint32_t>());
        uint32_t err = 0;
        XRL_HIP(hipMemcpyAsync(&err, d_err.p, 4, hipMemcpyDeviceToHost, s));
        XRL_HIP(hipStreamSynchronize(s));
        if (err) fail("xrl_queries_tfidf_device: a column id outside [0, cols) (the reference's idx_idf.at() throws)");
        set_view(*q, m.device, csr_view(rows, cols, d_row_ptr, d_col_idx, dst, nnz));
        return q.release();
    });
}

void* xrl_queries_from_device_drm(void* model, uint32_t rows, uint32_t cols, const float* d_val) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        Model& m = *as_model(model);
        if (rows && cols && !d_val) fail("xrl_queries_from_device_drm: null device pointer");
        auto q = std::make_unique<Queries>();
        set_view(*q, m.device, dense_view(rows, cols, d_val));
        return q.release();
    });
}

// [X_feat | X_emb] as one CSR the handle owns (the body of the two concat makers; runs inside their exception barrier)
static void* concat_csr(void* model, uint32_t rows, uint32_t sparse_cols, const uint64_t* d_row_ptr, const uint32_t* d_col_idx, const float* d_val,
                        uint64_t nnz, uint32_t dense_cols, const float* d_emb, int normalize_emb, void* hip_stream) {
    Model& m = *as_model(model);
    if (rows && (!d_row_ptr || (nnz && (!d_col_idx || !d_val)) || (dense_cols && !d_emb))) fail("xrl_queries_concat_device: null device pointer");
    use_device(m.device);
    auto q = std::make_unique<Queries>();
    DevCsr& o = q->own;
    o.nnz = nnz + (uint64_t)rows * dense_cols;
    o.ptr.reserve(((size_t)rows + 1) * 8); o.idx.reserve(o.nnz * 4); o.val.reserve(o.nnz * 4);
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : m.stream;
    launch_concat_csr(d_row_ptr, d_col_idx, d_val, d_emb, rows, sparse_cols, dense_cols, normalize_emb, o.ptr.as<uint64_t>(), o.idx.as<uint32_t>(), o.val.as<float>(), s);
    XRL_HIP(hipStreamSynchronize(s));
    set_own_csr(*q, m.device, rows, sparse_cols + dense_cols);
    return q.release();
}

void* xrl_queries_concat_device(void* model, uint32_t rows, uint32_t sparse_cols, const uint64_t* d_row_ptr, const uint32_t* d_col_idx,
                                const float* d_val, uint64_t nnz, uint32_t dense_cols, const float* d_emb, void* hip_stream) {
    return xrl_queries_concat_device_ex(model, rows, sparse_cols, d_row_ptr, d_col_idx, d_val, nnz, dense_cols, d_emb, 0, hip_stream);
}

void* xrl_queries_concat_device_ex(void* model, uint32_t rows, uint32_t sparse_cols, const uint64_t* d_row_ptr, const uint32_t* d_col_idx,
                                   const float* d_val, uint64_t nnz, uint32_t dense_cols, const float* d_emb, int normalize_emb, void* hip_stream) {
    return guarded_value((void*)nullptr, [&] {
        return concat_csr(model, rows, sparse_cols, d_row_ptr, d_col_idx, d_val, nnz, dense_cols, d_emb, normalize_emb, hip_stream);
    });
}

void* xrl_queries_concat_handle(void* model, void* queries, uint32_t dense_cols, const float* d_emb, int normalize_emb, void* hip_stream) {
    return guarded_value((void*)nullptr, [&] {
        if (!queries) fail("xrl_queries_concat_handle: null query handle");
        const QueriesDev& X = static_cast<Queries*>(queries)->dev;
        if (X.dense) fail("xrl_queries_concat_handle: the query handle must hold a CSR");
        return concat_csr(model, X.rows, X.cols, X.row_ptr, X.col_idx, X.val, X.nnz, dense_cols, d_emb, normalize_emb, hip_stream);
    });
}

int xrl_queries_info(void* queries, uint64_t* out4) {
    return guarded_value(-1, [&] {
        if (!queries || !out4) fail("null argument");
        const Queries* q = static_cast<const Queries*>(queries);
        out4[0] = q->dev.rows; out4[1] = q->dev.cols; out4[2] = q->dev.dense ? (uint64_t)q->dev.rows * q->dev.cols : q->dev.nnz; out4[3] = q->dev.dense ? 1 : 0;
        return 0;
    });
}

int xrl_queries_download(void* queries, uint64_t* row_ptr, uint32_t* col_idx, float* val) {
    return guarded_value(-1, [&] {
        if (!queries || !val) fail("null argument");
        const Queries* q = static_cast<const Queries*>(queries);
        XRL_HIP(hipSetDevice(q->device));
        XRL_HIP(hipDeviceSynchronize());
        if (q->dev.dense) {
            XRL_HIP(hipMemcpy(val, q->dev.val, (size_t)q->dev.rows * q->dev.cols * 4, hipMemcpyDeviceToHost));
        } else {
            if (!row_ptr || (q->dev.nnz && !col_idx)) fail("null argument");
            download_csr(q->dev, row_ptr, col_idx, val);
        }
        return 0;
    });
}

void xrl_queries_free(void* queries) { guarded([&] { free_handle(queries); }); }

// xrl_predict_device and xrl_predict_device_rows (`ranged`: the scratch is sized for any row range of these queries)
static int predict_device_entry(const char* what, bool ranged, void* model, void* queries, uint32_t beam_size, const char* post_processor,
                                uint32_t only_topk, uint32_t* d_out_idx, float* d_out_val, uint32_t* d_out_cnt, uint32_t out_stride,
                                void* hip_stream, int sync, uint32_t row_begin = 0, uint32_t row_count = 0xFFFFFFFFu) {
    return guarded_value(-1, [&] {
        Model& m = *as_model(model);
        if (!queries || !d_out_idx || !d_out_val || !d_out_cnt) fail(std::string(what) + ": null argument");
        std::lock_guard<std::mutex> g(m.mu);
        use_device(m.device);
        const QueriesDev& X = static_cast<Queries*>(queries)->dev;
        PredictOpts o; o.beam_size = beam_size; o.only_topk = only_topk; o.post_processor = post_processor;
        if (ranged) o.reserve_rows = X.rows;
        predict_device(m, X, o, d_out_idx, d_out_val, d_out_cnt, out_stride, static_cast<hipStream_t>(hip_stream), sync != 0, row_begin, row_count);
        return 0;
    });
}

int xrl_predict_device(void* model, void* queries, uint32_t beam_size, const char* post_processor, uint32_t only_topk,
                       uint32_t* d_out_idx, float* d_out_val, uint32_t* d_out_cnt, uint32_t out_stride,
                       void* hip_stream, int sync) {
    return predict_device_entry("xrl_predict_device", false, model, queries, beam_size, post_processor, only_topk, d_out_idx, d_out_val, d_out_cnt, out_stride, hip_stream, sync);
}

int xrl_predict_device_rows(void* model, void* queries, uint32_t beam_size, const char* post_processor, uint32_t only_topk,
                            uint32_t* d_out_idx, float* d_out_val, uint32_t* d_out_cnt, uint32_t out_stride,
                            void* hip_stream, int sync, uint32_t row_begin, uint32_t row_count) {
    return predict_device_entry("xrl_predict_device_rows", true, model, queries, beam_size, post_processor, only_topk, d_out_idx, d_out_val, d_out_cnt, out_stride, hip_stream, sync, row_begin, row_count);
}

// xrl_ensemble_device and xrl_ensemble_methods_device (`methods`: no finish, no threshold, only_topk cuts every method)
static int ensemble_entry(const char* name, bool methods, int device, uint32_t n_models, uint32_t rows, const uint32_t* const* d_idx,
                          const float* const* d_val, const uint32_t* const* d_cnt, const uint32_t* in_stride, int mode, const float* threshold,
                          uint32_t only_topk, uint32_t* d_out_idx, float* d_out_val, uint32_t* d_out_cnt, uint32_t out_stride, void* hip_stream, int sync) {
    return guarded_value(-1, [&] {
        // every argument is checked before the GPU is required
        const std::string what = std::string(name) + ": ";
        if (!d_idx || !d_val || !d_cnt || !in_stride || !d_out_idx || !d_out_val || !d_out_cnt) fail(what + "null argument");
        if (n_models == 0 || n_models > (uint32_t)kEnsembleMaxModels) fail(what + "n_models must be 1.." + std::to_string(kEnsembleMaxModels) + ", got " + std::to_string(n_models));
        EnsembleArgs A{};
        uint64_t total = 0;
        for (uint32_t m = 0; m < n_models; ++m) {
            if (!d_idx[m] || !d_val[m] || !d_cnt[m]) fail(what + "null device pointer for model " + std::to_string(m));
            A.idx[m] = d_idx[m]; A.val[m] = d_val[m]; A.cnt[m] = d_cnt[m]; A.stride[m] = in_stride[m];
            total += in_stride[m];
        }
        if (total > kEnsembleMaxTotal) fail(what + "the input strides sum to " + std::to_string(total) + ", more than " + std::to_string(kEnsembleMaxTotal));
        if (methods) {
            if (mode == kEnsembleFinish) fail(what + "method 1 (finish) is served by xrl_ensemble_device");
            if (mode < kEnsembleAverage || mode > kEnsembleRoundRobin) fail(what + "unknown method " + std::to_string(mode));
        } else {
            if (mode != kEnsembleAverage && mode != kEnsembleFinish && mode != kEnsembleRankAverage) fail(what + "unknown mode " + std::to_string(mode));
            if (mode != kEnsembleFinish && (threshold || only_topk)) fail(what + "threshold and only_topk belong to mode finish");
        }
        const uint64_t longest = only_topk ? std::min<uint64_t>(total, only_topk) : total;
        if (out_stride < longest) fail(what + "out_stride " + std::to_string(out_stride) + " smaller than the longest possible row, " + std::to_string(longest));
        if (rows == 0) return 0;
        require_gpu();
        use_device(device);
        A.n_models = n_models; A.rows = rows; A.mode = mode;
        A.has_threshold = threshold ? 1 : 0; A.threshold = threshold ? *threshold : 0.0f; A.only_topk = only_topk;
        A.out_idx = d_out_idx; A.out_val = d_out_val; A.out_cnt = d_out_cnt; A.out_stride = out_stride;
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        // the device scalar of rank_average and round_robin lives and dies in stream order: no synchronisation, and concurrent calls do not share it
        void* mm = nullptr;
        if (mode == kEnsembleRankAverage || mode == kEnsembleRoundRobin) XRL_HIP(hipMallocAsync(&mm, sizeof(uint32_t), s));
        try { launch_ensemble(A, static_cast<uint32_t*>(mm), s); }
        catch (...) { if (mm) (void)hipFreeAsync(mm, s); throw; }
        if (mm) XRL_HIP(hipFreeAsync(mm, s));
        if (sync) XRL_HIP(hipStreamSynchronize(s));
        return 0;
    });
}

int xrl_ensemble_device(int device, uint32_t n_models, uint32_t rows, const uint32_t* const* d_idx, const float* const* d_val,
                        const uint32_t* const* d_cnt, const uint32_t* in_stride, int mode, const float* threshold, uint32_t only_topk,
                        uint32_t* d_out_idx, float* d_out_val, uint32_t* d_out_cnt, uint32_t out_stride, void* hip_stream, int sync) {
    return ensemble_entry("xrl_ensemble_device", false, device, n_models, rows, d_idx, d_val, d_cnt, in_stride, mode, threshold, only_topk, d_out_idx, d_out_val, d_out_cnt, out_stride, hip_stream, sync);
}

int xrl_ensemble_methods_device(int device, uint32_t n_models, uint32_t rows, const uint32_t* const* d_idx, const float* const* d_val,
                                const uint32_t* const* d_cnt, const uint32_t* in_stride, int method, uint32_t only_topk,
                                uint32_t* d_out_idx, float* d_out_val, uint32_t* d_out_cnt, uint32_t out_stride, void* hip_stream, int sync) {
    return ensemble_entry("xrl_ensemble_methods_device", true, device, n_models, rows, d_idx, d_val, d_cnt, in_stride, method, nullptr, only_topk, d_out_idx, d_out_val, d_out_cnt, out_stride, hip_stream, sync);
}

int xrl_metrics_device(int device, uint32_t rows, const uint32_t* d_idx, const float* d_val, const uint32_t* d_cnt, uint32_t stride,
                       const uint64_t* d_true_ptr, const uint32_t* d_true_idx, uint32_t topk, uint64_t* d_matched, double* d_recall_sum,
                       void* hip_stream, int sync) {
    return guarded_value(-1, [&] {
        // every argument is checked before a GPU is required
        const std::string what = "xrl_metrics_device: ";
        if (!d_idx || !d_val || !d_cnt || !d_true_ptr || !d_true_idx || !d_matched || !d_recall_sum) fail(what + "null argument");
        if (stride == 0 || stride > kMetricsMax) fail(what + "stride must be 1.." + std::to_string(kMetricsMax) + ", got " + std::to_string(stride));
        if (topk == 0 || topk > kMetricsMax) fail(what + "topk must be 1.." + std::to_string(kMetricsMax) + ", got " + std::to_string(topk));
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        if (rows == 0) {                                                // no rows: the sums are zero (without a GPU there is nothing to fill)
            int n = 0;
            if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return 0;
            use_device(device);
            XRL_HIP(hipMemsetAsync(d_matched, 0, (size_t)topk * sizeof(uint64_t), s));
            XRL_HIP(hipMemsetAsync(d_recall_sum, 0, (size_t)topk * sizeof(double), s));
            if (sync) XRL_HIP(hipStreamSynchronize(s));
            return 0;
        }
        require_gpu();
        use_device(device);
        MetricsArgs A{};
        A.idx = d_idx; A.val = d_val; A.cnt = d_cnt; A.stride = stride; A.rows = rows; A.topk = topk;
        A.true_ptr = d_true_ptr; A.true_idx = d_true_idx; A.matched = d_matched; A.recall_sum = d_recall_sum;
        // the partial sums live and die in stream order: no synchronisation, and concurrent calls do not share them
        void* scratch = nullptr;
        XRL_HIP(hipMallocAsync(&scratch, metrics_scratch_bytes(rows, topk), s));
        try { launch_metrics(A, scratch, s); }
        catch (...) { (void)hipFreeAsync(scratch, s); throw; }
        XRL_HIP(hipFreeAsync(scratch, s));
        if (sync) XRL_HIP(hipStreamSynchronize(s));
        return 0;
    });
}

int xrl_predict_selected_device(void* model, void* queries, const char* post_processor, const uint32_t* d_sel_idx, const uint32_t* d_sel_cnt,
                                uint32_t sel_stride, uint32_t* d_out_idx, float* d_out_val, uint32_t* d_out_cnt, uint32_t out_stride,
                                uint32_t* d_status, void* hip_stream, int sync) {
    return guarded_value(-1, [&] {
        // every argument is checked before the GPU is touched
        const std::string what = "xrl_predict_selected_device: ";
        if (!model || !queries || !d_sel_idx || !d_out_idx || !d_out_val || !d_out_cnt) fail(what + "null argument");
        Model& m = *as_model(model);
        const Queries& q = *static_cast<Queries*>(queries);
        if (sel_stride == 0 || sel_stride > kSelectMaxStride) fail(what + "sel_stride must be 1.." + std::to_string(kSelectMaxStride) + ", got " + std::to_string(sel_stride) + " (the host entry point serves longer rows)");
        if (out_stride < sel_stride) fail(what + "out_stride " + std::to_string(out_stride) + " smaller than sel_stride " + std::to_string(sel_stride));
        if (q.device != m.device) fail(what + "the queries live on device " + std::to_string(q.device) + ", the model on device " + std::to_string(m.device));
        std::lock_guard<std::mutex> g(m.mu);
        try { check_selected_inputs(m, q.dev); }
        catch (const Error& e) { fail(what + e.what()); }
        if (q.dev.rows == 0) return 0;
        use_device(m.device);
        predict_selected_device(m, q.dev, post_processor, d_sel_idx, d_sel_cnt, sel_stride, d_out_idx, d_out_val, d_out_cnt, out_stride, d_status,
                                static_cast<hipStream_t>(hip_stream), sync != 0);
        return 0;
    });
}

int xrl_predict_stats(void* model, void* queries, uint32_t beam_size, const char* post_processor, uint32_t only_topk,
                      double* stats_out, uint32_t stats_cap) {
    return guarded_value(-1, [&] {
        Model& m = *as_model(model);
        if (!queries || !stats_out) fail("xrl_predict_stats: null argument");
        if (stats_cap < kStatsPerLayer * m.layers.size()) fail("xrl_predict_stats: stats_out too small (need 8*depth doubles)");
        std::lock_guard<std::mutex> g(m.mu);
        if (m.constrained) fail("xrl_predict_stats: not available while an output constraint is set (the constrained route runs none of the counted kernels)");
        use_device(m.device);
        if (!m.ws) m.ws = std::make_unique<Workspace>();
        const QueriesDev& X = static_cast<Queries*>(queries)->dev;
        const uint32_t k = effective_topk(m, only_topk);
        Workspace& ws = *m.ws;
        ws.out_idx.reserve((size_t)X.rows * k * 4); ws.out_val.reserve((size_t)X.rows * k * 4); ws.out_cnt.reserve((size_t)X.rows * 4);
        PredictOpts o; o.beam_size = beam_size; o.only_topk = only_topk; o.post_processor = post_processor; o.stats_out = stats_out;
        const bool was = m.profiling; m.profiling = false;
        predict_device(m, X, o, ws.out_idx.as<uint32_t>(), ws.out_val.as<float>(), ws.out_cnt.as<uint32_t>(), k, m.stream, true);
        m.profiling = was;
        return 0;
    });
}

// xrl_set_output_constraint and xrl_set_output_constraint_device
static int set_constraint_entry(const char* what, void* model, const uint32_t* labels, uint64_t n, bool on_device, void* hip_stream) {
    return guarded_value(-1, [&] {
        Model& m = *as_model(model);
        std::lock_guard<std::mutex> g(m.mu);
        use_device(m.device);
        set_output_constraint(m, labels, n, on_device, static_cast<hipStream_t>(hip_stream), what);
        return 0;
    });
}

int xrl_set_output_constraint(void* model, const uint32_t* labels, uint64_t n) {
    return set_constraint_entry("xrl_set_output_constraint", model, labels, n, false, nullptr);
}

int xrl_set_output_constraint_device(void* model, const uint32_t* d_labels, uint64_t n, void* hip_stream) {
    return set_constraint_entry("xrl_set_output_constraint_device", model, d_labels, n, true, hip_stream);
}

int xrl_clear_output_constraint(void* model) {
    return guarded_value(-1, [&] {
        Model& m = *as_model(model);
        std::lock_guard<std::mutex> g(m.mu);
        use_device(m.device);
        clear_output_constraint(m);
        return 0;
    });
}

int xrl_output_constraint_info(void* model, uint64_t* out, uint32_t cap) {
    return guarded_value(-1, [&] {
        Model& m = *as_model(model);
        std::lock_guard<std::mutex> g(m.mu);
        const uint32_t n = 1u + (uint32_t)m.layers.size();
        for (uint32_t i = 0; i < n && i < cap && out; ++i) {
            if (i == 0) { out[0] = m.constrained ? 1 : 0; continue; }
            const Layer& L = *m.layers[i - 1];
            out[i] = L.view.active ? L.view.kept : L.n_children;
        }
        return (int)n;
    });
}

int xrl_debug_output_constraint_view(void* model, uint32_t layer, uint32_t* chunk_col_out, uint64_t chunk_col_cap, uint32_t* perm_inv_out, uint64_t perm_inv_cap) {
    return guarded_value(-1, [&] {
        Model& m = *as_model(model);
        if (layer >= m.layers.size()) fail("xrl_debug_output_constraint_view: layer out of range");
        std::lock_guard<std::mutex> g(m.mu);
        const Layer& L = *m.layers[layer];
        if (!L.view.active) return 0;
        use_device(m.device);
        XRL_HIP(hipDeviceSynchronize());
        const uint64_t n_cc = std::min<uint64_t>(chunk_col_cap, (uint64_t)L.dev.n_parents + 1), n_pi = std::min<uint64_t>(perm_inv_cap, L.view.kept);
        if (chunk_col_out && n_cc) XRL_HIP(hipMemcpy(chunk_col_out, L.view.d_chunk_col.p, n_cc * 4, hipMemcpyDeviceToHost));
        if (perm_inv_out && n_pi) XRL_HIP(hipMemcpy(perm_inv_out, L.view.d_perm_inv.p, n_pi * 4, hipMemcpyDeviceToHost));
        return 1;
    });
}

uint32_t xrl_effective_topk(void* model, uint32_t only_topk) {
    return guarded_value(0u, [&] { return effective_topk(*as_model(model), only_topk); });
}

void xrl_profile_enable(void* model, int enable) { guarded([&] { as_model(model)->profiling = enable != 0; }); }
void xrl_profile_reset(void* model) { guarded([&] { Model& m = *as_model(model); resolve_profile(m); m.profile.clear(); }); }
uint32_t xrl_profile_get(void* model, xrl_profile_rec_t* out, uint32_t cap) {
    uint32_t n = 0;
    guarded([&] {
        Model& m = *as_model(model);
        resolve_profile(m);
        n = (uint32_t)m.profile.size();
        for (uint32_t i = 0; i < n && i < cap && out; ++i) {
            std::memset(&out[i], 0, sizeof(out[i]));
            std::strncpy(out[i].name, m.profile[i].name.c_str(), sizeof(out[i].name) - 1);
            out[i].layer = m.profile[i].layer; out[i].launches = m.profile[i].launches;
            out[i].ms = m.profile[i].ms;
        }
    });
    return n;
}

uint32_t xrl_debug_split_chunk(const uint64_t* cum, uint32_t n, uint64_t limit) {
    return guarded_value(0u, [&] { if (!cum) fail("null cum"); return split_chunk(cum, n, limit); });
}

uint64_t xrl_debug_layout_rows(const uint32_t* rptr, uint32_t nrows, int align, uint32_t* ext_out) {
    return guarded_value((uint64_t)0, [&] { if (!rptr) fail("null rptr"); return layout_tile_rows(rptr, nrows, align != 0, ext_out); });
}

uint32_t xrl_debug_host_batches(const uint64_t* row_ptr, uint32_t rows, uint32_t cols, int host_batch_mb, uint32_t* rb_out, uint32_t cap) {
    return guarded_value(0u, [&] {
        HostX x; x.given = true; x.csr = row_ptr != nullptr; x.rows = rows; x.cols = cols; x.row_ptr = row_ptr;
        const std::vector<uint32_t> rb = plan_row_batches(x, host_batch_mb, staged_upload(x, 1));
        for (size_t i = 0; i < rb.size() && i < cap && rb_out; ++i) rb_out[i] = rb[i];
        return (uint32_t)rb.size();
    });
}

int xrl_debug_k2_form(uint32_t k, uint32_t cand_stride, int64_t k2_big_min_k, int stage, uint32_t limited_cands, uint32_t* ns_out) {
    return guarded_value(-1, [&] {
        const K2Choice c = k2_form(k, cand_stride, k2_big_min_k, stage, limited_cands);
        if (ns_out) *ns_out = c.ns;
        return (int)c.form;
    });
}

// every integer option that is a plain store into Model::Options, under the member's own name (include/xrl_abi.h documents the keys)
#define XRL_OPT(name) {#name, &Model::Options::name}
static const struct { const char* name; int Model::Options::*field; } kIntOptions[] = {
    XRL_OPT(k1_group), XRL_OPT(sort_min_tiles), XRL_OPT(sort_rest), XRL_OPT(sort_rest_min), XRL_OPT(prune_mid), XRL_OPT(leaf_fuse), XRL_OPT(leaf_tail), XRL_OPT(tile_rows),
    XRL_OPT(k2_big_min_k), XRL_OPT(qsort), XRL_OPT(qsort_min_parents), XRL_OPT(qsort_min_rows), XRL_OPT(presence), XRL_OPT(adaptive), XRL_OPT(prune),
    XRL_OPT(host_pipeline), XRL_OPT(host_batch_mb), XRL_OPT(host_register), XRL_OPT(overlap_min_rows),
    XRL_OPT(dense_layers), XRL_OPT(k1q_fuse), XRL_OPT(k1g_first), XRL_OPT(k1g_min_items), XRL_OPT(k1g_variant),
    XRL_OPT(k1_wpb), XRL_OPT(k1_lds_pad), XRL_OPT(k1_ablate),   // debug: wavefronts per K1 workgroup, occupancy experiments, timing ablations only
};
#undef XRL_OPT

static void set_option_one(Model& m, const char* key, int64_t value) {
    if (!std::strcmp(key, "max_batch_rows")) { m.opt.max_batch_rows = value; return; }
    if (!std::strcmp(key, "reserve_rows")) {
        // a serving process that knows its largest batch sizes the result buffers of the host ABI once, at start-up (pinned host memory: rows x
        // the model's default top-k x 8 bytes, + the device side), instead of inside its first large call
        if (value < 0 || value > 0x7FFFFFFF) fail("reserve_rows: expected 0 .. 2^31-1");
        std::lock_guard<std::mutex> g(m.mu);
        use_device(m.device);
        if (!m.ws) m.ws = std::make_unique<Workspace>();
        reserve_outputs(m, (uint32_t)value, effective_topk(m, 0));
        return;
    }
    for (const auto& o : kIntOptions)
        if (!std::strcmp(key, o.name)) { m.opt.*o.field = (int)value; if (o.field == &Model::Options::adaptive) m.fb.restage(); return; }
    fail(std::string("unknown option ") + key);
}

int xrl_set_option(void* model, const char* key, int64_t value) {
    return guarded_value(-1, [&] {
        Model& m = *as_model(model);
        if (!key) fail("null key");
        if (!std::strcmp(key, "devices")) {
            // the handle serves c_xlinear_predict_* from `value` devices: this one plus value-1 replicas of the compiled model,
            // placed on the following physical devices (wrapping around: with fewer GPUs than requested several replicas share one,
            // which is how a one-GPU box tests the sharded path)
            if (value < 1 || value > 64) fail("devices: expected 1..64");
            if (m.src_kind < 0 && value > 1) fail("devices: only models loaded from a folder can be replicated");
            std::lock_guard<std::mutex> g(m.mu);
            if (m.constrained && value > 1) fail("devices: the handle carries an output constraint, which replicas do not share (xrl_clear_output_constraint first)");
            int ndev = 0;
            XRL_HIP(hipGetDeviceCount(&ndev));
            m.replicas.clear();
            for (int64_t i = 1; i < value; ++i) {
                const int dev = (m.device + (int)i) % std::max(1, ndev);
                use_device(dev);
                std::unique_ptr<Model> r = m.src_kind == 0 ? load_model_from_disk(m.src_path, m.weight_matrix_type) : load_mmap_model_from_disk(m.src_path);
                r->device = dev;
                r->opt = m.opt;
                m.replicas.push_back(std::move(r));
            }
            use_device(m.device);
        } else {
            set_option_one(m, key, value);
            for (auto& r : m.replicas) set_option_one(*r, key, value);
        }
        return 0;
    });
}

void xrl_debug_k1_phases(unsigned long long* out8, int reset) { guarded([&] { k1_phase_read(out8, reset != 0); }); }

uint32_t xrl_layer_info(void* model, uint32_t layer, uint64_t* out, uint32_t cap) {
    uint32_t n = 0;
    guarded([&] {
        Model& m = *as_model(model);
        if (layer >= m.layers.size()) fail("xrl_layer_info: layer out of range");
        const Layer& L = *m.layers[layer];
        const uint64_t rec[12] = {
            (uint64_t)(L.dev.bucket ? 1 : (L.dev.bitmap64 ? 2 : 0)), L.bk_levels, (uint64_t)(L.dev.wd ? 1 : 0), 1ull << L.dev.d_gp_log2,
            L.dev.d_ld, L.n_tiles, L.nnz, L.dense_bytes, L.w_rows, L.n_children, L.max_tile_cols, L.device_bytes};
        n = 12;
        for (uint32_t i = 0; i < n && i < cap && out; ++i) out[i] = rec[i];
    });
    return n;
}

uint64_t xrl_model_device_bytes(void* model) {
    return guarded_value((uint64_t)0, [&] { return as_model(model)->device_bytes(); });
}

}  // extern "C"
