// TF-IDF query producer (libpecos.cpp:398-445): c_tfidf_load / c_tfidf_destruct / c_tfidf_predict with the
// reference's signatures, and xrl_tfidf_predict_device, which leaves X in HBM for xrl_predict_device.
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include "xrl_abi_common.h"
#include "xrl_tfidf.h"
#include "xrl_tfidf_train.h"
#include "xrl_tokenize.h"

#include <sys/stat.h>
#include <cerrno>

using namespace xrl;

namespace {
// pinned staging for the H2D copy of the term counts: the worker threads of the host half write straight into it (no intermediate, no page
// faults -- pinned memory is resident), and the copy runs at link speed instead of through the runtime's pageable path.  Grows, never shrinks;
// one producer call per handle at a time uses it.
struct PinnedStage {
    void* p = nullptr; size_t cap = 0; std::mutex mu;
    ~PinnedStage() { if (p) (void)hipHostFree(p); }
    void* need(size_t bytes) {
        if (bytes > cap) {
            if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
            const size_t want = bytes + bytes / 4 + (1u << 20);
            XRL_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
            cap = want;
        }
        return p;
    }
};

// dst <- src on host threads, 1 MiB pieces
void parallel_copy(void* dst, const void* src, size_t bytes, int threads) {
    const size_t piece = (size_t)1 << 20, n = (bytes + piece - 1) / piece;
    unsigned nt = threads > 0 ? (unsigned)threads : std::min(32u, std::max(1u, std::thread::hardware_concurrency()));
    nt = (unsigned)std::max<size_t>(1, std::min<size_t>(nt, n));
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t i = next.fetch_add(1, std::memory_order_relaxed);
            if (i >= n) break;
            std::memcpy(static_cast<char*>(dst) + i * piece, static_cast<const char*>(src) + i * piece, std::min(piece, bytes - i * piece));
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
}

struct TfidfHandle {
    TfidfVectorizer v;
    std::vector<float> idf_all;                  // the base vectorizers' idf side by side (hstack column order)
    mutable PinnedStage stage;
    // c_tfidf_predict's stream, created once per (handle, device) instead of per call
    mutable std::mutex stream_mu;
    mutable hipStream_t stream = nullptr;
    mutable int stream_device = -1;
    // call with the staging lock (stage.mu) HELD and keep it until the stream has been synchronised: a caller that switched devices
    // replaces the stream, which must not happen under another thread's transfer
    hipStream_t stream_on(int device) const {
        std::lock_guard<std::mutex> g(stream_mu);
        if (stream && stream_device != device) { (void)hipSetDevice(stream_device); (void)hipStreamDestroy(stream); stream = nullptr; (void)hipSetDevice(device); }
        if (!stream) { XRL_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)); stream_device = device; }
        return stream;
    }
    // The device tokenizer's tables (K9): a copy of every base vectorizer's s, l, token arena, uni, packed, gen and n-gram arena in HBM with
    // their views, built under dev_mu by the first device-tokenizer call on a device and kept until the handle goes.
    struct DeviceTables { std::vector<DevBuf> bufs; std::vector<TokBase> bases; uint64_t bytes = 0; };
    mutable std::mutex dev_mu;
    mutable std::map<int, std::unique_ptr<DeviceTables>> dev_tables;
    mutable std::atomic<uint64_t> forms[4] = {};    // segments served by the LDS form, by the global form; batches; calls (xrl_debug_tfidf_device_forms)
    TrainForms train_forms;                         // what training did (xrl_debug_tfidf_train_forms); zeros for a loaded handle
    const DeviceTables& tables_on(int device) const {
        std::lock_guard<std::mutex> g(dev_mu);
        auto it = dev_tables.find(device);
        if (it != dev_tables.end()) return *it->second;
        auto T = std::make_unique<DeviceTables>();
        auto put = [&](const void* src, size_t bytes) -> const void* {
            if (!bytes) return nullptr;
            T->bufs.emplace_back();
            T->bufs.back().upload_raw(src, bytes);
            T->bytes += bytes;
            return T->bufs.back().p;
        };
        uint32_t col_off = 0;
        for (const TfidfBase& B : v.base) {
            TokBase D;
            D.tv = B.vocab.view(); D.gv = B.features.view();
            D.tv.s = static_cast<const tft::ShortEntry*>(put(B.vocab.s.data(), B.vocab.s.size() * sizeof(tft::ShortEntry)));
            D.tv.l = static_cast<const tft::LongEntry*>(put(B.vocab.l.data(), B.vocab.l.size() * sizeof(tft::LongEntry)));
            D.tv.arena = static_cast<const char*>(put(B.vocab.arena.data(), B.vocab.arena.size()));
            D.gv.uni = static_cast<const uint32_t*>(put(B.features.uni.data(), B.features.uni.size() * 4));
            D.gv.packed = static_cast<const tft::PackedEntry*>(put(B.features.packed.data(), B.features.packed.size() * sizeof(tft::PackedEntry)));
            D.gv.gen = static_cast<const tft::GenEntry*>(put(B.features.gen.data(), B.features.gen.size() * sizeof(tft::GenEntry)));
            D.gv.arena = static_cast<const int32_t*>(put(B.features.arena.data(), B.features.arena.size() * 4));
            D.tok_type = B.tok_type; D.min_ngram = B.min_ngram; D.max_ngram = B.max_ngram; D.max_length = B.max_length;
            D.col_off = col_off; col_off += B.nr_features;
            T->bases.push_back(D);
        }
        return *(dev_tables[device] = std::move(T));
    }
    ~TfidfHandle() {
        if (stream) { (void)hipSetDevice(stream_device); (void)hipStreamDestroy(stream); }
        for (auto& kv : dev_tables) { (void)hipSetDevice(kv.first); kv.second.reset(); }   // (freed with their device set)
    }
};

// c.ptr holds the SEGMENT pointer of nb base vectorizers side by side -> the hstacked CSR's row pointer (every nb-th entry; h_seg: the
// segment pointer on the host when the host counted, nullptr: gathered by a kernel on s).  Returns the segment pointer, which the work
// enqueued on s may still read: the caller keeps it until s is synchronised.
DevBuf seg_to_row_ptr(DevCsr& c, const std::vector<uint64_t>* h_seg, uint32_t nb, uint32_t rows, hipStream_t s) {
    if (nb == 1) return {};
    DevBuf seg = std::move(c.ptr);
    if (h_seg) {
        std::vector<uint64_t> row_ptr((size_t)rows + 1);
        for (size_t r = 0; r <= rows; ++r) row_ptr[r] = (*h_seg)[r * nb];
        c.ptr.upload(row_ptr);
    } else {
        c.ptr.reserve(((size_t)rows + 1) * 8);
        launch_seg_to_row_ptr(seg.as<uint64_t>(), nb, rows, c.ptr.as<uint64_t>(), s);
    }
    return seg;
}

// The weighting tail both count forms share: q->own holds the term counts (idx, val, nnz) and, as ptr, their segment pointer (h_seg: as in
// seg_to_row_ptr) -> per-base K5, the ensemble's norm, one synchronise.
void tfidf_weight_counts(const TfidfHandle& H, Queries* q, const std::vector<uint64_t>* h_seg, uint32_t rows, int device, hipStream_t s) {
    const TfidfVectorizer& V = H.v;
    const uint32_t nb = (uint32_t)V.base.size();
    DevCsr& c = q->own;
    DevBuf d_idf, d_err;
    d_idf.upload(H.idf_all);
    d_err.reserve(4); XRL_HIP(hipMemsetAsync(d_err.p, 0, 4, s));
    for (uint32_t b = 0; b < nb; ++b) {
        const TfidfBase& B = V.base[b];
        launch_tfidf_weight(c.ptr.as<uint64_t>(), c.idx.as<uint32_t>(), c.val.as<float>(), B.use_idf ? d_idf.as<float>() : nullptr, rows, V.nr_features,
                            B.binary ? 1 : 0, B.sublinear_tf ? 1 : 0, B.norm_p, c.val.as<float>(), s, nb, b, d_err.as<uint32_t>());
    }
    // whole rows: the hstacked CSR's row pointer; the ensemble's normalisation (Vectorizer::predict, tfidf.hpp:1405-1430)
    const DevBuf seg = seg_to_row_ptr(c, h_seg, nb, rows, s);
    if (nb > 1 || V.norm_p != V.base[0].norm_p)
        launch_tfidf_weight(c.ptr.as<uint64_t>(), c.idx.as<uint32_t>(), c.val.as<float>(), nullptr, rows, V.nr_features, 0, 0, V.norm_p, c.val.as<float>(), s);
    uint32_t err = 0;
    XRL_HIP(hipMemcpyAsync(&err, d_err.p, 4, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    if (err) fail("tfidf: a feature id outside the model's feature range");
    set_own_csr(*q, device, rows, V.nr_features);
}

// texts -> term counts (host threads, into pinned staging) -> device -> weighting + normalisation (K5): a query handle that owns its three arrays
std::unique_ptr<Queries> tfidf_to_device(const TfidfHandle& H, const char* const* corpus, const size_t* doc_lens, size_t nr_doc, int threads, int device, hipStream_t s) {
    if (nr_doc > 0xFFFFFFFFull) fail("tfidf: too many documents");
    const TfidfVectorizer& V = H.v;
    const uint32_t rows = (uint32_t)nr_doc;
    use_device(device);
    std::lock_guard<std::mutex> stage_lock(H.stage.mu);          // held until the stream has consumed the staging buffer (the synchronize below)
    if (!s) s = H.stream_on(device);                             // the handle's pooled stream, taken under the staging lock
    std::vector<uint64_t> seg_ptr;
    uint32_t* h_col = nullptr; float* h_cnt = nullptr; uint64_t nnz = 0;
    V.count_corpus(corpus, doc_lens, nr_doc, threads, seg_ptr, [&](uint64_t n, uint32_t*& c, float*& v) {
        char* base = static_cast<char*>(H.stage.need((size_t)n * 8 + 16));
        c = h_col = reinterpret_cast<uint32_t*>(base); v = h_cnt = reinterpret_cast<float*>(base + (size_t)n * 4);
        nnz = n;
    });
    auto q = std::make_unique<Queries>();
    DevCsr& c = q->own;
    c.nnz = nnz;
    c.ptr.upload(seg_ptr);
    c.idx.reserve((size_t)nnz * 4); c.val.reserve((size_t)nnz * 4);
    if (nnz) {
        XRL_HIP(hipMemcpyAsync(c.idx.p, h_col, (size_t)nnz * 4, hipMemcpyHostToDevice, s));
        XRL_HIP(hipMemcpyAsync(c.val.p, h_cnt, (size_t)nnz * 4, hipMemcpyHostToDevice, s));
    }
    tfidf_weight_counts(H, q.get(), &seg_ptr, rows, device, s);
    return q;
}

// Texts in HBM -> term counts on the device (K9), synchronised.  A caller's d_status takes every document's status and no status fails
// the call; without one the lowest bad document fails it, in the host tokenizer's words where the host fails too.
void tfidf_count_on_device(const TfidfHandle& H, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len, const uint64_t* h_doc_len,
                           uint64_t nr_doc, uint32_t* d_status, int device, hipStream_t s, TokCounts& C) {
    if (nr_doc > 0xFFFFFFFFull) fail("tfidf: too many documents");
    const TfidfHandle::DeviceTables& T = H.tables_on(device);
    DevBuf own_status;
    const bool report = d_status != nullptr;
    if (!report) { own_status.reserve(nr_doc * 4); d_status = own_status.as<uint32_t>(); }
    tokenize_count_device(T.bases, d_text, d_doc_off, d_doc_len, h_doc_len, nr_doc, d_status, s, C);
    H.forms[0] += C.lds_segments; H.forms[1] += C.global_segments; H.forms[2] += C.batches; H.forms[3] += 1;
    if (report) return;
    if (C.first_bad[0] != ~0ull) fail("the string is not utf-8 encoded! (document " + std::to_string(C.first_bad[0]) + ")");
    if (C.first_bad[1] != ~0ull)
        fail("tfidf (device tokenizer): document " + std::to_string(C.first_bad[1]) + " holds a UTF-8 lead byte followed by too few continuation bytes, "
             "which the host tokenizer decodes along another path: use the host tokenizer for this text");
}

// text -> counts (K9) -> the weighting tail: X ready for xrl_predict_device
std::unique_ptr<Queries> tfidf_device_text_to_x(const TfidfHandle& H, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len,
                                                const uint64_t* h_doc_len, uint64_t nr_doc, int device, hipStream_t s) {
    TokCounts C;
    tfidf_count_on_device(H, d_text, d_doc_off, d_doc_len, h_doc_len, nr_doc, nullptr, device, s, C);
    auto q = std::make_unique<Queries>();
    q->own = std::move(C.csr);
    tfidf_weight_counts(H, q.get(), nullptr, (uint32_t)nr_doc, device, s);
    return q;
}
}  // namespace

extern "C" {

void* c_tfidf_load(const char* model_dir) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        if (!model_dir) fail("null model_dir");
        auto h = std::make_unique<TfidfHandle>();
        h->v.load(model_dir);
        for (const auto& b : h->v.base) h->idf_all.insert(h->idf_all.end(), b.idf.begin(), b.idf.end());
        return h.release();
    });
}

void c_tfidf_destruct(void* ptr) { guarded([&] { delete static_cast<TfidfHandle*>(ptr); }); }

uint32_t xrl_tfidf_nr_features(void* ptr) {
    uint32_t v = 0;
    guarded([&] { if (!ptr) fail("null vectorizer handle"); v = static_cast<TfidfHandle*>(ptr)->v.nr_features; });
    return v;
}

// documents -> weighted CSR on the device -> the caller's arrays through ONE allocator call (shared by c_tfidf_predict and c_tfidf_predict_from_file)
// The weighting half on the HOST, for calls of a handful of documents (the reference serves nr_doc == 1 with a direct host call, libpecos.cpp:437-439:
// microseconds -- a device round trip costs a hundred times that).  tfidf.hpp:798-822 operation by operation in fp32, like the kernel
// (csrc/xrl_features.hip): sequential norm in ascending feature order, separate multiply and add (-ffp-contract=off), the double log of :801 rounded once.
static void tfidf_weight_host(const uint64_t* row_ptr, const uint32_t* col, float* val, const float* idf, uint32_t rows, uint32_t cols, bool binary,
                              bool sublinear, int norm_p, uint32_t seg_stride, uint32_t seg_off) {
    if (norm_p != 1 && norm_p != 2) fail("tfidf: invalid normalize option, norm_p: [ 1| 2]");
    for (uint32_t r = 0; r < rows; ++r) {
        const uint64_t b = row_ptr[(uint64_t)r * seg_stride + seg_off], e = row_ptr[(uint64_t)r * seg_stride + seg_off + 1];
        float denom = 0.0f;
        for (uint64_t t = b; t < e; ++t) {
            float v = binary ? 1.0f : val[t];
            if (sublinear) v = (float)(std::log((double)v) + 1.0);
            if (idf) {
                if (col[t] >= cols) fail("tfidf: a feature id outside the model's feature range");
                v = v * idf[col[t]];
            }
            val[t] = v;
            const float term = norm_p == 1 ? std::fabs(v) : v * v;
            denom = denom + term;
        }
        if (std::fabs(denom) < FLT_EPSILON) denom = 1.0f;
        else if (norm_p == 2) denom = std::sqrt(denom);
        for (uint64_t t = b; t < e; ++t) val[t] = val[t] / denom;
    }
}

constexpr size_t kTfidfHostDocs = 4;   // c_tfidf_predict calls of at most this many documents are weighted on the host

static void tfidf_predict_small_on_host(const TfidfHandle& H, const char* const* corpus, const size_t* doc_lens, size_t nr_doc, py_sparse_allocator_t pred_alloc) {
    const TfidfVectorizer& V = H.v;
    const uint32_t nb = (uint32_t)V.base.size(), rows = (uint32_t)nr_doc;
    std::vector<uint64_t> seg_ptr;
    std::vector<uint32_t> h_col; std::vector<float> h_val;
    V.count_corpus(corpus, doc_lens, nr_doc, 1, seg_ptr, [&](uint64_t n, uint32_t*& c, float*& v) { h_col.resize(n + 1); h_val.resize(n + 1); c = h_col.data(); v = h_val.data(); });
    const uint64_t nnz = seg_ptr.empty() ? 0 : seg_ptr.back();
    for (uint32_t b = 0; b < nb; ++b) {
        const TfidfBase& B = V.base[b];
        tfidf_weight_host(seg_ptr.data(), h_col.data(), h_val.data(), B.use_idf ? H.idf_all.data() : nullptr, rows, V.nr_features, B.binary, B.sublinear_tf, B.norm_p, nb, b);
    }
    std::vector<uint64_t> row_ptr((size_t)rows + 1);
    for (size_t r = 0; r <= rows; ++r) row_ptr[r] = seg_ptr[r * nb];
    if (nb > 1 || V.norm_p != V.base[0].norm_p)
        tfidf_weight_host(row_ptr.data(), h_col.data(), h_val.data(), nullptr, rows, V.nr_features, false, false, V.norm_p, 1, 0);
    uint32_t* indices = nullptr; uint64_t* indptr = nullptr; float* data = nullptr;
    pred_alloc(false, rows, V.nr_features, nnz, &indices, &indptr, &data);
    if (!indptr || (nnz && (!indices || !data))) fail("allocator returned null");
    std::memcpy(indptr, row_ptr.data(), ((size_t)rows + 1) * 8);
    if (nnz) { std::memcpy(indices, h_col.data(), (size_t)nnz * 4); std::memcpy(data, h_val.data(), (size_t)nnz * 4); }
}

static void tfidf_predict_to_host(const TfidfHandle& H, const char* const* corpus, const size_t* doc_lens, size_t nr_doc, int threads, py_sparse_allocator_t pred_alloc) {
    const char* hs = std::getenv("XRL_TFIDF_HOST_DOCS");                     // XRL_TFIDF_HOST_DOCS=0: always the device (tests; read per call)
    if (!(hs && hs[0] == '0') && nr_doc <= kTfidfHostDocs) { tfidf_predict_small_on_host(H, corpus, doc_lens, nr_doc, pred_alloc); return; }
    use_device(g_device);
    // (stream = nullptr: tfidf_to_device takes the handle's pooled stream under its staging lock and holds the lock until it has synchronised)
    std::unique_ptr<Queries> q = tfidf_to_device(H, corpus, doc_lens, nr_doc, threads, g_device, nullptr);
    uint32_t* indices = nullptr; uint64_t* indptr = nullptr; float* data = nullptr;
    const uint64_t nnz = q->dev.nnz;
    pred_alloc(false, q->dev.rows, q->dev.cols, nnz, &indices, &indptr, &data);
    if (!indptr || (nnz && (!indices || !data))) fail("allocator returned null");
    XRL_HIP(hipMemcpy(indptr, q->dev.row_ptr, ((size_t)q->dev.rows + 1) * 8, hipMemcpyDeviceToHost));
    if (nnz) {
        // D2H into the pinned staging buffer (link speed), then host threads spread it over the allocator's fresh arrays: their first touch
        // in parallel, instead of the runtime's single-threaded pageable path
        std::lock_guard<std::mutex> stage_lock(H.stage.mu);
        const size_t nb4 = (size_t)nnz * 4;
        char* st = static_cast<char*>(H.stage.need(2 * nb4));
        XRL_HIP(hipMemcpy(st, q->dev.col_idx, nb4, hipMemcpyDeviceToHost));
        XRL_HIP(hipMemcpy(st + nb4, q->dev.val, nb4, hipMemcpyDeviceToHost));
        parallel_copy(indices, st, nb4, threads);
        parallel_copy(data, st + nb4, nb4, threads);
    }
}

void c_tfidf_predict(void* ptr, void* corpus_ptr, const size_t* doc_lens, size_t nr_doc, int threads, py_sparse_allocator_t pred_alloc) {
    guarded([&] {
        if (!ptr || !pred_alloc) fail("c_tfidf_predict: null argument");
        if (nr_doc == 0) fail("Invalid nr_doc 0");                         // libpecos.cpp:442-444
        if (!corpus_ptr || !doc_lens) fail("c_tfidf_predict: null corpus");
        require_gpu();
        tfidf_predict_to_host(*static_cast<TfidfHandle*>(ptr), static_cast<const char* const*>(corpus_ptr), doc_lens, nr_doc, threads, pred_alloc);
    });
}

// c_tfidf_predict_from_file (libpecos.cpp:413-425 -> Vectorizer::predict_from_file, tfidf.hpp:1041-1120, 1365-1389): one document per LINE of the
// file.  The reference cuts the file into chunks at newlines (file_util.hpp:180-200) and every chunk into lines (append_lines_to_string_view,
// tfidf.hpp:279-294): every '\n' ends a document (empty lines are documents), and a last line WITHOUT a newline is a document too -- with the
// terminating NUL that load_file_block appends counted into its length (tfidf.hpp:290-293 takes `end - start` after the loop has walked over it),
// which is reproduced here.  buffer_size only sizes the reference's read chunks: the file is read whole.
void c_tfidf_predict_from_file(void* ptr, void* corpus_fname_ptr, size_t fname_len, size_t buffer_size, int threads, py_sparse_allocator_t pred_alloc) {
    (void)buffer_size;
    guarded([&] {
        if (!ptr || !pred_alloc || !corpus_fname_ptr) fail("c_tfidf_predict_from_file: null argument");
        require_gpu();
        const std::string fname(static_cast<const char*>(corpus_fname_ptr), fname_len);
        std::FILE* fp = std::fopen(fname.c_str(), "rb");
        if (!fp) fail("c_tfidf_predict_from_file: can't read " + fname);
        std::vector<char> buf;
        {
            std::fseek(fp, 0, SEEK_END);
            const long sz = std::ftell(fp);
            std::fseek(fp, 0, SEEK_SET);
            if (sz < 0) { std::fclose(fp); fail("c_tfidf_predict_from_file: can't size " + fname); }
            buf.resize((size_t)sz + 1);
            const size_t got = sz ? std::fread(buf.data(), 1, (size_t)sz, fp) : 0;
            std::fclose(fp);
            if (got != (size_t)sz) fail("c_tfidf_predict_from_file: error reading " + fname);
            buf[(size_t)sz] = '\0';
        }
        const size_t n = buf.size() - 1;
        std::vector<const char*> docs; std::vector<size_t> lens;
        size_t start = 0;
        for (size_t i = 0; i < n; ++i)
            if (buf[i] == '\n') { docs.push_back(buf.data() + start); lens.push_back(i - start); start = i + 1; }
        if (start < n) { docs.push_back(buf.data() + start); lens.push_back(n + 1 - start); }   // (the NUL is part of the reference's last document)
        if (docs.empty()) fail("c_tfidf_predict_from_file: " + fname + " holds no document");
        tfidf_predict_to_host(*static_cast<TfidfHandle*>(ptr), docs.data(), lens.data(), docs.size(), threads, pred_alloc);
    });
}

void* xrl_tfidf_predict_device(void* vectorizer, void* model, void* corpus_ptr, const size_t* doc_lens, size_t nr_doc, int threads) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        if (!vectorizer) fail("xrl_tfidf_predict_device: null vectorizer handle");
        if (nr_doc && (!corpus_ptr || !doc_lens)) fail("xrl_tfidf_predict_device: null corpus");
        Model& m = *as_model(model);
        const TfidfHandle& H = *static_cast<TfidfHandle*>(vectorizer);
        return tfidf_to_device(H, static_cast<const char* const*>(corpus_ptr), doc_lens, nr_doc, threads, m.device, m.stream).release();
    });
}

// ---- the device tokenizer (K9): document bytes in HBM.  Null arguments are refused before the GPU is touched.
static void check_device_text_args(const char* what, void* vectorizer, void* model, const void* d_text, const void* d_doc_off, const void* d_doc_len, uint64_t nr_doc) {
    const std::string w = std::string(what) + ": ";
    if (!vectorizer) fail(w + "null vectorizer handle");
    if (!model) fail(w + "null model handle");
    if (nr_doc && (!d_text || !d_doc_off || !d_doc_len)) fail(w + "null text, offsets or lengths");
    if (nr_doc > 0xFFFFFFFFull) fail("tfidf: too many documents");
}

void* xrl_tfidf_counts_device(void* vectorizer, void* model, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len, uint64_t nr_doc,
                              uint32_t* d_status, void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        check_device_text_args("xrl_tfidf_counts_device", vectorizer, model, d_text, d_doc_off, d_doc_len, nr_doc);
        Model& m = *as_model(model);
        const TfidfHandle& H = *static_cast<TfidfHandle*>(vectorizer);
        use_device(m.device);
        std::lock_guard<std::mutex> stage_lock(H.stage.mu);      // (the pooled stream is handed out under this lock)
        hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : m.stream ? m.stream : H.stream_on(m.device);
        TokCounts C;
        tfidf_count_on_device(H, d_text, d_doc_off, d_doc_len, nullptr, nr_doc, d_status, m.device, s, C);
        const uint32_t nb = (uint32_t)H.v.base.size(), rows = (uint32_t)nr_doc;
        auto q = std::make_unique<Queries>();
        q->own = std::move(C.csr);
        const DevBuf seg = seg_to_row_ptr(q->own, nullptr, nb, rows, s);
        if (nb > 1) XRL_HIP(hipStreamSynchronize(s));            // (the segment pointer goes with this scope)
        set_own_csr(*q, m.device, rows, H.v.nr_features);
        return q.release();
    });
}

void* xrl_tfidf_predict_device_text(void* vectorizer, void* model, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len, uint64_t nr_doc,
                                    void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        check_device_text_args("xrl_tfidf_predict_device_text", vectorizer, model, d_text, d_doc_off, d_doc_len, nr_doc);
        Model& m = *as_model(model);
        const TfidfHandle& H = *static_cast<TfidfHandle*>(vectorizer);
        use_device(m.device);
        std::lock_guard<std::mutex> stage_lock(H.stage.mu);
        hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : m.stream ? m.stream : H.stream_on(m.device);
        return tfidf_device_text_to_x(H, d_text, d_doc_off, d_doc_len, nullptr, nr_doc, m.device, s).release();
    });
}

void* xrl_tfidf_predict_device_tok(void* vectorizer, void* model, void* corpus_ptr, const size_t* doc_lens, size_t nr_doc, int tokenizer, int threads) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        if (!vectorizer) fail("xrl_tfidf_predict_device_tok: null vectorizer handle");
        if (!model) fail("xrl_tfidf_predict_device_tok: null model handle");
        if (nr_doc && (!corpus_ptr || !doc_lens)) fail("xrl_tfidf_predict_device_tok: null corpus");
        if (tokenizer != 0 && tokenizer != 1) fail("xrl_tfidf_predict_device_tok: tokenizer must be 0 (host) or 1 (device)");
        if (nr_doc > 0xFFFFFFFFull) fail("tfidf: too many documents");
        Model& m = *as_model(model);
        const TfidfHandle& H = *static_cast<TfidfHandle*>(vectorizer);
        const char* const* corpus = static_cast<const char* const*>(corpus_ptr);
        if (tokenizer == 0) return tfidf_to_device(H, corpus, doc_lens, nr_doc, threads, m.device, m.stream).release();
        use_device(m.device);
        std::lock_guard<std::mutex> stage_lock(H.stage.mu);      // held until the stream has consumed the staging buffer
        hipStream_t s = m.stream ? m.stream : H.stream_on(m.device);
        // the corpus packed into the pinned staging as [offsets u64 | lengths u64 | bytes], one copy to the device
        std::vector<uint64_t> off((size_t)nr_doc + 1, 0);
        for (size_t d = 0; d < nr_doc; ++d) off[d + 1] = off[d] + doc_lens[d];
        const size_t head = nr_doc * 16, total = head + (size_t)off[nr_doc];
        char* st = static_cast<char*>(H.stage.need(total + 16));
        std::memcpy(st, off.data(), nr_doc * 8);
        for (size_t d = 0; d < nr_doc; ++d) reinterpret_cast<uint64_t*>(st + nr_doc * 8)[d] = doc_lens[d];
        {
            unsigned nt = threads > 0 ? (unsigned)threads : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
            nt = (unsigned)std::max<size_t>(1, std::min<size_t>(nt, (size_t)off[nr_doc] >> 20));
            auto work = [&](unsigned t) {
                for (size_t d = nr_doc * t / nt, e = nr_doc * (t + 1) / nt; d < e; ++d)
                    if (doc_lens[d]) std::memcpy(st + head + off[d], corpus[d], doc_lens[d]);
            };
            std::vector<std::thread> th;
            for (unsigned t = 1; t < nt; ++t) th.emplace_back(work, t);
            work(0);
            for (auto& x : th) x.join();
        }
        DevBuf d_in;
        d_in.reserve(total + 16);
        if (total) XRL_HIP(hipMemcpyAsync(d_in.p, st, total, hipMemcpyHostToDevice, s));
        const uint64_t* d_off = d_in.as<uint64_t>();
        return tfidf_device_text_to_x(H, reinterpret_cast<const uint8_t*>(d_in.p) + head, d_off, d_off + nr_doc, reinterpret_cast<const uint64_t*>(st + nr_doc * 8), nr_doc,
                                      m.device, s).release();
    });
}

uint64_t xrl_tfidf_device_bytes(void* vectorizer, int device) {
    return guarded_value((uint64_t)0, [&]() -> uint64_t {
        if (!vectorizer) fail("xrl_tfidf_device_bytes: null vectorizer handle");
        const TfidfHandle& H = *static_cast<TfidfHandle*>(vectorizer);
        std::lock_guard<std::mutex> g(H.dev_mu);
        auto it = H.dev_tables.find(device);
        return it == H.dev_tables.end() ? 0 : it->second->bytes;
    });
}

// debug: out[0..n) <- {segments the LDS form served, segments the global form served, batches, calls} of the device tokenizer since the load
int xrl_debug_tfidf_device_forms(void* vectorizer, uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&]() -> int {
        if (!vectorizer || !out) fail("xrl_debug_tfidf_device_forms: null argument");
        const TfidfHandle& H = *static_cast<TfidfHandle*>(vectorizer);
        for (uint32_t i = 0; i < n && i < 4; ++i) out[i] = H.forms[i].load();
        return 0;
    });
}

// ---- training (K15, xrl_tfidf_train.hip), saving, export
// what the arguments alone decide: refused before a GPU is required
static void check_train_args(const std::string& w, const TfidfVectorizerParam* param, uint64_t nr_doc) {
    if (!param) fail(w + "null param");
    if (nr_doc == 0) fail(w + "Invalid nr_doc 0");
    if (nr_doc > 0xFFFFFFFFull) fail(w + "too many documents (2^32 or more)");
    if (param->num_base_vect <= 0) fail(w + "num_base_vect must be positive");
    if (!param->base_param_ptr) fail(w + "null base_param_ptr");
    if (param->norm_p != 1 && param->norm_p != 2) fail(w + "invalid normalize option, norm_p: [ 1| 2]");
    for (int32_t b = 0; b < param->num_base_vect; ++b) {
        const TfidfBaseVectorizerParam& P = param->base_param_ptr[b];
        if (P.tok_type != 10 && P.tok_type != 20 && P.tok_type != 30) fail(w + "received unknown tok_type: " + std::to_string(P.tok_type));
        if (P.tok_type == 30) fail(w + "tok_type 30 (char_wb) is not served by device training");
        if (P.min_df_ratio < 0 || P.max_df_ratio <= P.min_df_ratio || P.max_df_ratio > 1.0) fail(w + "expect 0 <= min_df_ratio < max_df_ratio <= 1.0");
        if (P.min_ngram <= 0 || P.min_ngram > P.max_ngram) fail(w + "expect 0 < min_ngram <= max_ngram");
        if (P.norm_p != 1 && P.norm_p != 2) fail(w + "invalid normalize option, norm_p: [ 1| 2]");
    }
}

static TfidfHandle* train_handle(const std::string& w, const TfidfVectorizerParam* param, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len,
                                 const uint64_t* h_doc_off, const uint64_t* h_doc_len, uint64_t nr_doc, hipStream_t s) {
    auto h = std::make_unique<TfidfHandle>();
    TfidfVectorizer& V = h->v;
    const std::vector<TfidfBaseVectorizerParam> params(param->base_param_ptr, param->base_param_ptr + param->num_base_vect);
    V.base.resize(params.size());
    V.norm_p = param->norm_p;
    for (size_t b = 0; b < params.size(); ++b) {
        const TfidfBaseVectorizerParam& P = params[b];
        TfidfBase& B = V.base[b];
        B.tok_type = P.tok_type; B.min_ngram = P.min_ngram; B.max_ngram = P.max_ngram; B.max_length = P.max_length; B.norm_p = P.norm_p;
        B.binary = P.binary; B.use_idf = P.use_idf; B.sublinear_tf = P.sublinear_tf;
        B.max_feature = P.max_feature; B.min_df_cnt = P.min_df_cnt; B.max_df_cnt = P.max_df_cnt; B.min_df_ratio = P.min_df_ratio; B.max_df_ratio = P.max_df_ratio;
        B.smooth_idf = P.smooth_idf; B.add_one_idf = P.add_one_idf; B.keep_frequent_feature = P.keep_frequent_feature;
    }
    uint64_t first_bad[2];
    tfidf_train_device(V.base, params, d_text, d_doc_off, d_doc_len, h_doc_off, h_doc_len, nr_doc, s, h->train_forms, first_bad);
    if (first_bad[0] != ~0ull) fail(w + "the string is not utf-8 encoded! (document " + std::to_string(first_bad[0]) + ")");
    if (first_bad[1] != ~0ull)
        fail(w + "document " + std::to_string(first_bad[1]) + " holds a UTF-8 lead byte followed by too few continuation bytes, which the reference's "
             "sequential decode reads along another path: not served by device training");
    uint64_t tot = 0;
    for (const auto& b : V.base) { tot += b.nr_features; h->idf_all.insert(h->idf_all.end(), b.idf.begin(), b.idf.end()); }
    if (tot > 0xFFFFFFFFull) fail(w + "too many features");
    V.nr_features = (uint32_t)tot;
    return h.release();
}

// the tokens and n-grams a base vectorizer's tables hold, in table order
static void enumerate_base(const TfidfBase& B, std::vector<std::pair<std::string, int32_t>>& tokens, std::vector<int32_t>& flat, std::vector<uint64_t>& off,
                           std::vector<uint32_t>& ids) {
    tokens.clear(); flat.clear(); ids.clear(); off.assign(1, 0);
    for (size_t i = 0; i < B.vocab.s.size(); ++i) {
        const tft::ShortEntry& e = B.vocab.s[i];
        if (!e.len) continue;
        std::string t(e.len, '\0');
        for (uint32_t j = 0; j < e.len; ++j) t[j] = (char)(uint8_t)(e.key >> (8 * j));
        tokens.emplace_back(std::move(t), e.idx);
    }
    for (size_t i = 0; i < B.vocab.l.size(); ++i) {
        const tft::LongEntry& e = B.vocab.l[i];
        if (e.len) tokens.emplace_back(B.vocab.arena.substr(e.off, e.len), e.idx);
    }
    const NgramTable& G = B.features;
    for (size_t t = 0; t < G.uni.size(); ++t)
        if (G.uni[t] != NgramTable::kNone) { flat.push_back((int32_t)t); off.push_back(flat.size()); ids.push_back(G.uni[t] - 1u); }
    const uint64_t field = G.pack_bits >= 64 ? ~0ull : (1ull << G.pack_bits) - 1;
    for (size_t i = 0; i < G.packed.size(); ++i) {
        const tft::PackedEntry& e = G.packed[i];
        if (e.id1 == NgramTable::kNone) continue;
        for (unsigned sh = 0; sh < 64; sh += G.pack_bits) {
            const uint64_t f = (e.key >> sh) & field;
            if (!f) break;
            flat.push_back((int32_t)(uint32_t)(f - 1));
        }
        off.push_back(flat.size()); ids.push_back(e.id1 - 1u);
    }
    for (size_t i = 0; i < G.gen.size(); ++i) {
        const tft::GenEntry& e = G.gen[i];
        if (e.id1 == NgramTable::kNone) continue;
        flat.insert(flat.end(), G.arena.begin() + e.off, G.arena.begin() + e.off + e.n);
        off.push_back(flat.size()); ids.push_back(e.id1 - 1u);
    }
}

static void make_dir(const std::string& d, const char* what) {
    if (mkdir(d.c_str(), 0777) == -1 && errno != EEXIST) fail(std::string("xrl_tfidf_save: Unable to create ") + what + " at " + d);
}
static std::FILE* open_w(const std::string& f) {
    std::FILE* fp = std::fopen(f.c_str(), "wb");
    if (!fp) fail("xrl_tfidf_save: Unable to save to " + f);
    return fp;
}
// a float as nlohmann prints it: the double it converts to, with enough digits to read back exactly, always with a '.' or an exponent
static std::string json_float(float v) {
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%.17g", (double)v);
    std::string s(buf);
    if (s.find_first_of(".en") == std::string::npos) s += ".0";
    return s;
}

static void save_base(const TfidfBase& B, const std::string& dir) {
    make_dir(dir, "save folder");
    make_dir(dir + "/tokenizer", "save folder");
    make_dir(dir + "/vectorizer", "save folder");
    std::vector<std::pair<std::string, int32_t>> tokens; std::vector<int32_t> flat; std::vector<uint64_t> off; std::vector<uint32_t> ids;
    enumerate_base(B, tokens, flat, off, ids);
    std::FILE* fp = open_w(dir + "/tokenizer/config.json");
    std::fprintf(fp, "{\n    \"token_type\": %d\n}", B.tok_type);
    std::fclose(fp);
    fp = open_w(dir + "/tokenizer/vocab.txt");
    std::fprintf(fp, "%zu\n", tokens.size());
    for (const auto& t : tokens) { std::fprintf(fp, "%d\t", t.second); std::fwrite(t.first.data(), 1, t.first.size(), fp); std::fputc('\n', fp); }
    std::fclose(fp);
    const auto tf = [](bool b) { return b ? "true" : "false"; };
    fp = open_w(dir + "/vectorizer/config.json");
    std::fprintf(fp,
                 "{\n    \"kwargs\": {\n        \"add_one_idf\": %s,\n        \"binary\": %s,\n        \"keep_frequent_feature\": %s,\n        \"max_df_cnt\": %d,\n"
                 "        \"max_df_ratio\": %s,\n        \"max_feature\": %d,\n        \"max_length\": %d,\n        \"min_df_cnt\": %d,\n        \"min_df_ratio\": %s,\n"
                 "        \"ngram_range\": [\n            %d,\n            %d\n        ],\n        \"norm_p\": \"%s\",\n        \"smooth_idf\": %s,\n"
                 "        \"sublinear_tf\": %s,\n        \"use_idf\": %s\n    },\n    \"type\": \"tfidf\"\n}",
                 tf(B.add_one_idf), tf(B.binary), tf(B.keep_frequent_feature), B.max_df_cnt, json_float(B.max_df_ratio).c_str(), B.max_feature, B.max_length, B.min_df_cnt,
                 json_float(B.min_df_ratio).c_str(), B.min_ngram, B.max_ngram, B.norm_p == 1 ? "l1" : "l2", tf(B.smooth_idf), tf(B.sublinear_tf), tf(B.use_idf));
    std::fclose(fp);
    fp = open_w(dir + "/vectorizer/tfidf-model.txt");
    std::fprintf(fp, "%zu\n", ids.size());
    for (size_t f = 0; f < ids.size(); ++f) {
        const float v = ids[f] < B.idf.size() ? B.idf[ids[f]] : 0.0f;
        std::fprintf(fp, "%d\t%f\t%zu", (int)ids[f], v, (size_t)(off[f + 1] - off[f]));
        for (uint64_t i = off[f]; i < off[f + 1]; ++i) std::fprintf(fp, i == off[f] ? "\t%d" : " %d", flat[i]);
        std::fputc('\n', fp);
    }
    std::fclose(fp);
}

void* xrl_tfidf_train(void* corpus_ptr, const size_t* doc_lens, size_t nr_doc, const TfidfVectorizerParam* param, int threads) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const std::string w = "xrl_tfidf_train: ";
        if (!corpus_ptr || !doc_lens) fail(w + "null corpus");
        check_train_args(w, param, nr_doc);
        require_gpu();
        use_device(g_device);
        const char* const* corpus = static_cast<const char* const*>(corpus_ptr);
        // the corpus packed into pinned staging as [offsets u64 | lengths u64 | bytes], one copy to the device (as xrl_tfidf_predict_device_tok)
        std::vector<uint64_t> off((size_t)nr_doc + 1, 0), len((size_t)nr_doc);
        for (size_t d = 0; d < nr_doc; ++d) { len[d] = doc_lens[d]; off[d + 1] = off[d] + doc_lens[d]; }
        const size_t head = nr_doc * 16, total = head + (size_t)off[nr_doc];
        PinnedStage stage;
        char* st = static_cast<char*>(stage.need(total + 16));
        std::memcpy(st, off.data(), nr_doc * 8);
        std::memcpy(st + nr_doc * 8, len.data(), nr_doc * 8);
        {
            unsigned nt = threads > 0 ? (unsigned)threads : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
            nt = (unsigned)std::max<size_t>(1, std::min<size_t>(nt, (size_t)off[nr_doc] >> 20));
            auto work = [&](unsigned t) {
                for (size_t d = nr_doc * t / nt, e = nr_doc * (t + 1) / nt; d < e; ++d)
                    if (doc_lens[d]) std::memcpy(st + head + off[d], corpus[d], doc_lens[d]);
            };
            std::vector<std::thread> th;
            for (unsigned t = 1; t < nt; ++t) th.emplace_back(work, t);
            work(0);
            for (auto& x : th) x.join();
        }
        hipStream_t s = nullptr;
        XRL_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        struct Drop { hipStream_t s; ~Drop() { (void)hipStreamDestroy(s); } } drop{s};
        DevBuf d_in;
        d_in.reserve(total + 16);
        XRL_HIP(hipMemcpyAsync(d_in.p, st, total, hipMemcpyHostToDevice, s));
        const uint64_t* d_off = d_in.as<uint64_t>();
        return train_handle(w, param, reinterpret_cast<const uint8_t*>(d_in.p) + head, d_off, d_off + nr_doc, off.data(), len.data(), nr_doc, s);
    });
}

void* xrl_tfidf_train_device(int device, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len, uint64_t nr_doc,
                             const TfidfVectorizerParam* param, void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const std::string w = "xrl_tfidf_train_device: ";
        if (!d_text || !d_doc_off || !d_doc_len) fail(w + "null text, offsets or lengths");
        check_train_args(w, param, nr_doc);
        require_gpu();
        use_device(device);
        hipStream_t s = static_cast<hipStream_t>(hip_stream), own = nullptr;
        if (!s) { XRL_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking)); s = own; }
        struct Drop { hipStream_t s; ~Drop() { if (s) (void)hipStreamDestroy(s); } } drop{own};
        std::vector<uint64_t> off((size_t)nr_doc), len((size_t)nr_doc);
        XRL_HIP(hipMemcpyAsync(off.data(), d_doc_off, nr_doc * 8, hipMemcpyDeviceToHost, s));
        XRL_HIP(hipMemcpyAsync(len.data(), d_doc_len, nr_doc * 8, hipMemcpyDeviceToHost, s));
        XRL_HIP(hipStreamSynchronize(s));
        return train_handle(w, param, d_text, d_doc_off, d_doc_len, off.data(), len.data(), nr_doc, s);
    });
}

void xrl_tfidf_save(void* vectorizer, const char* model_dir) {
    guarded([&] {
        if (!vectorizer || !model_dir) fail("xrl_tfidf_save: null argument");
        const TfidfVectorizer& V = static_cast<TfidfHandle*>(vectorizer)->v;
        const std::string dir(model_dir);
        make_dir(dir, "save folder");
        std::FILE* fp = open_w(dir + "/meta.json");
        std::fprintf(fp, "{\n    \"kwargs\": {\n        \"norm_p\": %d,\n        \"num_base_vect\": %zu\n    },\n    \"type\": \"tfidf\"\n}", V.norm_p, V.base.size());
        std::fclose(fp);
        for (size_t b = 0; b < V.base.size(); ++b) save_base(V.base[b], dir + "/" + std::to_string(b) + ".base");
    });
}

void* xrl_tfidf_transform_device(void* vectorizer, int device, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len, uint64_t nr_doc,
                                 uint32_t* d_status, void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const std::string w = "xrl_tfidf_transform_device: ";
        if (!vectorizer) fail(w + "null vectorizer handle");
        if (nr_doc && (!d_text || !d_doc_off || !d_doc_len)) fail(w + "null text, offsets or lengths");
        if (nr_doc > 0xFFFFFFFFull) fail("tfidf: too many documents");
        require_gpu();
        const TfidfHandle& H = *static_cast<TfidfHandle*>(vectorizer);
        use_device(device);
        std::lock_guard<std::mutex> stage_lock(H.stage.mu);      // (the pooled stream is handed out under this lock)
        hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : H.stream_on(device);
        if (!d_status) return tfidf_device_text_to_x(H, d_text, d_doc_off, d_doc_len, nullptr, nr_doc, device, s).release();
        TokCounts C;
        tfidf_count_on_device(H, d_text, d_doc_off, d_doc_len, nullptr, nr_doc, d_status, device, s, C);
        auto q = std::make_unique<Queries>();
        q->own = std::move(C.csr);
        tfidf_weight_counts(H, q.get(), nullptr, (uint32_t)nr_doc, device, s);
        return q.release();
    });
}

int xrl_tfidf_export(void* vectorizer, uint32_t base, uint64_t* sizes, uint8_t* tok_bytes, uint64_t* tok_off, int32_t* tok_ids, int32_t* ng_flat, uint64_t* ng_off,
                     uint32_t* ng_ids, float* idf) {
    return guarded_value(-1, [&]() -> int {
        if (!vectorizer || !sizes) fail("xrl_tfidf_export: null argument");
        const TfidfVectorizer& V = static_cast<TfidfHandle*>(vectorizer)->v;
        if (base >= V.base.size()) fail("xrl_tfidf_export: base " + std::to_string(base) + " of " + std::to_string(V.base.size()));
        const TfidfBase& B = V.base[base];
        std::vector<std::pair<std::string, int32_t>> tokens; std::vector<int32_t> flat; std::vector<uint64_t> off; std::vector<uint32_t> ids;
        enumerate_base(B, tokens, flat, off, ids);
        uint64_t bytes = 0;
        for (const auto& t : tokens) bytes += t.first.size();
        sizes[0] = tokens.size(); sizes[1] = bytes; sizes[2] = ids.size(); sizes[3] = flat.size(); sizes[4] = B.idf.size();
        uint64_t at = 0;
        for (size_t i = 0; i < tokens.size(); ++i) {
            if (tok_off) tok_off[i] = at;
            if (tok_bytes) std::memcpy(tok_bytes + at, tokens[i].first.data(), tokens[i].first.size());
            if (tok_ids) tok_ids[i] = tokens[i].second;
            at += tokens[i].first.size();
        }
        if (tok_off) tok_off[tokens.size()] = at;
        if (ng_flat && !flat.empty()) std::memcpy(ng_flat, flat.data(), flat.size() * 4);
        if (ng_off) std::memcpy(ng_off, off.data(), off.size() * 8);
        if (ng_ids && !ids.empty()) std::memcpy(ng_ids, ids.data(), ids.size() * 4);
        if (idf && !B.idf.empty()) std::memcpy(idf, B.idf.data(), B.idf.size() * 4);
        return 0;
    });
}

int xrl_debug_tfidf_train_forms(void* vectorizer, uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&]() -> int {
        if (!vectorizer || !out) fail("xrl_debug_tfidf_train_forms: null argument");
        const TrainForms& F = static_cast<TfidfHandle*>(vectorizer)->train_forms;
        const uint64_t v[11] = {F.vocab_docs, F.df_lds, F.df_global, F.batches, F.distinct_tokens, F.distinct_ngrams, F.long_compares, F.table_grows,
                                F.us_vocab, F.us_df, F.us_order};
        for (uint32_t i = 0; i < n && i < 11; ++i) out[i] = v[i];
        return 0;
    });
}

// host only (no GPU): the hstacked TERM-COUNT CSR the device weighting starts from -- what the tokenizer and the n-gram lookup produce
void xrl_tfidf_counts(void* ptr, void* corpus_ptr, const size_t* doc_lens, size_t nr_doc, int threads, py_sparse_allocator_t alloc) {
    guarded([&] {
        if (!ptr || !alloc || (nr_doc && (!corpus_ptr || !doc_lens))) fail("xrl_tfidf_counts: null argument");
        const TfidfVectorizer& V = static_cast<TfidfHandle*>(ptr)->v;
        std::vector<uint64_t> seg_ptr;
        uint32_t* indices = nullptr; uint64_t* indptr = nullptr; float* data = nullptr;
        // the allocator's arrays ARE the destination: the worker threads fill (and first-touch) them in parallel
        V.count_corpus(static_cast<const char* const*>(corpus_ptr), doc_lens, nr_doc, threads, seg_ptr, [&](uint64_t n, uint32_t*& c, float*& v) {
            alloc(false, nr_doc, V.nr_features, n, &indices, &indptr, &data);
            if (!indptr || (n && (!indices || !data))) fail("allocator returned null");
            c = indices; v = data;
        });
        const size_t nb = V.base.size();
        for (size_t r = 0; r <= nr_doc; ++r) indptr[r] = seg_ptr[r * nb];
    });
}

}  // extern "C"
