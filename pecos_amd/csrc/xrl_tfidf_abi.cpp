// TF-IDF query producer (libpecos.cpp:398-445): c_tfidf_load / c_tfidf_destruct / c_tfidf_predict with the
// reference's signatures, and the xrl_tfidf_* entry points that leave X in HBM for xrl_predict_device, count on the device (K9) and train
// there (K15).  Host texts reach X through tfidf_to_device (host counts) or pack_corpus + tfidf_text_to_queries (device counts); text in
// HBM through tfidf_text_to_queries alone.  The model files, saving included, are xrl_tfidf.cpp's.
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

// The one threaded host copy of this file: copy(t, nt) moves share t of nt of a payload of `bytes` bytes, on nt host threads (the
// caller's is one).  nt is the caller's `threads`, or without one (<= 0) the hardware's up to 16; never more than one thread per whole
// MiB of payload, and at least one.
template <class Copy> void copy_on_host_threads(size_t bytes, int threads, const Copy& copy) {
    unsigned nt = threads > 0 ? (unsigned)threads : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    nt = (unsigned)std::max<size_t>(1, std::min<size_t>(nt, bytes >> 20));
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(copy, t, nt);
    copy(0u, nt);
    for (auto& x : th) x.join();
}

// dst <- src on host threads, one contiguous share each
void parallel_copy(void* dst, const void* src, size_t bytes, int threads) {
    copy_on_host_threads(bytes, threads, [&](unsigned t, unsigned nt) {
        const size_t b = bytes / nt * t, e = t + 1 == nt ? bytes : bytes / nt * (t + 1);
        std::memcpy(static_cast<char*>(dst) + b, static_cast<const char*>(src) + b, e - b);
    });
}

// A host corpus packed into pinned staging as [offsets u64 | lengths u64 | bytes] on host threads: one copy takes it to the device.
// The staging stays the host copy of the offsets and lengths, so it must outlive their readers.
struct PackedCorpus {
    const char* st = nullptr; size_t nr_doc = 0, head = 0, total = 0;         // staging; its header's bytes; header + text
    const uint64_t* off() const { return reinterpret_cast<const uint64_t*>(st); }
    const uint64_t* len() const { return off() + nr_doc; }
    // (every caller's next step: the device copy, ordered on s, in a buffer with the 16 spare bytes the staging has)
    DevBuf upload(hipStream_t s) const {
        DevBuf d;
        d.reserve(total + 16);
        if (total) XRL_HIP(hipMemcpyAsync(d.p, st, total, hipMemcpyHostToDevice, s));
        return d;
    }
};
PackedCorpus pack_corpus(PinnedStage& stage, const char* const* corpus, const size_t* doc_lens, size_t nr_doc, int threads) {
    uint64_t bytes = 0;
    for (size_t d = 0; d < nr_doc; ++d) bytes += doc_lens[d];
    PackedCorpus P;
    P.nr_doc = nr_doc; P.head = nr_doc * 16; P.total = P.head + (size_t)bytes;
    char* const st = static_cast<char*>(stage.need(P.total + 16));
    P.st = st;
    uint64_t* const off = reinterpret_cast<uint64_t*>(st); uint64_t* const len = off + nr_doc;
    uint64_t at = 0;
    for (size_t d = 0; d < nr_doc; ++d) { off[d] = at; len[d] = doc_lens[d]; at += doc_lens[d]; }
    copy_on_host_threads((size_t)bytes, threads, [&](unsigned t, unsigned nt) {
        for (size_t d = nr_doc * t / nt, e = nr_doc * (t + 1) / nt; d < e; ++d)
            if (len[d]) std::memcpy(st + P.head + off[d], corpus[d], len[d]);
    });
    return P;
}

struct TfidfHandle {
    TfidfVectorizer v;
    mutable PinnedStage stage;
    // c_tfidf_predict's stream, created once per (handle, device) instead of per call
    mutable std::mutex stream_mu;
    mutable hipStream_t stream = nullptr;
    mutable int stream_device = -1;
    // call with the staging lock (stage.mu) HELD: StagedStream does
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

// What every device call of a handle starts with: `device` set, the handle's staging lock taken, a stream chosen -- the caller's, else
// the model's, else the handle's pooled one.  The lock lives as long as this object, and this object until the stream has been
// synchronised: the staging buffer belongs to the transfer enqueued on the stream, and a call that switched devices REPLACES the pooled
// stream, which must not happen under another thread's transfer.
struct StagedStream {
    std::unique_lock<std::mutex> lock;
    hipStream_t s = nullptr;
    StagedStream(const TfidfHandle& H, int device, void* caller, hipStream_t model) {
        use_device(device);
        lock = std::unique_lock<std::mutex>(H.stage.mu);
        s = caller ? static_cast<hipStream_t>(caller) : model ? model : H.stream_on(device);
    }
};

// the hstacked CSR's row pointer out of the segment pointer of nb base vectorizers side by side: every nb-th entry
std::vector<uint64_t> row_ptr_of(const std::vector<uint64_t>& seg_ptr, size_t nb, size_t rows) {
    std::vector<uint64_t> row_ptr(rows + 1);
    for (size_t r = 0; r <= rows; ++r) row_ptr[r] = seg_ptr[r * nb];
    return row_ptr;
}

// c.ptr holds the SEGMENT pointer of nb base vectorizers side by side -> the hstacked CSR's row pointer (every nb-th entry; h_seg: the
// segment pointer on the host when the host counted, nullptr: gathered by a kernel on s).  Returns the segment pointer, which the work
// enqueued on s may still read: the caller keeps it until s is synchronised.
DevBuf seg_to_row_ptr(DevCsr& c, const std::vector<uint64_t>* h_seg, uint32_t nb, uint32_t rows, hipStream_t s) {
    if (nb == 1) return {};
    DevBuf seg = std::move(c.ptr);
    if (h_seg) {
        c.ptr.upload(row_ptr_of(*h_seg, nb, rows));
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
    d_idf.upload(V.idf_all);
    d_err.reserve(4); XRL_HIP(hipMemsetAsync(d_err.p, 0, 4, s));
    for (uint32_t b = 0; b < nb; ++b) {
        const TfidfBase& B = V.base[b];
        launch_tfidf_weight(c.ptr.as<uint64_t>(), c.idx.as<uint32_t>(), c.val.as<float>(), B.use_idf ? d_idf.as<float>() : nullptr, rows, V.nr_features,
                            B.binary ? 1 : 0, B.sublinear_tf ? 1 : 0, B.norm_p, c.val.as<float>(), s, nb, b, d_err.as<uint32_t>());
    }
    // whole rows: the hstacked CSR's row pointer; the ensemble's normalisation
    const DevBuf seg = seg_to_row_ptr(c, h_seg, nb, rows, s);
    if (V.ensemble_norm_runs())
        launch_tfidf_weight(c.ptr.as<uint64_t>(), c.idx.as<uint32_t>(), c.val.as<float>(), nullptr, rows, V.nr_features, 0, 0, V.norm_p, c.val.as<float>(), s);
    uint32_t err = 0;
    XRL_HIP(hipMemcpyAsync(&err, d_err.p, 4, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    if (err) fail("tfidf: a feature id outside the model's feature range");
    set_own_csr(*q, device, rows, V.nr_features);
}

// texts -> term counts (host threads, into pinned staging) -> device -> weighting + normalisation (K5): a query handle that owns its three arrays
std::unique_ptr<Queries> tfidf_to_device(const TfidfHandle& H, const char* const* corpus, const size_t* doc_lens, size_t nr_doc, int threads, int device,
                                         hipStream_t model_stream) {
    if (nr_doc > 0xFFFFFFFFull) fail("tfidf: too many documents");
    const TfidfVectorizer& V = H.v;
    const uint32_t rows = (uint32_t)nr_doc;
    const StagedStream on(H, device, nullptr, model_stream);     // (until tfidf_weight_counts has synchronised)
    const hipStream_t s = on.s;
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

// The one path from text in HBM to a query handle: counts (K9), then either the weighting tail (X ready for xrl_predict_device) or, for
// the counts themselves, the row pointer alone.  d_status as for tfidf_count_on_device.  Synchronised when it returns.
std::unique_ptr<Queries> tfidf_text_to_queries(const TfidfHandle& H, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len,
                                               const uint64_t* h_doc_len, uint64_t nr_doc, uint32_t* d_status, bool weighted, int device, hipStream_t s) {
    TokCounts C;
    tfidf_count_on_device(H, d_text, d_doc_off, d_doc_len, h_doc_len, nr_doc, d_status, device, s, C);
    const uint32_t nb = (uint32_t)H.v.base.size(), rows = (uint32_t)nr_doc;
    auto q = std::make_unique<Queries>();
    q->own = std::move(C.csr);
    if (weighted) { tfidf_weight_counts(H, q.get(), nullptr, rows, device, s); return q; }
    const DevBuf seg = seg_to_row_ptr(q->own, nullptr, nb, rows, s);
    if (nb > 1) XRL_HIP(hipStreamSynchronize(s));                // (the segment pointer goes with this scope)
    set_own_csr(*q, device, rows, H.v.nr_features);
    return q;
}

// the caller's arrays for a rows x cols CSR of nnz entries: ONE allocator call, refused when it hands back nothing to write to
struct CsrArrays { uint32_t* indices = nullptr; uint64_t* indptr = nullptr; float* data = nullptr; };
CsrArrays alloc_csr(py_sparse_allocator_t alloc, uint64_t rows, uint64_t cols, uint64_t nnz) {
    CsrArrays a;
    alloc(false, rows, cols, nnz, &a.indices, &a.indptr, &a.data);
    if (!a.indptr || (nnz && (!a.indices || !a.data))) fail("allocator returned null");
    return a;
}
}  // namespace

extern "C" {

void* c_tfidf_load(const char* model_dir) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        if (!model_dir) fail("null model_dir");
        auto h = std::make_unique<TfidfHandle>();
        h->v.load(model_dir);
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
        tfidf_weight_host(seg_ptr.data(), h_col.data(), h_val.data(), B.use_idf ? V.idf_all.data() : nullptr, rows, V.nr_features, B.binary, B.sublinear_tf, B.norm_p, nb, b);
    }
    const std::vector<uint64_t> row_ptr = row_ptr_of(seg_ptr, nb, rows);
    if (V.ensemble_norm_runs())
        tfidf_weight_host(row_ptr.data(), h_col.data(), h_val.data(), nullptr, rows, V.nr_features, false, false, V.norm_p, 1, 0);
    const CsrArrays out = alloc_csr(pred_alloc, rows, V.nr_features, nnz);
    std::memcpy(out.indptr, row_ptr.data(), ((size_t)rows + 1) * 8);
    if (nnz) { std::memcpy(out.indices, h_col.data(), (size_t)nnz * 4); std::memcpy(out.data, h_val.data(), (size_t)nnz * 4); }
}

static void tfidf_predict_to_host(const TfidfHandle& H, const char* const* corpus, const size_t* doc_lens, size_t nr_doc, int threads, py_sparse_allocator_t pred_alloc) {
    const char* hs = std::getenv("XRL_TFIDF_HOST_DOCS");                     // XRL_TFIDF_HOST_DOCS=0: always the device (tests; read per call)
    if (!(hs && hs[0] == '0') && nr_doc <= kTfidfHostDocs) { tfidf_predict_small_on_host(H, corpus, doc_lens, nr_doc, pred_alloc); return; }
    // (no model, so no model stream: the handle's pooled one)
    std::unique_ptr<Queries> q = tfidf_to_device(H, corpus, doc_lens, nr_doc, threads, g_device, nullptr);
    const uint64_t nnz = q->dev.nnz;
    const CsrArrays out = alloc_csr(pred_alloc, q->dev.rows, q->dev.cols, nnz);
    XRL_HIP(hipMemcpy(out.indptr, q->dev.row_ptr, ((size_t)q->dev.rows + 1) * 8, hipMemcpyDeviceToHost));
    if (nnz) {
        // D2H into the pinned staging buffer (link speed), then host threads spread it over the allocator's fresh arrays: their first touch
        // in parallel, instead of the runtime's single-threaded pageable path
        std::lock_guard<std::mutex> stage_lock(H.stage.mu);
        const size_t nb4 = (size_t)nnz * 4;
        char* st = static_cast<char*>(H.stage.need(2 * nb4));
        XRL_HIP(hipMemcpy(st, q->dev.col_idx, nb4, hipMemcpyDeviceToHost));
        XRL_HIP(hipMemcpy(st + nb4, q->dev.val, nb4, hipMemcpyDeviceToHost));
        parallel_copy(out.indices, st, nb4, threads);
        parallel_copy(out.data, st + nb4, nb4, threads);
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

// host texts -> X on the model's device, behind xrl_tfidf_predict_device (tokenizer 0) and xrl_tfidf_predict_device_tok, which check their
// arguments in their own words first.  Tokenizer 1: the corpus goes through the handle's staging to the device in one copy, K9 counts.
static void* tfidf_predict_device_from_host(void* vectorizer, void* model, void* corpus_ptr, const size_t* doc_lens, size_t nr_doc, int tokenizer, int threads) {
    Model& m = *as_model(model);
    const TfidfHandle& H = *static_cast<TfidfHandle*>(vectorizer);
    const char* const* corpus = static_cast<const char* const*>(corpus_ptr);
    if (tokenizer == 0) return tfidf_to_device(H, corpus, doc_lens, nr_doc, threads, m.device, m.stream).release();
    const StagedStream on(H, m.device, nullptr, m.stream);
    const PackedCorpus P = pack_corpus(H.stage, corpus, doc_lens, nr_doc, threads);
    const DevBuf d_in = P.upload(on.s);
    const uint64_t* d_off = d_in.as<uint64_t>();
    return tfidf_text_to_queries(H, d_in.as<uint8_t>() + P.head, d_off, d_off + nr_doc, P.len(), nr_doc, nullptr, true, m.device, on.s).release();
}

void* xrl_tfidf_predict_device(void* vectorizer, void* model, void* corpus_ptr, const size_t* doc_lens, size_t nr_doc, int threads) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        if (!vectorizer) fail("xrl_tfidf_predict_device: null vectorizer handle");
        if (nr_doc && (!corpus_ptr || !doc_lens)) fail("xrl_tfidf_predict_device: null corpus");
        return tfidf_predict_device_from_host(vectorizer, model, corpus_ptr, doc_lens, nr_doc, 0, threads);
    });
}

void* xrl_tfidf_predict_device_tok(void* vectorizer, void* model, void* corpus_ptr, const size_t* doc_lens, size_t nr_doc, int tokenizer, int threads) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        if (!vectorizer) fail("xrl_tfidf_predict_device_tok: null vectorizer handle");
        if (!model) fail("xrl_tfidf_predict_device_tok: null model handle");
        if (nr_doc && (!corpus_ptr || !doc_lens)) fail("xrl_tfidf_predict_device_tok: null corpus");
        if (tokenizer != 0 && tokenizer != 1) fail("xrl_tfidf_predict_device_tok: tokenizer must be 0 (host) or 1 (device)");
        if (nr_doc > 0xFFFFFFFFull) fail("tfidf: too many documents");
        return tfidf_predict_device_from_host(vectorizer, model, corpus_ptr, doc_lens, nr_doc, tokenizer, threads);
    });
}

// ---- the device tokenizer (K9): document bytes in HBM.  Null arguments are refused before the GPU is touched (model_missing: false too
// for the entry point that takes a device instead of a model).
static void check_device_text_args(const std::string& w, void* vectorizer, bool model_missing, const void* d_text, const void* d_doc_off, const void* d_doc_len,
                                   uint64_t nr_doc) {
    if (!vectorizer) fail(w + "null vectorizer handle");
    if (model_missing) fail(w + "null model handle");
    if (nr_doc && (!d_text || !d_doc_off || !d_doc_len)) fail(w + "null text, offsets or lengths");
    if (nr_doc > 0xFFFFFFFFull) fail("tfidf: too many documents");
}

// resident text -> a query handle on the model's device and, without a caller's stream, the model's stream
static void* tfidf_model_text_to_queries(const char* what, void* vectorizer, void* model, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len,
                                         uint64_t nr_doc, uint32_t* d_status, bool weighted, void* hip_stream) {
    check_device_text_args(what, vectorizer, !model, d_text, d_doc_off, d_doc_len, nr_doc);
    Model& m = *as_model(model);
    const TfidfHandle& H = *static_cast<TfidfHandle*>(vectorizer);
    const StagedStream on(H, m.device, hip_stream, m.stream);
    return tfidf_text_to_queries(H, d_text, d_doc_off, d_doc_len, nullptr, nr_doc, d_status, weighted, m.device, on.s).release();
}

void* xrl_tfidf_counts_device(void* vectorizer, void* model, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len, uint64_t nr_doc,
                              uint32_t* d_status, void* hip_stream) {
    return guarded_value((void*)nullptr, [&] {
        return tfidf_model_text_to_queries("xrl_tfidf_counts_device: ", vectorizer, model, d_text, d_doc_off, d_doc_len, nr_doc, d_status, false, hip_stream);
    });
}

void* xrl_tfidf_predict_device_text(void* vectorizer, void* model, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len, uint64_t nr_doc,
                                    void* hip_stream) {
    return guarded_value((void*)nullptr, [&] {
        return tfidf_model_text_to_queries("xrl_tfidf_predict_device_text: ", vectorizer, model, d_text, d_doc_off, d_doc_len, nr_doc, nullptr, true, hip_stream);
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
    for (size_t b = 0; b < params.size(); ++b) set_base_params(V.base[b], params[b]);
    uint64_t first_bad[2];
    tfidf_train_device(V.base, params, d_text, d_doc_off, d_doc_len, h_doc_off, h_doc_len, nr_doc, s, h->train_forms, first_bad);
    if (first_bad[0] != ~0ull) fail(w + "the string is not utf-8 encoded! (document " + std::to_string(first_bad[0]) + ")");
    if (first_bad[1] != ~0ull)
        fail(w + "document " + std::to_string(first_bad[1]) + " holds a UTF-8 lead byte followed by too few continuation bytes, which the reference's "
             "sequential decode reads along another path: not served by device training");
    V.finish(w);
    return h.release();
}

void* xrl_tfidf_train(void* corpus_ptr, const size_t* doc_lens, size_t nr_doc, const TfidfVectorizerParam* param, int threads) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const std::string w = "xrl_tfidf_train: ";
        if (!corpus_ptr || !doc_lens) fail(w + "null corpus");
        check_train_args(w, param, nr_doc);
        require_gpu();
        use_device(g_device);
        PinnedStage stage;                                       // (there is no handle yet: a staging of the call's own)
        const PackedCorpus P = pack_corpus(stage, static_cast<const char* const*>(corpus_ptr), doc_lens, nr_doc, threads);
        hipStream_t s = nullptr;
        XRL_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        struct Drop { hipStream_t s; ~Drop() { (void)hipStreamDestroy(s); } } drop{s};
        const DevBuf d_in = P.upload(s);
        const uint64_t* d_off = d_in.as<uint64_t>();
        return train_handle(w, param, d_in.as<uint8_t>() + P.head, d_off, d_off + nr_doc, P.off(), P.len(), nr_doc, s);
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
        static_cast<TfidfHandle*>(vectorizer)->v.save(model_dir);
    });
}

void* xrl_tfidf_transform_device(void* vectorizer, int device, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len, uint64_t nr_doc,
                                 uint32_t* d_status, void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        check_device_text_args("xrl_tfidf_transform_device: ", vectorizer, false, d_text, d_doc_off, d_doc_len, nr_doc);
        require_gpu();
        const TfidfHandle& H = *static_cast<TfidfHandle*>(vectorizer);
        const StagedStream on(H, device, hip_stream, nullptr);   // (no model: the caller's stream or the pooled one)
        return tfidf_text_to_queries(H, d_text, d_doc_off, d_doc_len, nullptr, nr_doc, d_status, true, device, on.s).release();
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
        B.enumerate(tokens, flat, off, ids);
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
        CsrArrays out;
        // the allocator's arrays ARE the destination: the worker threads fill (and first-touch) them in parallel
        V.count_corpus(static_cast<const char* const*>(corpus_ptr), doc_lens, nr_doc, threads, seg_ptr, [&](uint64_t n, uint32_t*& c, float*& v) {
            out = alloc_csr(alloc, nr_doc, V.nr_features, n);
            c = out.indices; v = out.data;
        });
        std::memcpy(out.indptr, row_ptr_of(seg_ptr, V.base.size(), nr_doc).data(), (nr_doc + 1) * 8);
    });
}

}  // extern "C"
