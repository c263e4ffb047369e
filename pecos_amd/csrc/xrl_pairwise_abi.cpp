// PairwiseANN (K18, xrl_pairwise.hip) behind the C ABI: the builds from host matrices, from arrays in HBM and from a folder saved by the reference's
// PairwiseANN.save, the writer of that folder, the searchers, the host entry points with the reference's argument list, the resident form and the
// counters the tests read.  Every argument is checked before a GPU is required; what the kernel later uses as an address is checked by the build.
#include <sys/stat.h>

#include <atomic>
#include <cerrno>
#include <cstring>
#include <memory>

#include "xrl_abi_common.h"
#include "xrl_ann_device.h"
#include "xrl_io.h"
#include "xrl_mmap.h"
#include "xrl_pairwise.h"

using namespace xrl;

namespace {

std::atomic<uint64_t> g_ctr[6];   // pairs by the sorted, the stream and the replay form, distance evaluations, second passes, the longest column met

const char* const kTypes[2] = {"pecos::ann::PairwiseANN<pecos::ann::FeatVecSparseIPSimd<uint32_t, float>, pecos::csr_t>",
                               "pecos::ann::PairwiseANN<pecos::ann::FeatVecDenseIPSimd<float>, pecos::drm_t>"};

// X_trn and Y_csc in host memory, not owned
struct HostPair {
    uint32_t rows = 0, labels = 0, feat_dim = 0;
    bool dense = false;
    const uint64_t* y_ptr = nullptr; const uint32_t* y_idx = nullptr; const float* y_val = nullptr; uint64_t nnz_y = 0;
    const uint64_t* x_ptr = nullptr; const uint32_t* x_idx = nullptr; const float* x_val = nullptr; uint64_t nnz_x = 0;   // dense: nnz_x = rows * feat_dim
};

PairIndex& as_index(const std::string& what, void* h) {
    if (!h) fail(what + "null index handle");
    return *static_cast<PairIndex*>(h);
}

bool finite_bits(float v) { uint32_t b; std::memcpy(&b, &v, 4); return (b & 0x7F800000u) != 0x7F800000u; }

// the build's checks on the host (the reader's: a folder is refused without a GPU), the flags of pairwise_check_index
uint32_t host_flags(const HostPair& m) {
    uint32_t f = 0;
    for (uint32_t c = 0; c < m.labels; ++c)
        if (m.y_ptr[c] > m.y_ptr[c + 1] || m.y_ptr[c + 1] > m.nnz_y || m.y_ptr[c + 1] - m.y_ptr[c] >= 0xFFFFFFFFull) f |= kPairBadYPtr;
    for (uint64_t p = 0; p < m.nnz_y; ++p) if (m.y_idx[p] >= m.rows) f |= kPairBadYRow;
    for (uint64_t p = 0; p < m.nnz_x; ++p) if (!finite_bits(m.x_val[p])) f |= kBadValue;
    for (uint32_t r = 0; !m.dense && r < m.rows; ++r) {
        const uint64_t b = m.x_ptr[r], e = m.x_ptr[r + 1];
        if (b > e || e > m.nnz_x) { f |= kBadPtr; continue; }
        for (uint64_t p = b; p < e; ++p) {
            if (m.x_idx[p] >= m.feat_dim) f |= kBadRange;
            if (p > b && m.x_idx[p] <= m.x_idx[p - 1]) f |= kBadOrder;
        }
    }
    return f;
}

void set_pointers(PairIndex& ix) {
    PairDev& d = ix.d;
    d.y_ptr = ix.y_ptr.as<uint64_t>(); d.y_idx = ix.y_idx.as<uint32_t>(); d.y_val = ix.y_val.as<float>();
    d.feat = ix.feat.as<float>(); d.row_ptr = ix.row_ptr.as<uint64_t>(); d.idx = ix.idx.as<uint32_t>(); d.val = ix.val.as<float>();
}

void check_built(const std::string& what, PairIndex& ix, hipStream_t s) {
    set_pointers(ix);
    if (const uint32_t f = pairwise_check_index(ix, s)) fail(pairwise_refusal(what, f, ix, "X_trn"));
}

std::unique_ptr<PairIndex> build_host(const std::string& what, const HostPair& m, int device) {
    require_gpu();
    use_device(device);
    auto ix = std::make_unique<PairIndex>();
    ix->device = device;
    ix->d.num_input = m.rows; ix->d.num_label = m.labels; ix->d.feat_dim = m.feat_dim; ix->d.dense = m.dense ? 1 : 0;
    ix->nnz_y = m.nnz_y; ix->nnz_x = m.nnz_x;
    ix->y_ptr.upload_raw(m.y_ptr, ((size_t)m.labels + 1) * 8); ix->y_idx.upload_raw(m.y_idx, m.nnz_y * 4); ix->y_val.upload_raw(m.y_val, m.nnz_y * 4);
    if (m.dense) ix->feat.upload_raw(m.x_val, m.nnz_x * 4);
    else { ix->row_ptr.upload_raw(m.x_ptr, ((size_t)m.rows + 1) * 8); ix->idx.upload_raw(m.x_idx, m.nnz_x * 4); ix->val.upload_raw(m.x_val, m.nnz_x * 4); }
    check_built(what, *ix, nullptr);
    return ix;
}

int train_host(const char* name, const HostX& x, const ScipyCscF32* pY, int device, void** handle) {
    return guarded_value(-1, [&] {
        const std::string what = std::string(name) + ": ";
        if (!handle) fail(what + "null argument (handle)");
        *handle = nullptr;
        if (!x.given || !pY) fail(what + "null argument (pX / pY)");
        if (x.rows != pY->rows) fail(what + "X_trn.rows != Y_csc.rows");
        if (!pY->col_ptr || (x.csr && !x.row_ptr)) fail(what + "null argument (a pointer array)");
        HostPair m;
        m.rows = x.rows; m.labels = pY->cols; m.feat_dim = x.cols; m.dense = !x.csr;
        m.y_ptr = pY->col_ptr; m.y_idx = pY->row_idx; m.y_val = pY->val; m.nnz_y = pY->col_ptr[pY->cols];
        m.x_ptr = x.row_ptr; m.x_idx = x.col_idx; m.x_val = x.val; m.nnz_x = x.elems();
        if ((m.nnz_y && (!m.y_idx || !m.y_val)) || (m.nnz_x && (!m.x_val || (x.csr && !m.x_idx)))) fail(what + "null argument (the stored entries)");
        *handle = build_host(what, m, device).release();
        return 0;
    });
}

// ---- the folder
struct Folder {
    HostPair m;
    std::unique_ptr<MmapReader> store;        // owns what m points into
};

void read_folder(const std::string& what, const std::string& dir, Folder& out) {
    const std::string cfg_path = dir + "/config.json";
    if (!file_exists(cfg_path)) fail(what + "Unable to open config file at " + cfg_path);
    const JsonValue cfg = parse_json_file(cfg_path);
    const JsonValue* t = cfg.get("pairwise_ann_t");
    const std::string type = t && t->type == JsonValue::STRING ? t->str : "not found";
    int kind = -1;
    for (int k = 0; k < 2; ++k) if (type == kTypes[k]) kind = k;
    if (kind < 0) fail(what + "Inconsistent PairwiseANN_T: cur = pecos::ann::PairwiseANN<FeatVec{Sparse,Dense}IPSimd, pecos::{csr,drm}_t> inp = " + type);
    const JsonValue* v = cfg.get("version");
    const std::string version = v && v->type == JsonValue::STRING ? v->str : "not found";
    if (version != "v1.0") fail(what + "Unable to load memory-mapped file with version = " + version);
    out.store = std::make_unique<MmapReader>(dir + "/index.mmap_store");
    MmapReader& r = *out.store;
    HostPair& m = out.m;
    m.dense = kind == 1;
    m.rows = r.one<uint32_t>(); m.labels = r.one<uint32_t>(); m.feat_dim = r.one<uint32_t>();
    const uint32_t y_rows = r.one<uint32_t>(), y_cols = r.one<uint32_t>();
    m.nnz_y = r.one<uint64_t>();
    m.y_ptr = r.many<uint64_t>((uint64_t)y_cols + 1); m.y_idx = r.many<uint32_t>(m.nnz_y); m.y_val = r.many<float>(m.nnz_y);
    const uint32_t x_rows = r.one<uint32_t>(), x_cols = r.one<uint32_t>();
    m.nnz_x = r.one<uint64_t>();
    if (!m.dense) { m.x_ptr = r.many<uint64_t>((uint64_t)x_rows + 1); m.x_idx = r.many<uint32_t>(m.nnz_x); }
    m.x_val = r.many<float>(m.nnz_x);
    if (y_rows != m.rows || y_cols != m.labels) fail(what + "Y_csc's shape differs from num_input_keys x num_label_keys");
    if (x_rows != y_rows) fail(what + "X_trn.rows != Y_csc.rows");
    if (x_cols != m.feat_dim) fail(what + "X_trn's columns differ from feat_dim");
    if (m.dense && m.nnz_x != (uint64_t)x_rows * x_cols) fail(what + "the dense X_trn does not hold rows * cols values");
    if (m.y_ptr[m.labels] != m.nnz_y || (!m.dense && m.x_ptr[m.rows] != m.nnz_x)) fail(what + "a pointer array does not end at its matrix's stored entries");
    PairIndex shape;
    shape.d.num_input = m.rows; shape.d.num_label = m.labels; shape.d.feat_dim = m.feat_dim;
    if (const uint32_t f = host_flags(m)) fail(pairwise_refusal(what, f, shape, "X_trn"));
}

// the reference's MmapStore writer: every block at the next multiple of 16, then the block table and the 16-byte signature
struct StoreWriter {
    FILE* fp;
    std::vector<std::pair<uint64_t, uint64_t>> blocks;
    uint64_t at = 0;
    void put(const void* src, uint64_t bytes) {
        static const char zeros[16] = {0};
        const uint64_t pad = (16 - at % 16) % 16;
        if (pad && std::fwrite(zeros, 1, pad, fp) != pad) fail("xrl_pairwise_save: write failed");
        at += pad;
        blocks.emplace_back(at, bytes);
        if (bytes && std::fwrite(src, 1, bytes, fp) != bytes) fail("xrl_pairwise_save: write failed");
        at += bytes;
    }
    template <class T> void one(T v) { put(&v, sizeof(T)); }
    template <class T> void many(const std::vector<T>& v, uint64_t n) { put(v.data(), n * sizeof(T)); }
    void finish() {
        const uint64_t meta = at, nb = blocks.size();
        const uint8_t sig[8] = {0x93u, 'P', 'E', 'C', 'O', 'S', (uint8_t)'<', 1};
        bool ok = std::fwrite(&nb, 8, 1, fp) == 1;
        for (const auto& b : blocks) ok = ok && std::fwrite(&b.first, 8, 1, fp) == 1 && std::fwrite(&b.second, 8, 1, fp) == 1;
        ok = ok && std::fwrite(sig, 1, 8, fp) == 8 && std::fwrite(&meta, 8, 1, fp) == 1;
        if (!ok) fail("xrl_pairwise_save: write failed");
    }
};

template <class T> std::vector<T> download(const DevBuf& b, uint64_t n) {
    std::vector<T> v(n);
    if (n) XRL_HIP(hipMemcpy(v.data(), b.p, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
}

void note(const PairCounters& c) {
    g_ctr[0] += c.sorted; g_ctr[1] += c.stream; g_ctr[2] += c.replay; g_ctr[3] += c.dist; g_ctr[4] += c.second_pass;
    uint64_t seen = g_ctr[5].load();
    while (seen < c.max_col && !g_ctr[5].compare_exchange_weak(seen, c.max_col)) {}
}

// what the two predict forms check alike, before a GPU is required
void check_predict(const std::string& what, const PairIndex& ix, bool csr, uint32_t q_rows, uint32_t q_cols, uint32_t batch_size, bool same_input) {
    if (csr == (ix.d.dense != 0)) fail(what + "the index holds " + (ix.d.dense ? "drm" : "csr") + " rows, the queries are " + (csr ? "csr" : "drm"));
    if (q_cols != ix.d.feat_dim) fail(what + "the queries have " + std::to_string(q_cols) + " columns, the index has feat_dim = " + std::to_string(ix.d.feat_dim));
    if (same_input && batch_size && q_rows == 0) fail(what + "is_same_input needs a first row, the queries have none");
    if (!same_input && q_rows != batch_size) fail(what + "the queries have " + std::to_string(q_rows) + " rows, batch_size = " + std::to_string(batch_size));
}

int predict_host(const char* name, void* handle, void* searchers, uint32_t batch_size, uint32_t only_topk, const HostX& x, const uint32_t* label_keys, uint32_t* Imat,
                 uint32_t* Mmat, float* Dmat, float* Vmat, bool same_input) {
    return guarded_value(-1, [&] {
        const std::string what = std::string(name) + ": ";
        PairIndex& ix = as_index(what, handle);
        if (!x.given) fail(what + "null X");
        check_predict(what, ix, x.csr, x.rows, x.cols, batch_size, same_input);
        if (!batch_size || !only_topk) return 0;
        if (!label_keys || !Imat || !Mmat || !Dmat || !Vmat) fail(what + "null argument (label_keys / Imat / Mmat / Dmat / Vmat)");
        if (x.csr && !x.row_ptr) fail(what + "null argument (X's row pointer)");
        require_gpu();
        use_device(ix.device);
        DevBuf ptr, idx, val, keys, oI, oM, oD, oV;
        QueriesDev Q{};
        upload_x(x, ptr, idx, val, Q);
        const size_t n_out = (size_t)batch_size * only_topk * 4;
        keys.upload_raw(label_keys, (size_t)batch_size * 4);
        oI.upload_raw(Imat, n_out); oM.upload_raw(Mmat, n_out); oD.upload_raw(Dmat, n_out); oV.upload_raw(Vmat, n_out);   // (the cells a pair does not reach keep the caller's values)
        PairCounters c;
        pairwise_search(name, ix, Q, x.cols, keys.as<uint32_t>(), batch_size, only_topk, same_input, oI.as<uint32_t>(), oM.as<uint32_t>(), oD.as<float>(), oV.as<float>(),
                        only_topk, static_cast<PairSearchers*>(searchers), nullptr, c);
        note(c);
        XRL_HIP(hipMemcpy(Imat, oI.p, n_out, hipMemcpyDeviceToHost)); XRL_HIP(hipMemcpy(Mmat, oM.p, n_out, hipMemcpyDeviceToHost));
        XRL_HIP(hipMemcpy(Dmat, oD.p, n_out, hipMemcpyDeviceToHost)); XRL_HIP(hipMemcpy(Vmat, oV.p, n_out, hipMemcpyDeviceToHost));
        return 0;
    });
}

void fill_info(const PairIndex& ix, uint64_t* out, uint32_t n) {
    const uint64_t bytes = 8ull * (ix.d.num_label + 1) + 8 * ix.nnz_y + (ix.d.dense ? 4 * ix.nnz_x : 8ull * (ix.d.num_input + 1) + 8 * ix.nnz_x);
    const uint64_t v[8] = {ix.d.num_input, ix.d.num_label, ix.d.feat_dim, (uint64_t)ix.d.dense, ix.nnz_y, ix.nnz_x, ix.d.max_col, bytes};
    for (uint32_t i = 0; out && i < n && i < 8; ++i) out[i] = v[i];
}

}  // namespace

extern "C" {

int xrl_pairwise_train_csr_f32(const ScipyCsrF32* pX, const ScipyCscF32* pY, int device, void** handle) {
    return train_host("xrl_pairwise_train_csr_f32", HostX(pX), pY, device, handle);
}

int xrl_pairwise_train_drm_f32(const ScipyDrmF32* pX, const ScipyCscF32* pY, int device, void** handle) {
    return train_host("xrl_pairwise_train_drm_f32", HostX(pX), pY, device, handle);
}

int xrl_pairwise_from_device(int device, uint32_t num_input, uint32_t num_label, uint32_t feat_dim, const float* d_x_val, uint64_t x_row_stride, const uint64_t* d_x_row_ptr,
                             const uint32_t* d_x_col_idx, uint64_t x_nnz, const uint64_t* d_yt_row_ptr, const uint32_t* d_yt_col_idx, const float* d_yt_val, uint64_t y_nnz,
                             void* hip_stream, void** handle) {
    return guarded_value(-1, [&] {
        const std::string what = "xrl_pairwise_from_device: ";
        if (!handle) fail(what + "null argument (handle)");
        *handle = nullptr;
        const bool csr = d_x_row_ptr != nullptr;
        if (!d_yt_row_ptr || (y_nnz && (!d_yt_col_idx || !d_yt_val))) fail(what + "null argument (the transpose of Y)");
        if (csr ? (x_nnz && (!d_x_col_idx || !d_x_val)) : ((uint64_t)num_input * feat_dim && !d_x_val)) fail(what + "null argument (X_trn)");
        if (!csr && x_row_stride < feat_dim) fail(what + "x_row_stride = " + std::to_string(x_row_stride) + " is below feat_dim = " + std::to_string(feat_dim));
        require_gpu();
        use_device(device);
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        auto ix = std::make_unique<PairIndex>();
        ix->device = device;
        ix->d.num_input = num_input; ix->d.num_label = num_label; ix->d.feat_dim = feat_dim; ix->d.dense = csr ? 0 : 1;
        ix->nnz_y = y_nnz; ix->nnz_x = csr ? x_nnz : (uint64_t)num_input * feat_dim;
        auto copy = [&](DevBuf& to, const void* from, size_t bytes) {
            to.reserve(bytes);
            if (bytes) XRL_HIP(hipMemcpyAsync(to.p, from, bytes, hipMemcpyDeviceToDevice, s));
        };
        copy(ix->y_ptr, d_yt_row_ptr, ((size_t)num_label + 1) * 8); copy(ix->y_idx, d_yt_col_idx, y_nnz * 4); copy(ix->y_val, d_yt_val, y_nnz * 4);
        if (csr) { copy(ix->row_ptr, d_x_row_ptr, ((size_t)num_input + 1) * 8); copy(ix->idx, d_x_col_idx, x_nnz * 4); copy(ix->val, d_x_val, x_nnz * 4); }
        else {
            ix->feat.reserve(ix->nnz_x * 4);
            if (ix->nnz_x) XRL_HIP(hipMemcpy2DAsync(ix->feat.p, (size_t)feat_dim * 4, d_x_val, x_row_stride * 4, (size_t)feat_dim * 4, num_input, hipMemcpyDeviceToDevice, s));
        }
        check_built(what, *ix, s);
        *handle = ix.release();
        return 0;
    });
}

int xrl_pairwise_load(const char* model_dir, int device, void** handle) {
    return guarded_value(-1, [&] {
        const std::string what = "xrl_pairwise_load: ";
        if (!model_dir || !handle) fail(what + "null argument");
        *handle = nullptr;
        Folder f;
        read_folder(what, model_dir, f);
        *handle = build_host(what, f.m, device).release();
        return 0;
    });
}

int xrl_pairwise_check_folder(const char* model_dir, uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&] {
        const std::string what = "xrl_pairwise_load: ";
        if (!model_dir) fail(what + "null argument");
        Folder f;
        read_folder(what, model_dir, f);
        PairIndex ix;
        ix.d.num_input = f.m.rows; ix.d.num_label = f.m.labels; ix.d.feat_dim = f.m.feat_dim; ix.d.dense = f.m.dense ? 1 : 0;
        ix.nnz_y = f.m.nnz_y; ix.nnz_x = f.m.nnz_x;
        for (uint32_t c = 0; c < f.m.labels; ++c) ix.d.max_col = std::max<uint32_t>(ix.d.max_col, (uint32_t)(f.m.y_ptr[c + 1] - f.m.y_ptr[c]));
        fill_info(ix, out, n);
        return 0;
    });
}

int xrl_pairwise_save(void* handle, const char* model_dir) {
    return guarded_value(-1, [&] {
        const std::string what = "xrl_pairwise_save: ";
        const PairIndex& ix = as_index(what, handle);
        if (!model_dir) fail(what + "null argument");
        const std::string dir = model_dir;
        if (::mkdir(dir.c_str(), 0777) == -1 && errno != EEXIST) fail(what + "Unable to create save folder at " + dir);
        // config.json as nlohmann::json::dump(4) prints it: the keys in ascending order, no final newline
        const std::string cfg = std::string("{\n    \"pairwise_ann_t\": \"") + kTypes[ix.d.dense ? 1 : 0] + "\",\n    \"train_params\": {\n        \"feat_dim\": " +
                                std::to_string(ix.d.feat_dim) + ",\n        \"nnz_of_X\": " + std::to_string(ix.nnz_x) + ",\n        \"nnz_of_Y\": " + std::to_string(ix.nnz_y) +
                                ",\n        \"num_input_keys\": " + std::to_string(ix.d.num_input) + ",\n        \"num_label_keys\": " + std::to_string(ix.d.num_label) +
                                "\n    },\n    \"version\": \"v1.0\"\n}";
        FILE* fc = std::fopen((dir + "/config.json").c_str(), "wb");
        if (!fc) fail(what + "Unable to save config file to " + dir + "/config.json");
        const bool ok = std::fwrite(cfg.data(), 1, cfg.size(), fc) == cfg.size();
        if (std::fclose(fc) != 0 || !ok) fail(what + "write failed");
        use_device(ix.device);
        const auto y_ptr = download<uint64_t>(ix.y_ptr, (uint64_t)ix.d.num_label + 1);
        const auto y_idx = download<uint32_t>(ix.y_idx, ix.nnz_y);
        const auto y_val = download<float>(ix.y_val, ix.nnz_y);
        FILE* fp = std::fopen((dir + "/index.mmap_store").c_str(), "wb");
        if (!fp) fail(what + "cannot open " + dir + "/index.mmap_store");
        struct Close { FILE* f; ~Close() { if (f) std::fclose(f); } } close{fp};
        StoreWriter w{fp};
        w.one<uint32_t>(ix.d.num_input); w.one<uint32_t>(ix.d.num_label); w.one<uint32_t>(ix.d.feat_dim);
        w.one<uint32_t>(ix.d.num_input); w.one<uint32_t>(ix.d.num_label); w.one<uint64_t>(ix.nnz_y);
        w.many(y_ptr, y_ptr.size()); w.many(y_idx, ix.nnz_y); w.many(y_val, ix.nnz_y);
        w.one<uint32_t>(ix.d.num_input); w.one<uint32_t>(ix.d.feat_dim); w.one<uint64_t>(ix.nnz_x);
        if (ix.d.dense) w.many(download<float>(ix.feat, ix.nnz_x), ix.nnz_x);
        else {
            const auto x_ptr = download<uint64_t>(ix.row_ptr, (uint64_t)ix.d.num_input + 1);
            w.many(x_ptr, x_ptr.size()); w.many(download<uint32_t>(ix.idx, ix.nnz_x), ix.nnz_x); w.many(download<float>(ix.val, ix.nnz_x), ix.nnz_x);
        }
        w.finish();
        close.f = nullptr;
        if (std::fclose(fp) != 0) fail(what + "write failed");
        return 0;
    });
}

void xrl_pairwise_destruct(void* handle) {
    guarded([&] {
        PairIndex* ix = static_cast<PairIndex*>(handle);
        if (!ix) return;
        (void)hipSetDevice(ix->device);
        delete ix;
    });
}

int xrl_pairwise_info(void* handle, uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&] {
        const PairIndex& ix = as_index("xrl_pairwise_info: ", handle);
        if (!out) fail("xrl_pairwise_info: null argument");
        fill_info(ix, out, n);
        return 0;
    });
}

void* xrl_pairwise_searchers_create(void* handle, uint32_t num_searcher) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const PairIndex& ix = as_index("xrl_pairwise_searchers_create: ", handle);
        if (num_searcher == 0) fail("xrl_pairwise_searchers_create: num_searcher == 0");
        require_gpu();
        use_device(ix.device);
        auto sc = std::make_unique<PairSearchers>();
        pairwise_searchers_reserve(*sc, ix, std::min(num_searcher, kPairMaxSlots));
        return sc.release();
    });
}

void xrl_pairwise_searchers_destruct(void* searchers) {
    guarded([&] {
        PairSearchers* sc = static_cast<PairSearchers*>(searchers);
        if (!sc) return;
        (void)hipSetDevice(sc->device);
        delete sc;
    });
}

int xrl_pairwise_predict_csr_f32(void* handle, void* searchers, uint32_t batch_size, uint32_t only_topk, const ScipyCsrF32* pQ, const uint32_t* label_keys, uint32_t* Imat,
                                 uint32_t* Mmat, float* Dmat, float* Vmat, int is_same_input) {
    return predict_host("xrl_pairwise_predict_csr_f32", handle, searchers, batch_size, only_topk, HostX(pQ), label_keys, Imat, Mmat, Dmat, Vmat, is_same_input != 0);
}

int xrl_pairwise_predict_drm_f32(void* handle, void* searchers, uint32_t batch_size, uint32_t only_topk, const ScipyDrmF32* pQ, const uint32_t* label_keys, uint32_t* Imat,
                                 uint32_t* Mmat, float* Dmat, float* Vmat, int is_same_input) {
    return predict_host("xrl_pairwise_predict_drm_f32", handle, searchers, batch_size, only_topk, HostX(pQ), label_keys, Imat, Mmat, Dmat, Vmat, is_same_input != 0);
}

int xrl_pairwise_predict_device(void* handle, void* searchers, uint32_t batch_size, uint32_t only_topk, uint32_t q_rows, uint32_t q_cols, const float* d_q_val,
                                uint64_t q_row_stride, const uint64_t* d_q_row_ptr, const uint32_t* d_q_col_idx, uint64_t q_nnz, const uint32_t* d_label_keys, uint32_t* d_Imat,
                                uint32_t* d_Mmat, float* d_Dmat, float* d_Vmat, uint64_t out_stride, int is_same_input, void* hip_stream) {
    return guarded_value(-1, [&] {
        const std::string what = "xrl_pairwise_predict_device: ";
        PairIndex& ix = as_index(what, handle);
        const bool csr = d_q_row_ptr != nullptr;
        check_predict(what, ix, csr, q_rows, q_cols, batch_size, is_same_input != 0);
        if (out_stride < only_topk) fail(what + "out_stride = " + std::to_string(out_stride) + " is below only_topk = " + std::to_string(only_topk));
        if (!csr && q_row_stride < q_cols) fail(what + "q_row_stride = " + std::to_string(q_row_stride) + " is below feat_dim = " + std::to_string(q_cols));
        if (!batch_size || !only_topk) return 0;
        if (!d_label_keys || !d_Imat || !d_Mmat || !d_Dmat || !d_Vmat) fail(what + "null argument (label_keys / Imat / Mmat / Dmat / Vmat)");
        if (csr ? (q_nnz && (!d_q_col_idx || !d_q_val)) : (q_cols && !d_q_val)) fail(what + "null argument (the queries)");
        require_gpu();
        use_device(ix.device);
        const QueriesDev Q = csr ? csr_view(q_rows, q_cols, d_q_row_ptr, d_q_col_idx, d_q_val, q_nnz) : dense_view(q_rows, q_cols, d_q_val);
        PairCounters c;
        pairwise_search("xrl_pairwise_predict_device", ix, Q, q_row_stride, d_label_keys, batch_size, only_topk, is_same_input != 0, d_Imat, d_Mmat, d_Dmat, d_Vmat, out_stride,
                        static_cast<PairSearchers*>(searchers), static_cast<hipStream_t>(hip_stream), c);
        note(c);
        return 0;
    });
}

int xrl_debug_pairwise_counters(uint64_t* out, uint32_t n, int reset) {
    return guarded_value(-1, [&] {
        if (!out && n) fail("xrl_debug_pairwise_counters: null argument");
        for (uint32_t i = 0; i < n && i < 6; ++i) out[i] = g_ctr[i].load();
        if (reset) for (auto& v : g_ctr) v = 0;
        return 0;
    });
}

int xrl_debug_pairwise_caps(uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&] {
        if (!out) fail("xrl_debug_pairwise_caps: null argument");
        const uint64_t v[4] = {kPairCap, kPairKeep, kPairQueryLds, kPairMaxSlots};
        for (uint32_t i = 0; i < n && i < 4; ++i) out[i] = v[i];
        return 0;
    });
}

}  // extern "C"
