// HNSW graph construction (K19, xrl_hnsw_train.hip) behind the C ABI: training from host matrices and from arrays in HBM, the writer of the
// reference's folder (any HnswIndex handle, trained or loaded), the level plan and the counters the tests read.  Every argument is checked before
// a GPU is required; the items are checked on the device by the kernels that check K17's queries.
#include <sys/stat.h>

#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstring>
#include <memory>

#include "xrl_abi_common.h"
#include "xrl_ann_device.h"
#include "xrl_hnsw_train.h"

using namespace xrl;

namespace {

std::atomic<uint64_t> g_ctr[6];   // HnswTrainCounters, in its order

const char* const kTypes[4] = {
    "pecos::ann::HNSW<float, pecos::ann::FeatVecSparseIPSimd<uint32_t, float>>", "pecos::ann::HNSW<float, pecos::ann::FeatVecSparseL2Simd<uint32_t, float>>",
    "pecos::ann::HNSW<float, pecos::ann::FeatVecDenseIPSimd<float>>", "pecos::ann::HNSW<float, pecos::ann::FeatVecDenseL2Simd<float>>"};

// what every training entry point refuses alike, before a GPU is required -> l2
int check_params(const std::string& what, uint32_t rows, uint32_t M, uint32_t efC, const char* metric) {
    if (!metric) fail(what + "null argument (metric)");
    const std::string m = metric;
    if (m != "ip" && m != "l2") fail(what + "metric = " + m + " is not implemented (ip, l2)");
    if (M < 2) fail(what + "M = " + std::to_string(M) + " is below 2 (1 / log(M) is not finite at 1)");
    if (M > kHnswTrainMaxM) fail(what + "M = " + std::to_string(M) + " is above " + std::to_string(kHnswTrainMaxM) + " (maxM0 = 2 M above the " + std::to_string(kHnswLdsDegree) + " neighbours staged in LDS)");
    if (efC == 0) fail(what + "efC == 0");
    if (efC > kHnswCap) fail(what + "efC = " + std::to_string(efC) + " is above CAP = " + std::to_string(kHnswCap));
    if (rows == 0) fail(what + "X has no rows");
    return m == "l2";
}

std::unique_ptr<HnswIndex> new_index(int device, uint32_t rows, uint32_t cols, bool dense, int l2, uint32_t M, uint32_t efC) {
    auto ix = std::make_unique<HnswIndex>();
    ix->device = device; ix->efC = efC;
    ix->d.num_node = rows; ix->d.feat_dim = cols; ix->d.maxM = M; ix->d.maxM0 = 2 * M; ix->d.dense = dense; ix->d.l2 = l2;
    return ix;
}

// the items are in ix's buffers: check them on the device, plan the levels, build the graph
void* finish(const std::string& what, std::unique_ptr<HnswIndex> ix, uint64_t nnz, int max_level_upper_bound, hipStream_t s) {
    HnswDev& d = ix->d;
    QueriesDev X{};
    if (d.dense) { d.feat = ix->feat.as<float>(); X = dense_view(d.num_node, d.feat_dim, d.feat); ix->bytes = 4ull * d.num_node * d.feat_dim; }
    else {
        d.row_ptr = ix->row_ptr.as<uint64_t>(); d.idx = ix->idx.as<uint32_t>(); d.val = ix->val.as<float>();
        X = csr_view(d.num_node, d.feat_dim, d.row_ptr, d.idx, d.val, nnz);
        ix->bytes = 8ull * (d.num_node + 1ull) + 8ull * nnz;
    }
    const uint32_t f = hnsw_check_items(X, d.feat_dim, s);
    if (f & kBadPtr) fail(what + "the row pointers of X are not ascending within its stored entries");
    if (f & kBadRange) fail(what + "a row of X has a column id at or above feat_dim = " + std::to_string(d.feat_dim));
    if (f & kBadOrder) fail(what + "a row of X has unsorted or repeated column ids");
    if (f & kBadValue) fail(what + "a value of X is not finite");
    HnswTrainCounters c;
    hnsw_train(*ix, hnsw_level_plan(d.num_node, d.maxM, max_level_upper_bound), s, c);
    g_ctr[0] += c.dist_search; g_ctr[1] += c.dist_select; g_ctr[2] += c.dist_reverse; g_ctr[3] += c.rewritten; g_ctr[4] += c.sort_rank; g_ctr[5] += c.sort_replay;
    return ix.release();
}

int train_host(const char* name, const HostX& x, uint32_t M, uint32_t efC, int max_level_upper_bound, const char* metric, int device, void** handle) {
    return guarded_value(-1, [&] {
        const std::string what = std::string(name) + ": ";
        if (!handle) fail(what + "null argument (handle)");
        *handle = nullptr;
        if (!x.given) fail(what + "null X");
        const int l2 = check_params(what, x.rows, M, efC, metric);
        if (x.csr && !x.row_ptr) fail(what + "null argument (X's row pointer)");
        const uint64_t n = x.elems();
        if (n && (!x.val || (x.csr && !x.col_idx))) fail(what + "null argument (the stored entries of X)");
        require_gpu();
        use_device(device);
        auto ix = new_index(device, x.rows, x.cols, !x.csr, l2, M, efC);
        if (x.csr) { ix->row_ptr.upload_raw(x.row_ptr, ((size_t)x.rows + 1) * 8); ix->idx.upload_raw(x.col_idx, n * 4); ix->val.upload_raw(x.val, n * 4); }
        else ix->feat.upload_raw(x.val, n * 4);
        *handle = finish(what, std::move(ix), x.csr ? n : 0, max_level_upper_bound, nullptr);
        return 0;
    });
}

// the reference's MmapStore writer: every block at the next multiple of 16, then the block table and the 16-byte signature
struct StoreWriter {
    FILE* fp;
    std::vector<std::pair<uint64_t, uint64_t>> blocks;
    uint64_t at = 0;
    void put(const void* src, uint64_t bytes) {
        static const char zeros[16] = {0};
        const uint64_t pad = (16 - at % 16) % 16;
        if (pad && std::fwrite(zeros, 1, pad, fp) != pad) fail("xrl_hnsw_save: write failed");
        at += pad;
        blocks.emplace_back(at, bytes);
        if (bytes && std::fwrite(src, 1, bytes, fp) != bytes) fail("xrl_hnsw_save: write failed");
        at += bytes;
    }
    void u32(uint32_t v) { put(&v, 4); }
    template <class T> void vec(const std::vector<T>& v) { const uint64_t n = v.size(); put(&n, 8); put(v.data(), n * sizeof(T)); }
    void finish() {
        const uint64_t meta = at, nb = blocks.size();
        const uint8_t sig[8] = {0x93u, 'P', 'E', 'C', 'O', 'S', (uint8_t)'<', 1};
        bool ok = std::fwrite(&nb, 8, 1, fp) == 1;
        for (const auto& b : blocks) ok = ok && std::fwrite(&b.first, 8, 1, fp) == 1 && std::fwrite(&b.second, 8, 1, fp) == 1;
        ok = ok && std::fwrite(sig, 1, 8, fp) == 8 && std::fwrite(&meta, 8, 1, fp) == 1;
        if (!ok) fail("xrl_hnsw_save: write failed");
    }
};

template <class T> std::vector<T> download(const void* p, uint64_t n) {
    std::vector<T> v(n);
    if (n) XRL_HIP(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
}

}  // namespace

extern "C" {

int xrl_hnsw_train_csr_f32(const ScipyCsrF32* pX, uint32_t M, uint32_t efC, int32_t threads, int32_t max_level_upper_bound, const char* metric, int device, void** handle) {
    (void)threads;
    return train_host("xrl_hnsw_train_csr_f32", HostX(pX), M, efC, max_level_upper_bound, metric, device, handle);
}

int xrl_hnsw_train_drm_f32(const ScipyDrmF32* pX, uint32_t M, uint32_t efC, int32_t threads, int32_t max_level_upper_bound, const char* metric, int device, void** handle) {
    (void)threads;
    return train_host("xrl_hnsw_train_drm_f32", HostX(pX), M, efC, max_level_upper_bound, metric, device, handle);
}

int xrl_hnsw_train_device(int device, uint32_t rows, uint32_t cols, const float* d_val, uint64_t row_stride, const uint64_t* d_row_ptr, const uint32_t* d_col_idx, uint64_t nnz,
                          void* smat, uint32_t M, uint32_t efC, int32_t threads, int32_t max_level_upper_bound, const char* metric, void* hip_stream, void** handle) {
    (void)threads;
    return guarded_value(-1, [&] {
        const std::string what = "xrl_hnsw_train_device: ";
        if (!handle) fail(what + "null argument (handle)");
        *handle = nullptr;
        if (smat) {                                                    // an xrl_smat handle stands for the CSR arrays
            const Queries& m = csr_handle(what, smat, "X");
            if (m.device != device) fail(what + "X is on device " + std::to_string(m.device) + ", not " + std::to_string(device));
            rows = m.dev.rows; cols = m.dev.cols; d_row_ptr = m.dev.row_ptr; d_col_idx = m.dev.col_idx; d_val = m.dev.val; nnz = m.dev.nnz;
        }
        const bool csr = d_row_ptr != nullptr;
        const int l2 = check_params(what, rows, M, efC, metric);
        if (!csr && row_stride < cols) fail(what + "row_stride = " + std::to_string(row_stride) + " is below feat_dim = " + std::to_string(cols));
        if (csr ? (nnz && (!d_col_idx || !d_val)) : (cols && !d_val)) fail(what + "null argument (the items)");
        require_gpu();
        use_device(device);
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        auto ix = new_index(device, rows, cols, !csr, l2, M, efC);
        if (csr) {                                                     // device to device, into the index's own arrays
            ix->row_ptr.reserve(((size_t)rows + 1) * 8); ix->idx.reserve(nnz * 4); ix->val.reserve(nnz * 4);
            XRL_HIP(hipMemcpyAsync(ix->row_ptr.p, d_row_ptr, ((size_t)rows + 1) * 8, hipMemcpyDeviceToDevice, s));
            if (nnz) {
                XRL_HIP(hipMemcpyAsync(ix->idx.p, d_col_idx, nnz * 4, hipMemcpyDeviceToDevice, s));
                XRL_HIP(hipMemcpyAsync(ix->val.p, d_val, nnz * 4, hipMemcpyDeviceToDevice, s));
            }
        } else {
            ix->feat.reserve((size_t)rows * cols * 4);
            if (cols) XRL_HIP(hipMemcpy2DAsync(ix->feat.p, (size_t)cols * 4, d_val, row_stride * 4, (size_t)cols * 4, rows, hipMemcpyDeviceToDevice, s));
        }
        *handle = finish(what, std::move(ix), csr ? nnz : 0, max_level_upper_bound, s);
        return 0;
    });
}

int xrl_hnsw_save(void* handle, const char* model_dir) {
    return guarded_value(-1, [&] {
        const std::string what = "xrl_hnsw_save: ";
        if (!handle) fail(what + "null index handle");
        if (!model_dir) fail(what + "null argument");
        const HnswIndex& ix = *static_cast<const HnswIndex*>(handle);
        const HnswDev& d = ix.d;
        const std::string dir = model_dir;
        if (::mkdir(dir.c_str(), 0777) == -1 && errno != EEXIST) fail(what + "Unable to create save folder at " + dir);
        // config.json as nlohmann::json::dump(4) prints it: the keys in ascending order, no final newline
        const std::string cfg = std::string("{\n    \"hnsw_t\": \"") + kTypes[(d.dense ? 2 : 0) + (d.l2 ? 1 : 0)] + "\",\n    \"train_params\": {\n        \"efC\": " + std::to_string(ix.efC) +
                                ",\n        \"init_node\": " + std::to_string(d.init_node) + ",\n        \"maxM\": " + std::to_string(d.maxM) + ",\n        \"maxM0\": " +
                                std::to_string(d.maxM0) + ",\n        \"max_level\": " + std::to_string(d.max_level) + ",\n        \"num_node\": " + std::to_string(d.num_node) +
                                "\n    },\n    \"version\": \"v2.0\"\n}";
        FILE* fc = std::fopen((dir + "/config.json").c_str(), "wb");
        if (!fc) fail(what + "Unable to save config file to " + dir + "/config.json");
        const bool ok = std::fwrite(cfg.data(), 1, cfg.size(), fc) == cfg.size();
        if (std::fclose(fc) != 0 || !ok) fail(what + "write failed");
        use_device(ix.device);
        const uint32_t N = d.num_node, L = d.l1_levels;
        const auto l0_deg = download<uint32_t>(d.l0_deg, N), l0_nbr = download<uint32_t>(d.l0_nbr, (uint64_t)N * d.maxM0);
        const auto l1_deg = download<uint32_t>(d.l1_deg, (uint64_t)N * L), l1_nbr = download<uint32_t>(d.l1_nbr, (uint64_t)N * L * d.maxM);
        std::vector<float> feat, val;
        std::vector<uint64_t> row_ptr;
        std::vector<uint32_t> idx;
        if (d.dense) feat = download<float>(d.feat, (uint64_t)N * d.feat_dim);
        else {
            row_ptr = download<uint64_t>(d.row_ptr, (uint64_t)N + 1);
            idx = download<uint32_t>(d.idx, row_ptr[N]); val = download<float>(d.val, row_ptr[N]);
        }
        // graph_l0's records: degree, maxM0 ids, the item (its length, its values, a sparse item's ids)
        const uint64_t hood = 4ull * (1ull + d.maxM0);
        std::vector<uint64_t> start((size_t)N + 1, 0);
        for (uint32_t i = 0; i < N; ++i) start[i + 1] = start[i] + hood + 4 + (d.dense ? 4ull * d.feat_dim : 8ull * (row_ptr[i + 1] - row_ptr[i]));
        std::vector<char> buf(start[N], 0);
        for (uint32_t i = 0; i < N; ++i) {
            char* rec = buf.data() + start[i];
            std::memcpy(rec, &l0_deg[i], 4);
            std::memcpy(rec + 4, &l0_nbr[(size_t)i * d.maxM0], 4ull * d.maxM0);
            const uint32_t len = d.dense ? d.feat_dim : (uint32_t)(row_ptr[i + 1] - row_ptr[i]);
            std::memcpy(rec + hood, &len, 4);
            if (d.dense) std::memcpy(rec + hood + 4, feat.data() + (size_t)i * d.feat_dim, 4ull * len);
            else if (len) { std::memcpy(rec + hood + 4, &val[row_ptr[i]], 4ull * len); std::memcpy(rec + hood + 4 + 4ull * len, &idx[row_ptr[i]], 4ull * len); }
        }
        std::vector<uint32_t> b1((size_t)N * L * (1ull + d.maxM), 0);    // graph_l1: per node and level, degree then maxM ids
        for (uint64_t r = 0; r < (uint64_t)N * L; ++r) {
            b1[r * (1ull + d.maxM)] = l1_deg[r];
            std::memcpy(&b1[r * (1ull + d.maxM) + 1], &l1_nbr[r * d.maxM], 4ull * d.maxM);
        }
        FILE* fp = std::fopen((dir + "/index.mmap_store").c_str(), "wb");
        if (!fp) fail(what + "cannot open " + dir + "/index.mmap_store");
        struct Close { FILE* f; ~Close() { if (f) std::fclose(f); } } close{fp};
        StoreWriter w{fp};
        w.u32(N); w.u32(d.maxM); w.u32(d.maxM0); w.u32(ix.efC); w.u32(d.max_level); w.u32(d.init_node);
        w.u32(N); w.u32(d.feat_dim); w.u32(d.maxM0); w.u32(d.dense ? (uint32_t)(start[N] / N) : 0u);   // (node_mem_size is set for fixed-size items only)
        w.vec(start); w.vec(buf);
        w.u32(N); w.u32(L); w.u32(d.maxM); w.u32(L * (1u + d.maxM)); w.u32(1u + d.maxM);
        w.vec(b1);
        w.finish();
        close.f = nullptr;
        if (std::fclose(fp) != 0) fail(what + "write failed");
        return 0;
    });
}

int xrl_debug_hnsw_levels(uint32_t n, uint32_t M, int32_t max_level_upper_bound, uint32_t* out) {
    return guarded_value(-1, [&] {
        const std::string what = "xrl_debug_hnsw_levels: ";
        if (!out && n) fail(what + "null argument");
        if (M < 2) fail(what + "M = " + std::to_string(M) + " is below 2 (1 / log(M) is not finite at 1)");
        const auto level = hnsw_level_plan(n, M, max_level_upper_bound);
        if (n) std::memcpy(out, level.data(), (size_t)n * 4);
        return 0;
    });
}

int xrl_debug_hnsw_train_counters(uint64_t* out, uint32_t n, int reset) {
    return guarded_value(-1, [&] {
        if (!out && n) fail("xrl_debug_hnsw_train_counters: null argument");
        for (uint32_t i = 0; i < n && i < 6; ++i) out[i] = g_ctr[i].load();
        if (reset) for (auto& v : g_ctr) v = 0;
        return 0;
    });
}

}  // extern "C"
