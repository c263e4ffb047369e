// HNSW search (K17, xrl_hnsw.hip) behind the C ABI: the loader of a folder saved by the reference's HNSW.save, the searchers, the host
// entry points with the reference's argument list, the resident form and the counters the tests read.  The loader checks on the host everything
// the kernel later uses as an address or relies on (neighbour ids, degrees, a node listed twice, init_node, ascending sparse ids, finite values).
// Every argument is checked before a GPU is required.
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>

#include "xrl_abi_common.h"
#include "xrl_hnsw.h"
#include "xrl_io.h"
#include "xrl_mmap.h"

using namespace xrl;

namespace {

std::atomic<uint64_t> g_ctr[8];   // distance evaluations, pops, admissions, upper-level passes, largest cand size, queries rerun, queries by the LDS form, by the HBM form

const char* const kTypes[4] = {
    "pecos::ann::HNSW<float, pecos::ann::FeatVecSparseIPSimd<uint32_t, float>>", "pecos::ann::HNSW<float, pecos::ann::FeatVecSparseL2Simd<uint32_t, float>>",
    "pecos::ann::HNSW<float, pecos::ann::FeatVecDenseIPSimd<float>>", "pecos::ann::HNSW<float, pecos::ann::FeatVecDenseL2Simd<float>>"};

HnswIndex& as_index(const std::string& what, void* h) {
    if (!h) fail(what + "null index handle");
    return *static_cast<HnswIndex*>(h);
}

bool finite_bits(float v) { uint32_t b; std::memcpy(&b, &v, 4); return (b & 0x7F800000u) != 0x7F800000u; }

// one neighbourhood: degree, then ids; `seen` is a scratch of num_node zeros, left as zeros
void check_neighbourhood(const std::string& what, uint32_t node, uint32_t level, const uint32_t* rec, uint32_t max_degree, uint32_t num_node, std::vector<uint8_t>& seen) {
    const std::string where = "node " + std::to_string(node) + ", level " + std::to_string(level) + ": ";
    const uint32_t deg = rec[0];
    if (deg > max_degree) fail(what + where + "degree " + std::to_string(deg) + " is above " + (level ? "maxM = " : "maxM0 = ") + std::to_string(max_degree));
    std::string bad;
    for (uint32_t j = 0; j < deg && bad.empty(); ++j) {
        const uint32_t nb = rec[1 + j];
        if (nb >= num_node) bad = "neighbour id " + std::to_string(nb) + " is not below num_node = " + std::to_string(num_node);
        else if (seen[nb]) bad = "node " + std::to_string(nb) + " is listed twice in one neighbourhood";
        else seen[nb] = 1;
    }
    for (uint32_t j = 0; j < deg; ++j) if (rec[1 + j] < num_node) seen[rec[1 + j]] = 0;
    if (!bad.empty()) fail(what + where + bad);
}

std::unique_ptr<HnswIndex> load_index(const std::string& dir, int device, bool upload) {
    const std::string what = "xrl_hnsw_load: ";
    const std::string cfg_path = dir + "/config.json";
    if (!file_exists(cfg_path)) fail(what + "Unable to open config file at " + cfg_path);
    const JsonValue cfg = parse_json_file(cfg_path);
    const JsonValue* t = cfg.get("hnsw_t");
    const std::string type = t && t->type == JsonValue::STRING ? t->str : "not found";
    int kind = -1;
    for (int k = 0; k < 4; ++k) if (type == kTypes[k]) kind = k;
    if (kind < 0) fail(what + "Inconsistent HNSW_T: hnsw_t_cur = pecos::ann::HNSW<float, FeatVec{Sparse,Dense}{IP,L2}Simd> hnsw_t_cur = " + type);
    const JsonValue* v = cfg.get("version");
    const std::string version = v && v->type == JsonValue::STRING ? v->str : "not found";
    if (version != "v2.0") fail(what + "Unable to load memory-mapped file with version = " + version);

    auto ix = std::make_unique<HnswIndex>();
    ix->device = device;
    HnswDev& d = ix->d;
    d.dense = kind >= 2; d.l2 = kind & 1;
    MmapReader r(dir + "/index.mmap_store");
    d.num_node = r.one<uint32_t>(); d.maxM = r.one<uint32_t>(); d.maxM0 = r.one<uint32_t>(); ix->efC = r.one<uint32_t>();
    d.max_level = r.one<uint32_t>(); d.init_node = r.one<uint32_t>();
    // graph_l0: num_node, feat_dim, max_degree, node_mem_size, mem_start_of_node, buffer
    const uint32_t n0 = r.one<uint32_t>(); d.feat_dim = r.one<uint32_t>();
    const uint32_t deg0 = r.one<uint32_t>(), node_mem = r.one<uint32_t>();
    uint64_t n_start = 0, n_buf = 0;
    const uint64_t* start = r.vec<uint64_t>(n_start);
    const char* buf = r.vec<char>(n_buf);
    // graph_l1: num_node, max_level, max_degree, node_mem_size, level_mem_size, buffer
    const uint32_t n1 = r.one<uint32_t>(); d.l1_levels = r.one<uint32_t>();
    const uint32_t deg1 = r.one<uint32_t>(), node_mem1 = r.one<uint32_t>(), level_mem1 = r.one<uint32_t>();
    uint64_t n_buf1 = 0;
    const uint32_t* buf1 = r.vec<uint32_t>(n_buf1);

    const uint32_t N = d.num_node;
    if (d.init_node >= N) fail(what + "init_node = " + std::to_string(d.init_node) + " is not below num_node = " + std::to_string(N));
    if (n0 != N || n1 != N) fail(what + "the graphs' num_node differ from the index's");
    if (deg0 != d.maxM0 || (d.l1_levels && deg1 != d.maxM)) fail(what + "the graphs' max_degree differ from maxM0 / maxM");
    if (d.max_level > d.l1_levels) fail(what + "max_level = " + std::to_string(d.max_level) + " is above the " + std::to_string(d.l1_levels) + " stored upper levels");
    if (n_start != (uint64_t)N + 1) fail(what + "mem_start_of_node has " + std::to_string(n_start) + " entries, expected num_node + 1");
    const uint64_t hood = 4ull * (1ull + d.maxM0);
    if (d.dense && ((uint64_t)node_mem != hood + 4 + 4ull * d.feat_dim || n_buf != (uint64_t)N * node_mem)) fail(what + "the dense node records do not have the size of maxM0 and feat_dim");
    if (d.l1_levels && (level_mem1 != 1 + d.maxM || (uint64_t)node_mem1 != (uint64_t)d.l1_levels * level_mem1)) fail(what + "the upper-level records do not have the size of maxM and max_level");
    if (n_buf1 != (uint64_t)N * d.l1_levels * (d.l1_levels ? level_mem1 : 0)) fail(what + "the upper-level buffer does not have num_node records");

    // split the interleaved records (degree, neighbours, feature vector) into arrays
    std::vector<uint8_t> seen(N, 0);
    std::vector<uint32_t> l0_deg(N), l0_nbr((size_t)N * d.maxM0, 0), l1_deg((size_t)N * d.l1_levels), l1_nbr((size_t)N * d.l1_levels * d.maxM, 0);
    std::vector<float> feat;
    std::vector<uint64_t> row_ptr;
    std::vector<uint32_t> idx;
    std::vector<float> val;
    if (d.dense) feat.resize((size_t)N * d.feat_dim);
    else row_ptr.assign((size_t)N + 1, 0);
    for (uint32_t i = 0; i < N; ++i) {
        const uint64_t at = d.dense ? (uint64_t)i * node_mem : start[i];
        // (no sum with a value read from the file before that value is known to lie in the buffer: a crafted start near 2^64 would wrap it)
        if (!d.dense && (at % 4 || at > n_buf || n_buf - at < hood + 4 || start[i + 1] > n_buf || start[i + 1] < at || start[i + 1] - at < hood + 4))
            fail(what + "node " + std::to_string(i) + ": its record leaves the buffer");
        const uint32_t* rec = reinterpret_cast<const uint32_t*>(buf + at);
        check_neighbourhood(what, i, 0, rec, d.maxM0, N, seen);
        l0_deg[i] = rec[0];
        std::memcpy(&l0_nbr[(size_t)i * d.maxM0], rec + 1, 4ull * rec[0]);
        const uint32_t len = rec[1 + d.maxM0];
        const float* fv = reinterpret_cast<const float*>(rec + 2 + d.maxM0);
        if (d.dense) {
            if (len != d.feat_dim) fail(what + "node " + std::to_string(i) + ": a dense item of " + std::to_string(len) + " values, feat_dim = " + std::to_string(d.feat_dim));
        } else if ((start[i + 1] - at - hood - 4) / 8 < len) fail(what + "node " + std::to_string(i) + ": its sparse item leaves its record");
        for (uint32_t k = 0; k < len; ++k)
            if (!finite_bits(fv[k])) fail(what + "node " + std::to_string(i) + ": a stored value is not finite");
        if (d.dense) std::memcpy(&feat[(size_t)i * d.feat_dim], fv, 4ull * len);
        else {
            const uint32_t* fi = reinterpret_cast<const uint32_t*>(fv + len);
            for (uint32_t k = 0; k < len; ++k) {
                if (fi[k] >= d.feat_dim) fail(what + "node " + std::to_string(i) + ": a sparse item's id " + std::to_string(fi[k]) + " reaches feat_dim = " + std::to_string(d.feat_dim));
                if (k && fi[k] <= fi[k - 1]) fail(what + "node " + std::to_string(i) + ": a sparse item's ids are not strictly ascending");
            }
            idx.insert(idx.end(), fi, fi + len); val.insert(val.end(), fv, fv + len);
            row_ptr[i + 1] = idx.size();
        }
        for (uint32_t l = 1; l <= d.l1_levels; ++l) {
            const uint32_t* rec1 = buf1 + (uint64_t)i * node_mem1 + (uint64_t)(l - 1) * level_mem1;
            check_neighbourhood(what, i, l, rec1, d.maxM, N, seen);
            l1_deg[(size_t)i * d.l1_levels + (l - 1)] = rec1[0];
            std::memcpy(&l1_nbr[((size_t)i * d.l1_levels + (l - 1)) * d.maxM], rec1 + 1, 4ull * rec1[0]);
        }
    }
    ix->bytes = 4ull * (l0_deg.size() + l0_nbr.size() + l1_deg.size() + l1_nbr.size() + feat.size() + idx.size() + val.size()) + 8ull * row_ptr.size();
    if (upload) {
        require_gpu();
        use_device(device);
        ix->l0_deg.upload(l0_deg); ix->l0_nbr.upload(l0_nbr); ix->l1_deg.upload(l1_deg); ix->l1_nbr.upload(l1_nbr);
        d.l0_deg = ix->l0_deg.as<uint32_t>(); d.l0_nbr = ix->l0_nbr.as<uint32_t>(); d.l1_deg = ix->l1_deg.as<uint32_t>(); d.l1_nbr = ix->l1_nbr.as<uint32_t>();
        if (d.dense) { ix->feat.upload(feat); d.feat = ix->feat.as<float>(); }
        else {
            ix->row_ptr.upload(row_ptr); ix->idx.upload(idx); ix->val.upload(val);
            d.row_ptr = ix->row_ptr.as<uint64_t>(); d.idx = ix->idx.as<uint32_t>(); d.val = ix->val.as<float>();
        }
    }
    return ix;
}

void note(const HnswCounters& c) {
    g_ctr[0] += c.dist; g_ctr[1] += c.pops; g_ctr[2] += c.admissions; g_ctr[3] += c.passes;
    uint64_t seen = g_ctr[4].load();
    while (seen < c.max_cand && !g_ctr[4].compare_exchange_weak(seen, c.max_cand)) {}
    g_ctr[5] += c.rerun; g_ctr[6] += c.lds_queries; g_ctr[7] += c.hbm_queries;
}

void check_common(const std::string& what, const HnswIndex& ix, bool csr, uint32_t cols, uint32_t efS, uint32_t topk, const void* searchers) {
    if (csr == (ix.d.dense != 0))
        fail(what + "the index holds " + (ix.d.dense ? "drm" : "csr") + " items, the queries are " + (csr ? "csr" : "drm"));
    if (cols != ix.d.feat_dim) fail(what + "X has " + std::to_string(cols) + " columns, the index has feat_dim = " + std::to_string(ix.d.feat_dim));
    if (topk == 0) fail(what + "topk == 0");
    if (efS == 0) fail(what + "efS == 0");
    (void)searchers;
}

int predict_host(const char* name, void* handle, const HostX& x, uint32_t* ret_idx, float* ret_val, uint32_t efS, uint32_t topk, void* searchers) {
    return guarded_value(-1, [&] {
        const std::string what = std::string(name) + ": ";
        HnswIndex& ix = as_index(what, handle);
        if (!x.given) fail(what + "null X");
        check_common(what, ix, x.csr, x.cols, efS, topk, searchers);
        if (x.rows && (!ret_idx || !ret_val)) fail(what + "null argument (ret_idx / ret_val)");
        if (!x.rows) return 0;
        if (x.csr && !x.row_ptr) fail(what + "null argument (X's row pointer)");
        require_gpu();
        use_device(ix.device);
        DevBuf ptr, idx, val, o_idx, o_dist, o_cnt;
        QueriesDev X{};
        upload_x(x, ptr, idx, val, X);
        const size_t n_out = (size_t)x.rows * topk;
        o_idx.reserve(n_out * 4); o_dist.reserve(n_out * 4); o_cnt.reserve((size_t)x.rows * 4);
        HnswCounters c;
        hnsw_search(name, ix, X, x.cols, efS, topk, o_idx.as<uint32_t>(), o_dist.as<float>(), o_cnt.as<uint32_t>(), topk, static_cast<HnswSearchers*>(searchers), nullptr, c);
        note(c);
        std::vector<uint32_t> h_idx(n_out), h_cnt(x.rows);
        std::vector<float> h_dist(n_out);
        XRL_HIP(hipMemcpy(h_idx.data(), o_idx.p, n_out * 4, hipMemcpyDeviceToHost));
        XRL_HIP(hipMemcpy(h_dist.data(), o_dist.p, n_out * 4, hipMemcpyDeviceToHost));
        XRL_HIP(hipMemcpy(h_cnt.data(), o_cnt.p, (size_t)x.rows * 4, hipMemcpyDeviceToHost));
        for (uint32_t r = 0; r < x.rows; ++r) {                        // a row that found fewer than topk items leaves the rest of its row untouched
            const size_t at = (size_t)r * topk, n = std::min(h_cnt[r], topk);
            std::memcpy(ret_idx + at, h_idx.data() + at, n * 4);
            std::memcpy(ret_val + at, h_dist.data() + at, n * 4);
        }
        return 0;
    });
}

}  // namespace

extern "C" {

int xrl_hnsw_load(const char* model_dir, int device, void** handle) {
    return guarded_value(-1, [&] {
        if (!model_dir || !handle) fail("xrl_hnsw_load: null argument");
        *handle = nullptr;
        *handle = load_index(model_dir, device, true).release();
        return 0;
    });
}

int xrl_hnsw_check_folder(const char* model_dir, uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&] {
        if (!model_dir) fail("xrl_hnsw_load: null argument");
        const auto ix = load_index(model_dir, 0, false);
        const uint64_t v[10] = {ix->d.num_node, ix->d.feat_dim, ix->d.maxM, ix->d.maxM0, ix->efC, ix->d.max_level, ix->d.init_node, (uint64_t)ix->d.dense, (uint64_t)ix->d.l2, ix->bytes};
        for (uint32_t i = 0; out && i < n && i < 10; ++i) out[i] = v[i];
        return 0;
    });
}

void xrl_hnsw_destruct(void* handle) {
    guarded([&] {
        HnswIndex* ix = static_cast<HnswIndex*>(handle);
        if (!ix) return;
        (void)hipSetDevice(ix->device);
        delete ix;
    });
}

int xrl_hnsw_info(void* handle, uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&] {
        const HnswIndex& ix = as_index("xrl_hnsw_info: ", handle);
        if (!out) fail("xrl_hnsw_info: null argument");
        const uint64_t v[10] = {ix.d.num_node, ix.d.feat_dim, ix.d.maxM, ix.d.maxM0, ix.efC, ix.d.max_level, ix.d.init_node, (uint64_t)ix.d.dense, (uint64_t)ix.d.l2, ix.bytes};
        for (uint32_t i = 0; i < n && i < 10; ++i) out[i] = v[i];
        return 0;
    });
}

void* xrl_hnsw_searchers_create(void* handle, uint32_t num_searcher) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const HnswIndex& ix = as_index("xrl_hnsw_searchers_create: ", handle);
        if (num_searcher == 0) fail("xrl_hnsw_searchers_create: num_searcher == 0");
        require_gpu();
        use_device(ix.device);
        auto sc = std::make_unique<HnswSearchers>();
        hnsw_searchers_reserve(*sc, ix, std::min(num_searcher, kHnswMaxSlots), nullptr);
        XRL_HIP(hipStreamSynchronize(nullptr));
        return sc.release();
    });
}

void xrl_hnsw_searchers_destruct(void* searchers) {
    guarded([&] {
        HnswSearchers* sc = static_cast<HnswSearchers*>(searchers);
        if (!sc) return;
        (void)hipSetDevice(sc->device);
        delete sc;
    });
}

int xrl_hnsw_predict_csr_f32(void* handle, const ScipyCsrF32* pX, uint32_t* ret_idx, float* ret_val, uint32_t efS, uint32_t topk, int32_t threads, void* searchers) {
    (void)threads;
    return predict_host("xrl_hnsw_predict_csr_f32", handle, HostX(pX), ret_idx, ret_val, efS, topk, searchers);
}

int xrl_hnsw_predict_drm_f32(void* handle, const ScipyDrmF32* pX, uint32_t* ret_idx, float* ret_val, uint32_t efS, uint32_t topk, int32_t threads, void* searchers) {
    (void)threads;
    return predict_host("xrl_hnsw_predict_drm_f32", handle, HostX(pX), ret_idx, ret_val, efS, topk, searchers);
}

int xrl_hnsw_predict_device(void* handle, uint32_t rows, uint32_t cols, const float* d_val, uint64_t row_stride, const uint64_t* d_row_ptr, const uint32_t* d_col_idx,
                            uint64_t nnz, uint32_t efS, uint32_t topk, uint32_t* d_idx, float* d_dist, uint32_t* d_count, uint64_t out_stride, void* searchers,
                            void* hip_stream) {
    return guarded_value(-1, [&] {
        const std::string what = "xrl_hnsw_predict_device: ";
        HnswIndex& ix = as_index(what, handle);
        const bool csr = d_row_ptr != nullptr;
        check_common(what, ix, csr, cols, efS, topk, searchers);
        if (out_stride < topk) fail(what + "out_stride = " + std::to_string(out_stride) + " is below topk = " + std::to_string(topk));
        if (!csr && row_stride < cols) fail(what + "row_stride = " + std::to_string(row_stride) + " is below feat_dim = " + std::to_string(cols));
        if (!rows) return 0;
        if (!d_idx || !d_dist || !d_count) fail(what + "null argument (d_idx / d_dist / d_count)");
        if (csr ? (nnz && (!d_col_idx || !d_val)) : (cols && !d_val)) fail(what + "null argument (the queries)");
        require_gpu();
        use_device(ix.device);
        const QueriesDev X = csr ? csr_view(rows, cols, d_row_ptr, d_col_idx, d_val, nnz) : dense_view(rows, cols, d_val);
        HnswCounters c;
        hnsw_search("xrl_hnsw_predict_device", ix, X, row_stride, efS, topk, d_idx, d_dist, d_count, out_stride, static_cast<HnswSearchers*>(searchers),
                    static_cast<hipStream_t>(hip_stream), c);
        note(c);
        return 0;
    });
}

int xrl_debug_hnsw_counters(uint64_t* out, uint32_t n, int reset) {
    return guarded_value(-1, [&] {
        if (!out && n) fail("xrl_debug_hnsw_counters: null argument");
        for (uint32_t i = 0; i < n && i < 8; ++i) out[i] = g_ctr[i].load();
        if (reset) for (auto& v : g_ctr) v = 0;
        return 0;
    });
}

int xrl_debug_hnsw_caps(uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&] {
        if (!out) fail("xrl_debug_hnsw_caps: null argument");
        const uint64_t v[4] = {kHnswCap, kHnswCandCap, kHnswLdsDegree, kHnswMaxSlots};
        for (uint32_t i = 0; i < n && i < 4; ++i) out[i] = v[i];
        return 0;
    });
}

}  // extern "C"
