// Label clustering (K11, xrl_cluster.hip): c_run_clustering_csr_f32 / c_run_clustering_drm_f32 with the reference's signatures
// (libpecos.cpp:357-370 -> Tree::run_clustering, clustering.hpp:403-503), the resident form xrl_run_clustering_device over an
// xrl_smat_* handle, and the two exports the tests read.  Every argument is checked, and the plan drawn, before a GPU is required.
#include <mutex>

#include "xrl_abi_common.h"
#include "xrl_cluster.h"

using namespace xrl;

namespace {

std::mutex g_forms_mu;
ClusterForms g_forms;                                   // of the last clustering of this process

void keep_forms(const ClusterForms& f) { std::lock_guard<std::mutex> g(g_forms_mu); g_forms = f; }

// upload, run, copy the codes back
void cluster_host(const char* what, const ScipyCsrF32& x, const ClusterPlan& plan, const ClusteringParam* param, uint32_t* label_codes) {
    require_gpu();
    use_device(g_device);
    DevCsr X;
    QueriesDev Xv;
    upload_x(HostX(&x), X.ptr, X.idx, X.val, Xv);
    DevBuf codes;
    codes.reserve((size_t)x.rows * 4);
    ClusterForms forms;
    cluster_device(what, Xv, plan, *param, codes.as<uint32_t>(), nullptr, nullptr, forms);
    keep_forms(forms);
    XRL_HIP(hipMemcpy(label_codes, codes.p, (size_t)x.rows * 4, hipMemcpyDeviceToHost));
}

}  // namespace

extern "C" {

void c_run_clustering_csr_f32(const ScipyCsrF32* X, size_t depth, ClusteringParam* param, uint32_t* label_codes) {
    guarded([&] {
        const char* what = "c_run_clustering_csr_f32";
        if (!X || !X->row_ptr || !param || !label_codes) fail(std::string(what) + ": null argument");
        if (X->rows && X->row_ptr[X->rows] && (!X->col_idx || !X->val)) fail(std::string(what) + ": null indices or values");
        cluster_host(what, *X, make_cluster_plan(what, X->rows, X->cols, X->row_ptr[X->rows], depth, param), param, label_codes);
    });
}

// the same computation on rows that store every entry, zeros included (the reference's drm_t rows are dense vectors, and its
// get_nnz is rows * cols, so the norm order never switches)
void c_run_clustering_drm_f32(const ScipyDrmF32* X, size_t depth, ClusteringParam* param, uint32_t* label_codes) {
    guarded([&] {
        const char* what = "c_run_clustering_drm_f32";
        if (!X || !param || !label_codes) fail(std::string(what) + ": null argument");
        if (X->rows && X->cols && !X->val) fail(std::string(what) + ": null values");
        const uint64_t n = (uint64_t)X->rows * X->cols;
        const ClusterPlan plan = make_cluster_plan(what, X->rows, X->cols, n, depth, param);        // refusals come before the index arrays are built
        std::vector<uint64_t> ptr((size_t)X->rows + 1);
        std::vector<uint32_t> idx((size_t)n);
        for (uint64_t r = 0; r <= X->rows; ++r) ptr[r] = r * X->cols;
        for (uint64_t i = 0; i < n; ++i) idx[i] = (uint32_t)(i % X->cols);
        const ScipyCsrF32 csr{X->rows, X->cols, ptr.data(), idx.data(), X->val};
        cluster_host(what, csr, plan, param, label_codes);
    });
}

int xrl_run_clustering_device(void* smat, uint64_t depth, const ClusteringParam* param, uint32_t* d_codes, float* d_scores, void* hip_stream) {
    return guarded_value(-1, [&] {
        const char* what = "xrl_run_clustering_device";
        if (!smat) fail(std::string(what) + ": null matrix handle");
        if (!param || !d_codes) fail(std::string(what) + ": null argument");
        const Queries& m = *static_cast<Queries*>(smat);
        if (m.dev.dense) fail(std::string(what) + ": the feature matrix must be a CSR handle");
        const ClusterPlan plan = make_cluster_plan(what, m.dev.rows, m.dev.cols, m.dev.nnz, depth, param);
        require_gpu();
        use_device(m.device);
        ClusterForms forms;
        cluster_device(what, m.dev, plan, *param, d_codes, d_scores, static_cast<hipStream_t>(hip_stream), forms);
        keep_forms(forms);
        return 0;
    });
}

int xrl_debug_cluster_plan(uint64_t rows, uint64_t cols, uint64_t nnz, uint64_t depth, const ClusteringParam* param, uint32_t* node_seed, uint32_t* level_info,
                           uint32_t* work, uint32_t* perm) {
    return guarded_value(-1, [&] {
        const ClusterPlan plan = make_cluster_plan("xrl_debug_cluster_plan", rows, cols, nnz, depth, param);
        if (node_seed) std::copy(plan.node_seed.begin(), plan.node_seed.end(), node_seed);
        for (uint32_t d = 0; d < plan.depth; ++d) {
            const ClusterLevel& lv = plan.levels[d];
            if (level_info) { level_info[2 * d] = lv.sampled; level_info[2 * d + 1] = lv.first_touch; }
            for (uint32_t i = 0; work && i < (1u << d); ++i) {
                uint32_t* w = work + 4 * ((size_t)(1u << d) + i);
                w[0] = lv.beg[i]; w[1] = lv.work_end[i];
                w[2] = lv.r_pos.empty() ? 0u : lv.r_pos[i]; w[3] = lv.l_pos.empty() ? 0u : lv.l_pos[i];
            }
            if (perm) {
                if (lv.sampled) std::copy(lv.perm.begin(), lv.perm.end(), perm + (size_t)d * rows);
                else for (uint64_t p = 0; p < rows; ++p) perm[(size_t)d * rows + p] = (uint32_t)p;
            }
        }
        return 0;
    });
}

int xrl_debug_cluster_forms(uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&] {
        if (!out) fail("xrl_debug_cluster_forms: null argument");
        std::lock_guard<std::mutex> g(g_forms_mu);
        std::vector<uint64_t> v{g_forms.lane_runs, g_forms.wave_runs, g_forms.seg_sorts,
                                g_forms.switch_level == kClusterNoSwitch ? ~0ull : (uint64_t)g_forms.switch_level, (uint64_t)g_forms.iters.size()};
        v.insert(v.end(), g_forms.iters.begin(), g_forms.iters.end());
        for (uint32_t i = 0; i < n && i < v.size(); ++i) out[i] = v[i];
        return 0;
    });
}

}  // extern "C"
