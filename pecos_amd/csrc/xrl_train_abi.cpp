// Ranker training (K13, xrl_train.hip): xrl_single_layer_train_csr_f32 / _drm_f32 with the signatures of the reference's
// c_xlinear_single_layer_train_* (libpecos.cpp:277-316 -> multilabel_train_with_codes, linear_solver.hpp:797-860) under this library's own
// prefix -- a binding that takes this library first and the reference for the rest keeps the reference's trainer and all its solvers --,
// the resident form xrl_train_layer_device over xrl_smat_* handles, and the counters the tests read.  Every argument is checked before a
// GPU is required where no data is read.
#include <memory>
#include <mutex>

#include "xrl_abi_common.h"
#include "xrl_newton.h"
#include "xrl_train.h"

using namespace xrl;

namespace {

std::mutex g_counters_mu;
TrainCounters g_counters;                                  // of the last training of this process

NewtonCounters g_newton_counters;                          // of the last primal training of this process

void keep_counters(const TrainCounters& c) { std::lock_guard<std::mutex> g(g_counters_mu); g_counters = c; }
void keep_counters(const NewtonCounters& c) { std::lock_guard<std::mutex> g(g_counters_mu); g_newton_counters = c; }

// the solvers an entry point serves: K13's two dual ones, or (newton) K16's primal one
void check_solver(const std::string& what, const TrainParams& p, bool newton) {
    if (newton) check_newton_params(what, p); else check_train_params(what, p);
}

TrainParams make_params(double threshold, uint32_t max_nonzeros, int solver_type, double Cp, double Cn, uint64_t max_iter, double eps, double bias) {
    TrainParams p;
    p.threshold = threshold; p.max_nonzeros = max_nonzeros; p.solver_type = solver_type; p.Cp = Cp; p.Cn = Cn; p.max_iter = max_iter; p.eps = eps; p.bias = bias;
    return p;
}

void check_csc(const std::string& what, const char* name, const ScipyCscF32* m) {
    if (!m->col_ptr) fail(what + "null column pointer (" + name + ")");
    if (m->cols && m->col_ptr[m->cols] && !m->row_idx) fail(what + "null row indices (" + name + ")");
}

// the CSC arrays of a matrix are the CSR arrays of its transpose
HostX transposed(const ScipyCscF32* m, ScipyCsrF32& hold) {
    hold = ScipyCsrF32{m->cols, m->rows, m->col_ptr, m->row_idx, m->val};
    return HostX(&hold);
}

struct Uploaded { DevCsr own; QueriesDev v{}; };

void upload(const HostX& x, Uploaded& u) { upload_x(x, u.own.ptr, u.own.idx, u.own.val, u.v); u.own.nnz = u.v.nnz; }

// a pattern: the values are never read, so none are sent (Y, C and M may come without any)
void upload_pattern(const ScipyCscF32* m, Uploaded& u) {
    const uint64_t nnz = m->cols ? m->col_ptr[m->cols] : 0;
    u.own.ptr.upload_raw(m->col_ptr, ((size_t)m->cols + 1) * 8);
    u.own.idx.upload_raw(m->row_idx, (size_t)nnz * 4);
    u.own.nnz = nnz;
    u.v = csr_view(m->cols, m->rows, u.own.ptr.as<uint64_t>(), u.own.idx.as<uint32_t>(), nullptr, nnz);
}

// upload, train, copy back as the reference's COO at threads = 1: jobs code-major in C's stored order
void train_host(const char* what_c, const ScipyCsrF32& X, const ScipyCscF32* pY, const ScipyCscF32* pC, const ScipyCscF32* pM, const ScipyCscF32* pR,
                py_coo_allocator_t coo_alloc, const TrainParams& p, bool newton) {
    const std::string what = std::string(what_c) + ": ";
    check_solver(what, p, newton);
    if (!pY) fail(what + "null Y");
    if (!coo_alloc) fail(what + "null allocator");
    check_csc(what, "Y", pY);
    const bool coded = pC && pM;
    if (pY->rows != X.rows) fail(what + "Y.rows != X.rows (" + std::to_string(pY->rows) + " != " + std::to_string(X.rows) + ")");
    if (X.rows >= (1u << 31)) fail(what + "2^31 rows or more");
    if (coded) {
        check_csc(what, "C", pC);
        check_csc(what, "M", pM);
        if (pC->rows != pY->cols) fail(what + "C.rows != Y.cols (" + std::to_string(pC->rows) + " != " + std::to_string(pY->cols) + ")");
        if (pM->rows != X.rows) fail(what + "M.rows != X.rows (" + std::to_string(pM->rows) + " != " + std::to_string(X.rows) + ")");
        if (pM->cols != pC->cols) fail(what + "M.cols != C.cols (" + std::to_string(pM->cols) + " != " + std::to_string(pC->cols) + ")");
        if (pC->col_ptr[pC->cols] >= 0xFFFFFFFFull) fail(what + "2^32 - 1 jobs or more");
        std::vector<uint8_t> seen(pY->cols, 0);
        for (uint64_t x = 0, e = pC->col_ptr[pC->cols]; x < e; ++x) {
            const uint32_t l = pC->row_idx[x];
            if (l >= pY->cols) fail(what + "C holds an id that is not below " + std::to_string(pY->cols));
            if (seen[l]++) fail(what + "a label is listed under two columns of C (or twice in one); a label has one weight vector");
        }
    }
    if (pR) {
        check_csc(what, "R", pR);
        if (pR->rows != pY->rows || pR->cols != pY->cols) fail(what + "R's shape differs from Y's");
        const uint64_t nnz = pY->col_ptr[pY->cols];
        if (pR->col_ptr[pR->cols] != nnz || !std::equal(pY->col_ptr, pY->col_ptr + pY->cols + 1, pR->col_ptr) || (nnz && !std::equal(pY->row_idx, pY->row_idx + nnz, pR->row_idx)))
            fail(what + "R does not share Y's pattern (indptr and indices)");
        if (nnz && !pR->val) fail(what + "null values (R)");
    }
    require_gpu();
    use_device(g_device);
    Uploaded x, y, c, m;
    DevBuf r;
    upload(HostX(&X), x);
    upload_pattern(pY, y);
    if (coded) { upload_pattern(pC, c); upload_pattern(pM, m); }
    if (pR) r.upload_raw(pR->val, (size_t)pY->col_ptr[pY->cols] * 4);
    DevCsr wt;
    if (newton) {
        NewtonCounters counters;
        train_layer_newton_device(what_c, x.v, y.v, pR ? r.as<float>() : nullptr, coded ? &c.v : nullptr, coded ? &m.v : nullptr, p, nullptr, wt, counters);
        keep_counters(counters);
    } else {
        TrainCounters counters;
        train_layer_device(what_c, x.v, y.v, pR ? r.as<float>() : nullptr, coded ? &c.v : nullptr, coded ? &m.v : nullptr, p, nullptr, wt, counters);
        keep_counters(counters);
    }
    const uint32_t L = pY->cols;
    std::vector<uint64_t> ptr((size_t)L + 1);
    std::vector<uint32_t> idx((size_t)wt.nnz);
    std::vector<float> val((size_t)wt.nnz);
    download_csr(csr_view(L, X.cols + (p.bias > 0 ? 1u : 0u), wt.ptr.as<uint64_t>(), wt.idx.as<uint32_t>(), wt.val.as<float>(), wt.nnz), ptr.data(), idx.data(), val.data());
    uint64_t* rows = nullptr;
    uint64_t* cols = nullptr;
    float* vals = nullptr;
    coo_alloc((uint64_t)X.cols + (p.bias > 0 ? 1u : 0u), L, wt.nnz, &rows, &cols, &vals);
    if (wt.nnz && (!rows || !cols || !vals)) fail(what + "the allocator returned null");
    uint64_t o = 0;
    auto emit = [&](uint32_t label) {
        for (uint64_t x0 = ptr[label]; x0 < ptr[label + 1]; ++x0, ++o) { rows[o] = idx[x0]; cols[o] = label; vals[o] = val[x0]; }
    };
    if (coded) for (uint64_t x0 = 0, e = pC->col_ptr[pC->cols]; x0 < e; ++x0) emit(pC->row_idx[x0]);
    else for (uint32_t l = 0; l < L; ++l) emit(l);
}

void train_csr(const char* what, bool newton, const ScipyCsrF32* pX, const ScipyCscF32* pY, const ScipyCscF32* pC, const ScipyCscF32* pM, const ScipyCscF32* pR,
               py_coo_allocator_t coo_alloc, const TrainParams& p) {
    guarded([&] {
        if (!pX || !pX->row_ptr) fail(std::string(what) + ": null X");
        if (pX->rows >= (1u << 31)) fail(std::string(what) + ": 2^31 rows or more");          // (before the row pointer's end is read)
        if (pX->rows && pX->row_ptr[pX->rows] && (!pX->col_idx || !pX->val)) fail(std::string(what) + ": null indices or values (X)");
        train_host(what, *pX, pY, pC, pM, pR, coo_alloc, p, newton);
    });
}

// the same computation on rows that store every entry, zeros included: the reference's dense rows are walked over all cols
void train_drm(const char* what, bool newton, const ScipyDrmF32* pX, const ScipyCscF32* pY, const ScipyCscF32* pC, const ScipyCscF32* pM, const ScipyCscF32* pR,
               py_coo_allocator_t coo_alloc, const TrainParams& p) {
    guarded([&] {
        if (!pX) fail(std::string(what) + ": null X");
        if (pX->rows >= (1u << 31)) fail(std::string(what) + ": 2^31 rows or more");
        if (pX->rows && pX->cols && !pX->val) fail(std::string(what) + ": null values (X)");
        check_solver(std::string(what) + ": ", p, newton);                                          // refusals come before the index arrays are built
        const uint64_t n = (uint64_t)pX->rows * pX->cols;
        std::vector<uint64_t> ptr((size_t)pX->rows + 1);
        std::vector<uint32_t> idx((size_t)n);
        for (uint64_t r = 0; r <= pX->rows; ++r) ptr[r] = r * pX->cols;
        for (uint64_t i = 0; i < n; ++i) idx[i] = (uint32_t)(i % pX->cols);
        const ScipyCsrF32 csr{pX->rows, pX->cols, ptr.data(), idx.data(), pX->val};
        train_host(what, csr, pY, pC, pM, pR, coo_alloc, p, newton);
    });
}

void* train_resident(const char* what_c, bool newton, void* X, void* Yt, void* Ct_or_null, void* Mt_or_null, void* Rt_or_null, const TrainParams& p, void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const std::string what = std::string(what_c) + ": ";
        const double bias = p.bias;
        check_solver(what, p, newton);
        const Queries& x = csr_handle(what, X, "X");
        const Queries& y = csr_handle(what, Yt, "Yt");
        if (Ct_or_null && !Mt_or_null) fail(what + "Ct comes without Mt");
        const Queries* c = Ct_or_null ? &csr_handle(what, Ct_or_null, "Ct") : nullptr;
        const Queries* m = c ? &csr_handle(what, Mt_or_null, "Mt") : nullptr;
        const Queries* r = Rt_or_null ? &csr_handle(what, Rt_or_null, "Rt") : nullptr;
        for (const Queries* o : {&y, c, m, r})
            if (o && o->device != x.device) fail(what + "the operands are on devices " + std::to_string(x.device) + " and " + std::to_string(o->device) + "; training needs all on one");
        if (y.dev.cols != x.dev.rows) fail(what + "Yt.cols != X.rows (" + std::to_string(y.dev.cols) + " != " + std::to_string(x.dev.rows) + ")");
        if (x.dev.rows >= (1u << 31)) fail(what + "2^31 rows or more");
        if (c) {
            if (c->dev.cols != y.dev.rows) fail(what + "Ct.cols != Yt.rows (" + std::to_string(c->dev.cols) + " != " + std::to_string(y.dev.rows) + ")");
            if (m->dev.cols != x.dev.rows) fail(what + "Mt.cols != X.rows (" + std::to_string(m->dev.cols) + " != " + std::to_string(x.dev.rows) + ")");
            if (m->dev.rows != c->dev.rows) fail(what + "Mt.rows != Ct.rows (" + std::to_string(m->dev.rows) + " != " + std::to_string(c->dev.rows) + ")");
        }
        if ((c ? c->dev.nnz : (uint64_t)y.dev.rows) >= 0xFFFFFFFFull) fail(what + "2^32 - 1 jobs or more");
        if (r && (r->dev.rows != y.dev.rows || r->dev.cols != y.dev.cols || r->dev.nnz != y.dev.nnz)) fail(what + "Rt does not share Yt's pattern (shape or stored entries)");
        require_gpu();
        use_device(x.device);
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        if (r) same_pattern_device(what_c, y.dev, r->dev, s);
        auto out = std::make_unique<Queries>();
        if (newton) {
            NewtonCounters counters;
            train_layer_newton_device(what_c, x.dev, y.dev, r ? r->dev.val : nullptr, c ? &c->dev : nullptr, m ? &m->dev : nullptr, p, s, out->own, counters);
            keep_counters(counters);
        } else {
            TrainCounters counters;
            train_layer_device(what_c, x.dev, y.dev, r ? r->dev.val : nullptr, c ? &c->dev : nullptr, m ? &m->dev : nullptr, p, s, out->own, counters);
            keep_counters(counters);
        }
        set_own_csr(*out, x.device, y.dev.rows, x.dev.cols + (bias > 0 ? 1u : 0u));
        return out.release();
    });
}

}  // namespace

extern "C" {

void xrl_single_layer_train_csr_f32(const ScipyCsrF32* pX, const ScipyCscF32* pY, const ScipyCscF32* pC, const ScipyCscF32* pM, const ScipyCscF32* pR,
                                          py_coo_allocator_t coo_alloc, double threshold, uint32_t max_nonzeros_per_label, int solver_type, double Cp, double Cn,
                                          size_t max_iter, double eps, double bias, int threads) {
    (void)threads;
    train_csr("xrl_single_layer_train_csr_f32", false, pX, pY, pC, pM, pR, coo_alloc, make_params(threshold, max_nonzeros_per_label, solver_type, Cp, Cn, max_iter, eps, bias));
}

void xrl_single_layer_train_drm_f32(const ScipyDrmF32* pX, const ScipyCscF32* pY, const ScipyCscF32* pC, const ScipyCscF32* pM, const ScipyCscF32* pR,
                                          py_coo_allocator_t coo_alloc, double threshold, uint32_t max_nonzeros_per_label, int solver_type, double Cp, double Cn,
                                          size_t max_iter, double eps, double bias, int threads) {
    (void)threads;
    train_drm("xrl_single_layer_train_drm_f32", false, pX, pY, pC, pM, pR, coo_alloc, make_params(threshold, max_nonzeros_per_label, solver_type, Cp, Cn, max_iter, eps, bias));
}

void* xrl_train_layer_device(void* X, void* Yt, void* Ct_or_null, void* Mt_or_null, void* Rt_or_null, double threshold, uint32_t max_nonzeros_per_label,
                             int solver_type, double Cp, double Cn, uint64_t max_iter, double eps, double bias, void* hip_stream) {
    return train_resident("xrl_train_layer_device", false, X, Yt, Ct_or_null, Mt_or_null, Rt_or_null,
                          make_params(threshold, max_nonzeros_per_label, solver_type, Cp, Cn, max_iter, eps, bias), hip_stream);
}

// ---- the primal L2-loss SVC (K16): the same argument lists, solver_type == 2
void xrl_single_layer_train_newton_csr_f32(const ScipyCsrF32* pX, const ScipyCscF32* pY, const ScipyCscF32* pC, const ScipyCscF32* pM, const ScipyCscF32* pR,
                                           py_coo_allocator_t coo_alloc, double threshold, uint32_t max_nonzeros_per_label, int solver_type, double Cp, double Cn,
                                           size_t max_iter, double eps, double bias, int threads) {
    (void)threads;
    train_csr("xrl_single_layer_train_newton_csr_f32", true, pX, pY, pC, pM, pR, coo_alloc, make_params(threshold, max_nonzeros_per_label, solver_type, Cp, Cn, max_iter, eps, bias));
}

void xrl_single_layer_train_newton_drm_f32(const ScipyDrmF32* pX, const ScipyCscF32* pY, const ScipyCscF32* pC, const ScipyCscF32* pM, const ScipyCscF32* pR,
                                           py_coo_allocator_t coo_alloc, double threshold, uint32_t max_nonzeros_per_label, int solver_type, double Cp, double Cn,
                                           size_t max_iter, double eps, double bias, int threads) {
    (void)threads;
    train_drm("xrl_single_layer_train_newton_drm_f32", true, pX, pY, pC, pM, pR, coo_alloc, make_params(threshold, max_nonzeros_per_label, solver_type, Cp, Cn, max_iter, eps, bias));
}

void* xrl_train_layer_newton_device(void* X, void* Yt, void* Ct_or_null, void* Mt_or_null, void* Rt_or_null, double threshold, uint32_t max_nonzeros_per_label,
                                    int solver_type, double Cp, double Cn, uint64_t max_iter, double eps, double bias, void* hip_stream) {
    return train_resident("xrl_train_layer_newton_device", true, X, Yt, Ct_or_null, Mt_or_null, Rt_or_null,
                          make_params(threshold, max_nonzeros_per_label, solver_type, Cp, Cn, max_iter, eps, bias), hip_stream);
}

int xrl_debug_newton_counters(uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&] {
        if (!out) fail("xrl_debug_newton_counters: null argument");
        std::lock_guard<std::mutex> g(g_counters_mu);
        const NewtonCounters& c = g_newton_counters;
        const uint64_t v[kNewtonCounterCount] = {c.jobs, c.batches, c.slots, c.stride, c.newton_iters, c.cg_iters, c.hv_calls, c.halvings, c.end_before_first, c.end_gradient,
                                                 c.end_linesearch, c.end_actred, c.end_cap, c.cg_dhd, c.cg_q, c.cg_positive, c.cg_cap, c.lane_rows, c.wave_rows, c.nonfinite_jobs};
        for (uint32_t i = 0; i < n && i < kNewtonCounterCount; ++i) out[i] = v[i];
        return 0;
    });
}

int xrl_debug_train_counters(uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&] {
        if (!out) fail("xrl_debug_train_counters: null argument");
        std::lock_guard<std::mutex> g(g_counters_mu);
        const TrainCounters& c = g_counters;
        const uint64_t v[kTrainCounterCount] = {c.jobs, c.batches, c.slots, c.stride, c.iters, c.shrinks, c.reactivations, c.max_iter_stops, c.clipped, c.lane_rows,
                                                c.wave_rows, c.extensions, c.reruns};
        for (uint32_t i = 0; i < n && i < kTrainCounterCount; ++i) out[i] = v[i];
        return 0;
    });
}

}  // extern "C"
