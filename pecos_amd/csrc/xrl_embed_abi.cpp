// Label embeddings on the device (K12, xrl_embed.hip, composed with K10): the transpose, row normalisation and hstack of matrix handles,
// and xrl_label_embedding_device = LabelEmbeddingFactory.create (pecos/xmc/base.py:1903-2094) for CSR operands.  Every argument is
// checked before a GPU is required.
#include <atomic>
#include <memory>

#include "xrl_abi_common.h"
#include "xrl_embed.h"
#include "xrl_spgemm.h"

using namespace xrl;

namespace {

std::atomic<uint64_t> g_forms[4];                          // of this process since the load: EmbedForms' four counts

void count_forms(const EmbedForms& f) { g_forms[0] += f.t_lds; g_forms[1] += f.t_big; g_forms[2] += f.n_lane; g_forms[3] += f.n_wave; }

void check_transposable(const std::string& what, const Queries& m) {
    if (m.dev.nnz >= 0xFFFFFFFFull) fail(what + ": a transpose serves fewer than 2^32 - 1 stored entries");
}

std::unique_ptr<Queries> own_handle(DevCsr&& c, int device, uint32_t rows, uint32_t cols) {
    auto m = std::make_unique<Queries>();
    m->own = std::move(c);
    set_own_csr(*m, device, rows, cols);
    return m;
}

// a copy of v's row pointer and column ids with room for its values
void copy_pattern(const QueriesDev& v, hipStream_t s, DevCsr& out) {
    out.ptr.reserve(((size_t)v.rows + 1) * 8); out.idx.reserve(v.nnz * 4); out.val.reserve(v.nnz * 4);
    out.nnz = v.nnz;
    XRL_HIP(hipMemcpyAsync(out.ptr.p, v.row_ptr, ((size_t)v.rows + 1) * 8, hipMemcpyDeviceToDevice, s));
    if (v.nnz) XRL_HIP(hipMemcpyAsync(out.idx.p, v.col_idx, v.nnz * 4, hipMemcpyDeviceToDevice, s));
}

// both row normalisation entry points: the handle's rows by `norm`, in place or into a new owned handle
int normalize_rows_handle(const char* what, void* A, int norm, int in_place, void** out, void* hip_stream) {
    const Queries& a = csr_handle(std::string(what) + ": ", A, "A");
    if (!in_place && !out) fail(std::string(what) + ": null argument (out)");
    require_gpu();
    use_device(a.device);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    EmbedForms f;
    if (in_place) {
        normalize_rows_device(what, a.dev, const_cast<float*>(a.dev.val), s, f, norm);
    } else {
        DevCsr n;
        copy_pattern(a.dev, s, n);
        normalize_rows_device(what, a.dev, n.val.as<float>(), s, f, norm);
        *out = own_handle(std::move(n), a.device, a.dev.rows, a.dev.cols).release();
    }
    count_forms(f);
    return 0;
}

}  // namespace

extern "C" {

void* xrl_smat_transpose_device(void* A, void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const char* what = "xrl_smat_transpose_device";
        const Queries& a = csr_handle(std::string(what) + ": ", A, "A");
        check_transposable(what, a);
        require_gpu();
        use_device(a.device);
        DevCsr t;
        EmbedForms f;
        transpose_device(what, a.dev, static_cast<hipStream_t>(hip_stream), t, f);
        count_forms(f);
        return own_handle(std::move(t), a.device, a.dev.cols, a.dev.rows).release();
    });
}

int xrl_smat_normalize_rows_device(void* A, int in_place, void** out, void* hip_stream) {
    return guarded_value(-1, [&] { return normalize_rows_handle("xrl_smat_normalize_rows_device", A, 2, in_place, out, hip_stream); });
}

int xrl_smat_normalize_rows_norm_device(void* A, int norm, int in_place, void** out, void* hip_stream) {
    return guarded_value(-1, [&] {
        const char* what = "xrl_smat_normalize_rows_norm_device";
        if (norm < 1 || norm > 3) fail(std::string(what) + ": unknown norm " + std::to_string(norm) + " (1 = l1, 2 = l2, 3 = max)");
        return normalize_rows_handle(what, A, norm, in_place, out, hip_stream);
    });
}

void* xrl_smat_hstack_device(void* const* mats, uint32_t n, void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const char* what = "xrl_smat_hstack_device";
        if (!mats || n == 0) fail(std::string(what) + ": no matrices");
        std::vector<QueriesDev> views;
        uint64_t cols = 0;
        const Queries& first = csr_handle(std::string(what) + ": ", mats[0], "matrix 0");
        for (uint32_t i = 0; i < n; ++i) {
            const Queries& m = csr_handle(std::string(what) + ": ", mats[i], "matrix " + std::to_string(i));
            if (m.device != first.device)
                fail(std::string(what) + ": the matrices are on devices " + std::to_string(first.device) + " and " + std::to_string(m.device) + "; an hstack needs all on one");
            if (m.dev.rows != first.dev.rows)
                fail(std::string(what) + ": matrix " + std::to_string(i) + " has " + std::to_string(m.dev.rows) + " rows, matrix 0 has " + std::to_string(first.dev.rows));
            cols += m.dev.cols;
            views.push_back(m.dev);
        }
        if (cols >= (1ull << 32)) fail(std::string(what) + ": the columns add up to 2^32 or more (" + std::to_string(cols) + ")");
        require_gpu();
        use_device(first.device);
        DevCsr h;
        hstack_device(what, views, static_cast<hipStream_t>(hip_stream), h);
        return own_handle(std::move(h), first.device, first.dev.rows, (uint32_t)cols).release();
    });
}

void* xrl_label_embedding_device(void* Y, void* X, void* Z_or_null, int method, int normalized_Y, void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const std::string what = "xrl_label_embedding_device";
        if (method < 0 || method > 2) fail(what + ": unknown method " + std::to_string(method) + " (0 = pifa, 1 = pifa_lf_concat, 2 = pii)");
        const Queries& y = csr_handle(what + ": ", Y, "Y");
        check_transposable(what, y);
        const Queries* x = nullptr;
        const Queries* z = nullptr;
        if (method != 2) {
            x = &csr_handle(what + ": ", X, "X");
            if (x->device != y.device) fail(what + ": Y and X are on devices " + std::to_string(y.device) + " and " + std::to_string(x->device));
            if (y.dev.rows != x->dev.rows) fail(what + ": Y.rows != X.rows (" + std::to_string(y.dev.rows) + " != " + std::to_string(x->dev.rows) + ")");
        }
        if (method == 1) {
            z = &csr_handle(what + ": ", Z_or_null, "Z");
            if (z->device != y.device) fail(what + ": Y and Z are on devices " + std::to_string(y.device) + " and " + std::to_string(z->device));
            if (z->dev.rows != y.dev.cols) fail(what + ": Z.rows != Y.cols (" + std::to_string(z->dev.rows) + " != " + std::to_string(y.dev.cols) + ")");
            if ((uint64_t)x->dev.cols + z->dev.cols >= (1ull << 32)) fail(what + ": X.cols + Z.cols is 2^32 or more");
        }
        require_gpu();
        use_device(y.device);
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        EmbedForms f;
        DevCsr yt;
        {
            QueriesDev yn = y.dev;
            DevBuf nval;                                   // the normalised Y is a private copy of its values: Y stays as it is
            if (method != 2 && normalized_Y) {
                nval.reserve(y.dev.nnz * 4);
                normalize_rows_device(what.c_str(), y.dev, nval.as<float>(), s, f);
                yn.val = nval.as<float>();
            }
            transpose_device(what.c_str(), yn, s, yt, f);
        }
        const QueriesDev ytv = csr_view(y.dev.cols, y.dev.rows, yt.ptr.as<uint64_t>(), yt.idx.as<uint32_t>(), yt.val.as<float>(), yt.nnz);
        std::unique_ptr<Queries> e;
        if (method == 2) {
            e = own_handle(std::move(yt), y.device, y.dev.cols, y.dev.rows);
        } else {
            SpgemmOut p;
            spgemm_device(ytv, x->dev, false, true, s, p);
            e = own_handle(std::move(p.z), y.device, y.dev.cols, x->dev.cols);
        }
        normalize_rows_device(what.c_str(), e->dev, const_cast<float*>(e->dev.val), s, f);
        count_forms(f);
        if (method != 1) return e.release();
        DevCsr h;
        hstack_device(what.c_str(), {e->dev, z->dev}, s, h);
        return own_handle(std::move(h), y.device, y.dev.cols, x->dev.cols + z->dev.cols).release();
    });
}

int xrl_debug_embed_forms(uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&] {
        if (!out) fail("xrl_debug_embed_forms: null argument");
        const uint64_t v[5] = {kEmbedCap, g_forms[0].load(), g_forms[1].load(), g_forms[2].load(), g_forms[3].load()};
        for (uint32_t i = 0; i < n && i < 5; ++i) out[i] = v[i];
        return 0;
    });
}

}  // extern "C"
