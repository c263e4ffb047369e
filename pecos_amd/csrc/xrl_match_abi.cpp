// Matching matrices in HBM (K14, xrl_match.hip): xrl_smat_pattern_union_device over xrl_smat_* handles and the counters the tests read.
// Every argument is checked before a GPU is required.
#include <atomic>
#include <memory>

#include "xrl_abi_common.h"
#include "xrl_match.h"

using namespace xrl;

namespace {
std::atomic<uint64_t> g_forms[4];                          // rows served in LDS, by the HBM sort; entries read, written
std::atomic<uint64_t> g_last_bound{0};
}  // namespace

namespace xrl {
void note_cand_bound(uint64_t bound) { g_last_bound = bound; }
}  // namespace xrl

extern "C" {

void* xrl_smat_pattern_union_device(void* const* mats, uint32_t n, void* hip_stream) {
    return guarded_value((void*)nullptr, [&]() -> void* {
        const std::string what = "xrl_smat_pattern_union_device: ";
        if (n == 0 || !mats) fail(what + "no operands; a union needs at least one");
        std::vector<QueriesDev> ops;
        const Queries* first = nullptr;
        for (uint32_t k = 0; k < n; ++k) {
            const Queries& m = csr_handle(what, mats[k], "operand " + std::to_string(k));
            if (!first) first = &m;
            if (m.dev.rows != first->dev.rows || m.dev.cols != first->dev.cols)
                fail(what + "operand " + std::to_string(k) + " has shape " + std::to_string(m.dev.rows) + " x " + std::to_string(m.dev.cols) + ", operand 0 has " +
                     std::to_string(first->dev.rows) + " x " + std::to_string(first->dev.cols));
            if (m.device != first->device)
                fail(what + "the operands are on devices " + std::to_string(first->device) + " and " + std::to_string(m.device) + "; a union needs all on one");
            ops.push_back(m.dev);
        }
        require_gpu();
        use_device(first->device);
        auto out = std::make_unique<Queries>();
        MatchCounters c;
        pattern_union_device("xrl_smat_pattern_union_device", ops, first->dev.rows, first->dev.cols, static_cast<hipStream_t>(hip_stream), out->own, c);
        g_forms[0] += c.lds_rows; g_forms[1] += c.big_rows; g_forms[2] += c.read; g_forms[3] += c.written;
        set_own_csr(*out, first->device, first->dev.rows, first->dev.cols);
        return out.release();
    });
}

int xrl_smat_check_relevance_device(void* Y, void* R, uint64_t* status, void* hip_stream) {
    return guarded_value(-1, [&] {
        const std::string what = "xrl_smat_check_relevance_device: ";
        const Queries& y = csr_handle(what, Y, "Y");
        const Queries& r = csr_handle(what, R, "R");
        if (!status) fail(what + "null argument (status)");
        if (y.dev.rows != r.dev.rows || y.dev.cols != r.dev.cols)
            fail(what + "R has shape " + std::to_string(r.dev.rows) + " x " + std::to_string(r.dev.cols) + ", Y has " + std::to_string(y.dev.rows) + " x " +
                 std::to_string(y.dev.cols));
        if (y.device != r.device) fail(what + "Y and R are on devices " + std::to_string(y.device) + " and " + std::to_string(r.device));
        require_gpu();
        use_device(y.device);
        check_relevance_device(y.dev, r.dev, static_cast<hipStream_t>(hip_stream), status);
        return 0;
    });
}

int xrl_debug_match_forms(uint64_t* out, uint32_t n) {
    return guarded_value(-1, [&] {
        if (!out) fail("xrl_debug_match_forms: null argument");
        const uint64_t v[5] = {g_forms[0].load(), g_forms[1].load(), g_forms[2].load(), g_forms[3].load(), g_last_bound.load()};
        for (uint32_t i = 0; i < n && i < 5; ++i) out[i] = v[i];
        return 0;
    });
}

}  // extern "C"
