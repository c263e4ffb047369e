// Output constraint on the device: XLinearModel.set_output_constraint (pecos/xmc/base.py:1796-1824) without rewriting, saving and
// reloading a model.  The reference deletes from every C, bottom-up, the entries whose row is not kept, and keeps for the layer above the
// columns that still hold an entry; it stops at the first layer whose kept set is the whole layer.  A layer's candidate set is defined by
// LayerDev::chunk_col (a parent's range in the stored child order) and LayerDev::perm_inv (stored position -> original child id) and by
// nothing else, so the pruned C is a second pair of those arrays -- Layer::view -- listing the kept children in their stored order.  A child's
// score depends only on its own column of W and on its parent's score, and ties break by candidate position: deleting candidates keeps
// the order of the rest, and no weight format is rebuilt.
//
//   kc_mark      flags of the kept labels; the lowest index of an id >= nr_pred_cols by atomicMin
//   kc_count     how many flags of a layer are set (the rule's early stop compares it with the layer's size)
//   kc_parent    one wavefront per parent, 64 children of its range at a time: the kept ones counted (pass 0: also the parent's flag for the
//                layer above) or, after an exclusive scan of the counts (rocPRIM), written to perm_inv' in order (pass 1)
//   k1p_constrained_kernel   K1C's twin (xrl_pairs.hip): the candidates of the view scored with the arithmetic of the handle's route
//
// The setter is synchronous: it reads the counts and chunk_col' back (the view's candidate bound is the sum of the beam's largest KEPT chunks).
#include "xrl_constrain.h"

#include <algorithm>

#include "xrl_devprim.h"
#include "xrl_pairs.h"

namespace xrl {

namespace {

constexpr unsigned long long kNoBadIndex = ~0ull;

__global__ void __launch_bounds__(256)
kc_mark(const uint32_t* __restrict__ labels, uint64_t n, uint32_t n_flags, uint32_t* __restrict__ flags, unsigned long long* __restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t lab = labels[i];
    if (lab < n_flags) flags[lab] = 1u;                    // (duplicates store the same word)
    else atomicMin(bad, (unsigned long long)i);
}

__global__ void __launch_bounds__(256) kc_count(const uint32_t* __restrict__ flags, uint32_t n_flags, uint32_t* __restrict__ total) {
    uint32_t c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_flags; i += (uint64_t)gridDim.x * 256u) c += flags[i] ? 1u : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += (uint32_t)__shfl_down((int)c, d, 64);
    if ((threadIdx.x & 63u) == 0u && c) atomicAdd(total, c);
}

struct ParentArgs {
    const uint32_t* chunk_col; const uint32_t* perm_inv;   // the layer as loaded (perm_inv may be null: stored position = child id)
    const uint32_t* flags; uint32_t n_flags;               // kept children of this layer, by original id
    uint32_t n_parents;
    uint32_t* cnt;                                         // pass 0: [n_parents] kept children of every parent
    uint32_t* parent_flags;                                // pass 0: [n_parents] the kept set of the layer above (may be null: root layer)
    const uint32_t* new_chunk_col; uint32_t* new_perm_inv; // pass 1: the scanned counts; the kept children's original ids, in stored order
};

template <int PASS>
__global__ void __launch_bounds__(256) kc_parent(ParentArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= a.n_parents) return;                          // (whole wavefronts)
    const uint32_t b = a.chunk_col[p], e = a.chunk_col[p + 1];
    uint32_t seen = 0;
    const uint32_t dst = PASS == 1 ? a.new_chunk_col[p] : 0u;
    for (uint32_t base = b; base < e; base += 64u) {
        const uint32_t pos = base + (uint32_t)lane;
        bool kept = false; uint32_t id = 0;
        if (pos < e) { id = a.perm_inv ? a.perm_inv[pos] : pos; kept = id < a.n_flags && a.flags[id] != 0u; }
        const unsigned long long m = __ballot(kept);
        if (PASS == 1 && kept) a.new_perm_inv[dst + seen + lanes_below(m)] = id;
        seen += (uint32_t)__popcll(m);
        if (e - base <= 64u) break;                        // (base + 64 may wrap on the last range of a 2^32-child layer)
    }
    if (PASS == 0 && lane == 0) { a.cnt[p] = seen; if (a.parent_flags) a.parent_flags[p] = seen ? 1u : 0u; }
}

uint32_t count_flags(const uint32_t* flags, uint32_t n_flags, uint32_t* d_total, hipStream_t s) {
    uint32_t total = 0;
    XRL_HIP(hipMemsetAsync(d_total, 0, 4, s));
    if (n_flags) {
        const uint32_t blocks = (uint32_t)std::min<uint64_t>(1024, ((uint64_t)n_flags + 255) / 256);
        hipLaunchKernelGGL(kc_count, dim3(blocks), dim3(256), 0, s, flags, n_flags, d_total);
        XRL_LAUNCH_CHECK();
    }
    XRL_HIP(hipMemcpyAsync(&total, d_total, 4, hipMemcpyDeviceToHost, s));
    XRL_HIP(hipStreamSynchronize(s));
    return total;
}

}  // namespace

void clear_output_constraint(Model& m) {
    XRL_HIP(hipDeviceSynchronize());                       // no predict of the handle may still read a view
    for (auto& L : m.layers) {
        const uint64_t models = L->device_bytes - L->buffer_bytes();   // (like ensure_device_csc: device_bytes also carries what the Model holds for the layer)
        L->view.clear();
        L->device_bytes = L->buffer_bytes() + models;
    }
    m.constrained = false;
}

void set_output_constraint(Model& m, const uint32_t* labels, uint64_t n, bool on_device, hipStream_t s, const char* what) {
    const std::string w = std::string(what) + ": ";
    if (!labels) fail(w + "null label list");
    if (n == 0) fail(w + "an empty label list would leave nothing to predict (xrl_clear_output_constraint removes a constraint)");
    if (!m.replicas.empty()) fail(w + "not available on a handle that serves from several devices (option \"devices\" > 1)");
    for (const auto& L : m.layers)
        if (!L->csc_ready && !L->w_host && L->w_path.empty()) fail(w + "this handle carries no CSC weights (an mmap model folder): the constrained route cannot score it");
    const size_t T = m.layers.size();
    if (!s) s = m.stream;
    XRL_HIP(hipDeviceSynchronize());                       // the handle's predicts, on whatever stream, are over; the caller's labels are written

    // ---- mark
    const uint32_t n_labels = m.layers[T - 1]->c_rows;     // nr_pred_cols
    DevBuf d_labels, flags[2], d_words, d_cnt, d_tmp;
    if (!on_device) { d_labels.upload_raw(labels, n * 4); labels = d_labels.as<uint32_t>(); }
    d_words.reserve(16);                                   // [0, 8) the lowest bad index, [8, 12) a flag count
    unsigned long long* d_bad = d_words.as<unsigned long long>(); uint32_t* d_total = d_words.as<uint32_t>() + 2;
    flags[0].reserve((size_t)n_labels * 4);
    XRL_HIP(hipMemsetAsync(flags[0].p, 0, (size_t)n_labels * 4, s));
    XRL_HIP(hipMemsetAsync(d_bad, 0xFF, 8, s));
    const uint64_t mark_blocks = (n + 255) / 256;
    if (mark_blocks > 0x7FFFFFFFull) fail(w + "label list too long");
    hipLaunchKernelGGL(kc_mark, dim3((uint32_t)mark_blocks), dim3(256), 0, s, labels, n, n_labels, flags[0].as<uint32_t>(), d_bad);
    XRL_LAUNCH_CHECK();
    unsigned long long bad = kNoBadIndex;
    XRL_HIP(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, s));
    uint32_t kept = count_flags(flags[0].as<uint32_t>(), n_labels, d_total, s);   // (synchronises: `bad` has arrived too)
    if (bad != kNoBadIndex) {
        uint32_t v = 0;
        XRL_HIP(hipMemcpy(&v, labels + bad, 4, hipMemcpyDeviceToHost));
        fail(w + "labels[" + std::to_string(bad) + "] = " + std::to_string(v) + " is out of range (the model predicts " + std::to_string(n_labels) + " labels)");
    }

    // ---- compact, bottom-up, into views of their own: the constraint in force stays until every layer is built
    std::vector<ConstraintView> next(T);
    int cur = 0;
    uint32_t n_flags = n_labels;                           // words of flags[cur]
    for (size_t l = T; l-- > 0;) {
        Layer& L = *m.layers[l];
        if (kept == L.c_rows) break;                       // the rule's stop: this layer and every layer above keep their C as loaded
        const uint32_t P = L.dev.n_parents;
        ConstraintView& V = next[l];
        d_cnt.reserve(((size_t)P + 1) * 4);
        XRL_HIP(hipMemsetAsync(d_cnt.p, 0, ((size_t)P + 1) * 4, s));
        flags[cur ^ 1].reserve((size_t)P * 4);
        ParentArgs a{};
        a.chunk_col = L.dev.chunk_col; a.perm_inv = L.dev.perm_inv; a.flags = flags[cur].as<uint32_t>(); a.n_flags = n_flags; a.n_parents = P;
        a.cnt = d_cnt.as<uint32_t>(); a.parent_flags = flags[cur ^ 1].as<uint32_t>();
        const dim3 grid((P + 3u) / 4u), block(256);
        if (P) { hipLaunchKernelGGL(kc_parent<0>, grid, block, 0, s, a); XRL_LAUNCH_CHECK(); }
        V.d_chunk_col.reserve(((size_t)P + 1) * 4);
        exclusive_scan(d_tmp, a.cnt, V.d_chunk_col.as<uint32_t>(), (size_t)P + 1, s);
        std::vector<uint32_t> cc((size_t)P + 1);
        XRL_HIP(hipMemcpyAsync(cc.data(), V.d_chunk_col.p, ((size_t)P + 1) * 4, hipMemcpyDeviceToHost, s));
        XRL_HIP(hipStreamSynchronize(s));
        V.kept = cc[P];
        V.d_perm_inv.reserve((size_t)std::max<uint64_t>(1, V.kept) * 4);
        a.new_chunk_col = V.d_chunk_col.as<uint32_t>(); a.new_perm_inv = V.d_perm_inv.as<uint32_t>();
        if (P && V.kept) { hipLaunchKernelGGL(kc_parent<1>, grid, block, 0, s, a); XRL_LAUNCH_CHECK(); }
        V.chunk_sizes_desc.resize(P);
        for (uint32_t p = 0; p < P; ++p) V.chunk_sizes_desc[p] = cc[p + 1] - cc[p];
        std::sort(V.chunk_sizes_desc.begin(), V.chunk_sizes_desc.end(), std::greater<uint32_t>());
        V.active = true;
        cur ^= 1; n_flags = P;
        if (l > 0) kept = count_flags(flags[cur].as<uint32_t>(), P, d_total, s);   // the kept set of the layer above: the parents that still have a child
    }
    XRL_HIP(hipStreamSynchronize(s));
    if (!next[T - 1].active) { clear_output_constraint(m); return; }   // every label kept: the rule stops at once
    // everything that can fail comes first (the CSC copy of W the route scores against); the swap itself only moves buffers, so a
    // handle never carries the new view on some layers and the old state on others
    for (auto& L : m.layers) ensure_device_csc(*L);
    for (size_t l = 0; l < T; ++l) {
        Layer& L = *m.layers[l];
        const uint64_t models = L.device_bytes - L.buffer_bytes();
        L.view = std::move(next[l]);
        L.device_bytes = L.buffer_bytes() + models;
    }
    m.constrained = true;
}

// ---------------------------------------------------------------------------------------------
// K1P: every candidate K0 laid out over the view, 16 lanes per (query, kept child) pair
// ---------------------------------------------------------------------------------------------
struct K1PArgs {
    CscDev W; QueriesDev X;
    const uint32_t* chunk_col; const uint32_t* perm_inv;
    const uint32_t* p_idx; const float* p_val; const uint32_t* p_cnt; uint32_t p_stride;
    const uint32_t* cand_off; const uint32_t* ncand; float* cand;
    uint32_t row0, nrows, beam_in, cand_stride;
    int pp_kind, pp_p, first_layer, implicit_root, chain, bias_first;
};

template <int PPC>
__global__ void __launch_bounds__(256) k1p_constrained_kernel(K1PArgs a) {
    const int lane = threadIdx.x & 63, lig = lane % PG, gbase = lane - lig;
    const uint64_t g = (uint64_t)blockIdx.x * PAIRS_PER_BLOCK + threadIdx.x / PG;
    const uint64_t q = g / a.cand_stride;
    if (q >= a.nrows) return;
    const uint32_t pos = (uint32_t)(g - q * a.cand_stride);
    if (pos >= a.ncand[q]) return;
    // position -> (beam slot, kept child): prolongate's layout (K0) over the view
    uint32_t parent = 0, off = 0; float pscore = 1.0f;
    if (!a.implicit_root) {
        const uint32_t cnt = min(a.p_cnt[q], a.beam_in);
        uint32_t jj = 0;
        for (uint32_t j = 1; j < cnt; ++j) if (a.cand_off[q * a.beam_in + j] <= pos) jj = j; else break;
        off = a.cand_off[q * a.beam_in + jj];
        parent = a.p_idx[q * a.p_stride + jj]; pscore = a.p_val[q * a.p_stride + jj];
    }
    const uint32_t child = a.chunk_col[parent] + (pos - off);
    const uint32_t col = a.perm_inv ? a.perm_inv[child] : child;         // W's own column id
    const float res = a.chain == kChainCsc ? csc_route_product(a.W, a.X, (uint64_t)a.row0 + q, col, lig, gbase)
                                           : chunked_route_product(a.W, a.X, (uint64_t)a.row0 + q, col, a.bias_first, lig, gbase);
    if (lig == 0) {
        float v = pp_transform<PPC>(a.pp_kind, a.pp_p, res);
        if (!a.first_layer) v = pp_combine(a.pp_kind, v, pscore);
        a.cand[q * a.cand_stride + pos] = v;
    }
}

void launch_k1p_constrained(const LayerDev& V, const uint64_t* col_ptr, const uint32_t* row_idx, const float* val, const LayerPlan& P, int chain,
                            const QueriesDev& X, BeamDev prev, const uint32_t* cand_off, const uint32_t* ncand, float* cand, hipStream_t s) {
    if (P.nrows == 0) return;
    K1PArgs a;
    a.W = CscDev{col_ptr, row_idx, val, V.w_rows, V.bias}; a.X = X;
    a.chunk_col = V.chunk_col; a.perm_inv = V.perm_inv;
    a.p_idx = prev.idx; a.p_val = prev.val; a.p_cnt = prev.cnt; a.p_stride = prev.stride;
    a.cand_off = cand_off; a.ncand = ncand; a.cand = cand;
    a.row0 = P.row0; a.nrows = P.nrows; a.beam_in = P.beam_in; a.cand_stride = P.cand_stride;
    a.pp_kind = P.pp.kind; a.pp_p = P.pp.p; a.first_layer = P.first_layer; a.implicit_root = P.implicit_root;
    a.chain = chain; a.bias_first = P.bias_first;
    const uint64_t groups = (uint64_t)P.nrows * P.cand_stride;
    const uint64_t blocks = (groups + PAIRS_PER_BLOCK - 1) / PAIRS_PER_BLOCK;
    if (blocks > 0x7FFFFFFFull) fail("k1p: grid too large; lower max_batch_rows");
    if (pp_class(P.pp)) hipLaunchKernelGGL(k1p_constrained_kernel<1>, dim3((uint32_t)blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k1p_constrained_kernel<0>, dim3((uint32_t)blocks), dim3(256), 0, s, a);
    XRL_LAUNCH_CHECK();
}

}  // namespace xrl
