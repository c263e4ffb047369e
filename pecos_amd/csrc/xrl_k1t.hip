// K1T: the tile-format layer product on TILE ROWS held densely -- compute_sparse_predictions + chunk_ops<csr, bin_search>
// (inference.hpp:925-1007, 769-813) + bias + post-processor + combine (:506-518, 192-240, 1360-1384) for sparse queries.
//
// The tile format's own kernel (k1_kernel, xrl_k1.hip) keeps a tile row as a list of {column, value} entries and applies a
// row to accumulators that live in LDS (the lanes of an item stride over the row's entries, each a read-modify-write of one LDS word).
// On a model the bound does not prune (Amazon-670K-hard: 4.9 M leaf items of ~47 matched rows x ~26 entries) that kernel is bound by
// vector-instruction issue: per matched row an extent lookup, a unit queue, a column select and an LDS read-add-write.
//
// Here every tile row that holds at least one weight is ALSO stored densely (LayerDev::wt): `wt_stride` = G * NR floats per row, column c
// of the tile at position c, kMissing (-0.0) where W has no entry, one all-missing pad row after every tile's rows.  A matched row is
// then ONE NR-dword load per lane (lane `lig` of the item's G lanes owns columns NR*lig .. NR*lig+NR-1: the G lanes read the row's
// G*NR*4 bytes contiguously) and NR multiply + NR add on accumulators held in REGISTERS: no extents, no unit queue, no LDS traffic but
// the hit queue.  With 288 GB of HBM the copy is cheap (Amazon-670K's leaf: 4.9 M rows x 384 B = 1.9 GB beside 1.0 GB of entries).
//
// Arithmetic: acc = fl32(acc + fl32(x * w)) per matched row in ascending feature order, separate multiply and add (no FMA), bias
// LAST (inference.hpp:806-811; HASH_CHUNKED: first, :716-722) -- the reference's order.  A missing cell multiplies by -0.0: for a
// finite x the product is a zero and leaves every reachable accumulator unchanged (accumulators start at +0.0 and can never become
// -0.0; same argument as the dense row format, xrl_model.h kMissing).  A drain that holds a NON-FINITE x (inf * -0.0 = NaN) runs
// the exact loop, which skips the cells whose bits are kMissing (an explicit -0.0 weight is stored as +0.0: identical for every x).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "xrl_device.h"
#include "xrl_kernels.h"
#include "xrl_items.h"

namespace xrl {

namespace {

struct K1TArgs {
    LayerDev L;
    QueriesDev X;
    const ItemDesc* items;
    const uint32_t* n_items;     // device count of (tile-sorted, all active) items, or nullptr: natural order
    float* cand;
    uint64_t n_slots;
    int pp_kind, pp_p, first_layer, bias_first;
    uint32_t n_vblocks;
    uint32_t* fb_out;            // pruning feedback: the launch's item count goes to this host-visible word
    uint32_t wt_bytes;           // BUF: size of the whole tile-row array (one buffer resource)
    // SEL (the selecting epilogue): the previous beam, the guard flags and where the layer's top-k goes
    const uint32_t* p_cnt; const float* p_val; uint32_t p_stride, beam_in;
    const uint32_t* xok; const uint32_t* perm_inv;
    uint32_t* out_idx; float* out_val; uint32_t* out_cnt; uint32_t* done;
    uint32_t out_stride, k;
    int mult;
    // SEL, items == nullptr: the item is DERIVED (k0_prolongate folded into this launch) and the offsets K0 would have written go out here
    const uint32_t* p_idx; const uint64_t* x_row_ptr;   // (x_row_ptr: of the batch's first row)
    uint32_t cand_stride; uint32_t* cand_off; uint32_t* ncand;
    // SEL, rest_q != nullptr: the unfinished queries are appended to this list (count *rest_cnt): the later stages' launches walk it
    uint32_t* rest_q; uint32_t* rest_cnt;
};

template <int NR> struct RowVec;
template <> struct RowVec<1> { float v[1]; };
template <> struct alignas(8) RowVec<2> { float v[2]; };
template <> struct RowVec<3> { float v[3]; };
template <> struct alignas(16) RowVec<4> { float v[4]; };

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <int NR> __device__ __forceinline__ RowVec<NR> row_load_buf(__amdgpu_buffer_rsrc_t rs, uint32_t voff);
template <> __device__ __forceinline__ RowVec<1> row_load_buf<1>(__amdgpu_buffer_rsrc_t rs, uint32_t voff) { return __builtin_bit_cast(RowVec<1>, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)voff, 0, 0)); }
template <> __device__ __forceinline__ RowVec<2> row_load_buf<2>(__amdgpu_buffer_rsrc_t rs, uint32_t voff) { return __builtin_bit_cast(RowVec<2>, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)voff, 0, 0)); }
template <> __device__ __forceinline__ RowVec<3> row_load_buf<3>(__amdgpu_buffer_rsrc_t rs, uint32_t voff) {
    const auto t = __builtin_amdgcn_raw_buffer_load_b96(rs, (int)voff, 0, 0);
    RowVec<3> r; r.v[0] = __uint_as_float(t[0]); r.v[1] = __uint_as_float(t[1]); r.v[2] = __uint_as_float(t[2]); return r;
}
template <> __device__ __forceinline__ RowVec<4> row_load_buf<4>(__amdgpu_buffer_rsrc_t rs, uint32_t voff) { return __builtin_bit_cast(RowVec<4>, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, 0, 0)); }

// G lanes per item (64 / G items per wavefront), NR columns per lane; LK = row lookup: 0 rank-bitmap {bits32, rank}, 2 {bits64, rank, -};
// BUF: the whole tile-row array is under 4 GiB and is addressed through ONE buffer resource with 32-bit byte offsets (a hit's queue word
// is its row's absolute offset: one vector add per row instead of a 64-bit address).
// SEL (G == 32, items in query order, one item per query = beam slot 0, one tile per parent): the FIRST STAGE of a bound-pruned layer in one
// launch.  When the feature loop ends, the 32 lanes of an item hold every candidate K2 would rank for that query (rank_limit == 1), so the
// epilogue does K2's work on them in registers -- the done flag, the top-k, the child ids -- two queries per wavefront, and stores the
// candidate row only for the queries that are not done (the later stages rank it again together with the other slots' scores).
template <int G, int NR, int PPC, int LK, bool BUF, bool SEL>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8))) k1t_kernel(K1TArgs a) {
    constexpr int W = 64 / G, H = 64, U = (G >= 16) ? 64 / G : 8, UNR = 8, STRIDE = G * NR;
    __shared__ uint2 hq_all[4 * W * (H + UNR)];
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t vblock = blockIdx.x * 4u + wave;
    if (vblock >= a.n_vblocks) return;
    const int lane = threadIdx.x & 63;
    const int grp = lane / G, lig = lane % G;
    uint2* __restrict__ my_hq = hq_all + ((size_t)wave * W + grp) * (H + UNR);   // hits {x value, byte offset of the row in the tile's block}

    // SEL without an item list: what k0_prolongate lays out for beam slot 0 of query q when a parent is one tile (its first column is the
    // chunk's: out_off = q * cand_stride).  The 32 lanes of the half load the same words; one hop more than reading the item (beam -> ptile -> tile).
    auto derive_item = [&](uint64_t q) {
        const uint32_t cnt = min(a.p_cnt[q], a.beam_in);
        const uint32_t parent = cnt ? a.p_idx[q * a.p_stride] : 0u;
        const float ps = a.p_val[q * a.p_stride];
        const uint64_t xb = a.x_row_ptr[q];
        const uint32_t xl = (uint32_t)(a.x_row_ptr[q + 1] - xb);
        const uint32_t t0 = a.L.ptile[parent], t1 = a.L.ptile[parent + 1];
        return make_item((uint32_t)q, (cnt && t1 > t0) ? t0 : kNoTile, (uint32_t)q * a.cand_stride, ps, xb, xl);
    };
    ItemDesc it;
    if (SEL && !a.items && !a.n_items) {   // derived items come in query order only, never with a list count (launch_k1t)
        const uint64_t slot = (uint64_t)vblock * W + grp;
        it = slot < a.n_slots ? derive_item(slot) : make_item(0u, kNoTile, 0u, 0.f, 0, 0u);
    } else if (!fetch_item<W>(a.items, a.n_items, a.n_slots, a.fb_out, vblock, grp, lane, it)) return;
    bool active = it.tile != kNoTile;
    TileDesc td{};
    uint64_t xe = 0, cur = 0, wbase = 0;
    if (active) {
        td = a.L.tiles[it.tile];
        wbase = a.L.wt_base[it.tile];
        cur = it.x_begin; xe = it.x_begin + it.x_len;
    }
    const char* __restrict__ wrow = reinterpret_cast<const char*>(a.L.wt + (BUF ? 0ull : wbase) + (uint32_t)(NR * lig));
    const uint32_t tbase = BUF ? (uint32_t)(wbase * 4ull) : 0u;          // BUF: queue words are offsets in the whole array
    const uint32_t lane_off = (uint32_t)(NR * lig * 4);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.L.wt), 0, (int)(BUF ? a.wt_bytes : 0u), 0x00020000);
    const uint32_t pad_off = tbase + td.nrows * (uint32_t)(STRIDE * 4);  // the tile's all-missing pad row
    float acc[NR];
    {
        const float* __restrict__ bp = a.L.bias_prod + td.col_begin;
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const uint32_t c = (uint32_t)(NR * lig + k);
            acc[k] = (a.bias_first && a.L.has_bias && c < td.ncols) ? bp[c] : 0.0f;   // chunk_ops<csr, hash>: 0.0 + bias * w first
        }
    }
    const BmWord* __restrict__ bm = a.L.bitmap + (LK != 0 ? 0ull : (uint64_t)(active ? it.tile : 0u) * a.L.nwords);
    const BmWord64* __restrict__ bm64 = a.L.bitmap64 + (LK != 2 ? 0ull : (uint64_t)(active ? it.tile : 0u) * a.L.nwords64);
    const uint64_t xlast = xe > cur ? xe - 1 : 0;                       // a valid x index for clamped loads
    uint32_t nh = 0;                                                    // hits waiting in this item's queue
    bool nonfin = false;                                                // (wavefront-uniform) a queued hit carries a non-finite x

    auto drain = [&](auto exact_tag) {
        constexpr bool EX = decltype(exact_tag)::value;
        wave_sync_lds();
        uint32_t nh_max = nh;
#pragma unroll
        for (int d = G; d < 64; d <<= 1) nh_max = max(nh_max, (uint32_t)__shfl_xor((int)nh_max, d, 64));
        nh_max = __builtin_amdgcn_readfirstlane(nh_max);
        // every item's queue is read up to the longest one of the wavefront (rounded to the unroll): the rest multiplies +0.0 with the pad row
        for (uint32_t j = nh + (uint32_t)lig; j < ((nh_max + UNR - 1u) & ~(uint32_t)(UNR - 1)); j += G) my_hq[j] = make_uint2(0u, pad_off);
        wave_sync_lds();
#pragma unroll 1
        for (uint32_t h0 = 0; h0 < nh_max; h0 += UNR) {
            uint2 hv[UNR];
            RowVec<NR> w[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) hv[u] = my_hq[h0 + u];
#pragma unroll
            for (int u = 0; u < UNR; ++u) w[u] = BUF ? row_load_buf<NR>(wrs, hv[u].y + lane_off) : *reinterpret_cast<const RowVec<NR>*>(wrow + hv[u].y);
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const float x = __uint_as_float(hv[u].x);
#pragma unroll
                for (int k = 0; k < NR; ++k) {
                    const float s = __fadd_rn(acc[k], __fmul_rn(x, w[u].v[k]));   // scalar * val, then add: no fma (inference.hpp:512-517)
                    acc[k] = (EX && __float_as_uint(w[u].v[k]) == kMissing) ? acc[k] : s;
                }
            }
        }
        nh = 0;
    };
    auto drain_any = [&]() {
        if (nonfin) drain(std::true_type{}); else drain(std::false_type{});
        nonfin = false;
    };

    uint32_t skip = 0;                 // u-slices of the current step already queued (after an overflow)
    while (__any(cur < xe)) {
        bool overflow = false;
        {
            // ---- load step: U*G consecutive features of the item
            uint32_t f[U]; float v[U];
            load_features<G, U>(a.X.col_idx, a.X.val, cur, xe, xlast, a.L.w_rows, lig, f, v);
            bool nf = false;                   // a value of the row (not a clamped re-read past its end) is inf / NaN
#pragma unroll
            for (int u = 0; u < U; ++u) nf |= (cur + (uint64_t)(u * G + lig) < xe) & ((__float_as_uint(v[u]) & 0x7F800000u) == 0x7F800000u);
            nonfin = nonfin || __any(nf);
            // ---- row lookup: is feature f a row of the tile, and which -- the queue word is the byte offset of that row
            bool hit[U]; uint32_t off[U];
            if (LK == 0) probe_bitmap32<U>(bm, f, hit, off, [&](const BmWord& w, uint32_t before) { return tbase + (w.rank + before) * (uint32_t)(STRIDE * 4); });
            else probe_bitmap64<U>(bm64, f, hit, off, [&](const BmWord64& w, uint32_t before) { return tbase + (w.rank + before) * (uint32_t)(STRIDE * 4); });
            // ---- queue the hits in feature order; on overflow the queue is drained outside this scope and the step resumed
            overflow = queue_hits<G, U, H>(hit, v, off, my_hq, grp, lig, nh, skip, cur, xe);
        }
        if (__any(overflow)) drain_any();
    }
    drain_any();

    // ---- epilogue: bias (sparse X: LAST, inference.hpp:806-811), transform in fp64, combine with the parent's score, store
    if constexpr (SEL) {
        static_assert(G == 32, "the selecting epilogue ranks one item per half-wavefront");
        int lane_e = lane;                                              // (opaque: nothing derived from the lane id stays live across the feature loop)
        asm volatile("" : "+v"(lane_e));
        const int grp = lane_e >> 5, lig = lane_e & 31;
        const uint64_t slot = (uint64_t)vblock * W + grp;               // query order, one item per query: the slot IS the query
        const bool qv = slot < a.n_slots;
        const uint64_t q = qv ? slot : 0;
        if constexpr (NR == 4) {   // four columns per lane leave no registers to carry the item across the feature loop: it is read again
            it = a.items ? a.items[q] : derive_item(q);
            active = qv && it.tile != kNoTile;
            td = a.L.tiles[active ? it.tile : 0u];
        }
        // what k2_topk_wave reads for rank_limit == 1 (in flight during the transform)
        const uint32_t pc = a.p_cnt[q], xok = a.xok[q];
        const float ps_next = a.p_val[q * a.p_stride + 1u];             // (beam_in >= 2 on a pruned layer: the word exists, valid or not)
        const float* __restrict__ bp = a.L.bias_prod + td.col_begin;
        const bool add_bias = a.L.has_bias != 0 && !a.bias_first;
        // candidate position = tile column NR * lig + k (slot 0, one tile); columns past the tile (and an inactive item) hold no candidate
        uint32_t key[NR], sb[NR];
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const uint32_t c = (uint32_t)(NR * lig + k);
            key[k] = 0u; sb[k] = 0u;
            if (active && c < td.ncols) {
                const float v = finish_score<PPC>(acc[k], add_bias, bp + c, a.pp_kind, a.pp_p, a.first_layer, it.pscore);
                sb[k] = __float_as_uint(v); key[k] = score_key(v);
            }
        }
        // done (before the extraction consumes the keys), as k2_topk_wave: k candidates of this slot score >= the best any later slot can reach
        const bool limited = min(pc, a.beam_in) > 1u;
        const uint32_t thr = score_key(a.mult ? fmaxf(ps_next, 0.0f) : ps_next);
        uint32_t c_lo = 0, c_hi = 0;
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const unsigned long long b = __ballot(key[k] >= thr);        // (thr >= 1: an empty slot never counts; each half against its own bound)
            c_lo += (uint32_t)__popc((uint32_t)b); c_hi += (uint32_t)__popc((uint32_t)(b >> 32));
        }
        const bool d = !limited || (xok != 0u && ps_next == ps_next && (grp ? c_hi : c_lo) >= a.k);
        if (!a.items && __any(qv && !d)) {
            // K0's other outputs, for the unfinished queries only (k0b_remaining and the later K2 launches skip a done query before they read
            // them): lane j of the half takes beam slot j (beam_in <= 32), an exclusive prefix sum of the chunk widths gives cand_off, the total ncand
            const uint32_t cnt = min(pc, a.beam_in);
            const bool mine = qv && !d && (uint32_t)lig < cnt;
            uint32_t wd = 0;
            if (mine) { const uint32_t pj = a.p_idx[q * a.p_stride + (uint32_t)lig]; wd = a.L.chunk_col[pj + 1] - a.L.chunk_col[pj]; }
            uint32_t incl = wd;
#pragma unroll
            for (int s = 1; s < 32; s <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, s, 32); if (lig >= s) incl += y; }
            const uint32_t total = (uint32_t)__shfl((int)incl, 31, 32);
            if (mine) a.cand_off[q * a.beam_in + (uint32_t)lig] = incl - wd;
            if (qv && !d && lig == 0) a.ncand[q] = total;
        }
        if (a.rest_q) {   // the later stages' list: one atomicAdd per wavefront, and only where one of its two queries is unfinished
            const unsigned long long um = __ballot(qv && !d && lig == 0);
            if (um) {
                uint32_t base = 0;
                if (lane_e == 0) base = atomicAdd(a.rest_cnt, (uint32_t)__popcll(um));
                base = (uint32_t)__shfl((int)base, 0, 64);
                if (qv && !d && lig == 0) a.rest_q[base + (grp ? (uint32_t)(um & 1ull) : 0u)] = (uint32_t)q;
            }
        }
        if (active && !d) {                                             // the later stages read the row of an unfinished query only (always: +0.034 ms on Amazon-670K)
            float* __restrict__ out = a.cand + it.out_off;
#pragma unroll
            for (int k = 0; k < NR; ++k) { const uint32_t c = (uint32_t)(NR * lig + k); if (c < td.ncols) out[c] = __uint_as_float(sb[k]); }
        }
        uint32_t osb, ops, kk_lo, kk_hi;
        halfwave_topk_extract<NR>(key, sb, a.k, lane_e, osb, ops, kk_lo, kk_hi);   // ties by position: see there
        const uint32_t kk = grp ? kk_hi : kk_lo;
        if (qv) {
            if ((uint32_t)lig < kk) {
                uint32_t child = td.col_begin + ops;                    // a one-tile parent: col_begin == chunk_col[parent]
                if (a.perm_inv) child = a.perm_inv[child];
                a.out_idx[q * a.out_stride + (uint32_t)lig] = child;
                a.out_val[q * a.out_stride + (uint32_t)lig] = __uint_as_float(osb);
            }
            if (lig == 0) { a.out_cnt[q] = kk; a.done[q] = d ? 1u : 0u; }
        }
        return;
    }
    if (!active) return;
    float* __restrict__ out = a.cand + it.out_off;
    const float* __restrict__ bp = a.L.bias_prod + td.col_begin;
    const bool add_bias = a.L.has_bias != 0 && !a.bias_first;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const uint32_t c = (uint32_t)(NR * lig + k);
        if (c < td.ncols) out[c] = finish_score<PPC>(acc[k], add_bias, bp + c, a.pp_kind, a.pp_p, a.first_layer, it.pscore);
    }
}

// tile rows, dense: wt[(wt_base[t] / stride + r) * stride + col] = the weight of tile t's row r at tile column col (an explicit -0.0 as +0.0);
// the buffer is pre-filled with kMissing.  One workgroup per tile, 32 lanes per row.
__global__ void __launch_bounds__(256)
tile_rows_kernel(const TileDesc* __restrict__ tiles, const uint32_t* __restrict__ row_ext, const Entry* __restrict__ entries,
                 const uint64_t* __restrict__ wt_base, uint32_t stride, uint32_t* __restrict__ wt) {
    const TileDesc td = tiles[blockIdx.x];
    uint32_t* __restrict__ dst = wt + wt_base[blockIdx.x];
    const uint32_t* __restrict__ ext = row_ext + td.rowptr_base;
    const Entry* __restrict__ ent = entries + td.ent_base;
    const uint32_t sub = threadIdx.x >> 5, l = threadIdx.x & 31u;
    for (uint32_t r = sub; r < td.nrows; r += 8u) {
        const uint32_t e = ext[r], start = e & 0x1FFFFFFu, len = (e >> 25) + 1u;
        for (uint32_t i = l; i < len; i += 32u) {
            const Entry x = ent[start + i];
            const uint32_t b = __float_as_uint(x.val);
            dst[(uint64_t)r * stride + x.col] = b == kMissing ? 0u : b;
        }
    }
}

}  // namespace

void k1t_shape(uint32_t max_tile_cols, int& g, int& nr) {
    g = max_tile_cols <= 8 ? 8 : max_tile_cols <= 16 ? 16 : 32;
    nr = (int)((max_tile_cols + (uint32_t)g - 1) / (uint32_t)g);
    if (nr < 1) nr = 1;
}

void launch_tile_rows(const LayerDev& L, uint64_t total_floats, uint32_t* wt, hipStream_t s) {
    XRL_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(wt), (int)kMissing, total_floats, s));
    if (L.n_tiles) {
        hipLaunchKernelGGL(tile_rows_kernel, dim3(L.n_tiles), dim3(256), 0, s, L.tiles, L.row_ext, L.entries, L.wt_base, L.wt_stride, wt);
        XRL_LAUNCH_CHECK();
    }
}

bool k1t_serves(const LayerDev& L, const QueriesDev& X) { return L.wt != nullptr && !X.dense && (L.bitmap || L.bitmap64) && !L.bucket; }

bool k1t_selects(const LayerDev& L, const LayerPlan& P, const QueriesDev& X) {
    int g, nr;
    k1t_shape(L.max_tile_cols, g, nr);
    return k1t_serves(L, X) && P.tune.tile_rows >= 1 && P.tune.ablate == 0 && L.max_tiles_per_parent == 1 && g == 32 && nr <= 4 &&
           P.k >= 1 && P.k <= kTopkExtractMaxK && P.beam_in >= 2 && !P.implicit_root && !P.first_layer && k2_wave_path(P);
}

void launch_k1t(const LayerDev& L, const LayerPlan& P, const QueriesDev& X, const void* items, const uint32_t* n_items, float* cand, hipStream_t s,
                const K1TSelect* sel) {
    if (P.nrows == 0) return;
    K1TArgs a{};
    a.L = L; a.X = X; a.items = static_cast<const ItemDesc*>(items); a.n_items = n_items; a.cand = cand;
    // (with `sel`, P is the WHOLE layer's plan -- `limited` needs its beam_in -- and the launch covers slot 0 of every query, one tile each)
    a.n_slots = sel ? (uint64_t)P.nrows : (uint64_t)P.nrows * P.beam_in * L.max_tiles_per_parent;
    a.pp_kind = P.pp.kind; a.pp_p = P.pp.p; a.first_layer = P.first_layer; a.bias_first = P.bias_first;
    a.fb_out = (n_items && P.fb_host && P.layer >= 0 && P.layer < kFbLayers) ? P.fb_host + fb_items_word(P.layer) : nullptr;
    int g, nr;
    k1t_shape(L.max_tile_cols, g, nr);
    if ((uint32_t)(g * nr) != L.wt_stride || nr > 4) fail("k1t: the layer's tile rows were laid out for another shape");
    const uint64_t vblocks = (a.n_slots + (uint64_t)(64 / g) - 1) / (uint64_t)(64 / g);
    if (vblocks > 0x7FFFFFFFull) fail("k1t: grid too large; lower max_batch_rows");
    a.n_vblocks = (uint32_t)vblocks;
    const int ppc = pp_class(P.pp);
    const int lk = L.bitmap64 ? 2 : 0;
    const bool buf = L.wt_bytes != 0 && L.wt_bytes < 0xFFFFFF00ull;   // (gfx9 range-checks voffset against num_records: the array's bytes)
    a.wt_bytes = buf ? (uint32_t)L.wt_bytes : 0u;
    if (sel) {
        if (n_items || !k1t_selects(L, P, X)) fail("k1t: the selecting epilogue does not serve this launch");
        sel->io.check("k1t", true);
        a.p_cnt = sel->prev.cnt; a.p_val = sel->prev.val; a.p_stride = sel->prev.stride; a.beam_in = P.beam_in;
        a.xok = sel->io.xok; a.perm_inv = L.perm_inv;
        a.out_idx = sel->out.idx; a.out_val = sel->out.val; a.out_cnt = sel->out.cnt; a.done = sel->io.done;
        a.out_stride = sel->out.stride; a.k = P.k;
        a.mult = (P.pp.kind == PP_SIGMOID || P.pp.kind == PP_LP_HINGE) ? 1 : 0;
        if (!items) {
            if (!sel->cand_off || !sel->ncand || P.beam_in > 32u) fail("k1t: the launch cannot derive its items");
            if ((uint64_t)P.nrows * P.cand_stride > 0xFFFFFFFFull) fail("k1t: candidate buffer exceeds 2^32 floats; lower max_batch_rows");
            a.p_idx = sel->prev.idx; a.x_row_ptr = X.row_ptr + P.row0; a.cand_stride = P.cand_stride; a.cand_off = sel->cand_off; a.ncand = sel->ncand;
        }
        a.rest_q = sel->io.rest_q; a.rest_cnt = sel->io.rest_cnt;
    }
    const dim3 grid((a.n_vblocks + 3u) / 4u), block(256);
#define XRL_K1T_L(GG, NN, BB, SS) do { \
        if (ppc) { if (lk) hipLaunchKernelGGL((k1t_kernel<GG, NN, 1, 2, BB, SS>), grid, block, 0, s, a); else hipLaunchKernelGGL((k1t_kernel<GG, NN, 1, 0, BB, SS>), grid, block, 0, s, a); } \
        else     { if (lk) hipLaunchKernelGGL((k1t_kernel<GG, NN, 0, 2, BB, SS>), grid, block, 0, s, a); else hipLaunchKernelGGL((k1t_kernel<GG, NN, 0, 0, BB, SS>), grid, block, 0, s, a); } } while (0)
#define XRL_K1T(GG, NN) do { if (buf) XRL_K1T_L(GG, NN, true, false); else XRL_K1T_L(GG, NN, false, false); } while (0)
#define XRL_K1T_S(NN) do { if (sel) { if (buf) XRL_K1T_L(32, NN, true, true); else XRL_K1T_L(32, NN, false, true); } else XRL_K1T(32, NN); } while (0)
    if (g == 8) XRL_K1T(8, 1);
    else if (g == 16) XRL_K1T(16, 1);
    else if (nr == 1) XRL_K1T_S(1);
    else if (nr == 2) XRL_K1T_S(2);
    else if (nr == 3) XRL_K1T_S(3);
    else XRL_K1T_S(4);
#undef XRL_K1T_S
#undef XRL_K1T
#undef XRL_K1T_L
    XRL_LAUNCH_CHECK();
}

}  // namespace xrl
