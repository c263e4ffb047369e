// K1: the tile-format layer product of the XR-Linear beam search, hand-written for gfx950 (CDNA4, 64-wide wavefronts).
//
//   K1 k1_kernel       compute_sparse_predictions + chunk_ops + transform + combine
//                                                           inference.hpp:925-1007, 769-839, 506-518,
//                                                           1360-1384, PostProcessor :192-240
//
// Arithmetic contract (verified bit-for-bit against the compiled reference, see oracle/):
// every output column accumulates fl32(acc + fl32(x_f * w)) over matched features in ASCENDING
// feature id, bias last (sparse X) / first (dense X); no FMA anywhere (built with
// -ffp-contract=off and explicit __fmul_rn/__fadd_rn); transforms in fp64 then rounded to fp32.
//
// Work decomposition: one ITEM = (query, beam parent, column tile).  A wavefront carries 64/G
// items, G lanes each ("wavefront-segmented"): the G lanes probe G consecutive query features
// per step against the tile's rank-bitmap (one 8-byte load per probe, coalesced x reads), hits are
// compacted IN ORDER into a small per-item LDS FIFO with a segmented ballot/popcount, and the
// FIFO is drained row by row with the G lanes striding over the row's entries (distinct output
// columns -> no conflicts), accumulators living in LDS.  Rows are drained in feature order, so
// the per-column summation order is exactly the reference's.  (Up to the FIFO: the tile walk of xrl_items.h, shared with K1T.)
//
// What bounds K1 on MI355X (profiles/): not HBM bytes and, since the drain was rewritten, not
// VALU issue (50-65 % busy) but the stream of 128-byte lines its 8-byte gathers request from the L2 -- hence one
// 4-byte packed extent per row, rows placed so that none straddles an extra line, bitmap words that return the
// first row's extent with the probe, lanes past a unit's end re-reading its first entry.
#include <hip/hip_runtime.h>

#include "xrl_device.h"
#include "xrl_kernels.h"
#include "xrl_items.h"

namespace xrl {

struct K1Args {
    LayerDev L;
    QueriesDev X;
    const ItemDesc* items;
    const uint32_t* n_items;     // device count of (tile-sorted, all active) items, or nullptr: natural order
    float* cand;
    uint64_t n_slots;
    uint32_t row0, acc_stride;
    int pp_kind, pp_p, first_layer;
    int bias_first;              // sparse X, HASH_CHUNKED arithmetic: accumulators start at the bias product, nothing is added at the end
    int ablate;                  // debug: phase-skipping mask for timing ablations (0 in production)
    uint32_t lds_per_wave;       // bytes of dynamic LDS owned by each wavefront of a block
    uint32_t n_vblocks;          // number of wavefront-sized work blocks
    unsigned long long* phase;   // debug (ablate bit 6): per-phase cycle totals [prologue, fill, D1, D3, epilogue, waves]
    uint32_t* fb_out;            // pruning feedback: the launch's item count (a later stage of a bound-pruned layer) goes to this host-visible word
    uint32_t stride_vblocks;     // k1_list_kernel: the grid is a fixed number of wavefronts, each walks the list's work blocks with this stride
};

template <int G, int PPC, class ACC>
__device__ __forceinline__ void k1_epilogue(const K1Args& a, const ItemDesc& it, const TileDesc& td, int lig, ACC&& acc_at,
                                            bool add_bias) {
    // every column's accumulator becomes its score (finish_score) in the child block
    if (it.tile == kNoTile || (a.ablate & 16)) return;
    float* __restrict__ out = a.cand + it.out_off;
    const float* __restrict__ bp = a.L.bias_prod + td.col_begin;
    if (a.ablate & 8) {   // debug: no transform
        for (uint32_t c = lig; c < td.ncols; c += G) {
            const float acc = add_bias ? __fadd_rn(acc_at(c), bp[c]) : acc_at(c);
            out[c] = a.first_layer ? acc : pp_combine(a.pp_kind, acc, it.pscore);
        }
        return;
    }
    for (uint32_t c = lig; c < td.ncols; c += G) out[c] = finish_score<PPC>(acc_at(c), add_bias, bp + c, a.pp_kind, a.pp_p, a.first_layer, it.pscore);
}

// ---- sparse queries: chunk_ops<csr, bin_search>, inference.hpp:769-813 --------------------------
// One wavefront = 64/G items, G lanes each.  Per step every lane fetches U query features
// (U*G consecutive features per item; all x loads, then all bitmap probes, are in flight together),
// hits are compacted IN FEATURE ORDER into a small per-item LDS FIFO (segmented ballot/popcount),
// then one lane per hit fetches the row extent and its first two entries (all hits of all items at
// once), and finally the rows are applied in order with the G lanes on distinct columns.
// NS = number of G-wide UNITS a tile row can span (NS*G >= widest tile of the layer).
struct __attribute__((packed, aligned(4))) RowExt { uint32_t start, end; };

template <int G, int NS> struct K1Cfg {
    static constexpr int W = 64 / G;                      // items per wavefront
#ifndef XRL_K1_FEAT
#define XRL_K1_FEAT 64
#endif
    static constexpr int U = (G >= 16) ? XRL_K1_FEAT / G : 8;     // query features per lane per step (XRL_K1_FEAT per item)
    static constexpr int H = (G > 32) ? 2 * G : 64;       // hit queue depth per item (>= G)
    static constexpr int UH = H * NS;                     // unit queue depth per item
#ifndef XRL_K1_P
#define XRL_K1_P 4
#endif
#ifndef XRL_K1_CLAMP
#define XRL_K1_CLAMP 1
#endif
#ifndef XRL_K1_NB
#define XRL_K1_NB 2
#endif
    static constexpr int P = XRL_K1_P;                    // units per register batch
    static constexpr int NB = XRL_K1_NB;                  // batches in the ring: NB-1 are loading while one is applied
    static constexpr int TAIL = (2 * NB - 1) * P;         // empty units readable past the longest queue
    static constexpr size_t lds_bytes(uint32_t acc_stride) {
        return (size_t)W * (UH + TAIL) * 8 + (size_t)W * H * 8 + (size_t)W * (acc_stride + G) * 4;
    }
};

#ifndef XRL_K1_WPE
#define XRL_K1_WPE 5
#endif
// LK = row lookup: 0 rank-bitmap {bits32, rank} (8 B / 32 features), 1 bucket table + binary search,
//      2 rank-bitmap {bits64, rank, extent of the word's first row} (16 B / 64 features; sparse tiles)
// k1_run: the body of both kernels below.  PERSIST (k1_list_kernel): the wavefront walks a compacted list with a fixed grid; a kernel of its own so
// that the one-block-per-wavefront kernel keeps its registers.
template <int G, int NS, int PPC, bool DENSE, int LK, bool PERSIST>
__device__ __forceinline__ void k1_run(const K1Args& a) {
    constexpr int W = K1Cfg<G, NS>::W, H = K1Cfg<G, NS>::H, UH = K1Cfg<G, NS>::UH, P = K1Cfg<G, NS>::P, U = K1Cfg<G, NS>::U,
                  NB = K1Cfg<G, NS>::NB, TAIL = K1Cfg<G, NS>::TAIL;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
    // the wavefronts of a block are fully independent: each owns a slice of the dynamic LDS
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t vblock0 = blockIdx.x * (blockDim.x >> 6) + wave;
    if (vblock0 >= a.n_vblocks) return;
    unsigned char* smem = smem_all + (size_t)wave * a.lds_per_wave;
    uint2* uq = reinterpret_cast<uint2*>(smem);                        // units {x value, entry start | count << 25}
    uint2* hq = reinterpret_cast<uint2*>(uq + W * (UH + TAIL));                 // hits  {x value, row slot}
    float* acc = reinterpret_cast<float*>(hq + W * H);
    const uint32_t acc_item = a.acc_stride + G;                        // + one private dummy slot per lane

    const int lane = threadIdx.x & 63;
    const int grp = lane / G, lig = lane % G;
#ifdef XRL_K1_PHASE_PROF   // debug build only: per-phase cycle accounting costs ~12 VGPRs
    const bool prof = a.phase != nullptr;
    unsigned long long t_last = prof ? __builtin_readcyclecounter() : 0ull, t_ph[5] = {0, 0, 0, 0, 0};
    auto tick = [&](int ph) { if (prof) { const unsigned long long t = __builtin_readcyclecounter(); t_ph[ph] += t - t_last; t_last = t; } };
#else
    auto tick = [](int) {};
#endif
    auto body = [&](const uint32_t vblock) {
    ItemDesc it;
    if (!fetch_item<W>(a.items, a.n_items, a.n_slots, a.fb_out, vblock, grp, lane, it)) return;
    const bool active = it.tile != kNoTile;
    TileDesc td{};
    uint64_t xe = 0, cur = 0;
    if (active) {
        td = a.L.tiles[it.tile];
        cur = it.x_begin; xe = it.x_begin + it.x_len;   // CSR queries; unused for dense ones
    }
    const uint32_t* __restrict__ rp = a.L.row_ext + td.rowptr_base;
    const Entry* __restrict__ ent = a.L.entries + td.ent_base;
    float* __restrict__ my_acc = acc + (size_t)grp * acc_item;
    uint2* __restrict__ my_hq = hq + (size_t)grp * H;
    uint2* __restrict__ my_uq = uq + (size_t)grp * (UH + TAIL);
    const uint32_t dummy = a.acc_stride + (uint32_t)lig;
    if (DENSE || a.bias_first) {   // bias FIRST: dense queries (inference.hpp:824-830) and chunk_ops<csr, hash> (:716-722); bias_prod already holds 0.0f + bias*w
        const float* __restrict__ bp = a.L.bias_prod + td.col_begin;
        for (uint32_t c = lig; c < td.ncols; c += G) my_acc[c] = a.L.has_bias ? bp[c] : 0.0f;
    } else if (!(a.ablate & 32)) {
        for (uint32_t c = lig; c < td.ncols; c += G) my_acc[c] = 0.0f;   // std::fill(..., 0.0), inference.hpp:964
    }
    wave_sync_lds();
    if (a.ablate & 2) cur = xe;

    const BmWord* __restrict__ bm = a.L.bitmap + (LK != 0 ? 0ull : (uint64_t)(active ? it.tile : 0u) * a.L.nwords);
    const BmWord64* __restrict__ bm64 = a.L.bitmap64 + (LK != 2 ? 0ull : (uint64_t)(active ? it.tile : 0u) * a.L.nwords64);
    const uint32_t* __restrict__ bkt = LK == 1 ? a.L.bucket + (uint64_t)(active ? it.tile : 0u) * (a.L.bk_n + 1u) : nullptr;   // tile-relative row slots
    const uint32_t* __restrict__ ridx_t = a.L.row_idx + td.rowptr_base;                          // the tile's sorted row ids
    const uint64_t xlast = xe > cur ? xe - 1 : 0;                      // a valid x index for clamped loads
    uint32_t nh = 0;                                                   // hits waiting in this item's queue
    tick(0);

    auto drain = [&]() {
        if (a.ablate & 4) { nh = 0; return; }
        tick(1);
        wave_sync_lds();
        // ---- D1: one lane per hit fetches the row extent and cuts the row into units of <= G entries,
        //      written in order (segmented scan of the unit counts when a row can span several units)
        uint32_t nu = 0;                                               // units queued for this item
        for (uint32_t h0 = 0; __any(h0 < nh); h0 += G) {
            const uint32_t h = h0 + lig;
            const bool ok = h < nh;
            const uint2 hv = my_hq[ok ? h : 0u];
            // queue value: the row slot -- or, with 64-feature bitmap words, the packed extent itself unless its length
            // field reads 0x7F, which marks "slot in the low bits" (kRowLookup; extents of 128-entry rows take that route)
            const bool need = ok && (LK != 2 || DENSE || (hv.y >> 25) == 0x7Fu);
            const uint32_t s = need ? ((LK == 2 && !DENSE) ? (hv.y & 0x1FFFFFFu) : hv.y) : 0u;
            const uint32_t rl = rp[s];                                 // unconditional (slot 0 when not needed): packed {offset, length - 1}
            const uint32_t rx = need ? rl : hv.y;
            const uint32_t rs = rx & 0x1FFFFFFu;
            const uint32_t len = ok ? (rx >> 25) + 1u : 0u;
            uint32_t cnt = (NS == 1) ? (len ? 1u : 0u) : min((len + G - 1) / G, (uint32_t)NS);
            uint32_t incl = cnt;
            if (G > 1) {
#pragma unroll
                for (int d = 1; d < G; d <<= 1) { const uint32_t y = __shfl_up(incl, d, G); if (lig >= d) incl += y; }
            }
            const uint32_t base = nu + incl - cnt;
#pragma unroll
            for (int k = 0; k < NS; ++k)
                if ((uint32_t)k < cnt) {
                    const uint32_t n_k = (k == NS - 1) ? len - (uint32_t)k * G : min(len - (uint32_t)k * G, (uint32_t)G);
                    my_uq[base + k] = make_uint2(hv.x, (rs + (uint32_t)k * G) | (n_k << 25));   // offsets < 2^25: xrl_model.cpp max_tile_entries
                }
            nu += (G > 1) ? __shfl(incl, G - 1, G) : incl;
        }
        // every item's queue is read up to the longest queue of the wavefront (+ the prefetch distance):
        // fill the difference with empty units
        uint32_t nu_max = nu;
#pragma unroll
        for (int d = G; d < 64; d <<= 1) nu_max = max(nu_max, (uint32_t)__shfl_xor((int)nu_max, d, 64));
        nu_max = __builtin_amdgcn_readfirstlane(nu_max);
        for (uint32_t j = nu + lig; j < nu_max + (uint32_t)TAIL; j += G) my_uq[j] = make_uint2(0u, 0u);
        wave_sync_lds();
        tick(2);
        // ---- D3: units in order.  Two register batches of P units are in flight: while batch A is
        //      applied the entries of batch B are already loading.  Every load is unconditional and
        //      unclamped (a load behind a per-lane branch makes hipcc wait vmcnt(0) before each one): the
        //      queue ends with 2P empty units and lanes past a unit's end read whatever follows the row
        //      (the entry array is padded) and add it to a private dummy slot.  The lanes of a unit hold
        //      distinct columns.  LDS operations of one wavefront execute in order, so only a compiler
        //      fence separates units.
        const uint2* __restrict__ uqp = my_uq;
        struct Batch { uint32_t xv[P], cn[P]; Entry e[P]; };
        auto load_batch = [&](const uint2* q, Batch& B) {
            uint32_t st[P];
#pragma unroll
            for (int p = 0; p < P; ++p) { const uint2 d = q[p]; B.xv[p] = d.x; st[p] = d.y & 0x1FFFFFFu; B.cn[p] = d.y >> 25; }
#pragma unroll
            for (int p = 0; p < P; ++p) {
#if XRL_K1_CLAMP   // lanes past the unit's end re-read its first entry (no extra cache lines) instead of running on
                B.e[p] = ent[st[p] + ((uint32_t)lig < B.cn[p] ? (uint32_t)lig : 0u)];
#else
                B.e[p] = ent[st[p] + (uint32_t)lig];
#endif
            }
        };
        auto apply_batch = [&](const Batch& B) {
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const float v = __uint_as_float(B.xv[p]);
                const uint32_t ci = (uint32_t)lig < B.cn[p] ? B.e[p].col : dummy;
                my_acc[ci] = __fadd_rn(my_acc[ci], __fmul_rn(v, B.e[p].val));   // scalar * val, then add: no fma (inference.hpp:512-517)
                wave_sync_lds();
            }
        };
        Batch ring[NB];
#pragma unroll
        for (int b = 0; b < NB - 1; ++b) load_batch(uqp + b * P, ring[b]);
        for (uint32_t i0 = 0; i0 < nu_max; i0 += NB * P) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                load_batch(uqp + (b + NB - 1) * P, ring[(b + NB - 1) % NB]);
                apply_batch(ring[b]);
            }
            uqp += NB * P;
        }
        nh = 0;
        tick(3);
    };

    if (DENSE) {
        // chunk_ops<drm, bin_search>, inference.hpp:815-839: EVERY tile row (except the bias row, which is
        // the last one) is a hit with x value x[row feature]; rows go through the same unit queue.
        const float* __restrict__ xd = a.X.val + ((uint64_t)a.row0 + it.q) * a.X.cols;
        const uint32_t* __restrict__ ridx = a.L.row_idx + td.rowptr_base;
        uint32_t nr = active ? td.nrows : 0u;
        if (active && td.bias_slot != kNoBias) nr -= 1;
        for (uint32_t s0 = 0; __any(s0 < nr); s0 += H) {
            for (uint32_t j = lig; j < (uint32_t)H; j += G) {
                const uint32_t sidx = s0 + j;
                const bool ok = sidx < nr;
                const uint32_t f = ridx[ok ? sidx : 0u];
                const float xval = xd[f < a.X.cols ? f : 0u];
                if (ok) my_hq[j] = make_uint2(__float_as_uint(f < a.X.cols ? xval : 0.0f), sidx);
            }
            nh = s0 < nr ? min((uint32_t)H, nr - s0) : 0u;
            drain();
        }
        k1_epilogue<G, PPC>(a, it, td, lig, [&](uint32_t c) { return my_acc[c]; }, false);
        return;
    }
    uint32_t skip = 0;                 // u-slices of the current step already queued (after an overflow)
    while (__any(cur < xe)) {
        bool overflow = false;
        {
            // ---- load step: U*G consecutive features of the item
            uint32_t f[U]; float v[U];
            load_features<G, U>(a.X.col_idx, a.X.val, cur, xe, xlast, a.L.w_rows, lig, f, v);
            // ---- row lookup: is feature f a row of the tile, and which slot
            bool hit[U]; uint32_t slot[U];      // slot: what goes into the hit queue (row slot; LK 2: extent or marked slot)
            if (LK == 0) {
                if (a.ablate & 1) {   // debug: no probe finds a row
#pragma unroll
                    for (int u = 0; u < U; ++u) f[u] = 0xFFFFFFFFu;
                }
                probe_bitmap32<U>(bm, f, hit, slot, [](const BmWord& w, uint32_t before) { return w.rank + before; });
            } else if (LK == 2) {
                // the word carries the extent of its first row, so only hits on a later row of the word go through the extent table in D1
                probe_bitmap64<U>(bm64, f, hit, slot, [](const BmWord64& w, uint32_t before) { return before == 0u ? w.ext0 : (0xFE000000u | (w.rank + before)); });
            } else {
                // layers whose bitmaps would not fit in HBM: bucket table over feature-id ranges (one 8-byte load), then
                // `bk_levels` branch-free binary-search steps over the tile's sorted row ids (the reference's lookup is a
                // binary search too, inference.hpp:786-803) and one load to confirm the match
                uint32_t hi[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool inr = f[u] != 0xFFFFFFFFu;
                    const RowExt be = *reinterpret_cast<const RowExt*>(bkt + (inr ? (f[u] >> a.L.bk_shift) : 0u));
                    slot[u] = be.start; hi[u] = inr ? be.end : be.start;
                }
                for (uint32_t lv = a.L.bk_levels; lv > 0; --lv) {
                    const uint32_t stp = 1u << (lv - 1);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const uint32_t np = slot[u] + stp;
                        const bool in = np < hi[u];
                        const uint32_t r = ridx_t[in ? np : slot[u]];
                        slot[u] = (in && r <= f[u]) ? np : slot[u];
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) hit[u] = slot[u] < hi[u] && ridx_t[slot[u]] == f[u];
            }
            // ---- queue the hits in feature order; on overflow the queue is drained outside this scope and the step resumed
            overflow = queue_hits<G, U, H>(hit, v, slot, my_hq, grp, lig, nh, skip, cur, xe);
        }
        if (__any(overflow)) drain();
    }
    drain();
    k1_epilogue<G, PPC>(a, it, td, lig, [&](uint32_t c) { return my_acc[c]; }, a.L.has_bias != 0 && !a.bias_first);
#ifdef XRL_K1_PHASE_PROF
    if (prof) {
        tick(4);
        if (lane == 0) { for (int i = 0; i < 5; ++i) atomicAdd(&a.phase[i], t_ph[i]); atomicAdd(&a.phase[5], 1ull); }
    }
#endif
    };
    if constexpr (PERSIST) {
        // A later stage's compacted list usually fills a small part of the worst-case grid (Amazon-670K: 78 k items of 4.4 M slots -- 2.2 M wavefronts
        // that only read the count and leave cost more than the work): a fixed grid of wavefronts walks the list instead (wavefront-uniform loop).
        const uint32_t nb = (*a.n_items + W - 1) / W;
        if (a.fb_out && vblock0 == 0 && lane == 0) *a.fb_out = *a.n_items;          // (also when the list is empty)
        for (uint32_t vb = vblock0; vb < nb; vb += a.stride_vblocks) { body(vb); wave_sync_lds(); }
    } else body(vblock0);
}

template <int G, int NS, int PPC, bool DENSE, int LK>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(XRL_K1_WPE, 8))) k1_kernel(K1Args a) { k1_run<G, NS, PPC, DENSE, LK, false>(a); }

template <int G, int NS, int PPC, int LK>   // sparse queries, a compacted list (a.n_items): what launch_k1 picks for list_grid > 0
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) k1_list_kernel(K1Args a) { k1_run<G, NS, PPC, false, LK, true>(a); }

template <class KERNEL>
static void launch_k1_any(KERNEL kernel, K1Args a, int W, size_t lds_wave, const K1Tune& tune, hipStream_t s, uint32_t list_grid = 0) {
    lds_wave = (lds_wave + (size_t)std::max(0, tune.lds_pad) + 15) & ~(size_t)15;
    int wpb = (tune.wpb == 2 || tune.wpb == 4) ? tune.wpb : 1;
    while (wpb > 1 && lds_wave * wpb > 160 * 1024) wpb >>= 1;
    const size_t lds = lds_wave * wpb;
    if (lds > 160 * 1024) fail("k1: LDS request exceeds 160 KiB");
    if (lds > 48 * 1024)
        XRL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const uint64_t vblocks = (a.n_slots + W - 1) / W;
    const uint64_t blocks = (vblocks + wpb - 1) / wpb;
    if (vblocks > 0x7FFFFFFFull) fail("k1: grid too large; lower max_batch_rows");
    a.lds_per_wave = (uint32_t)lds_wave; a.n_vblocks = (uint32_t)vblocks;
    uint64_t grid = blocks;
    a.stride_vblocks = 0;
    if (list_grid) {   // k1_list_kernel: a fixed grid (a multiple of 8: block b stays on XCD b % 8), never larger than the worst-case one
        grid = std::min<uint64_t>(blocks, ((uint64_t)list_grid + 7) & ~7ull);
        a.stride_vblocks = (uint32_t)(grid * wpb); a.n_vblocks = (uint32_t)std::min<uint64_t>(vblocks, grid * wpb);
    }
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(64 * wpb), lds, s, a);
    XRL_LAUNCH_CHECK();
}

static unsigned long long* g_phase_buf = nullptr;   // debug only (k1_ablate bit 6): one per process
unsigned long long* k1_phase_buffer() {
    if (!g_phase_buf) { XRL_HIP(hipMalloc(&g_phase_buf, 8 * 8)); XRL_HIP(hipMemset(g_phase_buf, 0, 64)); }
    return g_phase_buf;
}
void k1_phase_read(unsigned long long out[8], bool reset) {
    XRL_HIP(hipDeviceSynchronize());
    XRL_HIP(hipMemcpy(out, k1_phase_buffer(), 64, hipMemcpyDeviceToHost));
    if (reset) XRL_HIP(hipMemset(g_phase_buf, 0, 64));
}

int k1_auto_group(const LayerDev& L, const Layer& host, int dense) {
    // lanes per item: a 16- or 32-lane group whose NS slices cover the widest tile row
    (void)host; (void)dense;
    if (L.max_tile_cols <= 8) return 8;
    if (L.max_tile_cols <= 16) return 16;
    return 32;
}

bool launch_k1(const LayerDev& L, const LayerPlan& P, const QueriesDev& X, const void* items, const uint32_t* n_items,
               float* cand, int group, hipStream_t s, uint32_t list_grid) {
    if (P.nrows == 0) return false;
    // K1T (densely held tile rows, accumulators in registers): measured faster on items in QUERY order (a bound-pruned layer's first stage: Amazon-670K
    // 1.010 -> 0.959 ms, Wiki10-31K 0.334 -> 0.286 ms) and slower on tile-sorted lists (Amazon-670K-hard 7.29 -> 8.48 ms: both kernels run at the L1-miss
    // request ceiling of ~80 G requests/s and a 384-byte dense row is 6 requests against ~4 for its entry list) -- tile_rows 1 = query-order launches only, 2 = all
    if ((P.tune.tile_rows >= 2 || (P.tune.tile_rows == 1 && !n_items)) && P.tune.ablate == 0 && k1t_serves(L, X)) { launch_k1t(L, P, X, items, n_items, cand, s); return false; }
    K1Args a;
    a.L = L; a.X = X; a.items = static_cast<const ItemDesc*>(items); a.n_items = n_items; a.cand = cand;
    a.n_slots = (uint64_t)P.nrows * P.beam_in * L.max_tiles_per_parent;
    a.row0 = P.row0; a.pp_kind = P.pp.kind; a.pp_p = P.pp.p; a.first_layer = P.first_layer; a.bias_first = P.bias_first;
    a.acc_stride = L.max_tile_cols | 1u;
    const int ablate = P.tune.ablate;
    a.ablate = ablate & 0xFF;
    // debug: bit 6 = per-phase cycle accounting; bits 8.. select one layer (value layer+1, 0 = every layer)
    a.phase = ((ablate & 64) && ((ablate >> 8) == 0 || (ablate >> 8) == P.layer + 1)) ? k1_phase_buffer() : nullptr;
    a.fb_out = (n_items && P.fb_host && P.layer >= 0 && P.layer < kFbLayers) ? P.fb_host + fb_items_word(P.layer) : nullptr;
    const int ppc = pp_class(P.pp);
    // (the fixed-grid form exists where it keeps everything in registers at 4 wavefronts per SIMD: sparse queries, 16 or 32 lanes per item, the
    //  post-processors of class 0; everything else keeps the worst-case grid)
    const bool persist = n_items != nullptr && list_grid > 0 && ablate == 0 && !X.dense && ppc == 0;
    bool ran_list = false;
#define XRL_K1_PP(GG, NN, DD, LL) do { if (ppc) launch_k1_any(&k1_kernel<GG, NN, 1, DD, LL>, a, 64 / GG, lds, P.tune, s); else launch_k1_any(&k1_kernel<GG, NN, 0, DD, LL>, a, 64 / GG, lds, P.tune, s); } while (0)
#define XRL_K1_LIST(GG, NN, LL) launch_k1_any(&k1_list_kernel<GG, NN, 0, LL>, a, 64 / GG, lds, P.tune, s, list_grid)
#define XRL_K1(GG, NN) do { \
        const size_t lds = K1Cfg<GG, NN>::lds_bytes(a.acc_stride); \
        if (X.dense) XRL_K1_PP(GG, NN, true, 0); \
        else if (L.bucket) XRL_K1_PP(GG, NN, false, 1); \
        else if (L.bitmap64) XRL_K1_PP(GG, NN, false, 2); \
        else XRL_K1_PP(GG, NN, false, 0); } while (0)
#define XRL_K1P(GG, NN) do { \
        if (!persist) { XRL_K1(GG, NN); break; } \
        const size_t lds = K1Cfg<GG, NN>::lds_bytes(a.acc_stride); \
        ran_list = true; \
        if (L.bucket) XRL_K1_LIST(GG, NN, 1); \
        else if (L.bitmap64) XRL_K1_LIST(GG, NN, 2); \
        else XRL_K1_LIST(GG, NN, 0); } while (0)
    // a tile row must fit NS units of `group` lanes; widen a (forced) group that is too narrow
    if (group < 1 || group > 64 || (group & (group - 1))) fail("k1: lanes-per-item must be a power of two in [1, 64]");
    auto max_ns = [](int g) { return g < 8 ? 1u : (g == 32 ? 4u : 2u); };
    auto units = [&](int g) { return (L.max_tile_cols + (uint32_t)g - 1) / (uint32_t)g; };
    while (group < 64 && units(group) > max_ns(group)) group <<= 1;
    const uint32_t ns = units(group);
    switch (group) {
    case 1: XRL_K1(1, 1); break;
    case 2: XRL_K1(2, 1); break;
    case 4: XRL_K1(4, 1); break;
    case 8: if (ns <= 1) XRL_K1(8, 1); else XRL_K1(8, 2); break;
    case 16: if (ns <= 1) XRL_K1P(16, 1); else XRL_K1P(16, 2); break;
    case 32: if (ns <= 1) XRL_K1P(32, 1); else if (ns == 2) XRL_K1P(32, 2); else if (ns == 3) XRL_K1P(32, 3); else XRL_K1P(32, 4); break;
    default: if (ns <= 1) XRL_K1(64, 1); else XRL_K1(64, 2); break;
    }
#undef XRL_K1P
#undef XRL_K1
#undef XRL_K1_LIST
#undef XRL_K1_PP
    return ran_list;
}

}  // namespace xrl
