// The (query, beam slot, tile) work item K0 lays out and K1 / K1T / K1G consume, and the TILE WALK K1 (xrl_k1.hip) and K1T (xrl_k1t.hip)
// share (device code only): an item's G lanes fetch the item, load U*G consecutive query features per step, probe the tile's rank-bitmap,
// and compact the hits IN FEATURE ORDER into the item's LDS queue; each kernel drains that queue its own way and scores the result.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "xrl_device.h"

namespace xrl {

struct alignas(16) ItemDesc {   // 32 bytes; tile == kNoTile: inactive slot
    uint32_t q, tile, out_off; float pscore;
    uint64_t x_begin; uint32_t x_len, pad;   // CSR queries: the query row's range in col_idx / val (saves K1 a dependent lookup)
};
__host__ __device__ inline ItemDesc make_item(uint32_t q, uint32_t tile, uint32_t out_off, float ps, uint64_t xb, uint32_t xl) {
    ItemDesc d; d.q = q; d.tile = tile; d.out_off = out_off; d.pscore = ps; d.x_begin = xb; d.x_len = xl; d.pad = 0u; return d;
}
constexpr uint32_t kNoTile = 0xFFFFFFFFu;

// XCD-aware block remap (blocks b, b+8, b+16, ... run on one XCD): give every XCD a CONTIGUOUS
// range of the tile-sorted work so a tile's data is fetched into one L2 only.  Bijective on [0, nb).
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t nb) {
    const uint32_t xcd = b & 7u, q = nb >> 3, r = nb & 7u;
    const uint32_t base = (xcd < r) ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q;
    return base + (b >> 3);
}

// Item fetch: the item of lane group `grp` of wavefront-sized work block `vblock` (W items per wavefront; an inactive one past the list's
// end), or false when the whole wavefront has nothing to do.  n_items: device count of a tile-sorted, all-active list (it also goes to
// the pruning-feedback word fb_out), or nullptr: natural order over n_slots slots.
template <int W>
__device__ __forceinline__ bool fetch_item(const ItemDesc* __restrict__ items, const uint32_t* __restrict__ n_items, uint64_t n_slots,
                                           uint32_t* fb_out, uint32_t vblock, int grp, int lane, ItemDesc& it) {
    it = make_item(0u, kNoTile, 0u, 0.f, 0, 0u);
    if (n_items) {   // tile-sorted list: every XCD takes a contiguous run of tiles
        const uint32_t n = *n_items, nb = (n + W - 1) / W;
        if (fb_out && vblock == 0 && lane == 0) *fb_out = n;
        if (vblock >= nb) return false;   // a compacted list (later stage of a pruned layer) usually fills a small part of the grid
        { const uint64_t slot = (uint64_t)xcd_remap(vblock, nb) * W + grp; if (slot < n) it = items[slot]; }
    } else {
        const uint64_t slot = (uint64_t)vblock * W + grp;
        if (slot < n_slots) it = items[slot];
    }
    return true;
}

// Load step: U*G consecutive features of the item, lane `lig` of its G lanes taking features cur + u*G + lig.  f[u] = 0xFFFFFFFF for a
// feature past the row's end or >= w_rows (no layer row); xlast is a valid x index of the row.
template <int G, int U>
__device__ __forceinline__ void load_features(const uint32_t* __restrict__ xi, const float* __restrict__ xv, uint64_t cur, uint64_t xe,
                                              uint64_t xlast, uint32_t w_rows, int lig, uint32_t (&f)[U], float (&v)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t t = cur + (uint64_t)(u * G + lig);
        const bool ok = t < xe;
        const uint64_t tc = ok ? t : xlast;          // clamped: the load itself is unconditional
        const uint32_t fi = xi[tc];
        const float vi = xv[tc];
        f[u] = (ok && fi < w_rows) ? fi : 0xFFFFFFFFu;
        v[u] = vi;
    }
}

// Row lookup: is feature f[u] a row of the tile (hit), and which -- row slot = w.rank + before (the set bits below the feature's own);
// qword(w, before) turns that into the kernel's queue word, qw[u].  32-feature words: one 8-byte load per probe.
template <int U, class QWORD>
__device__ __forceinline__ void probe_bitmap32(const BmWord* __restrict__ bm, const uint32_t (&f)[U], bool (&hit)[U], uint32_t (&qw)[U], QWORD&& qword) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool inr = f[u] != 0xFFFFFFFFu;
        const BmWord wi = bm[inr ? (f[u] >> 5) : 0u];
        const uint32_t b = f[u] & 31u;
        hit[u] = inr && ((wi.bits >> b) & 1u);
        qw[u] = qword(wi, (uint32_t)__popc(wi.bits & ((1u << b) - 1u)));
    }
}
// 64-feature words (sparse tiles: few rows per word): one 16-byte load per probe returns the word AND the extent of its first row
template <int U, class QWORD>
__device__ __forceinline__ void probe_bitmap64(const BmWord64* __restrict__ bm64, const uint32_t (&f)[U], bool (&hit)[U], uint32_t (&qw)[U], QWORD&& qword) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool inr = f[u] != 0xFFFFFFFFu;
        const BmWord64 wi = bm64[inr ? (f[u] >> 6) : 0u];
        const uint32_t b = f[u] & 63u;
        const unsigned long long bits = ((unsigned long long)wi.hi << 32) | wi.lo;
        hit[u] = inr && ((bits >> b) & 1ull);
        qw[u] = qword(wi, (uint32_t)__popcll(bits & ((1ull << b) - 1ull)));
    }
}

// Queue the hits of a step in feature order: slice u's hits go to my_hq[nh..] as {x value, qw[u]}, H hits deep.  If an item's queue
// fills up the step is abandoned at slice `skip` and true is returned: the caller drains the queue (outside the step's scope, so the
// step's registers are dead by then; nh = 0 afterwards), re-loads the SAME step and resumes it from that slice.  A completed step
// advances `cur`.  nh (hits waiting) and skip (slices of the current step already queued) start at 0 and live across steps.
template <int G, int U, int H>
__device__ __forceinline__ bool queue_hits(const bool (&hit)[U], const float (&v)[U], const uint32_t (&qw)[U], uint2* __restrict__ my_hq, int grp,
                                           int lig, uint32_t& nh, uint32_t& skip, uint64_t& cur, uint64_t xe) {
    const unsigned long long below = (1ull << lig) - 1ull;
    uint32_t done = skip;
    bool stopped = false;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned long long m = __ballot(hit[u]);
        const unsigned long long gm = (G == 64) ? m : ((m >> (grp * G)) & ((1ull << G) - 1ull));
        const uint32_t cnt = (uint32_t)__popcll(gm);
        if ((uint32_t)u >= done && !stopped) {
            if (nh + cnt <= (uint32_t)H) {
                if (hit[u]) my_hq[nh + (uint32_t)__popcll(gm & below)] = make_uint2(__float_as_uint(v[u]), qw[u]);
                nh += cnt; done = u + 1;
            } else {
                stopped = true;
            }
        }
    }
    if (done == (uint32_t)U) { if (cur < xe) cur += (uint64_t)U * G; skip = 0; } else skip = done;
    return done != (uint32_t)U;
}

// An accumulator becomes a score: bias (sparse X: LAST, inference.hpp:806-811; *bias is read only if add_bias), transform in fp64,
// combine with the parent's score (skipped on the first layer).
template <int PPC>
__device__ __forceinline__ float finish_score(float acc, bool add_bias, const float* __restrict__ bias, int pp_kind, int pp_p, int first_layer,
                                              float pscore) {
    if (add_bias) acc = __fadd_rn(acc, *bias);
    float v = pp_transform<PPC>(pp_kind, pp_p, acc);
    if (!first_layer) v = pp_combine(pp_kind, v, pscore);
    return v;
}

}  // namespace xrl
