// The tile format's prolongation on gfx950: child-block offsets and the work items of xrl_items.h that K1 / K1T / K1G consume.
//   K0  k0_prolongate   prolongate_predictions               inference.hpp:1155-1219
//   K0b k0b_remaining   the same for the later beam slots of the queries a bound-pruned layer's first stage left unfinished
#include <hip/hip_runtime.h>

#include "xrl_kernels.h"
#include "xrl_items.h"

namespace xrl {

// ---------------------------------------------------------------------------------------------
// K0: one thread per query.  Besides the child-block offsets (prolongate) it writes one 32-byte
// ITEM DESCRIPTOR per (query, beam slot, tile-in-parent) so that K1 starts from a single coalesced
// load instead of a chain of dependent lookups (beam -> parent -> tile range -> offsets).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k0_prolongate(const uint32_t* __restrict__ chunk_col, const uint32_t* __restrict__ ptile,
              const TileDesc* __restrict__ tiles, uint32_t nrows, uint32_t beam_in, uint32_t item_ranks, uint32_t TT, uint32_t cand_stride,
              int implicit_root, const uint32_t* __restrict__ p_idx, const float* __restrict__ p_val,
              const uint32_t* __restrict__ p_cnt, uint32_t p_stride, uint32_t* __restrict__ cand_off,
              uint32_t* __restrict__ ncand, ItemDesc* __restrict__ items, const uint64_t* __restrict__ x_row_ptr) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= nrows) return;
    uint64_t xb = 0; uint32_t xl = 0;
    if (x_row_ptr) { xb = x_row_ptr[q]; xl = (uint32_t)(x_row_ptr[q + 1] - xb); }
    const uint32_t cnt = implicit_root ? 1u : min(p_cnt[q], beam_in);
    uint32_t off = 0;
    // item descriptors are written for the first `item_ranks` beam slots only (all of them unless the layer runs the bound-pruned
    // two-phase scheme, where the later slots' items are laid out by k0b_remaining for the queries that still need them)
    for (uint32_t j = 0; j < beam_in; ++j) {
        ItemDesc* it = items + ((size_t)q * item_ranks + j) * TT;
        uint32_t nt = 0;
        if (j < cnt) {
            const uint32_t parent = implicit_root ? 0u : p_idx[(size_t)q * p_stride + j];
            const float ps = implicit_root ? 1.0f : p_val[(size_t)q * p_stride + j];
            const uint32_t cb = chunk_col[parent], t0 = ptile[parent];
            nt = ptile[parent + 1] - t0;
            cand_off[(size_t)q * beam_in + j] = off;
            if (j < item_ranks)
                for (uint32_t tt = 0; tt < nt; ++tt)
                    it[tt] = make_item(q, t0 + tt, q * cand_stride + off + (tiles[t0 + tt].col_begin - cb), ps, xb, xl);
            off += chunk_col[parent + 1] - cb;
        }
        if (j < item_ranks) for (uint32_t tt = nt; tt < TT; ++tt) it[tt] = make_item(q, kNoTile, 0u, 0.f, 0, 0u);
    }
    ncand[q] = off;
}

void launch_k0_prolongate(const LayerDev& L, const LayerPlan& P, const QueriesDev& X, BeamDev prev, uint32_t* cand_off,
                          uint32_t* ncand, void* items, hipStream_t s, uint32_t item_ranks) {
    if (P.nrows == 0) return;
    if ((uint64_t)P.nrows * P.cand_stride > 0xFFFFFFFFull) fail("k0: candidate buffer exceeds 2^32 floats; lower max_batch_rows");
    hipLaunchKernelGGL(k0_prolongate, dim3((P.nrows + 255) / 256), dim3(256), 0, s, L.chunk_col, L.ptile, L.tiles,
                       P.nrows, P.beam_in, std::min(item_ranks, P.beam_in), L.max_tiles_per_parent, P.cand_stride, P.implicit_root, prev.idx, prev.val,
                       prev.cnt, prev.stride, cand_off, ncand, static_cast<ItemDesc*>(items),
                       X.dense ? nullptr : X.row_ptr + P.row0);
    XRL_LAUNCH_CHECK();
}
size_t k0_item_bytes() { return sizeof(ItemDesc); }

// Bound-pruned layers, second phase: the items of beam slots >= first_rank, for the queries whose first phase did NOT already
// prove its top-k final (done[q] == 0), appended to a compact list (one atomicAdd per wavefront).
__global__ void __launch_bounds__(256)
k0b_remaining(const uint32_t* __restrict__ chunk_col, const uint32_t* __restrict__ ptile, const TileDesc* __restrict__ tiles,
              uint32_t nrows, uint32_t beam_in, uint32_t first_rank, uint32_t end_rank, uint32_t cand_stride, const uint32_t* __restrict__ p_idx,
              const float* __restrict__ p_val, const uint32_t* __restrict__ p_cnt, uint32_t p_stride, const uint32_t* __restrict__ cand_off,
              const uint32_t* __restrict__ done, ItemDesc* __restrict__ items, uint32_t* __restrict__ n_items,
              const uint64_t* __restrict__ x_row_ptr) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = q < nrows && !done[q];
    const uint32_t cnt = live ? min(min(p_cnt[q], beam_in), end_rank) : 0u;      // slots [first_rank, end_rank) of the unfinished queries
    uint32_t n = 0;
    for (uint32_t j = first_rank; j < cnt; ++j) { const uint32_t parent = p_idx[(size_t)q * p_stride + j]; n += ptile[parent + 1] - ptile[parent]; }
    uint32_t incl = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, d, 64); if (lane >= d) incl += y; }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
    uint32_t base = 0;
    if (lane == 63 && total) base = atomicAdd(n_items, total);
    base = (uint32_t)__shfl((int)base, 63, 64) + incl - n;
    if (n == 0) return;
    uint64_t xb = 0; uint32_t xl = 0;
    if (x_row_ptr) { xb = x_row_ptr[q]; xl = (uint32_t)(x_row_ptr[q + 1] - xb); }
    for (uint32_t j = first_rank; j < cnt; ++j) {
        const uint32_t parent = p_idx[(size_t)q * p_stride + j];
        const float ps = p_val[(size_t)q * p_stride + j];
        const uint32_t cb = chunk_col[parent], t0 = ptile[parent], nt = ptile[parent + 1] - t0;
        const uint32_t off = cand_off[(size_t)q * beam_in + j];
        for (uint32_t tt = 0; tt < nt; ++tt)
            items[base++] = make_item(q, t0 + tt, q * cand_stride + off + (tiles[t0 + tt].col_begin - cb), ps, xb, xl);
    }
}

// The same from the LIST of unfinished queries the first stage wrote (rest_q[0 .. *rest_cnt), any order): a small fixed grid, each wavefront takes
// GROUPS of 64 / lpq listed queries (wavefront-stride loop over the device-side count), lpq = min(slots per query, 64) lanes per query, a lane on the
// beam slots first_rank + its position, + lpq, ...; one prefix sum over the lanes' tile counts and ONE atomicAdd on n_items per group -- the
// returning atomics on that one word are what the batch-sized kernel spends its time on (one per wavefront that holds an unfinished query).
// The work is in proportion to the list, not to the batch.
__global__ void __launch_bounds__(256)
k0b_remaining_list(const uint32_t* __restrict__ chunk_col, const uint32_t* __restrict__ ptile, const TileDesc* __restrict__ tiles,
                   uint32_t nrows, uint32_t beam_in, uint32_t first_rank, uint32_t end_rank, uint32_t cand_stride, const uint32_t* __restrict__ p_idx,
                   const float* __restrict__ p_val, const uint32_t* __restrict__ p_cnt, uint32_t p_stride, const uint32_t* __restrict__ cand_off,
                   const uint32_t* __restrict__ rest_q, const uint32_t* __restrict__ rest_cnt, uint32_t lpq, ItemDesc* __restrict__ items,
                   uint32_t* __restrict__ n_items, const uint64_t* __restrict__ x_row_ptr) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave0 = blockIdx.x * 4u + (threadIdx.x >> 6), n_waves = gridDim.x * 4u;
    const uint32_t nq = min(*rest_cnt, nrows);                                   // (a query is listed at most once)
    const uint32_t qpw = 64u / lpq, qi = lane / lpq, j0 = first_rank + lane % lpq;
    for (uint32_t g = wave0; g * qpw < nq; g += n_waves) {
        const uint32_t i = g * qpw + qi;
        uint32_t q = (qi < qpw && i < nq) ? rest_q[i] : nrows;
        const bool live = q < nrows;
        if (!live) q = 0;
        const uint32_t cnt = live ? min(min(p_cnt[q], beam_in), end_rank) : 0u;  // slots [first_rank, end_rank) of the query
        uint32_t n = 0;
        for (uint32_t j = j0; j < cnt; j += lpq) { const uint32_t parent = p_idx[(size_t)q * p_stride + j]; n += ptile[parent + 1] - ptile[parent]; }
        uint32_t incl = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, d, 64); if (lane >= (uint32_t)d) incl += y; }
        const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
        if (total == 0) continue;
        uint32_t base = 0;
        if (lane == 63u) base = atomicAdd(n_items, total);
        base = (uint32_t)__shfl((int)base, 63, 64) + incl - n;
        uint64_t xb = 0; uint32_t xl = 0;
        if (n != 0 && x_row_ptr) { xb = x_row_ptr[q]; xl = (uint32_t)(x_row_ptr[q + 1] - xb); }
        for (uint32_t j = j0; n != 0 && j < cnt; j += lpq) {
            const uint32_t parent = p_idx[(size_t)q * p_stride + j];
            const float ps = p_val[(size_t)q * p_stride + j];
            const uint32_t cb = chunk_col[parent], t0 = ptile[parent], nt = ptile[parent + 1] - t0;
            const uint32_t off = cand_off[(size_t)q * beam_in + j];
            for (uint32_t tt = 0; tt < nt; ++tt)
                items[base++] = make_item(q, t0 + tt, q * cand_stride + off + (tiles[t0 + tt].col_begin - cb), ps, xb, xl);
        }
    }
}

void launch_k0b_remaining(const LayerDev& L, const LayerPlan& P, const QueriesDev& X, BeamDev prev, const uint32_t* cand_off, const Stage& st, void* items, hipStream_t s) {
    if (P.nrows == 0) return;
    const StageLinks& io = st.io; const uint32_t first_rank = st.slot_begin, end_rank = st.slot_end;
    io.check("k0b", false);
    if (io.rest_q) {   // (*io.n_items was zeroed together with *io.rest_cnt, before the first stage: StageLinks)
        const uint32_t hi = std::min(P.beam_in, end_rank);
        const uint32_t lpq = std::max(1u, std::min(hi > first_rank ? hi - first_rank : 1u, 64u));   // lanes per listed query: its slots, at most a wavefront
        hipLaunchKernelGGL(k0b_remaining_list, dim3(std::min<uint32_t>((P.nrows + 3u) / 4u, 512u)), dim3(256), 0, s, L.chunk_col, L.ptile, L.tiles, P.nrows, P.beam_in,
                           first_rank, end_rank, P.cand_stride, prev.idx, prev.val, prev.cnt, prev.stride, cand_off, io.rest_q, io.rest_cnt, lpq, static_cast<ItemDesc*>(items),
                           io.n_items, X.dense ? nullptr : X.row_ptr + P.row0);
        XRL_LAUNCH_CHECK();
        return;
    }
    XRL_HIP(hipMemsetAsync(io.n_items, 0, 4, s));
    hipLaunchKernelGGL(k0b_remaining, dim3((P.nrows + 255) / 256), dim3(256), 0, s, L.chunk_col, L.ptile, L.tiles, P.nrows, P.beam_in, first_rank, end_rank,
                       P.cand_stride, prev.idx, prev.val, prev.cnt, prev.stride, cand_off, io.done, static_cast<ItemDesc*>(items), io.n_items,
                       X.dense ? nullptr : X.row_ptr + P.row0);
    XRL_LAUNCH_CHECK();
}

}  // namespace xrl
