// The two counting sorts of the beam search (gfx950, LDS atomics only): the layer's work items by tile, and the queries of a row batch
// by the best parent of their beam, so that what shares weights runs on one XCD at about the same time.
#include <hip/hip_runtime.h>

#include "xrl_kernels.h"
#include "xrl_items.h"

namespace xrl {

// ---------------------------------------------------------------------------------------------
// Item ordering: counting sort of the layer's item descriptors by tile id, so that the wavefronts
// working on one tile run back to back on ONE XCD and find the tile's bitmap / rows / entries in
// that XCD's L2 instead of HBM (the reference sorts its (query, chunk) pairs by chunk for the same
// reason, inference.hpp:991-993).  Device-scope atomics are slow across the 8 XCDs, so the sort
// uses only LDS atomics: per-block LDS histograms -> per-(block, tile) offsets -> the shared
// single-block scan of the tile totals (launch_block_scan) -> LDS-ranked scatter.  Order
// inside a tile is arbitrary; results do not depend on it.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kSortChunk = 8192;    // item slots per block

__global__ void __launch_bounds__(256)
sort_hist_kernel(const ItemDesc* __restrict__ items, uint64_t n_slots, const uint32_t* __restrict__ n_dev, uint32_t T, uint32_t* __restrict__ H) {
    extern __shared__ uint32_t hist[];
    if (n_dev) n_slots = min(n_slots, (uint64_t)*n_dev);          // compacted list: only its first *n_dev slots are items
    if ((uint64_t)blockIdx.x * kSortChunk >= n_slots) return;      // (the later kernels skip this block's histogram as well)
    for (uint32_t t = threadIdx.x; t < T; t += 256) hist[t] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kSortChunk;
    for (uint32_t i = threadIdx.x; i < kSortChunk && base + i < n_slots; i += 256) {
        const uint32_t tile = items[base + i].tile;
        if (tile != kNoTile) atomicAdd(&hist[tile], 1u);
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < T; t += 256) H[(size_t)blockIdx.x * T + t] = hist[t];
}

// per tile: exclusive running sum over blocks (in place), total per tile
__global__ void __launch_bounds__(256)
sort_colsum_kernel(uint32_t* __restrict__ H, uint32_t B, const uint32_t* __restrict__ n_dev, uint32_t T, uint32_t* __restrict__ total) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= T) return;
    if (n_dev) B = min(B, (uint32_t)(((uint64_t)*n_dev + kSortChunk - 1) / kSortChunk));
    uint32_t run = 0;
    for (uint32_t b = 0; b < B; ++b) { const uint32_t c = H[(size_t)b * T + t]; H[(size_t)b * T + t] = run; run += c; }
    total[t] = run;
}

__global__ void __launch_bounds__(256)
sort_scatter_kernel(const ItemDesc* __restrict__ items, uint64_t n_slots, const uint32_t* __restrict__ n_dev, uint32_t T, const uint32_t* __restrict__ H,
                    const uint32_t* __restrict__ start, ItemDesc* __restrict__ sorted) {
    extern __shared__ uint32_t pos[];
    if (n_dev) n_slots = min(n_slots, (uint64_t)*n_dev);
    if ((uint64_t)blockIdx.x * kSortChunk >= n_slots) return;
    for (uint32_t t = threadIdx.x; t < T; t += 256) pos[t] = start[t] + H[(size_t)blockIdx.x * T + t];
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kSortChunk;
    for (uint32_t i = threadIdx.x; i < kSortChunk && base + i < n_slots; i += 256) {
        const ItemDesc d = items[base + i];
        if (d.tile != kNoTile) sorted[atomicAdd(&pos[d.tile], 1u)] = d;
    }
}

uint32_t sort_max_tiles() { return 36864; }   // LDS histogram: 4 B per tile, <= 144 KiB
size_t sort_hist_bytes(uint64_t n_slots, uint32_t T) { return ((n_slots + kSortChunk - 1) / kSortChunk) * (size_t)T * 4; }

void launch_sort_items(const LayerDev& L, uint64_t n_slots, const void* items, void* sorted, uint32_t* H,
                       uint32_t* start /*[n_tiles+1]*/, hipStream_t s, const uint32_t* n_dev) {
    if (n_slots == 0) return;
    const uint32_t T = L.n_tiles;
    if (T > sort_max_tiles()) fail("sort_items: too many tiles for the LDS histogram");
    const uint32_t B = (uint32_t)((n_slots + kSortChunk - 1) / kSortChunk);
    const size_t lds = (size_t)T * 4;
    if (lds > 48 * 1024) {   // per DEVICE attribute: set on every large launch (a per-thread cache would miss a second GPU)
        XRL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&sort_hist_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        XRL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&sort_scatter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    hipLaunchKernelGGL(sort_hist_kernel, dim3(B), dim3(256), lds, s, static_cast<const ItemDesc*>(items), n_slots, n_dev, T, H);
    hipLaunchKernelGGL(sort_colsum_kernel, dim3((T + 255) / 256), dim3(256), 0, s, H, B, n_dev, T, start);
    launch_block_scan(start, T, s);
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(B), dim3(256), lds, s, static_cast<const ItemDesc*>(items), n_slots, n_dev, T, H,
                       start, static_cast<ItemDesc*>(sorted));
    XRL_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// Query ordering for a query-stationary layer (K1Q): counting sort of the QUERIES by the best parent of their beam
// (beam slot 0 = the parent whose children a query most likely keeps), written as a permutation.  K1Q then runs query perm[i] in
// launch slot i and hands every XCD a CONTIGUOUS range of slots (xrl_k1q.hip), so that the queries of one region of the tree -- which
// share most of their beam parents and, on topical data, many of their features -- request their (feature, parent) weight segments
// through the same L2 at about the same time.  The reference orders its (query, chunk) work by chunk for the same reason
// (inference.hpp:969-993).  Results do not depend on the order: every query writes to its own row of the output.
// Same scheme as the item sort: per-block LDS histograms, per-(block, key) offsets, LDS-ranked scatter.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kQSortChunk = 2048;   // queries per block

__device__ __forceinline__ uint32_t qsort_key(const uint32_t* __restrict__ p_idx, const uint32_t* __restrict__ p_cnt, uint32_t p_stride, uint32_t q, uint32_t T) {
    return p_cnt[q] ? min(p_idx[(size_t)q * p_stride], T - 1u) : T - 1u;
}

__global__ void __launch_bounds__(256)
qsort_hist_kernel(const uint32_t* __restrict__ p_idx, const uint32_t* __restrict__ p_cnt, uint32_t p_stride, uint32_t nrows, uint32_t T, uint32_t* __restrict__ H) {
    extern __shared__ uint32_t hist[];
    for (uint32_t t = threadIdx.x; t < T; t += 256) hist[t] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kQSortChunk;
    for (uint32_t i = threadIdx.x; i < kQSortChunk && base + i < nrows; i += 256) atomicAdd(&hist[qsort_key(p_idx, p_cnt, p_stride, base + i, T)], 1u);
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < T; t += 256) H[(size_t)blockIdx.x * T + t] = hist[t];
}

__global__ void __launch_bounds__(256)
qsort_scatter_kernel(const uint32_t* __restrict__ p_idx, const uint32_t* __restrict__ p_cnt, uint32_t p_stride, uint32_t nrows, uint32_t T,
                     const uint32_t* __restrict__ H, const uint32_t* __restrict__ start, uint32_t* __restrict__ perm) {
    extern __shared__ uint32_t pos[];
    for (uint32_t t = threadIdx.x; t < T; t += 256) pos[t] = start[t] + H[(size_t)blockIdx.x * T + t];
    __syncthreads();
    const uint32_t base = blockIdx.x * kQSortChunk;
    for (uint32_t i = threadIdx.x; i < kQSortChunk && base + i < nrows; i += 256)
        perm[atomicAdd(&pos[qsort_key(p_idx, p_cnt, p_stride, base + i, T)], 1u)] = base + i;
}

uint32_t qsort_max_keys() { return 12288; }   // LDS histogram of 4 B per key: 48 KiB, no opt-in needed
size_t qsort_hist_bytes(uint32_t nrows, uint32_t T) { return ((size_t)(nrows + kQSortChunk - 1) / kQSortChunk) * (size_t)T * 4; }

void launch_sort_queries(BeamDev prev, uint32_t nrows, uint32_t n_keys, uint32_t* H, uint32_t* start /*[n_keys+1]*/, uint32_t* perm, hipStream_t s) {
    if (nrows == 0) return;
    if (n_keys == 0 || n_keys > qsort_max_keys()) fail("sort_queries: key range outside the LDS histogram");
    const uint32_t B = (nrows + kQSortChunk - 1) / kQSortChunk;
    const size_t lds = (size_t)n_keys * 4;
    hipLaunchKernelGGL(qsort_hist_kernel, dim3(B), dim3(256), lds, s, prev.idx, prev.cnt, prev.stride, nrows, n_keys, H);
    hipLaunchKernelGGL(sort_colsum_kernel, dim3((n_keys + 255) / 256), dim3(256), 0, s, H, B, nullptr, n_keys, start);
    launch_block_scan(start, n_keys, s);
    hipLaunchKernelGGL(qsort_scatter_kernel, dim3(B), dim3(256), lds, s, prev.idx, prev.cnt, prev.stride, nrows, n_keys, H, start, perm);
    XRL_LAUNCH_CHECK();
}

}  // namespace xrl
