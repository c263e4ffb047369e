// Kernels beside the timed path: a layer's stats (reference-layout bytes, matched work per item) and the step marker of kernel traces.
#include <hip/hip_runtime.h>

#include "xrl_kernels.h"
#include "xrl_items.h"

namespace xrl {

// Profiling aid: with XRL_STEP_MARKER=1 every predict_device call opens with this empty kernel, so that a rocprofv3 kernel trace can be
// cut into steps whatever kernels the layers run (scripts/pmc_traffic.py).  Never launched otherwise.
__global__ void step_marker_kernel() {}
void launch_step_marker(hipStream_t s) {
    hipLaunchKernelGGL(step_marker_kernel, dim3(1), dim3(64), 0, s);
    XRL_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// stats (not on the timed path): algorithmic bytes of the reference layout touched by a layer
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
stats_kernel(const float* __restrict__ chunk_alg, uint32_t nrows, uint32_t beam_in, int implicit_root,
             const uint32_t* __restrict__ p_idx, const uint32_t* __restrict__ p_cnt, uint32_t p_stride,
             const uint32_t* __restrict__ ncand, double* out2) {
    __shared__ double sb[256], sc[256];
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    double b = 0, c = 0;
    if (q < nrows) {
        const uint32_t cnt = implicit_root ? 1u : min(p_cnt[q], beam_in);
        for (uint32_t j = 0; j < cnt; ++j) b += chunk_alg[implicit_root ? 0u : p_idx[(size_t)q * p_stride + j]];
        c = ncand[q];
    }
    sb[threadIdx.x] = b; sc[threadIdx.x] = c;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) { sb[threadIdx.x] += sb[threadIdx.x + st]; sc[threadIdx.x] += sc[threadIdx.x + st]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { atomicAdd(&out2[0], sb[0]); atomicAdd(&out2[1], sc[0]); }
}

// matched work per (query, tile) item, counted by walking the item's query features against the tile's sorted row ids
// (independent of the row lookup structure the layer uses): out[0] items, [1] probes (= query features), [2] matched rows,
// [3] entries of the matched rows, [4] tile columns (scores written), [5] query features x tile columns (dense-format MACs)
__global__ void __launch_bounds__(256)
stats_items_kernel(LayerDev L, QueriesDev X, const ItemDesc* __restrict__ items, uint64_t n_slots, uint32_t row0, double* out6) {
    __shared__ double sh[6][256];
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    double v[6] = {0, 0, 0, 0, 0, 0};
    if (i < n_slots) {
        const ItemDesc it = items[i];
        if (it.tile != kNoTile) {
            const TileDesc td = L.tiles[it.tile];
            const uint32_t* __restrict__ ridx = L.row_idx + td.rowptr_base;
            const uint32_t* __restrict__ rext = L.row_ext + td.rowptr_base;
            uint32_t hits = 0, nx = 0; uint64_t ent = 0;
            if (X.dense) {
                nx = X.cols;
                const uint32_t nr = td.bias_slot != kNoBias ? td.nrows - 1 : td.nrows;
                hits = nr;
                for (uint32_t r = 0; r < nr; ++r) ent += (rext[r] >> 25) + 1u;
            } else {
                nx = it.x_len;
                uint32_t lo = 0;
                for (uint32_t t = 0; t < it.x_len; ++t) {
                    const uint32_t f = X.col_idx[it.x_begin + t];
                    uint32_t a = lo, b = td.nrows;
                    while (a < b) { const uint32_t mid = (a + b) >> 1; if (ridx[mid] < f) a = mid + 1; else b = mid; }
                    lo = a;
                    if (a < td.nrows && ridx[a] == f) { ++hits; ent += (rext[a] >> 25) + 1u; }
                }
            }
            v[0] = 1; v[1] = nx; v[2] = hits; v[3] = (double)ent; v[4] = td.ncols; v[5] = (double)nx * td.ncols;
        }
    }
    for (int k = 0; k < 6; ++k) sh[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) for (int k = 0; k < 6; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x < 6) atomicAdd(&out6[threadIdx.x], sh[threadIdx.x][0]);
}

void launch_stats(const LayerDev& L, const LayerPlan& P, const QueriesDev& X, BeamDev prev, const uint32_t* ncand, const void* items,
                  double* out8, hipStream_t s, uint64_t item_slots) {
    if (P.nrows == 0) return;
    if (ncand)   // (nullptr: only the items of a further item list of the same layer are added)
        hipLaunchKernelGGL(stats_kernel, dim3((P.nrows + 255) / 256), dim3(256), 0, s, L.chunk_alg_bytes, P.nrows,
                           P.beam_in, P.implicit_root, prev.idx, prev.cnt, prev.stride, ncand, out8);
    const uint64_t n_slots = item_slots ? item_slots : (uint64_t)P.nrows * P.beam_in * L.max_tiles_per_parent;
    if (n_slots == 0) return;
    hipLaunchKernelGGL(stats_items_kernel, dim3((uint32_t)((n_slots + 255) / 256)), dim3(256), 0, s, L, X,
                       static_cast<const ItemDesc*>(items), n_slots, P.row0, out8 + 2);
    XRL_LAUNCH_CHECK();
}

}  // namespace xrl
