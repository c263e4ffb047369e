// Output constraint on the device (xrl_constrain.hip): launch interface of the constrained route's pair kernel.  The setter itself
// (set_output_constraint / clear_output_constraint) is declared in xrl_model.h, the view it builds is Layer::view.
#pragma once
#include "xrl_kernels.h"

namespace xrl {

// Which chain K1P evaluates per (query, kept child) pair (xrl_pairs.h)
enum { kChainCsc = 0 /* csc_route_product: CSC handles, and dense X in every layout */, kChainChunked = 1 /* chunked_route_product, sparse X */ };

// K1P (k1p_constrained_kernel), K1C's twin: every candidate K0 laid out over `V` -- the layer's LayerDev with chunk_col / perm_inv pointing at the
// constraint's view -- scored against the CSC copy of W with the arithmetic of the handle's route.  16 lanes per pair.
void launch_k1p_constrained(const LayerDev& V, const uint64_t* col_ptr, const uint32_t* row_idx, const float* val, const LayerPlan& P, int chain,
                            const QueriesDev& X, BeamDev prev, const uint32_t* cand_off, const uint32_t* ncand, float* cand, hipStream_t s);

}  // namespace xrl
