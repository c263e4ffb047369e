// The host-ABI path of c_xlinear_predict_{csr,drm}_f32 (xrl_host_pipeline.cpp): what the other units of the C surface call.
#pragma once
#include <vector>

#include "xrl_abi_common.h"

namespace xrl {

// c_xlinear_predict_{csr,drm}_f32 behind the exception barrier: one device or the row shards of several, ONE allocator call
void predict_host(void* model, const HostX& x, uint32_t beam, const char* post_processor, uint32_t topk, py_sparse_allocator_t alloc);

// everything the host ABI needs that does not depend on the caller's X, created when a model is loaded from a folder
void warm_handle(Model& m);

// device + pinned host result buffers of the handle for `rows` rows of `k` cells
void reserve_outputs(Model& m, uint32_t rows, uint32_t k);

// X is on the device already: predict all its rows, bring the results to the host, hand them to the allocator as a CSR
void run_and_emit(Model& m, const QueriesDev& X, const PredictOpts& o, py_sparse_allocator_t alloc);

// The row batches of one pipelined call: boundaries rb[0] = 0 <= ... <= rb[n] = rows.  `staged` = staged_upload(x, host_pipeline); a call
// that is not staged is one batch.  Pure host arithmetic (xrl_debug_host_batches exports it for the tests).
bool staged_upload(const HostX& x, int host_pipeline);
std::vector<uint32_t> plan_row_batches(const HostX& x, int host_batch_mb, bool staged);

}  // namespace xrl
