// K10 (xrl_spgemm.hip): the sparse matrix product Z = A * B on the device, both operands CSR (u64 row_ptr, u32 col_idx, f32 val), with
// the arithmetic of the reference's smat_x_smat (pecos/core/utils/matrix.hpp:1075-1292) bit for bit -- the rule is stated in
// include/xrl_abi.h at xrl_sparse_matmul_device.
#pragma once
#include "xrl_kernels.h"

namespace xrl {

// CAP: the most products (pairs of a stored entry of A's row and a stored entry of the B row it names) of an output row the LDS form
// serves.  Per wavefront: CAP (column, sequence number) keys of 8 bytes + CAP products of 4 bytes = 12 KiB, + 1.1 KiB for one step's
// 64 (offset, B row start, a) triples and the first-touch bitmap: 13.1 KiB, so 12 wavefronts (3 per SIMD) share a CU's 160 KiB.  2048
// would leave 6 per CU (under 2 per SIMD: nothing hides the sort's LDS latency); 512 would send a beam-20 row of a branching-factor-32
// tree to the big form.  Which form serves a row follows from its product count alone (the flops pass).
constexpr uint32_t kSpgemmCap = 1024;
// scratch of one batch of big-form rows per product: two 8-byte sort keys, the product, the head flag and its scan
constexpr uint64_t kSpgemmBigBytesPerProduct = 28;

struct SpgemmOut {
    DevCsr z;                      // the product before eliminate_zeros
    DevCsr e;                      // with eliminate_zeros: the compacted product
    uint64_t lds_rows = 0, big_rows = 0, batches = 0;
};

// A and B: CSR views (the callers check); nnz bounds every row_ptr entry that is read.  Enqueues on s and synchronises it (once when no
// row needs the big form).  A.cols == B.rows is the caller's to check.  Fails when an entry of A names a row B does not have, or a row
// holds 2^31 products or more.
void spgemm_device(const QueriesDev& A, const QueriesDev& B, bool eliminate_zeros, bool sorted_indices, hipStream_t s, SpgemmOut& out);

// fixed-stride result (idx / val [rows * stride], cnt [rows] or nullptr = stride entries in every row; a count above the stride is read
// as the stride) -> CSR with the stored best-first order kept.  Enqueues on s and synchronises it.
void topk_to_csr_device(uint32_t rows, const uint32_t* d_idx, const float* d_val, const uint32_t* d_cnt, uint32_t stride, hipStream_t s, DevCsr& out);

}  // namespace xrl
