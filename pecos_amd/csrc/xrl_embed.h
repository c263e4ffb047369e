// K12 (xrl_embed.hip): the two primitives the label embeddings need on a CSR in HBM (u64 row_ptr, u32 col_idx, f32 val) -- the stable
// transpose (scipy's csr_tocsc) and the row normalisation (l2, l1, max) in sklearn's arithmetic -- and the hstack of CSRs.  The rules are stated
// in include/xrl_abi.h at xrl_label_embedding_device.
#pragma once
#include <vector>

#include "xrl_kernels.h"

namespace xrl {

// CAP: the most entries of an output row of the transpose whose source positions one wavefront sorts in LDS: CAP u32 positions = 4 KiB
// per wavefront, so a CU's 160 KiB is no limit on its occupancy.  Longer rows go through a segmented sort in HBM.
constexpr uint32_t kEmbedCap = 1024;
// rows of this many entries and more are summed by a wavefront (64 squares a step, the adds one chain), shorter ones one per lane
constexpr uint32_t kEmbedWaveRow = 64;
// scratch of a transpose per entry: the scattered positions, and their sorted copy when a row needs the big form; per output row 8 bytes
constexpr uint64_t kEmbedTransposeBytesPerEntry = 8;

// rows with entries only: transposed rows served in LDS / by the big form, normalised rows served one per lane / by a wavefront
struct EmbedForms { uint64_t t_lds = 0, t_big = 0, n_lane = 0, n_wave = 0; };

// out <- A^T (A.cols rows), every output row in source order (source row ascending, stored order inside a source row); duplicates and
// explicit zeros kept.  A: a CSR view with nnz < 2^32.  Fails when an entry of A names a column >= A.cols.  Enqueues on s and synchronises it.
void transpose_device(const char* what, const QueriesDev& A, hipStream_t s, DevCsr& out, EmbedForms& forms);

// out_val[x] <- A.val[x] / ||row|| by the rule R1 (norm = 2: l2), R1a (1: l1) or R1b (3: max); out_val may be A.val (in place).  norm = 3
// fails, before a value is written, on a row whose column ids are not strictly ascending.  Enqueues on s and synchronises it.
void normalize_rows_device(const char* what, const QueriesDev& A, float* out_val, hipStream_t s, EmbedForms& forms, int norm = 2);

// out <- [M0 M1 ...] of CSR views with one row count (the callers check it, and that the widths sum below 2^32).  Enqueues on s and synchronises it.
void hstack_device(const char* what, const std::vector<QueriesDev>& mats, hipStream_t s, DevCsr& out);

}  // namespace xrl
