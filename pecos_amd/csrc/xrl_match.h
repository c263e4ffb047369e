// K14 (xrl_match.hip): a matching matrix built in HBM -- the union of the patterns of several CSR operands of one shape -- and the two
// small kernels the resident single-layer predict needs around a beam that lives in HBM: the candidate bound and the fill_ones beam.
// The rules are stated in include/xrl_abi.h at xrl_smat_pattern_union_device and xrl_single_layer_predict_device.
#pragma once
#include <vector>

#include "xrl_kernels.h"

namespace xrl {

// CAP: the most stored entries, over all operands, of an output row the LDS form serves: CAP column ids of 4 bytes = 4 KiB per
// wavefront.  Rows above it go through the segmented sort in HBM.  Which form serves a row follows from its entry count alone.
constexpr uint32_t kMatchCap = 1024;
// scratch of one batch of big-form rows per entry: two 4-byte sort keys
constexpr uint64_t kMatchBigBytesPerEntry = 8;

struct MatchCounters { uint64_t lds_rows = 0, big_rows = 0, read = 0, written = 0; };

// The union of the patterns of ops (CSR views of rows x cols on the current device; values are never read; nnz bounds every row span):
// out <- a CSR with a 1.0f wherever an operand stores an entry, every row strictly ascending.  Enqueues on s and synchronises it.  Fails
// (message starts with `what`) when an operand stores a column id that is not below cols, or a row holds 2^31 entries or more.
void pattern_union_device(const char* what, const std::vector<QueriesDev>& ops, uint32_t rows, uint32_t cols, hipStream_t s, DevCsr& out, MatchCounters& c);

// Does R (CSR view; same shape and device as Y: the callers check it) store exactly Y's entries and no value below 0?  status[0] <- 0 yes,
// 1 the row pointers differ, 2 the column ids differ, 3 a value of R is below 0 (-0.0 and NaN are not) -- the first of these that
// check_relevance meets; status[1] <- the first row that offends so.  One pass (a wavefront per row), one 8-byte readback, one
// synchronise of s.  Every row span is clamped to both matrices' nnz.
void check_relevance_device(const QueriesDev& Y, const QueriesDev& R, hipStream_t s, uint64_t status[2]);

// A fixed-stride beam in HBM (idx [rows * stride], cnt [rows]; a count above the stride reads as the stride) against a layer's child
// ranges (chunk_col [n_parents + 1]): the largest per-row sum over the listed parents of their child counts, every occurrence of a
// repeated parent counted.  One 8-byte readback, one synchronise of s.  A parent id that is not below n_parents is never followed:
// bad_parent <- true and the return value is the largest such id.
uint64_t beam_cand_bound_device(const uint32_t* idx, const uint32_t* cnt, uint32_t stride, uint32_t rows, const uint32_t* chunk_col, uint32_t n_parents,
                                hipStream_t s, bool& bad_parent);

// the beam of fill_ones(rows, n_parents): every parent in every row, score 1
void fill_ones_beam_device(uint32_t* idx, float* val, uint32_t* cnt, uint32_t rows, uint32_t n_parents, hipStream_t s);

// xrl_debug_match_forms' last word (xrl_match_abi.cpp): the candidate bound the last resident single-layer predict sized its workspace with
void note_cand_bound(uint64_t bound);

}  // namespace xrl
