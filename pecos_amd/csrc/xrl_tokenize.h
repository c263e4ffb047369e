// K9 (xrl_tokenize.hip): the counting half of the TF-IDF producer on the device -- document bytes in HBM -> per (document, base
// vectorizer) segment the term counts TfidfBase::count appends (ascending feature ids + the base's column offset, counts as floats).
#pragma once
#include <vector>

#include "xrl_common.h"
#include "xrl_tfidf_tables.h"

namespace xrl {

// CAP: the most tokens, and the most n-gram positions, of a segment the LDS form serves.  Two arrays of CAP words (token indices, then
// run heads; feature-id occurrences) = 8 KiB per wavefront: 20 wavefronts (5 per SIMD) share a CU's 160 KiB.  Which form serves a segment
// follows from the document's LENGTH alone (tft::token_bound / occurrence_bound), so the host and the kernel decide alike.
constexpr uint32_t kTokCap = 1024;
// run scratch of one batch of documents: the sum of the segments' occurrence bounds stays below this many (id, count) pairs (256 MiB);
// a single document above it is a batch of its own
constexpr uint64_t kTokScratchEntries = 32ull << 20;
constexpr uint64_t kTokBatchDocs = 1ull << 22;       // ... and a batch holds at most this many documents

// one base vectorizer as K9 sees it: views of its tables in HBM and the parameters of TfidfBase::count
struct TokBase {
    tft::TokenView tv; tft::NgramView gv;
    int tok_type = 10, min_ngram = 1, max_ngram = 1, max_length = -1;
    uint32_t col_off = 0;
};

// whether the global form serves a document of len bytes under base B (the LDS form serves every other one)
XRL_HD bool tok_segment_is_big(int tok_type, int max_length, int min_ngram, int max_ngram, int max_n, uint64_t len) {
    const uint64_t tb = tft::token_bound(tok_type, max_length, len);
    return tb > kTokCap || tft::occurrence_bound(tb, min_ngram, tft::ngram_hi(max_ngram, max_n, tb)) > kTokCap;
}

struct TokCounts {
    DevCsr csr;                                      // ptr: the SEGMENT pointer [nr_doc * nb + 1]; idx / val: feature ids and counts
    uint64_t first_bad[2] = {~0ull, ~0ull};          // the lowest document with status 1 / status 2 (~0: none)
    uint64_t lds_segments = 0, global_segments = 0, batches = 0;
};

// Enqueues on s and synchronises it.  h_doc_len: the lengths on the host when the caller has them (nullptr: read back from d_doc_len).
// d_status [nr_doc] is overwritten: 0, or why the document's row was left empty (1: a stray continuation byte where a character starts --
// the host tokenizer fails; 2: a lead byte followed by too few continuation bytes -- the host's sequential decode takes another path).
void tokenize_count_device(const std::vector<TokBase>& bases, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len,
                           const uint64_t* h_doc_len, uint64_t nr_doc, uint32_t* d_status, hipStream_t s, TokCounts& out);
// row_ptr[r] = seg_ptr[r * nb] for r in [0, rows]
void launch_seg_to_row_ptr(const uint64_t* seg_ptr, uint32_t nb, uint32_t rows, uint64_t* row_ptr, hipStream_t s);

}  // namespace xrl
