// K15 (xrl_tfidf_train.hip): training of the TF-IDF vectorizer on the device -- document bytes in HBM -> per base vectorizer the
// vocabulary (token bytes -> rank), the document frequency of every n-gram of token ids, the kept features in the reference's order
// (pecos/core/utils/tfidf.hpp:558-594 Tokenizer::train, :452-499 count_ngrams, :871-957 merge_df_chunks) and their idf.
#pragma once
#include <vector>

#include "xrl_common.h"
#include "xrl_tfidf.h"

#include "../../include/xrl_abi.h"   // TfidfBaseVectorizerParam / TfidfVectorizerParam: the reference's structs (tfidf.hpp:66-116, :194-208)

namespace xrl {

// scratch of one batch of documents in the df pass: the sum of the documents' n-gram position bounds stays below this many 16-byte
// keys (512 MiB); a single document above it is a batch of its own.  XRL_TFIDF_TRAIN_SCRATCH_ENTRIES replaces it (tests), and caps
// the first size of the vocabulary pass's table, which then grows.
constexpr uint64_t kTrainScratchEntries = 32ull << 20;
constexpr uint64_t kTrainBatchDocs = 1ull << 22;
// the vocabulary table names a token by (offset of one occurrence in the text) << 24 | length
constexpr uint64_t kTrainMaxTextBytes = 1ull << 40;
constexpr uint64_t kTrainMaxTokenBytes = (1ull << 24) - 1;
constexpr int kTrainKeyBits = 128;

// counters of xrl_debug_tfidf_train_forms
struct TrainForms {
    uint64_t vocab_docs = 0;                 // documents the vocabulary pass walked (one form: nothing is kept per document)
    uint64_t df_lds = 0, df_global = 0;      // (document, base) segments of the df pass by form
    uint64_t batches = 0;                    // df batches over all bases
    uint64_t distinct_tokens = 0;            // over all distinct tokenizers
    uint64_t distinct_ngrams = 0;            // before the filter, over all bases
    uint64_t long_compares = 0;              // byte comparisons of tokens of more than 8 bytes in the vocabulary pass
    uint64_t table_grows = 0;                // reruns of the vocabulary pass with a larger table
    uint64_t us_vocab = 0, us_df = 0, us_order = 0;   // wall microseconds: vocabulary passes (host sort and table build included), df batches, merge + filter + order + idf
};

// the caller's parameters of one base vectorizer as the fields `load` would have read from a folder that states them
inline void set_base_params(TfidfBase& B, const TfidfBaseVectorizerParam& P) {
    B.tok_type = P.tok_type; B.min_ngram = P.min_ngram; B.max_ngram = P.max_ngram; B.max_length = P.max_length; B.norm_p = P.norm_p;
    B.binary = P.binary; B.use_idf = P.use_idf; B.sublinear_tf = P.sublinear_tf;
    B.max_feature = P.max_feature; B.min_df_cnt = P.min_df_cnt; B.max_df_cnt = P.max_df_cnt; B.min_df_ratio = P.min_df_ratio; B.max_df_ratio = P.max_df_ratio;
    B.smooth_idf = P.smooth_idf; B.add_one_idf = P.add_one_idf; B.keep_frequent_feature = P.keep_frequent_feature;
}

// bases[b]'s parameters are set by the caller (set_base_params); the call fills vocab, features, idf, nr_features, sort_shift.  d_text / d_doc_off / d_doc_len
// are device pointers; h_doc_off / h_doc_len the same arrays on the host.  first_bad: the lowest document with char status 1 / 2 (~0: none);
// when one is set nothing was trained.  Synchronises s.
void tfidf_train_device(std::vector<TfidfBase>& bases, const std::vector<TfidfBaseVectorizerParam>& params, const uint8_t* d_text, const uint64_t* d_doc_off,
                        const uint64_t* d_doc_len, const uint64_t* h_doc_off, const uint64_t* h_doc_len, uint64_t nr_doc, hipStream_t s, TrainForms& forms,
                        uint64_t first_bad[2]);

// the filter bounds of merge_df_chunks (tfidf.hpp:875-878): float products, std::round(float)
void tfidf_df_bounds(const TfidfBaseVectorizerParam& p, uint64_t nr_doc, uint64_t& real_min, uint64_t& real_max);
// idf of a feature (tfidf.hpp:955): the double log of a float quotient, clamped at 0, plus add_one, rounded to float once
float tfidf_idf(uint64_t nr_doc, uint64_t df, bool smooth_idf, bool add_one_idf);

}  // namespace xrl
