/*
 * xrl_abi.h -- C ABI of libxrl_amd.so, the MI355X-native XR-Linear inference library.
 *
 * Part 1 declares, with IDENTICAL names, argument order and meaning, the entry points the
 * reference (amzn/pecos @ 2024-10-20) exports from pecos.core.libpecos_float32 for its
 * XR-Linear inference path, so that the reference's ctypes binding
 * (pecos/core/base.py:799-976 link_xlinear_methods, :1499-1534 link_sparse_operations) can bind
 * this library for that path without change.  Every declaration cites the reference line it
 * replaces.  Part 2 is ADDITIVE (prefix xrl_): error reporting, device selection and a
 * device-resident variant of predict used for benchmarking and multi-GPU sharding.
 *
 * All pointers are plain host pointers unless a parameter is documented as a device pointer.
 * No torch / C++ types appear in any signature.
 */
#ifndef XRL_ABI_H
#define XRL_ABI_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only the entry points declared here are exported */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* ------------------------------------------------------------------------------------------
 * Matrix views handed over by the caller (read-only, valid for the duration of the call).
 * Layout-identical to pecos/core/utils/matrix.hpp:49-71 and the ctypes mirrors in
 * pecos/core/base.py:172-354.
 * ---------------------------------------------------------------------------------------- */
typedef struct {            /* matrix.hpp:49-55  ScipyCsrF32 */
    uint32_t rows, cols;
    uint64_t* row_ptr;      /* [rows+1] */
    uint32_t* col_idx;      /* [nnz], ascending inside a row (base.py:1073-1076) */
    float* val;             /* [nnz] */
} ScipyCsrF32;

typedef struct {            /* matrix.hpp:56-62  ScipyCscF32 */
    uint32_t rows, cols;
    uint64_t* col_ptr;      /* [cols+1] */
    uint32_t* row_idx;      /* [nnz], ascending inside a column */
    float* val;             /* [nnz] */
} ScipyCscF32;

typedef struct {            /* matrix.hpp:63-67  ScipyDrmF32: dense row-major */
    uint32_t rows, cols;
    float* val;             /* [rows*cols] */
} ScipyDrmF32;

typedef struct {            /* matrix.hpp:68-72  ScipyDcmF32: dense column-major */
    uint32_t rows, cols;
    float* val;             /* [rows*cols] */
} ScipyDcmF32;

/* matrix.hpp:47.  The callee passes the ADDRESSES of its three result pointers; the caller
 * allocates indices u32[nnz], indptr u64[rows+1 | cols+1], data f32[nnz] and writes their
 * addresses back (pecos/core/base.py:431-464).  Invoked exactly once per predict call,
 * synchronously on the calling thread, after all device work has completed. */
typedef void (*py_sparse_allocator_t)(bool is_col_major, uint64_t rows, uint64_t cols,
                                      uint64_t nnz, void* indices_pp, void* indptr_pp,
                                      void* data_pp);

/* ------------------------------------------------------------------------------------------
 * Part 1: reference-compatible entry points
 * ---------------------------------------------------------------------------------------- */

/* pecos/core/libpecos.cpp:116-119.  model_path = <model>/ranker (param.json + {d}.model/). */
void* c_xlinear_load_model_from_disk(const char* model_path);

/* libpecos.cpp:121-126.  weight_matrix_type in {0 CSC, 1 HASH_CHUNKED, 2 BINARY_SEARCH_CHUNKED}
 * (pecos/core/base.py:49).  This library has ONE device layout; the value is remembered only so
 * that c_xlinear_get_layer_type answers like the reference. */
void* c_xlinear_load_model_from_disk_ext(const char* model_path, int weight_matrix_type);

/* libpecos.cpp:128-131: load a memory-mapped model folder (*.mmap_store, param.json with is_mmap).
 * lazy_load is accepted and ignored: the model is copied to HBM either way. */
void* c_xlinear_load_mmap_model_from_disk(const char* model_path, const bool lazy_load);

/* libpecos.cpp:133-138: npz model folder -> mmap model folder in the reference's byte layout
 * (readable by the reference's own loader).  Host-only, needs no GPU. */
void c_xlinear_compile_mmap_model(const char* model_path, const char* mmap_model_path);

/* libpecos.cpp:140-143 */
void c_xlinear_destruct_model(void* ptr);

/* libpecos.cpp:147-150; attr in {depth, nr_features, nr_labels, nr_codes} (inference.hpp:2367-2379).
 * Additive attrs: nr_pred_cols (columns of predict()'s CSR), nr_bucket_layers / nr_bitmap64_layers (layers on the bucket / 64-feature-word row lookup),
 * nr_dense_layers (layers that also carry the dense row format), merged01 (1: levels 0 and 1 are also held as one merged dense matrix, which
 * K1Q's fused walk of the two levels reads with one load per feature; built only while its byte offsets fit 32 bits), device, nr_devices. */
uint32_t c_xlinear_get_int_attr(void* ptr, const char* attr);

/* libpecos.cpp:152-156 */
int c_xlinear_get_layer_type(void* ptr, int layer_depth);

/* libpecos.cpp:158-175 (C_XLINEAR_PREDICT).  0 / NULL overrides mean "use the model's per-layer
 * param.json value" (inference.hpp:2055-2058).  `threads` is accepted and ignored (the work runs
 * on the GPU).  Result: CSR rows x nr_labels, rows score-sorted, at most only_topk per row. */
void c_xlinear_predict_csr_f32(void* ptr, const ScipyCsrF32* input_x,
                               const uint32_t overridden_beam_size,
                               const char* overridden_post_processor_str,
                               const uint32_t overridden_only_topk, const int threads,
                               py_sparse_allocator_t pred_alloc);
void c_xlinear_predict_drm_f32(void* ptr, const ScipyDrmF32* input_x,
                               const uint32_t overridden_beam_size,
                               const char* overridden_post_processor_str,
                               const uint32_t overridden_only_topk, const int threads,
                               py_sparse_allocator_t pred_alloc);

/* libpecos.cpp:179-198 (C_XLINEAR_PREDICT_ON_SELECTED_OUTPUTS): scores for a given (query, label)
 * pattern.  The reference only offers this for weight_matrix_type == CSC (inference.hpp:2143-2147) and
 * uses the CSC arithmetic (vector_ops::inner_product, :1018-1078); this library accepts any handle and
 * reproduces that arithmetic and the reference's output order (the walk of
 * prolongate_sparse_predictions, :1302-1358).  Result CSR has selected_outputs_csr's row_ptr. */
void c_xlinear_predict_on_selected_outputs_csr_f32(void* ptr, const ScipyCsrF32* input_x,
                                                   const ScipyCsrF32* selected_outputs_csr,
                                                   const char* overridden_post_processor_str,
                                                   const int threads, py_sparse_allocator_t pred_alloc);
void c_xlinear_predict_on_selected_outputs_drm_f32(void* ptr, const ScipyDrmF32* input_x,
                                                   const ScipyCsrF32* selected_outputs_csr,
                                                   const char* overridden_post_processor_str,
                                                   const int threads, py_sparse_allocator_t pred_alloc);

/* libpecos.cpp:201-235 (C_XLINEAR_SINGLE_LAYER_PREDICT): one layer from caller-owned W / C,
 * optional previous-layer predictions csr_codes (NULL => all-ones N x C.cols, no combine). */
void c_xlinear_single_layer_predict_csr_f32(const ScipyCsrF32* input_x, const ScipyCsrF32* csr_codes,
                                            ScipyCscF32* W, ScipyCscF32* C,
                                            const char* post_processor_str, const uint32_t only_topk,
                                            const int num_threads, const float bias,
                                            py_sparse_allocator_t pred_alloc);
void c_xlinear_single_layer_predict_drm_f32(const ScipyDrmF32* input_x, const ScipyCsrF32* csr_codes,
                                            ScipyCscF32* W, ScipyCscF32* C,
                                            const char* post_processor_str, const uint32_t only_topk,
                                            const int num_threads, const float bias,
                                            py_sparse_allocator_t pred_alloc);

/* libpecos.cpp:237-274 (C_XLINEAR_SINGLE_LAYER_PREDICT_ON_SELECTED_OUTPUTS) */
void c_xlinear_single_layer_predict_on_selected_outputs_csr_f32(const ScipyCsrF32* input_x, const ScipyCsrF32* selected_outputs_csr,
                                                                const ScipyCsrF32* csr_codes, ScipyCscF32* W, ScipyCscF32* C,
                                                                const char* post_processor_str, const int num_threads,
                                                                const float bias, py_sparse_allocator_t pred_alloc);
void c_xlinear_single_layer_predict_on_selected_outputs_drm_f32(const ScipyDrmF32* input_x, const ScipyCsrF32* selected_outputs_csr,
                                                                const ScipyCsrF32* csr_codes, ScipyCscF32* W, ScipyCscF32* C,
                                                                const char* post_processor_str, const int num_threads,
                                                                const float bias, py_sparse_allocator_t pred_alloc);

/* libpecos.cpp:337-355 (C_SPARSE_INNER_PRODUCTS): val[i] = <X[X_row_idx[i],:], W[:,W_col_idx[i]]>,
 * `val` is caller-allocated f32[len] (pecos/core/utils/matrix.hpp:1049-1060). */
void c_sparse_inner_products_csr2csc_f32(const ScipyCsrF32* pX, const ScipyCscF32* pW, uint64_t len,
                                         uint32_t* X_row_idx, uint32_t* W_col_idx, float* val, int threads);
void c_sparse_inner_products_drm2csc_f32(const ScipyDrmF32* pX, const ScipyCscF32* pW, uint64_t len,
                                         uint32_t* X_row_idx, uint32_t* W_col_idx, float* val, int threads);
void c_sparse_inner_products_csr2dcm_f32(const ScipyCsrF32* pX, const ScipyDcmF32* pW, uint64_t len,
                                         uint32_t* X_row_idx, uint32_t* W_col_idx, float* val, int threads);
void c_sparse_inner_products_drm2dcm_f32(const ScipyDrmF32* pX, const ScipyDcmF32* pW, uint64_t len,
                                         uint32_t* X_row_idx, uint32_t* W_col_idx, float* val, int threads);

/* libpecos.cpp:320-334 (C_SPARSE_MATMUL -> smat_x_smat, matrix.hpp:1075-1292): Z = X * Y of two CSR / two CSC matrices through the
 * allocator, computed on the device (K10, csrc/xrl_spgemm.hip) by the rule stated at xrl_sparse_matmul_device below, bit for bit the
 * reference's arrays.  Both operands are uploaded to the calling thread's device (xrl_set_device); the allocator is called once,
 * synchronously, with (is_col_major, X.rows, Y.cols, nnz BEFORE eliminate_zeros), as the reference calls it; the result is copied back.
 * With eliminate_zeros the reference compacts in place inside those arrays, so indices / data past the final indptr[-1] keep what the
 * un-compacted product held at those positions: so do they here.  `threads` is accepted and ignored (the reference's result does not
 * depend on it).  The CSC form is the CSR form of the transposes, xrl_sparse_matmul_device's identity.  Refused, before a GPU is
 * required and with messages that start with the function's name: a null matrix, array or allocator; X.cols != Y.rows (which the
 * reference lets through, matrix.hpp:1085-1087).  Refused by the kernel's first pass: a row of the product that takes 2^31
 * multiplications or more. */
void c_sparse_matmul_csr_f32(const ScipyCsrF32* pX, const ScipyCsrF32* pY, py_sparse_allocator_t pred_alloc,
                             const bool eliminate_zeros, const bool sorted_indices, int threads);
void c_sparse_matmul_csc_f32(const ScipyCscF32* pX, const ScipyCscF32* pY, py_sparse_allocator_t pred_alloc,
                             const bool eliminate_zeros, const bool sorted_indices, int threads);

/* ------------------------------------------------------------------------------------------
 * Part 2: additive entry points (no reference counterpart)
 * ---------------------------------------------------------------------------------------- */

/* The reference throws C++ exceptions through extern "C" (process abort).  This library catches
 * everything; a failed call returns (NULL / 0 / without invoking the allocator) and leaves a
 * message here.  Thread-local; NULL when the last call on this thread succeeded. */
const char* xrl_last_error(void);
void xrl_clear_error(void);

const char* xrl_version(void);
int xrl_device_count(void);            /* hipGetDeviceCount; 0 when no GPU is visible */
int xrl_set_device(int device);        /* device used by subsequent loads on this thread; 0 = ok */

/* Host-only: parse a model folder exactly like the loader does (param.json + uncompressed npz),
 * WITHOUT touching a GPU.  Writes per layer {W.rows, W.cols, nnz(W), C.rows, C.cols, nnz(C)} into
 * out[6*layer ...] (up to cap values) and returns the depth, or -1 on error (see xrl_last_error). */
int xrl_inspect_model(const char* model_path, uint64_t* out, uint32_t cap);

/* Build a model from in-memory CSC layers (same semantics as loading the folder). */
void* xrl_model_create(uint32_t depth, const ScipyCscF32* const* W, const ScipyCscF32* const* C,
                       const float* bias, const uint32_t* only_topk,
                       const char* const* post_processor);

/* Device-resident queries: upload once, predict many times (bench / multi-GPU shards). */
void* xrl_queries_upload_csr(void* model, const ScipyCsrF32* X);
void* xrl_queries_upload_drm(void* model, const ScipyDrmF32* X);
/* Queries that are ALREADY in HBM (a GPU featurizer, a torch tensor): wrap device pointers without copying -- CSR with u64
 * row_ptr[rows+1], u32 col_idx (sorted inside every row, as the reference requires, pecos/core/base.py:1073-1076), f32 val; or a
 * dense row-major f32 matrix.  The handle does not own the arrays; they must stay valid until xrl_queries_free.  This is the
 * hand-off for the callers of SURVEY.md N4 (c_tfidf_predict's output, Text2Text, pecos/apps/text2text/model.py:416-417): no host
 * round trip of X. */
void* xrl_queries_from_device_csr(void* model, uint32_t rows, uint32_t cols, const uint64_t* d_row_ptr,
                                  const uint32_t* d_col_idx, const float* d_val, uint64_t nnz);
void* xrl_queries_from_device_drm(void* model, uint32_t rows, uint32_t cols, const float* d_val);
/* The weighting half of the reference's TF-IDF vectorizer on the device (BaseVectorizer::get_sorted_feature,
 * pecos/core/utils/tfidf.hpp:798-822; c_tfidf_predict, libpecos.cpp:427-445): a device CSR of term COUNTS (column ids ascending
 * inside every row, what the reference's tokenizer + n-gram lookup produce) -> binary / sublinear tf -> x idf (d_idf[cols], NULL =
 * use_idf false) -> l1 / l2 normalisation (norm_p 1 | 2), float32 operation by operation like the reference (bit-identical; sublinear_tf
 * is (float)(log((double)count) + 1.0), the double log of tfidf.hpp:801, rounded once).  The weighted values go to d_out (nnz floats,
 * caller-owned; may alias d_count) or, with d_out == NULL, into a buffer the returned query handle owns; the handle REFERENCES d_row_ptr / d_col_idx (and d_out): keep them
 * alive.  It feeds xrl_predict_device directly: the queries never visit the host. */
void* xrl_queries_tfidf_device(void* model, uint32_t rows, uint32_t cols, const uint64_t* d_row_ptr, const uint32_t* d_col_idx,
                               const float* d_count, uint64_t nnz, const float* d_idf, int binary, int sublinear_tf, int norm_p,
                               float* d_out, void* hip_stream);
/* ---- TF-IDF query producer with the reference's own entry points (libpecos.cpp:398-445 -> pecos/core/utils/tfidf.hpp) --------------
 * c_tfidf_load reads a folder written by the reference's Tfidf.save (one BaseVectorizer folder: tokenizer/{config.json, vocab.txt},
 * vectorizer/{config.json, tfidf-model.txt}; or an ensemble: meta.json + <i>.base/) -- host only.  c_tfidf_predict has the
 * reference's signature and result (host CSR through the allocator, rows = documents, sorted feature ids): the tokenizer and the
 * n-gram lookup run on host threads (`threads`, <= 0: all), their term counts go to the device once, weighting and normalisation run
 * there (K5) and the result is copied back -- bit-identical to the reference, sublinear_tf included.  Training, saving and the
 * *_from_file variants stay the reference's.
 * xrl_tfidf_predict_device is the same pipeline WITHOUT the copy back: it returns a query handle (xrl_queries_free) whose X lives in
 * the HBM of `model`'s device and feeds xrl_predict_device / xrl_predict_device_rows directly -- the call sites SURVEY.md 8f N4 names
 * (pecos/apps/text2text/model.py:416-417: preprocessor.predict -> xlinear predict) without any host round trip of X.
 * xrl_tfidf_counts (host only, tests): the hstacked CSR of term COUNTS the device half starts from. */
void* c_tfidf_load(const char* model_dir);
void c_tfidf_destruct(void* ptr);
void c_tfidf_predict(void* ptr, void* corpus_ptr /* const char** */, const size_t* doc_lens, size_t nr_doc, int threads, py_sparse_allocator_t pred_alloc);
/* libpecos.cpp:413-425: one document per line of a text file (buffer_size only sizes the reference's read chunks: ignored) */
void c_tfidf_predict_from_file(void* ptr, void* corpus_fname_ptr /* const char* */, size_t fname_len, size_t buffer_size, int threads, py_sparse_allocator_t pred_alloc);
uint32_t xrl_tfidf_nr_features(void* ptr);
void* xrl_tfidf_predict_device(void* vectorizer, void* model, void* corpus_ptr /* const char** */, const size_t* doc_lens, size_t nr_doc, int threads);
void xrl_tfidf_counts(void* ptr, void* corpus_ptr /* const char** */, const size_t* doc_lens, size_t nr_doc, int threads, py_sparse_allocator_t alloc);
/* ---- The tokenizer on the device (K9, csrc/xrl_tokenize.hip): term counts from document bytes that are in HBM ----------------------
 * d_text: bytes on `model`'s device, any alignment; document i is d_text[d_doc_off[i], d_doc_off[i] + d_doc_len[i]) -- offsets and
 * lengths apart, so documents may leave gaps, overlap or come in any address order (the host's char** + lengths).  The vectorizer's
 * tables are copied to the device by the first such call (xrl_tfidf_device_bytes reports their size; c_tfidf_destruct frees them).
 * The counts are the host tokenizer's (xrl_tfidf_counts) exactly.  Character tokenizers (token_type 20 / 30) decode in parallel, which
 * equals the host's sequential decode only where every lead byte is followed by the continuation bytes it names (or the buffer end);
 * a per-document status says where that does not hold, up to the max_length cut: 1 = a continuation byte where a character starts
 * (the host fails: "the string is not utf-8 encoded!"), 2 = a lead byte followed by too few continuation bytes (the host decodes on
 * along another path).  Without d_status the lowest such document fails the call (status 2: with the advice to use the host
 * tokenizer); with d_status [nr_doc] the call reports instead and leaves those rows empty.  nr_doc == 0 gives an empty handle; more
 * than 2^32 - 1 documents are refused; null arguments are refused before the GPU is touched.  hip_stream NULL = the model's stream.
 * The calls synchronise the stream; the caller's buffers must be complete when they are made. */
/* term-count CSR (unweighted; val = counts) as a query handle on model's device; xrl_queries_download reads it */
void* xrl_tfidf_counts_device(void* vectorizer, void* model, const uint8_t* d_text, const uint64_t* d_doc_off,
                              const uint64_t* d_doc_len, uint64_t nr_doc, uint32_t* d_status /* nr_doc, may be NULL */, void* hip_stream);
/* the same + the weighting tail xrl_tfidf_predict_device runs (per-base K5, ensemble norm): X ready for xrl_predict_device */
void* xrl_tfidf_predict_device_text(void* vectorizer, void* model, const uint8_t* d_text, const uint64_t* d_doc_off,
                                    const uint64_t* d_doc_len, uint64_t nr_doc, void* hip_stream);
/* host corpus (char** + lens): tokenizer 0 = xrl_tfidf_predict_device; 1 = packed into the handle's pinned staging, copied once, then as above */
void* xrl_tfidf_predict_device_tok(void* vectorizer, void* model, void* corpus_ptr /* const char** */, const size_t* doc_lens, size_t nr_doc,
                                   int tokenizer /* 0 host, 1 device */, int threads);
uint64_t xrl_tfidf_device_bytes(void* vectorizer, int device);
/* debug: out[0..n), n <= 4 <- {segments served by the LDS form, by the global form, batches, calls} of the device tokenizer since the load */
int xrl_debug_tfidf_device_forms(void* vectorizer, uint64_t* out, uint32_t n);
/* ---- Training the vectorizer on the device (K15, csrc/xrl_tfidf_train.hip) ----------------------------------------------------------
 * The reference's c_tfidf_train / c_tfidf_save under the xrl_ prefix, with its argument lists and its parameter structs
 * (tfidf.hpp:66-116, :194-208; a ctypes caller passes the reference's TfidfVectorizerParam as it is).  The trained model is the
 * reference's exactly: token id = rank of the token's bytes under unsigned-byte order (a prefix first), feature id = rank under
 * (df, n-gram length, token ids) inside the kept window, idf = the reference's expression in its precision.
 * The result is the handle type c_tfidf_load returns: every c_tfidf_* / xrl_tfidf_* call serves it, c_tfidf_destruct frees it.
 * Refused by name, before a GPU is required where the arguments decide it: null arguments; nr_doc == 0; nr_doc >= 2^32;
 * num_base_vect <= 0; a tok_type other than 10 / 20 / 30 ("received unknown tok_type: N"); tok_type 30 (char_wb: not served);
 * "expect 0 < min_ngram <= max_ngram"; "expect 0 <= min_df_ratio < max_df_ratio <= 1.0"; a norm_p other than 1 / 2; after the
 * vocabulary pass a max_ngram whose n-grams need more than 128 bits at the vocabulary's width; in char mode a document with status 1
 * (the host tokenizer's message and the document number) or status 2 (refused with the document number) anywhere in the document. */
typedef struct {            /* tfidf.hpp:66-116  TfidfBaseVectorizerParam */
    int32_t min_ngram, max_ngram;
    int32_t max_length, max_feature;
    float min_df_ratio, max_df_ratio;
    int32_t min_df_cnt, max_df_cnt;
    bool binary, use_idf, smooth_idf, add_one_idf, sublinear_tf, keep_frequent_feature;
    int32_t norm_p, tok_type;
} TfidfBaseVectorizerParam;
typedef struct {            /* tfidf.hpp:194-208  TfidfVectorizerParam */
    TfidfBaseVectorizerParam* base_param_ptr;
    int32_t num_base_vect;
    int32_t norm_p;
} TfidfVectorizerParam;
/* host corpus (char** + lens): packed on `threads` host threads, copied once, trained on the library's device (xrl_set_device) */
void* xrl_tfidf_train(void* corpus_ptr /* const char** */, const size_t* doc_lens, size_t nr_doc, const TfidfVectorizerParam* param, int threads);
/* the resident form: text, offsets and lengths in HBM on `device` as for xrl_tfidf_counts_device; the text never visits the host
 * (offsets and lengths are read back: 16 bytes a document).  hip_stream NULL = a stream of the call's own.  Synchronises the stream. */
void* xrl_tfidf_train_device(int device, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len, uint64_t nr_doc,
                             const TfidfVectorizerParam* param, void* hip_stream);
/* c_tfidf_save's folder: meta.json, <i>.base/tokenizer/{config.json,vocab.txt}, <i>.base/vectorizer/{config.json,tfidf-model.txt}, idf
 * printed with %f.  Serves trained and loaded handles (a loaded one states the training parameters its folder held).  The order of
 * the lines of vocab.txt / tfidf-model.txt is not the reference's hash-table order; the content is.  No GPU needed. */
void xrl_tfidf_save(void* vectorizer, const char* model_dir);
/* text in HBM -> the weighted X as an xrl_smat_* matrix handle on `device`; no XR-Linear model handle is needed.  d_status as for
 * xrl_tfidf_counts_device.  hip_stream NULL = the vectorizer's own stream. */
void* xrl_tfidf_transform_device(void* vectorizer, int device, const uint8_t* d_text, const uint64_t* d_doc_off, const uint64_t* d_doc_len,
                                 uint64_t nr_doc, uint32_t* d_status /* nr_doc, may be NULL */, void* hip_stream);
/* The content of base vectorizer `base`, for comparison without files.  sizes[5] <- {tokens, token bytes, n-grams, token ids of all
 * n-grams, idf entries}.  Every array may be NULL (sizes only); otherwise tok_bytes [sizes[1]], tok_off [sizes[0] + 1], tok_ids
 * [sizes[0]], ng_flat [sizes[3]], ng_off [sizes[2] + 1], ng_ids [sizes[2]], idf [sizes[4]].  Entries come in table order, not id
 * order.  Returns 0, or -1 with xrl_last_error set.  No GPU needed. */
int xrl_tfidf_export(void* vectorizer, uint32_t base, uint64_t* sizes, uint8_t* tok_bytes, uint64_t* tok_off, int32_t* tok_ids, int32_t* ng_flat,
                     uint64_t* ng_off, uint32_t* ng_ids, float* idf);
/* debug: out[0..n), n <= 11 <- {documents the vocabulary pass walked, (document, base) segments of the df pass served by the LDS form,
 * by the global form, df batches, distinct tokens, distinct n-grams before the filter, byte comparisons of tokens of more than 8
 * bytes, reruns of the vocabulary pass with a larger table, wall microseconds of the vocabulary passes (host sort and table build
 * included), of the df batches, of merge + filter + order + idf} of the training that made this handle (zeros for a loaded one) */
int xrl_debug_tfidf_train_forms(void* vectorizer, uint64_t* out, uint32_t n);
/* xrl_queries_concat_device_ex for a CSR query handle (e.g. xrl_tfidf_predict_device's): [X of the handle | X_emb] as a NEW handle on the
 * same device (XR-Transformer's concat_model call site, pecos/xmc/xtransformer/model.py:589-603, with both halves device-resident). */
void* xrl_queries_concat_handle(void* model, void* queries, uint32_t dense_cols, const float* d_emb, int normalize_emb, void* hip_stream);
/* The query form of XR-Transformer's concat_model (TransformerMatcher.concat_features + smat_util.hstack_csr,
 * pecos/xmc/xtransformer/matcher.py:864-890, model.py:589-603): [X_feat (device CSR, sparse_cols columns) | X_emb (device dense
 * rows x dense_cols)] assembled into one device CSR owned by the returned handle; every cell of the dense block becomes a stored
 * entry (zeros included), as smat_util.dense_to_csr does.  _ex with normalize_emb != 0 also applies sklearn's row-wise l2
 * normalize to X_emb on the device (the reference's default, matcher.py:879-880; values agree to ~1e-7 relative). */
void* xrl_queries_concat_device(void* model, uint32_t rows, uint32_t sparse_cols, const uint64_t* d_row_ptr,
                                const uint32_t* d_col_idx, const float* d_val, uint64_t nnz, uint32_t dense_cols,
                                const float* d_emb, void* hip_stream);
void* xrl_queries_concat_device_ex(void* model, uint32_t rows, uint32_t sparse_cols, const uint64_t* d_row_ptr,
                                   const uint32_t* d_col_idx, const float* d_val, uint64_t nnz, uint32_t dense_cols,
                                   const float* d_emb, int normalize_emb, void* hip_stream);
/* Shape of a query handle: out4 = {rows, cols, stored values (nnz, or rows x cols for a dense one), dense (0/1)}; and a copy of its
 * arrays back to the host (tests, debugging): CSR handles fill row_ptr[rows+1] / col_idx[nnz] / val[nnz], dense ones val[rows x cols]. */
int xrl_queries_info(void* queries, uint64_t* out4);
int xrl_queries_download(void* queries, uint64_t* row_ptr, uint32_t* col_idx, float* val);
void xrl_queries_free(void* queries);

/* Beam search with inputs already resident in HBM.  Writes fixed-stride results
 *   d_out_idx u32[rows*out_stride], d_out_val f32[rows*out_stride], d_out_cnt u32[rows]
 * into caller-provided DEVICE buffers (e.g. torch tensors) on `hip_stream` (a hipStream_t, NULL =
 * the library's own stream -- so a caller working on the legacy default stream, whose handle is NULL, must either pass
 * `sync` != 0 or use an explicit stream) and returns without synchronising when `sync` == 0.
 * out_stride must be >= the effective only_topk.  Returns 0 on success. */
int xrl_predict_device(void* model, void* queries, uint32_t beam_size, const char* post_processor,
                       uint32_t only_topk, uint32_t* d_out_idx, float* d_out_val,
                       uint32_t* d_out_cnt, uint32_t out_stride, void* hip_stream, int sync);

/* The same for rows [row_begin, row_begin + row_count) of the queries only; results land at the SAME rows of the output buffers.
 * Lets a caller pipeline a shard in pieces (bench.py: the all-gather of the first half runs under the second half's kernels). */
int xrl_predict_device_rows(void* model, void* queries, uint32_t beam_size, const char* post_processor,
                            uint32_t only_topk, uint32_t* d_out_idx, float* d_out_val,
                            uint32_t* d_out_cnt, uint32_t out_stride, void* hip_stream, int sync,
                            uint32_t row_begin, uint32_t row_count);

/* Ensembles on the device (K6): the fixed-stride results of n_models <= 8 predicts over the SAME rows -- model m's d_idx[m]
 * u32[rows*in_stride[m]], d_val[m] f32[rows*in_stride[m]], d_cnt[m] u32[rows], rows best first, as xrl_predict_device writes them;
 * a count above its stride is read as the stride -- merged into ONE fixed-stride result in the caller's device buffers, without a
 * visit to the host.  The four tables d_idx / d_val / d_cnt / in_stride are HOST arrays of n_models entries.  sum(in_stride) <= 1024.
 *   mode 0 average       CsrEnsembler.average (pecos/utils/smat_util.py:828-842): per label the fp32 sum of its scores in model order; with
 *                        two or more models a sum of exactly zero is not stored (scipy's CSR addition); rows ordered by (sum descending,
 *                        NaN last, label ascending); values sum / n_models
 *   mode 1 finish        Text2Text.predict's tail (pecos/apps/text2text/model.py:418-427): average; with a threshold, values <= *threshold and
 *                        zeros are dropped; rows ordered by (value descending, NaN last, label ascending) and cut to only_topk (0 = all)
 *   mode 2 rank_average  CsrEnsembler.rank_average (:845-859): position p of a row scores mm - p, mm = the longest row of any model in the
 *                        call (reduced on the device, no host synchronisation); rows ordered by (sum descending, label ascending); values
 *                        (double)sum / n_models, written as fp32
 * threshold (NULL = none) and only_topk belong to mode finish.  out_stride >= the longest possible row: sum(in_stride), or
 * min(sum(in_stride), only_topk) for finish with only_topk > 0.  Entries of an output row beyond its count are left untouched.
 * The work runs on `hip_stream` of `device` -- NULL is the device's default (null) stream here: the call has no model handle whose stream it
 * could borrow -- and the call returns without synchronising when `sync` == 0.  rows == 0 is a successful no-op.  Every argument is
 * checked before a GPU is required.  Returns 0 on success, -1 with a message in xrl_last_error otherwise. */
int xrl_ensemble_device(int device, uint32_t n_models, uint32_t rows,
                        const uint32_t* const* d_idx, const float* const* d_val, const uint32_t* const* d_cnt, const uint32_t* in_stride,
                        int mode /* 0 average, 1 finish, 2 rank_average */, const float* threshold /* NULL = none; finish only */,
                        uint32_t only_topk /* 0 = all; finish only */,
                        uint32_t* d_out_idx, float* d_out_val, uint32_t* d_out_cnt, uint32_t out_stride, void* hip_stream, int sync);

/* The other methods of CsrEnsembler on the device (K6 too), and the cut of TransformerMatcher.ensemble_prediction
 * (pecos/xmc/xtransformer/matcher.py:535-579).  Inputs, output, tables and capacity are xrl_ensemble_device's: n_models <= 8 results over
 * the same rows, sum(in_stride) <= 1024, a count above its stride is read as the stride, inputs are only read.  M = n_models; a "segment"
 * is one model's entries of a row, p an entry's position in its segment.
 *   method 0 average          as mode 0 of xrl_ensemble_device
 *   method 2 rank_average     as mode 2 of xrl_ensemble_device
 *   method 3 sigmoid_average  CsrEnsembler.sigmoid_average (smat_util.py:862-881): every score z becomes 1 / (1 + exp(-z)) in fp32 steps as
 *                             numpy takes them on a float32 array (exp rounded to fp32, one fp32 add, one fp32 division; NOT the
 *                             post-processor's sigmoid, which continues in double), then average.  sigmoid(+inf) = 1; sigmoid(z) = 0 once
 *                             exp(-z) overflows fp32, and for -inf; NaN stays NaN.  (The reference overwrites its arguments' data.)
 *   method 4 softmax_average  CsrEnsembler.softmax_average (:884-900, csr_row_softmax :788-811): per segment, over its stored entries
 *                             (explicit zeros included), x_max = the maximum (NaN when the segment holds a NaN), e_j = exp(x_j - x_max)
 *                             rounded to fp32, denominator = the fp64 sum of the e_j rounded once to fp32, value = e_j / denominator in
 *                             fp32; then average.  Order of the fp64 sum, a function of the inputs only: entry j of the row's
 *                             model-ordered list belongs to lane j % 64; every lane adds its entries of the segment in ascending j,
 *                             starting from 0.0; the 64 lane sums then meet in six exchange steps, s[l] = s[l] + s[l ^ d] for
 *                             d = 1, 2, 4, 8, 16, 32.  A segment whose maximum is +inf, or that is all -inf, comes out NaN by IEEE
 *                             arithmetic alone, as scipy's does.  An EMPTY segment contributes nothing (the reference raises ValueError
 *                             there: it takes the maximum of an empty array).
 *   method 5 round_robin      CsrEnsembler.round_robin (:903-923 with get_relevance_csr, :638-659), all in fp64, every operation rounded
 *                             on its own: base = 1.0 / (M + 1.0); the entry at position p of model m scores
 *                             (double)(mm - p) + (double)(M - m) * base, mm = the longest row of any model in the call (reduced on the
 *                             device, no host synchronisation); a label's key is the MAXIMUM over its holders; rows ordered by (key
 *                             descending, label ascending); values (float)(key / (double)M).  Scores are not read.
 *   method 1 (finish) is refused: it is xrl_ensemble_device's.
 * only_topk == 0 keeps the method's own order and length.  only_topk > 0 is ensemble_prediction's last line,
 * sorted_csr(pred.astype(float32), only_topk): the merged row is ranked AGAIN by its fp32 VALUE descending (NaN last, -0.0 tied with +0.0),
 * then label ascending, and the first only_topk entries are kept.  out_stride >= the longest possible row: sum(in_stride), or
 * min(sum(in_stride), only_topk) with only_topk > 0.  Entries of an output row beyond its count are left untouched.
 * Stream, `sync`, rows == 0 and the order of the checks are xrl_ensemble_device's: the work runs on `hip_stream` of `device` (NULL = the
 * null stream), returns without synchronising when `sync` == 0, the device scalar of methods 2 and 5 lives and dies in stream order,
 * rows == 0 is a successful no-op, every argument is checked before a GPU is required.  Returns 0 on success, -1 with a message
 * (starting "xrl_ensemble_methods_device: ") in xrl_last_error otherwise. */
int xrl_ensemble_methods_device(int device, uint32_t n_models, uint32_t rows,
                                const uint32_t* const* d_idx, const float* const* d_val, const uint32_t* const* d_cnt, const uint32_t* in_stride,
                                int method /* 0 average, 2 rank_average, 3 sigmoid_average, 4 softmax_average, 5 round_robin */,
                                uint32_t only_topk /* 0 = the method's own rows */,
                                uint32_t* d_out_idx, float* d_out_val, uint32_t* d_out_cnt, uint32_t out_stride, void* hip_stream, int sync);

/* Metrics on the device (K8): the sums behind precision and recall at 1 .. topk -- smat_util.Metrics.generate(tY, pY, topk)
 * (pecos/utils/smat_util.py:968-997) -- of ONE fixed-stride result (d_idx u32[rows*stride], d_val f32[rows*stride], d_cnt u32[rows], as
 * xrl_predict_device and xrl_ensemble_device write it; a count above the stride is read as the stride) against the true labels as a device CSR
 * pattern: d_true_ptr u64[rows+1], d_true_idx u32[...].  Row r of the call reads d_true_ptr[r] and d_true_ptr[r+1] as ABSOLUTE offsets into
 * d_true_idx, so a caller evaluates a window of rows by offsetting d_idx / d_val / d_cnt / d_true_ptr and passing d_true_idx as it is.
 *   order    a row's T = min(count, stride) entries are ranked as the reference's sorted_csr ranks them: value descending, -0.0 tied with
 *            +0.0, every NaN last, ties by label ascending.  The stored order is not trusted (predict breaks ties by candidate position);
 *            entries with score exactly 0 are entries.
 *   match    entry of rank p matches when its label occurs in the true row; cum[p] = matched entries of rank <= p
 *   carry    positions T <= p < topk carry cum[T-1]; a row with T == 0 adds nothing at all, whatever its true row holds
 *   sums     d_matched[p] = sum over rows of cum[p] (u64); d_recall_sum[p] = sum over rows of (double)cum[p] / (double)max(n_true, 1), each
 *            quotient correctly rounded; n_true = d_true_ptr[r+1] - d_true_ptr[r], duplicates included
 * The call returns the raw sums, not the metrics: they add over row batches and ranks, and prec[p] = matched[p] / rows / (p + 1),
 * recall[p] = recall_sum[p] / rows.
 * Preconditions (not checked): the labels of a result row are distinct; every true row is ascending.  Capacity: stride and topk in 1..1024.
 * Summation order, a function of the inputs only (no atomics; independent of the CU count and the launch order): with R(rows) =
 * 64 * max(1, ceil(rows / 262144)), block w = rows [w*R, (w+1)*R) is summed in ascending row order from 0.0, then the blocks in ascending w
 * from 0.0.  For rows <= R(rows) the fp64 sums are therefore the reference's own row-order sums, bit for bit; d_matched is exact always.
 * The work runs on `hip_stream` of `device` -- NULL is the device's default (null) stream -- with its scratch allocated and freed in stream
 * order, and the call returns without synchronising when `sync` == 0.  rows == 0 zero-fills both outputs when a GPU is visible and is a
 * successful no-op otherwise.  Every argument is checked before a GPU is required (messages start with "xrl_metrics_device: "): null
 * pointers, stride or topk outside 1..1024.  Returns 0 on success, -1 with a message in xrl_last_error otherwise. */
int xrl_metrics_device(int device, uint32_t rows,
                       const uint32_t* d_idx, const float* d_val, const uint32_t* d_cnt, uint32_t stride,
                       const uint64_t* d_true_ptr, const uint32_t* d_true_idx,
                       uint32_t topk, uint64_t* d_matched /* u64[topk] */, double* d_recall_sum /* f64[topk] */,
                       void* hip_stream, int sync);

/* SPARSE MATRIX PRODUCTS ON THE DEVICE (K10, csrc/xrl_spgemm.hip): clib.sparse_matmul (pecos/core/base.py:1460-1534) with the operands
 * and the product in HBM -- csr_codes * C^T of XR-Transformer's descent (pecos/xmc/xtransformer/matcher.py:723), Y * C of the matching
 * matrices and label roll-ups (pecos/xmc/base.py:556, 1520, 1550), S * C, the Yn^T * X inside xrl_label_embedding_device -- on matrix handles bound to a
 * DEVICE, not to a model.
 * THE RULE (smat_x_smat, matrix.hpp:1075-1292, bit for bit).  Z = A * B, A rows x inner, B inner x cols, both CSR (u64 row_ptr, u32
 * col_idx, f32 val).  For every row i of A walk its stored entries s = 0, 1, ... in STORED order (whatever it is, duplicates allowed);
 * for entry (k, a) walk the stored entries t = 0, 1, ... of row k of B in stored order (duplicates allowed): acc[j] = acc[j] + a * b,
 * a rounded multiply then a rounded add (no FMA), every acc from +0.0f -- so 0 + (-0) is +0, and the order of the additions to one column
 * is the order of the walk.  A column is touched by its first product, a zero product included.  Row i of Z: the touched columns,
 * ascending with sorted_indices, otherwise in the order of first touch.  With eliminate_zeros, entries with val == 0 are then dropped
 * (NaN stays).  Subnormal products and sums are kept.  The result is a function of the inputs only: no float atomics, no dependence on
 * the CU count, the launch order or a hash seed.
 * A CSC product X * W is xrl_sparse_matmul_device(W^T as CSR, X^T as CSR) read as CSC: the CSC arrays of a matrix are the CSR arrays of
 * its transpose, and (X * W)^T = W^T * X^T.
 * Capacity: an output row of at most 1024 products (xrl_spgemm.h: CAP) is served by one wavefront in LDS; longer rows go through HBM
 * scratch and a segmented sort, in batches that keep the scratch under 6 GiB.  Refused: a row of 2^31 products or more; an entry of A
 * whose column is not a row of B; operands on two devices; A.cols != B.rows ("X.cols != W.rows"); null handles and pointers (all but
 * the first two before a GPU is required; messages start with the function's name).
 *   xrl_smat_upload_csr          a host CSR copied to `device`; the handle owns the copy
 *   xrl_smat_from_device_csr     wraps arrays that are in HBM on `device`; NOT owned: keep them alive until xrl_smat_free; no GPU call
 *   xrl_smat_from_device_result  a fixed-stride result (d_idx / d_val [rows * stride], d_cnt [rows] or NULL = stride each; a count above
 *                                the stride is read as the stride -- what xrl_predict_device and xrl_ensemble_device write) compacted
 *                                into a CSR the handle owns, rows x cols, the stored best-first order kept; synchronises hip_stream
 *   xrl_smat_info                out[0..cap), cap <= 7 <- {rows, cols, nnz, device, address of row_ptr, of col_idx, of val}: a product
 *                                feeds xrl_queries_from_device_csr (sorted_indices, as queries must be) or a torch tensor view
 *   xrl_smat_download            row_ptr[rows + 1], col_idx[nnz], val[nnz] back to the host (synchronises the device)
 *   xrl_smat_copy_device         the same three arrays into the caller's buffers in HBM on the handle's device (e.g. torch tensors sized
 *                                from xrl_smat_info), on hip_stream, which it synchronises
 *   xrl_smat_free                frees the handle and what it owns (NULL: no-op)
 *   xrl_sparse_matmul_device     a NEW owned handle with Z = A * B on the operands' device, computed on hip_stream (NULL = the device's
 *                                null stream).  The call SYNCHRONISES the stream: once, to learn nnz, when every row fits the LDS form;
 *                                again per pass when rows need the big form or eliminate_zeros is set.  Zero rows, an empty operand and
 *                                nnz == 0 succeed and give an empty handle.  NULL + xrl_last_error on failure.
 *   xrl_debug_spgemm_forms       FOR TESTS ONLY: out[0..n), n <= 5 <- {CAP, rows served by the LDS form, rows served by the big form, batches
 *                                of the big form (its count pass), products computed} of this process since the library was loaded */
void* xrl_smat_upload_csr(int device, const ScipyCsrF32* X);
void* xrl_smat_from_device_csr(int device, uint32_t rows, uint32_t cols, const uint64_t* d_row_ptr, const uint32_t* d_col_idx,
                               const float* d_val, uint64_t nnz);
void* xrl_smat_from_device_result(int device, uint32_t rows, uint32_t cols, const uint32_t* d_idx, const float* d_val,
                                  const uint32_t* d_cnt /* NULL = stride each */, uint32_t stride, void* hip_stream);
int xrl_smat_info(void* smat, uint64_t* out, uint32_t cap);
int xrl_smat_download(void* smat, uint64_t* row_ptr, uint32_t* col_idx, float* val);
int xrl_smat_copy_device(void* smat, uint64_t* d_row_ptr, uint32_t* d_col_idx, float* d_val, void* hip_stream);
void xrl_smat_free(void* smat);
void* xrl_sparse_matmul_device(void* A, void* B, int eliminate_zeros, int sorted_indices, void* hip_stream);
int xrl_debug_spgemm_forms(uint64_t* out, uint32_t n);

/* ------------------------------------------------------------------------------------------
 * Label clustering on the device (K11, csrc/xrl_cluster.hip): the reference's balanced hierarchical 2-means (libpecos.cpp:357-370 ->
 * Tree::run_clustering, pecos/core/utils/clustering.hpp:403-503), which turns the rows of a feature matrix (label embeddings) into leaf
 * codes 0 .. 2^depth - 1.  The answer is the reference's at threads = 1; `threads` is accepted and ignored.
 * The rule.  Elements 0 .. L-1 in an array `elements`; an mt19937 seeded with `seed` draws one 32-bit seed per node id 0 .. 2^(depth+1)-1;
 * node 1 owns [0, L), the children of [s, e) own [s, m) and [m, e), m = (s + e) >> 1.  Level d = nodes 2^d .. 2^(d+1)-1, each with its
 * own mt19937 from its seed:
 *   1. the level's sample rate (clustering.hpp:156-167, float arithmetic); below 1 the node shuffles its range (std::shuffle; the
 *      shuffle stays) and works on its first size_t(rate * size) elements, split at their midpoint;
 *   2. iterations k = 0 .. kmeans_max_iter-1; every product and every addition is rounded, no FMA.  k = 0: r = randint(0, n-1),
 *      l = (r + randint(1, n-1)) % n over the n working elements, centre = x_r - x_l per feature.  k > 0, KMEANS (partition_algo 0):
 *      one accumulator per feature from +0, walked over the right half's elements in stored order (ascending id), each row in stored
 *      order, c[f] = c[f] + float(1.0 / |right|) * v, then over the left half with float(-1.0 / |left|).  SKMEANS (5): c1 sums the right
 *      half, c2 the left half; each is scaled by 1.0 / sqrt((double)||c||^2) when ||c||^2 > 0 (the double product rounded to float), then
 *      c1 - c2.  ||c||^2 is an fp32 chain of c[f] * c[f], in ascending f while the level is dense, and in the order of first touch during
 *      the accumulation once nnz / (nodes of the level * cols) < 1 has held at this or an earlier level.  score[e] = the fp32 chain over
 *      row e's stored entries of c[f] * v from +0.  The working range is sorted by (score ascending, id ascending), -0 == +0, then each
 *      half by id; the node stops when its first half is what it was before the sort;
 *   3. the node's children are the midpoint split of its whole range; a level that sampled scores and sorts the whole range once more
 *      with the last centre.
 * label_codes[elements[i]] = the leaf that owns position i.
 * Range.  Finite feature values are served by the rule, whatever leaves fp32's range on the way, for as long as no centre entry and no
 * score of any iteration of any node is a NaN.  A product, a sum or a norm that overflows is +-inf as the reference's: ||c||^2 = +inf is
 * positive, its scale is 1.0 / sqrt(inf) = 0.0, every finite entry of that half's centre becomes +-0 (both halves: the centre is zeros,
 * every score ties at 0 and the id splits the range); scores of +inf tie with each other, as do scores of -inf, and the id decides among
 * them.  ||c||^2 that is a positive subnormal scales like any other; ||c||^2 whose every square underflows is 0 and the centre is not
 * scaled.  Subnormal products and sums are kept.  Finite inputs that do produce a NaN (inf - inf in a centre or a score chain, 0 * inf
 * under an infinite norm) are as unpinned as non-finite feature values: the split's order (a < b, or a == b and the lower id) is no
 * strict weak order over a NaN and the reference's std::sort has no defined answer.  Neither is refused.
 * Refused before a GPU is required (messages start with the function's name): null pointers; 2^depth > rows; depth > 30; a sampled
 * node of fewer than 2 elements; the reference's invalid rates (0 < min <= max <= 1, 0 <= warmup_ratio <= 1); a partition_algo other
 * than 0 or 5.  Refused by a check kernel: a row whose column ids are not strictly ascending, or an id >= cols.  Scratch is one level
 * at a time; when it does not fit the message names the bytes needed.
 *   c_run_clustering_csr_f32 / _drm_f32   the reference's signatures: upload, run, copy label_codes [rows] back.  The dense form is the
 *                                same computation on rows that store every entry, zeros included, always with the dense norm order.
 *   xrl_run_clustering_device    the feature matrix is an xrl_smat_* CSR handle (e.g. the label embedding xrl_label_embedding_device leaves in HBM); d_codes [rows]
 *                                and d_scores (NULL or [depth * rows]: the reference's `scores` array as it stands after each level) are
 *                                in HBM on the handle's device.  Runs on hip_stream and synchronises it every iteration.  0, or -1 +
 *                                xrl_last_error.
 *   xrl_debug_cluster_plan       FOR TESTS ONLY, needs no GPU: the draws.  node_seed [2^(depth+1)]; level_info [2 * depth] = {sampled,
 *                                first-touch norm order} per level; work [4 * 2^depth], by node id = {range start, working end, position
 *                                of r, position of l}; perm [depth * rows] = each level's shuffle as source positions.  Each may be NULL.
 *   xrl_debug_cluster_forms      FOR TESTS ONLY: of the last clustering of this process, out[0..n) <- {runs served one per lane, runs
 *                                served by a wavefront (64 entries and more), segmented sorts issued, level at which the norm order
 *                                switched (~0: never, or KMEANS), depth, iterations run at level 0, 1, ...}; runs count once per level */
typedef struct {            /* clustering.hpp:35-72  ClusteringParam */
    size_t partition_algo;
    int seed;
    size_t kmeans_max_iter;
    int threads;
    float max_sample_rate, min_sample_rate, warmup_ratio;
} ClusteringParam;
void c_run_clustering_csr_f32(const ScipyCsrF32* X, size_t depth, ClusteringParam* param, uint32_t* label_codes);
void c_run_clustering_drm_f32(const ScipyDrmF32* X, size_t depth, ClusteringParam* param, uint32_t* label_codes);
int xrl_run_clustering_device(void* smat, uint64_t depth, const ClusteringParam* param, uint32_t* d_codes, float* d_scores /* NULL or [depth * rows] */,
                              void* hip_stream);
int xrl_debug_cluster_plan(uint64_t rows, uint64_t cols, uint64_t nnz, uint64_t depth, const ClusteringParam* param, uint32_t* node_seed, uint32_t* level_info,
                           uint32_t* work, uint32_t* perm);
int xrl_debug_cluster_forms(uint64_t* out, uint32_t n);

/* ------------------------------------------------------------------------------------------
 * LABEL EMBEDDINGS ON THE DEVICE (K12, csrc/xrl_embed.hip, composed with K10): LabelEmbeddingFactory.create (pecos/xmc/base.py:1903-2094)
 * for CSR operands, from a label matrix Y (samples x labels) and features X (samples x features) in HBM to the embedding E (labels x
 * features) in HBM -- the feature matrix of xrl_run_clustering_device -- bit for bit the reference's at threads = 1.
 * R1, row normalisation = sklearn.preprocessing.normalize(M, axis=1, norm="l2") on float32 CSR (inplace_csr_row_normalize_l2).  Per
 *   row, s is a DOUBLE that starts at +0.0; the stored entries are walked in STORED order: s = s + (double)fl32(v * v), the square a
 *   rounded fp32 product widened afterwards, the sum one chain (no tree: an fp32 result can see the order).  s == 0.0: the row stays as
 *   it is, explicit zeros included.  Otherwise n = sqrt(s) in double and every entry becomes (float)((double)v / n), both correctly
 *   rounded.  A square that overflows gives s = inf and a row of zeros; an inf entry becomes NaN and a NaN entry makes the whole row NaN
 *   (with the bits an x86 host leaves: the first NaN of the row quieted, a NaN entry its own bits quieted, inf / inf 0xFFC00000).
 *   Column ids and the row pointer are unchanged; duplicates and unsorted rows are walked as stored.
 * R1a, row normalisation under norm="l1" (inplace_csr_row_normalize_l1).  Per row, s is a DOUBLE that starts at +0.0; the stored entries
 *   are walked in STORED order: s = s + fabs((double)v), one chain (rows below 64 entries one per lane, longer ones by the wavefront, 64
 *   entries a step, the adds serial and identical on every lane).  s == 0.0: the row stays as it is.  Otherwise every entry becomes
 *   (float)((double)v / s): one double division, rounded to float once.  An inf entry gives s = inf: finite entries become signed zeros,
 *   the inf entries 0xFFC00000.  A NaN entry makes the whole row NaN with the bits an x86 host leaves: the first NaN of the row with its
 *   sign cleared (fabs) and quieted, a NaN entry its own bits quieted.  Duplicates and unsorted rows are walked as stored.
 * R1b, row normalisation under norm="max" (min_max_axis, then X.data /= norms).  n = the fp32 maximum of |v| over the row's stored entries
 *   (order-free: a wavefront reduction); n is NaN if any entry is a NaN, whichever lane holds it (numpy's maximum).  n == 0: the row stays
 *   as it is.  Otherwise every entry becomes v / n, ONE fp32 division; inf / inf is 0xFFC00000.  In a row with a NaN every entry becomes a
 *   NaN: a NaN entry its own bits quieted, the others "a NaN" (0x7FC00000 here; on the host the payload follows numpy's reduction order,
 *   so the contract is "is a NaN").  The reference sums entries with one column id before it takes the maximum: a row whose column ids
 *   are not STRICTLY ASCENDING is refused by a check kernel, by row, before a value is written (norm = 3 only).
 * R2, transposition = M.T.tocsr() (scipy's csr_tocsc).  Output row j holds every stored entry of column j ordered by SOURCE POSITION:
 *   source row ascending, stored order inside a source row.  Duplicates are kept, not summed; explicit zeros are kept; the output's
 *   column ids are the source row ids.  A function of the input only: integer atomics count and claim slots, the order inside an output
 *   row is then made the stable one (xrl_sparse_matmul_device sums a left row in stored order, so the order reaches the score bits).
 * R3, pifa(Y, X, normalized_Y): Yn = R1(Y) when normalized_Y, else Y; YT = R2(Yn); E = xrl_sparse_matmul_device(YT, X, eliminate_zeros
 *   = 0, sorted_indices = 1); R1(E) in place.
 * R4, pii(Y): R1(R2(Y)); Y is not normalised first.
 * R5, pifa_lf_concat(Y, X, Z), Z labels x label-features: hstack([E, Z]) -- per row E's entries as stored, then Z's entries as stored
 *   with E.cols added to their ids.
 * Capacity: an output row of the transpose of at most 1024 entries (xrl_embed.h: CAP) is ordered by one wavefront in LDS, longer ones by
 * a segmented sort in HBM; a transpose serves fewer than 2^32 - 1 stored entries.  Every call runs on hip_stream (NULL = the device's null
 * stream) and SYNCHRONISES it before it returns.  Refused, before a GPU is required (messages start with the function's name): null
 * handles; dense handles; Y.rows != X.rows; Z.rows != Y.cols; an unknown method; operands on two devices; widths that add up to 2^32 or
 * more; 2^32 - 1 entries or more to transpose.  Refused by a kernel: an entry to transpose whose column id is not below cols.  Zero
 * rows, zero columns and nnz == 0 succeed and give empty handles.  Dense X / Z and pifa_lf_convex_combine are not served.
 *   xrl_smat_transpose_device       a NEW owned handle, cols x rows, by R2
 *   xrl_smat_normalize_rows_device  R1 (L2 only).  in_place: writes the handle's own val array -- for a handle that wraps caller memory
 *                                   (xrl_smat_from_device_csr) that IS the caller's array; `out` is not touched.  Otherwise *out <- a NEW
 *                                   owned handle and A stays as it is.  0, or -1 + xrl_last_error
 *   xrl_smat_normalize_rows_norm_device  the same call under norm 1 = l1 (R1a), 2 = l2 (R1: the same kernel and bytes as the call above),
 *                                   3 = max (R1b); any other norm is refused before a GPU is required
 *   xrl_smat_hstack_device         a NEW owned handle [mats[0] mats[1] ...]: one row count, one device, n >= 1
 *   xrl_label_embedding_device      method 0 = pifa (R3), 1 = pifa_lf_concat (R5), 2 = pii (R4; X is ignored and may be NULL).  A NEW owned
 *                                   handle; the intermediates are freed; Y, X and Z stay as they are (the normalised Y is a private copy)
 *   xrl_debug_embed_forms           FOR TESTS ONLY: out[0..n), n <= 5 <- {CAP, transposed rows served in LDS, by the big form, normalised
 *                                   rows served one per lane, by a wavefront (64 entries and more)} of this process since the library
 *                                   was loaded; rows without entries are served by neither */
void* xrl_smat_transpose_device(void* A, void* hip_stream);
int xrl_smat_normalize_rows_device(void* A, int in_place, void** out, void* hip_stream);
int xrl_smat_normalize_rows_norm_device(void* A, int norm, int in_place, void** out, void* hip_stream);
void* xrl_smat_hstack_device(void* const* mats, uint32_t n, void* hip_stream);
void* xrl_label_embedding_device(void* Y, void* X, void* Z_or_null, int method, int normalized_Y, void* hip_stream);
int xrl_debug_embed_forms(uint64_t* out, uint32_t n);

/* ------------------------------------------------------------------------------------------
 * RANKER TRAINING ON THE DEVICE (K13, csrc/xrl_train.hip): one layer of XR-Linear's weights from X (N x d), the label matrix Y (N x L),
 * the label-to-cluster matrix C (L x K) and the matching matrix M (N x K) -- libpecos.cpp:277-316 -> multilabel_train_with_codes
 * (pecos/core/xmc/linear_solver.hpp:797-860) -- bit for bit the reference's at threads = 1.  `threads` is accepted and ignored: a
 * job's weights do not depend on it, only the order of the reference's COO does.  The reference is the one compiled with libstdc++
 * (std::shuffle and std::uniform_int_distribution are the library's) and without FMA.
 * THE RULE.  Only the PATTERNS of Y, C and M are read: explicit zeros count, values are ignored.  R (optional, Y's pattern) gives the
 * cost of a positive.
 *   Jobs (:828-844).  With C and M: for every column `code` of C in order, for every stored entry `label` of that column in STORED order,
 *     one job (code, label).  With C or M null (pure multi-label): one job per label 0 .. L-1.  Jobs are independent.
 *   Instances (:667-712).  index <- the stored row ids of M[:, code] in stored order (pure: 0 .. N-1), each with y = -1, cost = 1.  Then the
 *     stored row ids i of Y[:, label] in stored order: y[i] = +1; i is appended to index when M's column did not list it; cost[i] =
 *     R's value at that stored position, or 1.
 *   Storage.  w [d], b, alpha and QD are fp32.  G, C, PG, d and the alpha update are fp64, rounded on the store.
 *   Set-up (:438-447).  class_cost = y > 0 ? Cp : Cn (fp64).  diag_i = 0.5 / (class_cost * (double)cost_i) for the L2 loss
 *     (L2R_L2LOSS_SVC_DUAL = 1), 0 for the L1 loss (L2R_L1LOSS_SVC_DUAL = 3).  QD_i = fl32(diag_i), then QD_i = fl32((double)QD_i +
 *     ((double)xx + bb)): xx the fp32 chain from +0 over the row's stored entries of fl32(v * v) (matrix.hpp:837-859), bb = bias * bias
 *     when bias > 0, else 0.  alpha = 0, w = 0, b = 0.
 *   Sweep (:456-527), iter = 0 .. max_iter-1, active = |index| at first.  std::shuffle(index[0, active)) with ONE std::mt19937(0) per
 *     job that lives across its sweeps.  libstdc++'s shuffle: up to 65 535 elements an even count first swaps position 1 with a draw
 *     from {0, 1}, then positions i, i+1 are taken two at a time from one draw x in [0, (i+1)(i+2)): swap(i, x / (i+2)), swap(i+1, x %
 *     (i+2)); from 65 536 elements one draw in [0, i] per position i.  A draw in [0, r) is Lemire's: p = u64(next word) * r; when
 *     u32(p) < r, redraw while u32(p) < (2^32 - r) % r; the draw is p >> 32.  Then s = 0, 1, ... while s < active, i = index[s]:
 *       dot = the fp32 chain from +0 of fl32(w[f] * v) over row i's stored entries in stored order (matrix.hpp:870-877)
 *       G = y * ((double)dot + (bias > 0 ? (double)b * bias : 0)) - 1 + (double)alpha_i * diag_i;  C = inf (L2 loss), class_cost * cost (L1)
 *       alpha_i == 0: G > PGmax_old shrinks; else PG = min(G, 0).  alpha_i == C: G < PGmin_old shrinks; else PG = max(G, 0).  Else PG = G.
 *       Shrinking: active -= 1, swap(index[s], index[active]), and s is visited again.
 *       PGmax_new, PGmin_new follow PG.  When |PG| > 1e-12: alpha_i <- fl32(min(max(alpha_i - G / (double)QD_i, 0), C)); d = ((double)
 *       alpha_i - alpha_old) * y; w[f] <- fl32((double)w[f] + d * (double)v) per stored entry (an fp64 product and an fp64 add, :971-976);
 *       b <- fl32((double)b + d * bias) when bias > 0.
 *     After the sweep: PGmax_new - PGmin_new <= eps ends the job when active == |index|, otherwise active = |index| and the old bounds
 *     reset (a re-activation); else the old bounds become the new ones, PGmax_old <= 0 -> inf, PGmin_old >= 0 -> -inf.
 *   Emission (:718-779), fabs(v) >= threshold compared in fp64 (NaN fails).  max_nonzeros_per_label = 0: the features that pass, ascending,
 *     then the bias as row d when bias > 0 and it passes.  max_nonzeros_per_label = k > 0: of the features that pass, the k with the
 *     largest |w|, ties to the lower feature; when fewer than k pass, all of them and the bias (if it passes); otherwise the bias
 *     replaces the least kept feature when |b| > |w_least|.  The reference leaves the order inside such a label to std::nth_element; here
 *     a label's entries are ascending in both cases.
 * Pinned too (the reference's answer to each is sequential code that does not depend on `threads`, so none is refused):
 *   Repeated row ids.  A row id stored more than once in a column of Y: at EVERY stored position, in stored order, the row is appended to
 *     index when its cost reads 0 at that moment, then its cost becomes that position's R (or 1).  So the first occurrence of a row M
 *     does not list is appended, an occurrence that follows one whose R is +-0 is appended AGAIN (a cost of 0 reads as "not listed"; also
 *     in the pure form, where a job may list more instances than X has rows), and the last stored R stays.  A row id stored twice in a
 *     column of M is listed twice; alpha and QD are per row.  The device orders the 64 positions of a step by lane number, not by atomics.
 *   Non-finite values.  The set-up also runs w += (y * alpha) * x and b += (y * alpha) * bias with y * alpha = +-0 (:444-446): w[f] is a
 *     NaN wherever an instance stores an inf or a NaN at f, b is a NaN under an infinite bias.  Every comparison is the reference's as
 *     written: a NaN G neither shrinks nor counts as violated unless 0 < alpha < C, where PG = NaN; std::max(PGmax_new, PG) and std::min
 *     (PGmin_new, PG) never take a NaN PG; min(max(., 0), C) passes a NaN alpha on and ignores a NaN C.  Roundings to fp32 overflow to inf
 *     and go through subnormals; QD == 0 divides to +-inf (clipped at C under the L1 loss).  A NaN weight is NEVER emitted (it fails
 *     fabs(v) >= threshold, and a NaN threshold fails everything); +-inf weights are, and tie by the lower feature.
 *   Parameters.  Cp, Cn, eps, threshold, bias and R's values are used as given (0, negative, subnormal, inf, NaN).  The result has
 *     d + (bias > 0) rows: a zero, negative or NaN bias adds no row and takes no part.
 * Capacity.  One wavefront owns one job at a time, with a slot of scratch (w, a bitmap of touched features, index, alpha, QD, cost, y);
 * jobs go in batches whose emission staging stays under the budget (4 GiB each for slots and staging; XRL_TRAIN_SCRATCH_BYTES in the
 * environment replaces it).  All jobs read ONE table of mt19937(0) outputs the host fills (XRL_TRAIN_RANDOM_WORDS = its first length,
 * 2^22 by default); a job that reaches its end is run again after the table has grown fourfold.
 * Refused, with messages that start with the function's name.  Before a GPU is required: L2R_LR_DUAL (7), L2R_L2LOSS_SVC_PRIMAL (2) and
 * unknown solvers; null arguments; shape mismatches; operands on two devices; 2^31 rows or more; 2^32 - 1 jobs or more; (host forms) a
 * label listed twice in C, an R that does not share Y's pattern.  By check kernels: the same two for the resident form; a row of X whose
 * column ids are not strictly ascending (the lanes apply the axpy in parallel); ids out of range; row pointers that do not ascend.
 *   xrl_single_layer_train_csr_f32 / _drm_f32   the signatures of the reference's c_xlinear_single_layer_train_* and its COO allocator:
 *                                upload, train, copy back rows (features; d = the bias), cols (labels) and values in job order.  The
 *                                dense form is the same computation on rows that store every entry, zeros included.  The names carry
 *                                this library's prefix ON PURPOSE: a binding that resolves symbols here first and in the reference
 *                                otherwise (the drop-in deployment, tests/test_reference_binding.py) keeps the reference's trainer,
 *                                with L2R_LR_DUAL and L2R_L2LOSS_SVC_PRIMAL; a caller that wants K13 binds these two names with the
 *                                reference's argument list.
 *   xrl_train_layer_device       X (N x d), Yt (L x N), Ct (K x L) and Mt (K x N) are CSR handles of the transposes -- the CSC arrays the
 *                                solver reads; Ct and Mt NULL together = pure multi-label; Rt NULL or Yt's pattern.  A NEW owned handle with
 *                                W^T, L x (d + (bias > 0)): the CSC of W with ascending features; a label without a job has an empty row.
 *                                Runs on hip_stream and synchronises it per batch.  NULL + xrl_last_error on failure.
 *   xrl_debug_train_counters     FOR TESTS ONLY: of the last training of this process, out[0..n), n <= 13 <- {jobs, batches, slots, staging
 *                                stride, sweeps, shrink events, re-activations, jobs stopped by max_iter, alpha clipped at C, x'x rows
 *                                summed one per lane, by a wavefront (64 entries and more), table extensions, jobs run again} */
typedef void (*py_coo_allocator_t)(uint64_t rows, uint64_t cols, uint64_t nnz, void* row_pp, void* col_pp, void* val_pp);   /* matrix.hpp:46: u64 rows, u64 cols, f32 values */
void xrl_single_layer_train_csr_f32(const ScipyCsrF32* pX, const ScipyCscF32* pY, const ScipyCscF32* pC, const ScipyCscF32* pM, const ScipyCscF32* pR,
                                    py_coo_allocator_t coo_alloc, double threshold, uint32_t max_nonzeros_per_label, int solver_type, double Cp, double Cn,
                                          size_t max_iter, double eps, double bias, int threads);
void xrl_single_layer_train_drm_f32(const ScipyDrmF32* pX, const ScipyCscF32* pY, const ScipyCscF32* pC, const ScipyCscF32* pM, const ScipyCscF32* pR,
                                    py_coo_allocator_t coo_alloc, double threshold, uint32_t max_nonzeros_per_label, int solver_type, double Cp, double Cn,
                                          size_t max_iter, double eps, double bias, int threads);
void* xrl_train_layer_device(void* X, void* Yt, void* Ct_or_null, void* Mt_or_null, void* Rt_or_null, double threshold, uint32_t max_nonzeros_per_label,
                             int solver_type, double Cp, double Cn, uint64_t max_iter, double eps, double bias, void* hip_stream);
int xrl_debug_train_counters(uint64_t* out, uint32_t n);

/* The primal solver for the L2-loss SVC on the device (K16, csrc/xrl_newton.hip): L2R_L2LOSS_SVC_PRIMAL = 2 of the reference's solver table,
 * SVMWorker::solve_l2r_l2_svc_primal (linear_solver.hpp:407-417) over l2r_erm_fun / l2r_l2_svc_fun (:62-323), NEWTON::newton / pcg / norm
 * (utils/newton.hpp:98-273) and the vector helpers (utils/matrix.hpp:862-976).  Jobs, instances and emission are xrl_train_layer_device's
 * above, and so are the pinned answers to repeated row ids; the weights are the reference's at threads = 1 bit for bit (tests/
 * primal_training_rule.py states the rule in numpy).  The solver arrives under names of its own because the refusal of solver 2 through
 * the three entry points above is part of their contract.
 * Rule N, one job.  value_type is float: w, b, g, M, s, r, d, Hd, z, wx, tmp, their bias parts and c_i = fl32((double)cost_i * (y_i > 0 ? Cp :
 *   Cn)) are fp32; f, alpha, beta, zTr, dHd, Q, gnorm, wTw, sTs, wTs, gTs, xTs are fp64.  Every dot product is an fp32 chain from +0 of fp32
 *   products in index order, returned as fp32; norm is an fp64 chain of (double)g_i * g_i plus (double)bg * bg, then sqrt.  An axpy with an
 *   fp64 factor is y <- fl32((double)y + a * (double)x); with an fp32 factor it is fp32 throughout.  r / M is the fp32 quotient.  With
 *   bias <= 0 every bias part stays 0.
 *   fun:  wx_i = fl32((double)(w . x_i) + bias * (double)b) (bias > 0; else the dot); f = sum over index of (double)c_i * t * t with t = 1 -
 *     (double)y_i * wx_i where t > 0, an fp64 chain in index order, + 0.5 * wTw; wTw = (double)(w . w) + (double)b * b.
 *   grad: in index order tmp_i = wx_i * y_i (fp32); where tmp_i < 1, instance i is active: I[sizeI] = i and tmp[sizeI] = (c_i * y_i) *
 *     (tmp_i - 1) (fp32).  THE REFERENCE COMPACTS INTO tmp ITSELF: an instance whose row id is below sizeI at its turn overwrites that
 *     compacted slot with its raw tmp_i, and X_I' reads it.  This happens when a positive that M does not list is appended to index and
 *     its row id is below the count of active instances then; it is reproduced as written.  g = w + 2 * sum_I tmp[k] * x_I[k] (fp32 axpys
 *     in I's order, then x + 2y in fp32); bg = b + 2 * (sum of fl32((double)bg + bias * (double)tmp[k])).
 *   newton: w = 0; f, g at 0; gnorm0 = gnorm = norm(g).  gnorm <= eps * gnorm0 ends before the first iteration.  Up to 1000 iterations
 *     (NEWTON's own default: max_iter is NOT used): M = 1 + sum_I (x * x) * (2 * c_i) (fp32), bM = 1 + sum of bias * bias * 2 * (double)c_i
 *     rounded per term, then M <- fl32(0.99 + 0.01 * (double)M); s = pcg(); the line search; a step of 0 ends the job; grad; gnorm <= eps *
 *     gnorm0 ends it; so does |fold - f| <= 1e-12 * |f|.
 *   pcg: s = 0, r = -g, z = r / M, d = z; zTr = z . r; cgtol = min(0.5, sqrt(sqrt(zTr))); at most max(d + (bias > 0), 5) steps WITH d THE
 *     FEATURE COUNT OF X: Hd = d + 2 X_I' (c .* (X_I d)) with xTs_i = (double)c_i * ((double)(d . x_i) + bias * (double)bd) and fp64-factor
 *     axpys; dHd = d . Hd; dHd <= 1e-16 ends; alpha = zTr / dHd; s += alpha d; r -= alpha Hd; newQ = -0.5 * (double)fl32((s . r) - (s . g)) -
 *     0.5 * (double)fl32(bs * br - bs * bg); newQ <= 0 and newQ - Q <= 0 or the run ends ("quadratic approximation > 0"); step * (newQ - Q) >=
 *     cgtol * newQ ends; z = r / M; beta = (z . r) / zTr; d <- fl32((double)d + (beta - 1) * (double)d), then d <- fl32((double)d + (double)z).
 *   line search (l2r_l2_svc_fun's own; the base class's is dead code): tmp = X s (as wx above, with bs), sTs, wTs, gTs; alpha = 1, up to 20
 *     times: f = loss(wx + alpha * tmp) + (alpha * alpha * sTs + wTw) / 2 + alpha * wTs; f - fold <= 0.01 * alpha * gTs accepts, else alpha
 *     halves.  Accepted: wx_i <- fl32((double)wx_i + alpha * (double)tmp_i) ONCE PER LISTED POSITION, w += alpha s, b += alpha bs, wTw +=
 *     alpha * alpha * sTs + 2 * alpha * wTs.  After 20 halvings f = fold and the step is 0.
 *   wx and wTw (updated by the line search, read by grad and the next line search) and sizeI and I (from grad into the preconditioner
 *     and Hv) persist across the calls.
 * The compressed form.  A feature that no instance of a job stores stays +-0 in every vector and 1 in M, adds +-0 to chains that start at
 *   +0, and is emitted as +0.  The device therefore walks only the job's touched features, in ascending order -- as long as every scalar
 *   multiplied into a vector is finite.  A job whose pcg meets a non-finite alpha or beta fails the call, naming the first such label; a
 *   non-finite value stored in X fails it before training (a check kernel).  Cp, Cn, eps, bias, threshold and R's values are used as given.
 * Refused before a GPU is required, with the function's name first: solvers 1 and 3 (the message names the entry point above that serves
 *   them), 7 (its inner Newton steps call log in fp64, and the device's log is not the host library's), unknown solvers; and every
 *   refusal of the entry points above (nulls, shapes, two devices, 2^31 rows, 2^32 - 1 jobs, a label twice in C, R's pattern).
 *   xrl_single_layer_train_newton_csr_f32 / _drm_f32   xrl_single_layer_train_*'s argument lists and result, solver_type == 2
 *   xrl_train_layer_newton_device   xrl_train_layer_device's argument list and result: a NEW owned W^T handle
 *   xrl_debug_newton_counters    FOR TESTS ONLY: of the last primal training of this process, out[0..n), n <= 20 <- {jobs, batches, slots,
 *                                staging stride, Newton iterations, CG steps, Hv calls, line-search halvings, jobs ended before the
 *                                first iteration, jobs ended by the gradient test, by a failed line search, by a small actual reduction,
 *                                by the 1000-iteration cap, CG runs ended by dHd <= 1e-16, by the Q test, by a positive quadratic
 *                                approximation, by the step cap, instances (per listed position) whose feature row is summed one per
 *                                lane, by a wavefront (64 entries and more), jobs flagged non-finite} */
void xrl_single_layer_train_newton_csr_f32(const ScipyCsrF32* pX, const ScipyCscF32* pY, const ScipyCscF32* pC, const ScipyCscF32* pM, const ScipyCscF32* pR,
                                           py_coo_allocator_t coo_alloc, double threshold, uint32_t max_nonzeros_per_label, int solver_type, double Cp, double Cn,
                                           size_t max_iter, double eps, double bias, int threads);
void xrl_single_layer_train_newton_drm_f32(const ScipyDrmF32* pX, const ScipyCscF32* pY, const ScipyCscF32* pC, const ScipyCscF32* pM, const ScipyCscF32* pR,
                                           py_coo_allocator_t coo_alloc, double threshold, uint32_t max_nonzeros_per_label, int solver_type, double Cp, double Cn,
                                           size_t max_iter, double eps, double bias, int threads);
void* xrl_train_layer_newton_device(void* X, void* Yt, void* Ct_or_null, void* Mt_or_null, void* Rt_or_null, double threshold, uint32_t max_nonzeros_per_label,
                                    int solver_type, double Cp, double Cn, uint64_t max_iter, double eps, double bias, void* hip_stream);
int xrl_debug_newton_counters(uint64_t* out, uint32_t n);

/* Matcher-aware negatives (MAN) on the device: what joins a trained layer, its prediction and the next layer's matching matrix in HBM
 * (K14, csrc/xrl_match.hip; pecos_amd.train_chain_device runs the reference's loop, pecos/xmc/base.py:1512-1572, over them).
 * Rule U, xrl_smat_pattern_union_device(mats, n): n >= 1 matrix handles of one shape on one device.  A NEW owned CSR handle of that shape
 *   that stores 1.0f at (r, c) wherever at least one operand stores an entry at (r, c).  Values are never read: explicit zeros, NaN and
 *   negative values count.  An operand's row may store its columns in any order (a handle of xrl_smat_from_device_result is best first)
 *   and the same column more than once; every output row is strictly ascending, the row pointer u64.  This is the reference's
 *   M = csc_matrix(shape); M += binarized(A); M += binarized(B); ...; sort_indices() (base.py:1544-1565, 570-573) up to the values: where
 *   the reference stores 2.0 or 3.0 (an entry listed by two or three sources) this stores 1.0 -- the trainer reads only M's pattern.
 *   One wavefront per row orders the operands' column ids in LDS (rows of at most 1024 stored entries over all operands; longer rows
 *   through a segmented sort in HBM) and drops equal neighbours; count, scan, fill.  Runs on hip_stream and synchronises it.
 *   Refused, messages starting with the function's name.  Before a GPU is required: n == 0, a null handle, shapes that differ, operands
 *   on two devices.  By a check kernel: a column id that is not below cols (a refusal, the id is never an address); a row that stores 2^31
 *   entries or more over the operands.  NULL + xrl_last_error on failure.
 * Rule P, xrl_single_layer_predict_device: the resident form of c_xlinear_single_layer_predict_csr_f32 -- the same rule and the same bits,
 *   because it runs the same CSC route (K0 -> K1C -> K2) through the same row batches under the same workspace budget.  X: a CSR handle
 *   of the instances, read in place.  Wt: labels x (features + (bias > 0)), the CSC of W as xrl_train_layer_device leaves it, copied
 *   device to device (W never visits the host).  Ct: clusters x labels, the handle training took, copied to the host once for the tree
 *   bookkeeping (nr_labels entries); NULL = one cluster that holds every label.  Codes: a fixed-stride result in HBM (row r is
 *   d_codes_idx / d_codes_val [r * codes_stride ..], d_codes_cnt[r] entries; a count above the stride reads as the stride), used in place
 *   as the initial beam; a parent may be listed more than once and every occurrence is prolongated.  All three NULL = no csr_codes:
 *   with one cluster the implicit root, with several fill_ones (every cluster, score 1, no combine; libpecos.cpp:215-222).  The candidate
 *   row is sized by one kernel over the codes -- per row the sum over listed parents of their child counts, max-reduced -- and ONE 8-byte
 *   readback: after the copy of C, the call's only host synchronisation before the result.  Result: xrl_predict_device's contract -- row r of d_out_idx /
 *   d_out_val (row stride out_stride >= only_topk) holds d_out_cnt[r] pairs best first, entries beyond the count untouched, labels in the
 *   layer's own ids.  Runs on hip_stream (NULL: the default stream is synchronised, then a stream of the call's own) and synchronises it.
 *   Refused, messages starting with the function's name: null handles or outputs; only_topk == 0; out_stride < only_topk; codes given in
 *   part; operands on two devices; "Feature dimension of query and W do not match"; "Label dimension of C and
 *   W do not match"; by the bound kernel, "csr_codes: parent id .. out of range" (found and refused, never followed).  0 / -1.
 *   XRL_SINGLE_LAYER_MAX_BATCH_ROWS in the environment is the predict option max_batch_rows of the call's one-layer handle (tests).
 * Rule C, xrl_smat_check_relevance_device(Y, R, status): does R store exactly Y's entries and no negative value -- what MLProblem asks of a
 *   relevance matrix (check_relevance), answered in HBM.  Y and R: CSR handles of one shape on one device (both read as stored, so hand in
 *   both in the same orientation).  status[0] <- 0: equal row pointers, equal column ids position by position, no value of R below 0;
 *   1: the row pointers differ; 2: the column ids differ; 3: a value of R is below 0 (-0.0 and NaN are not below 0).  The code is the
 *   first of these that the host check meets (1 before 2 before 3); status[1] <- the first row that offends so (for code 1: the first row
 *   whose end differs).  One pass, one wavefront per row, every span clamped to both nnz; one readback; runs on hip_stream and
 *   synchronises it.  Refused before a GPU is required: null handles, dense handles, null status, shapes that differ, two devices.  0 / -1.
 *   xrl_debug_match_forms        FOR TESTS ONLY: out[0..n), n <= 5 <- {rows served in LDS, rows served by the HBM sort, entries read,
 *                                entries written (all four summed over the unions since the load), the candidate bound of the last
 *                                xrl_single_layer_predict_device} */
void* xrl_smat_pattern_union_device(void* const* mats, uint32_t n, void* hip_stream);
int xrl_single_layer_predict_device(void* X, void* Wt, void* Ct_or_null, const uint32_t* d_codes_idx, const float* d_codes_val, const uint32_t* d_codes_cnt,
                                    uint32_t codes_stride, const char* post_processor, uint32_t only_topk, float bias, uint32_t* d_out_idx, float* d_out_val,
                                    uint32_t* d_out_cnt, uint32_t out_stride, void* hip_stream);
int xrl_smat_check_relevance_device(void* Y, void* R, uint64_t* status, void* hip_stream);
int xrl_debug_match_forms(uint64_t* out, uint32_t n);

/* HNSW search on the device (K17, csrc/xrl_hnsw.hip): a folder saved by the reference's HNSW.save (c_model/: config.json + index.mmap_store) is
 * loaded into HBM and queried there; ids, order and distance bits are those of c_ann_hnsw_predict_{csr,drm}_{ip,l2}_f32 on the same folder
 * (sparse: on any x86 host; dense: the reference's avx512f clone -- DESIGN.md section 9 states both distance rules, the traversal and the
 * libstdc++ heaps).  Search only: nothing here trains or saves a graph, and the product-quantised index is not loaded.  The names are this
 * library's own on purpose: a handle of one library is never a handle of the other.
 *   xrl_hnsw_load(model_dir, device, &handle)   reads config.json (hnsw_t selects csr/drm x ip/l2; any other string is refused with "Inconsistent
 *       HNSW_T: ...", a version other than v2.0 with "Unable to load memory-mapped file with version = ..."), reads index.mmap_store, checks
 *       on the host and refuses by name: a neighbour id >= num_node, a degree above maxM0 / maxM, a node listed twice in one neighbourhood,
 *       init_node >= num_node, a sparse item whose ids are not strictly ascending or reach feat_dim, a non-finite stored value, records that
 *       leave the buffer.  Then splits the interleaved node records into arrays and uploads them.  0 / -1 + xrl_last_error.
 *   xrl_hnsw_check_folder(model_dir, out, n)    the same reading and the same refusals without a GPU; out as xrl_hnsw_info.  0 / -1.
 *   xrl_hnsw_info(handle, out, n)               out[0..n), n <= 10 <- {num_node, feat_dim, maxM, maxM0, efC, max_level, init_node, data type
 *       (0 csr, 1 drm), metric (0 ip, 1 l2), bytes held in HBM}.
 *   xrl_hnsw_searchers_create(handle, n)        device scratch for n wavefronts (at most 2048): visited marks and cand heaps.  A predict without
 *       searchers allocates per call and sizes the slots itself.  NULL + xrl_last_error on failure.  A searchers handle serves the index it was
 *       made for and ONE call at a time (a call regrows and reuses its work buffers until its last synchronisation): a call that finds the
 *       handle in use, on another thread or stream, is refused by name and never queued; make one handle per concurrent caller.
 *   xrl_hnsw_predict_{csr,drm}_f32              the reference's argument list on host arrays; `threads` is accepted and ignored.  Uploads,
 *       searches, copies back; row r writes its found entries (at most topk) at r * topk and leaves the rest of the row untouched.
 *       Finite inputs are served whatever their distances become: a distance that overflows is +inf or -inf as the reference's, a NaN distance
 *       (inf + -inf; the inputs are finite, so it is never a caller's NaN) carries the x86 host's default NaN 0xFFC00000, and NaNs sit in a
 *       row where libstdc++'s heaps leave them under the reference's comparisons, which are all false under a NaN -- among the numbers, not
 *       after them.  Subnormal distances are kept.  The same holds for xrl_hnsw_predict_device.
 *   xrl_hnsw_predict_device                     the resident form.  Queries: dense [rows, cols] at d_val with row_stride >= cols (d_row_ptr NULL), or
 *       a CSR triple d_row_ptr u64 [rows + 1], d_col_idx u32, d_val f32 with nnz stored entries.  Outputs d_idx / d_dist with row stride
 *       out_stride >= topk, and d_count [rows].  Runs on hip_stream; one synchronisation at the end, for the overflow flag of the cand heaps
 *       (a query that overflows its slot's cand capacity -- 4096 entries, XRL_HNSW_CAND_CAP in the environment for tests -- runs again with
 *       an entry per node).
 *   Refused by name, outputs unchanged: a null handle, the wrong data type for the handle, cols != feat_dim, topk == 0, efS == 0, out_stride <
 *   topk, row_stride < cols, null outputs, searchers of another index or in use, and by a check kernel row pointers that are not ascending within nnz, a query row with unsorted, repeated or out-of-range ids or a non-finite query value.  0 / -1.
 *   xrl_debug_hnsw_counters(out, n, reset)      FOR TESTS: out[0..n), n <= 8 <- {distance evaluations, pops, admissions, upper-level passes, the
 *       largest cand size, queries rerun, queries served by the LDS form of the topk heap, by the HBM form}, summed since the last reset.
 *       The first five count the attempt of a query that produced its answer: what an abandoned attempt (a cand heap that overflowed) did
 *       before it stopped is NOT counted, so they equal the reference's traversal and understate the work done by what the reruns repeat.
 *   xrl_debug_hnsw_caps(out, n)                 out[0..n), n <= 4 <- {CAP (largest efS' = max(efS, topk) of the LDS form), the default cand capacity,
 *       the largest degree staged in LDS, the largest slot count} */
int xrl_hnsw_load(const char* model_dir, int device, void** handle);
int xrl_hnsw_check_folder(const char* model_dir, uint64_t* out, uint32_t n);
void xrl_hnsw_destruct(void* handle);
int xrl_hnsw_info(void* handle, uint64_t* out, uint32_t n);
void* xrl_hnsw_searchers_create(void* handle, uint32_t num_searcher);
void xrl_hnsw_searchers_destruct(void* searchers);
int xrl_hnsw_predict_csr_f32(void* handle, const ScipyCsrF32* pX, uint32_t* ret_idx, float* ret_val, uint32_t efS, uint32_t topk, int32_t threads, void* searchers);
int xrl_hnsw_predict_drm_f32(void* handle, const ScipyDrmF32* pX, uint32_t* ret_idx, float* ret_val, uint32_t efS, uint32_t topk, int32_t threads, void* searchers);
int xrl_hnsw_predict_device(void* handle, uint32_t rows, uint32_t cols, const float* d_val, uint64_t row_stride, const uint64_t* d_row_ptr, const uint32_t* d_col_idx,
                            uint64_t nnz, uint32_t efS, uint32_t topk, uint32_t* d_idx, float* d_dist, uint32_t* d_count, uint64_t out_stride, void* searchers,
                            void* hip_stream);
int xrl_debug_hnsw_counters(uint64_t* out, uint32_t n, int reset);
int xrl_debug_hnsw_caps(uint64_t* out, uint32_t n);

/* predict_on_selected_outputs on the device (K7 + K4): score a given set of labels per query row through the tree, with labels, plan and
 * scores resident in HBM.  The labels arrive in the fixed-stride form xrl_predict_device writes and xrl_ensemble_device reads: row r is
 * d_sel_idx[r*sel_stride ..], d_sel_cnt[r] entries long (NULL = sel_stride each; a count above the stride is read as the stride), in any
 * order.  `queries` is any query handle of the model's device (CSR or dense, uploaded or wrapping caller memory); its rows are the rows.
 * Result: row r of d_out_idx / d_out_val (row stride out_stride >= sel_stride) holds d_out_cnt[r] (label, score) pairs -- the labels in the
 * order the reference's walk emits them for that set (prolongate_sparse_predictions, inference.hpp:1302-1358: the order of
 * c_xlinear_predict_on_selected_outputs_*), the scores its CSC-route arithmetic, bit for bit what that entry point returns.  Entries
 * beyond a row's count are left untouched.  post_processor NULL = each layer's own.
 * Bad rows: a row with a label >= nr_pred_cols (code 1), a label twice (2) or a label without a parent in some layer (3: pruned tree) gets
 * count 0; every other row is still correct.  d_status (u32[2], may be NULL) receives {code, row} of the LOWEST bad row, or
 * {0, 0xFFFFFFFF} when there is none.  With `sync` != 0 the library reads the status itself: on a bad row the call returns -1 and
 * xrl_last_error holds the host entry point's message for that row.  With `sync` == 0 the call returns 0 without synchronising and the
 * status is the caller's to read, in stream order.
 * One plan launch and one scoring launch per layer run on `hip_stream` (NULL = the handle's stream, as for xrl_predict_device), without a
 * host synchronisation between them.  Capacity: sel_stride <= 1024 labels per row (longer rows: the host entry point); trees only (a C
 * that lists a node under two parents is refused); mmap handles are refused like the host entry point refuses them.  Every argument is
 * checked before the GPU is touched (messages start with "xrl_predict_selected_device: "); zero rows is a successful no-op. */
int xrl_predict_selected_device(void* model, void* queries, const char* post_processor /* NULL = each layer's own */,
                                const uint32_t* d_sel_idx /* u32[rows*sel_stride] */, const uint32_t* d_sel_cnt /* u32[rows]; NULL = sel_stride each */,
                                uint32_t sel_stride,
                                uint32_t* d_out_idx, float* d_out_val, uint32_t* d_out_cnt, uint32_t out_stride /* >= sel_stride */,
                                uint32_t* d_status /* u32[2] {code, row}; may be NULL */, void* hip_stream, int sync);

/* OUTPUT CONSTRAINT: XLinearModel.set_output_constraint (pecos/xmc/base.py:1796-1824) on a loaded handle.  The beam search of the handle is
 * restricted to the given labels: a constrained predict returns, bit for bit (ids, order, scores, counts), what the same library -- or the
 * reference -- returns for a model folder whose C matrices were pruned by the reference's rule (bottom-up: delete every entry of C whose row
 * is not kept, keep for the layer above the columns that still hold an entry, stop at the first layer of which every node is kept), under
 * the handle's weight_matrix_type, for sparse and dense X.  Nothing is rewritten or recompiled: per layer, a second (child range, child id)
 * pair of arrays that lists the kept children in their stored order is built on the device (a few launches per layer), and every layer
 * then runs the CONSTRAINED ROUTE -- offsets, one 16-lane inner product per (query, kept child) against the CSC copy of W in the arithmetic
 * of the handle's layout, top-k -- whose grid shrinks with the kept set.  It is not the full-speed path: no bound pruning, no fused layers.
 *   labels / d_labels   n label ids (u32) on the host / in HBM on the handle's device (read on hip_stream, NULL = the handle's stream); any
 *                       order, duplicates allowed; a label the loaded tree does not contain is simply absent from the results
 *   n == 0 is refused.  An id >= nr_pred_cols is refused: xrl_last_error names the lowest such index, and the constraint that was in force
 *   stays in force.  A set that covers every label clears the constraint (the reference's rule stops at once).
 * Honoured by every predict that goes through the beam search on this handle: c_xlinear_predict_{csr,drm}_f32, xrl_predict_device,
 * xrl_predict_device_rows and the tf-idf forms.  NOT affected: the selected-outputs entry points (host and device), the single-layer API and
 * sparse_inner_products.  Refused: mmap handles (no CSC weights), handles with option "devices" > 1 (and "devices" > 1 on a constrained
 * handle), xrl_predict_stats on a constrained handle.
 * Setting and clearing are synchronous: they wait for the whole DEVICE (hipDeviceSynchronize) -- every stream a predict of the handle may run
 * on, the caller's included, and with them the work of every other handle of the process on that device -- and must not run
 * concurrently with a predict on the same handle.  Profile names of the route: "k0_constrained", "k1p_constrained", "k2_constrained".
 * xrl_output_constraint_info: out[0] = 1 if a constraint is in force, out[1 + l] = kept children of layer l (top-down; all of them for a layer
 * above the rule's stop); returns 1 + depth, the number of values available.  The setters and the clear return 0 on success, -1 with a message otherwise.
 * xrl_debug_output_constraint_view: FOR TESTS ONLY, NOT A STABLE INTERFACE (like the other xrl_debug_* entry points it may change or go
 * without notice): the kept-child ranges (n_parents + 1 words) and kept child ids of one layer; returns 1, or 0 when the layer runs on its
 * own arrays. */
int xrl_set_output_constraint(void* model, const uint32_t* labels, uint64_t n);
int xrl_set_output_constraint_device(void* model, const uint32_t* d_labels, uint64_t n, void* hip_stream);
int xrl_clear_output_constraint(void* model);
int xrl_output_constraint_info(void* model, uint64_t* out, uint32_t cap);
int xrl_debug_output_constraint_view(void* model, uint32_t layer, uint32_t* chunk_col_out, uint64_t chunk_col_cap, uint32_t* perm_inv_out, uint64_t perm_inv_cap);

/* Effective only_topk of the last layer for the given override (0 = model default). */
uint32_t xrl_effective_topk(void* model, uint32_t only_topk);

/* Profiling: when enabled, every kernel launch of predict is bracketed by a hipEvent pair recorded
 * on the stream the kernel is launched on (no synchronisation is added to the predict call).
 * xrl_profile_get synchronises, folds the pending pairs and fills up to `cap` records; it returns
 * the number of records available. */
typedef struct {
    char name[32];          /* kernel family: "k0_prolongate", "k1_sparse", "k1_dense", "k1q_dense", "k1q_dense_x", "k1c_csc", "k2_topk"; the constrained route: "k0_constrained", "k1p_constrained", "k2_constrained" */
    uint32_t layer;
    uint32_t launches;
    double ms;              /* accumulated GPU time of those launches */
    double reserved;
} xrl_profile_rec_t;
void xrl_profile_enable(void* model, int enable);
void xrl_profile_reset(void* model);
uint32_t xrl_profile_get(void* model, xrl_profile_rec_t* out, uint32_t cap);

/* One untimed predict (tile-format kernels) that also counts, per layer l, 8 doubles at stats_out[8l ...]:
 *   [0] algorithmic bytes of the reference-layout chunks streamed (8*E_p + 4*R_p + 4*(R_p+1) per (query, beam parent),
 *       every active chunk whole, no inter-query reuse)      [1] candidates evaluated
 *   [2] (query, tile) items   [3] row lookups (query features x items)   [4] matched tile rows   [5] entries of the matched rows
 *   [6] tile columns over the items (scores written)   [7] query features x tile columns over the items (dense-format weights)
 * [2..7] are the MATCHED work bench.py's roofline model is built from.  stats_cap >= 8*depth.  Returns 0 on success. */
int xrl_predict_stats(void* model, void* queries, uint32_t beam_size, const char* post_processor,
                      uint32_t only_topk, double* stats_out, uint32_t stats_cap);

/* Host-only pieces of the model compiler, exported so that they can be tested without a GPU.
 * xrl_debug_split_chunk: number of even column tiles for a chunk of n columns whose entry-count prefix sums are
 *   cum[0..n], such that every tile has <= 128 columns and fewer than `limit` entries (0: impossible).
 * xrl_debug_layout_rows: places a tile's rows (rptr[0..nrows] = packed CSR starts); with align != 0 a row that would touch
 *   more 128-byte lines than its length requires starts on the next 16-entry boundary.  Writes one packed extent
 *   `offset | (len-1) << 25` per row to ext_out (may be NULL) and returns the padded entry count of the tile. */
uint32_t xrl_debug_split_chunk(const uint64_t* cum, uint32_t n, uint64_t limit);
uint64_t xrl_debug_layout_rows(const uint32_t* rptr, uint32_t nrows, int align, uint32_t* ext_out);
/* Host-only piece of the host ABI: the row batches c_xlinear_predict_{csr,drm}_f32 cuts an X of this shape into at option
 * "host_batch_mb" (with "host_pipeline" on).  row_ptr[0..rows] for a CSR X, NULL for a dense rows x cols X.  Writes the boundaries
 * rb[0] = 0 <= ... <= rb[n] = rows to rb_out (at most cap of them; may be NULL) and returns their number n + 1. */
uint32_t xrl_debug_host_batches(const uint64_t* row_ptr, uint32_t rows, uint32_t cols, int host_batch_mb, uint32_t* rb_out, uint32_t cap);

/* Host-only piece of the per-query top-k (K2): the form launch_k2_topk takes for a layer that keeps k of the cand_stride candidates a query row
 * reserves, at option "k2_big_min_k".  stage: 0 = the whole row in one launch, 1 = a stage of the bound pruning on the batch-sized grid (limited_cands:
 * the most candidates a rank-limited stage looks at, 0 = the row), 2 = its last stage on the list of unfinished queries.  Returns 0 = k2_topk_wave<NS>,
 * 1 = k2_topk_list<NS>, 2 = k2_topk_reg, 3 = k2_topk_lds, 4 = the segmented sort (launch_k2_topk_big), or -1 with a message for a launch the library
 * refuses (k = 0; a pruning stage beyond the wave form's reach); *ns_out (may be NULL) receives NS for forms 0 and 1, else 0.  The launch itself
 * dispatches on this function. */
int xrl_debug_k2_form(uint32_t k, uint32_t cand_stride, int64_t k2_big_min_k, int stage, uint32_t limited_cands, uint32_t* ns_out);

/* Tuning knobs (benchmark / tests only).  Results never depend on them.
 *   "k1_group"            lanes per (query, tile) item in K1: 0 = auto, else a power of two <= 64
 *   "max_batch_rows"      rows of X per internal batch (0 = auto: candidate buffer <= 6 GiB)
 *   "sort_min_tiles"      tile-sort the items of layers with at least this many tiles (0 = never)
 *   "adaptive"            1 (default): PRUNING FEEDBACK -- the handle remembers, per layer, what the first stage of the bound pruning achieved on its
 *                         previous predicts (sampled device counters / the later stage's item count, read back without any synchronisation);
 *                         a layer whose first stage settled fewer than ~35 % of the queries runs UNSTAGED on the following predicts (every
 *                         candidate in one pass; tile format: on tile-sorted items) and is probed again every 32nd predict; 0: always staged
 *   "presence"            1 (default): K1Q on sparse X asks the layer's PRESENCE words (one bit per (feature, 16..32-column parent tile): "holds a weight")
 *                         before requesting a weight segment, on the layers that run unstaged -- prune = 0, or switched by the pruning feedback:
 *                         there every beam parent's segments are addressed and a third to a half of them are empty (Amazon-670K-hard: levels 0-3
 *                         11.9 -> 7.5 ms); 2: on every layer that has the words; 0: never.  XRL_PRESENCE=0 at load builds none.
 *   "prune_mid"           1 (default): bound-pruned tile-format layers entered with >= 16 beam parents score slots 1..4 in a MIDDLE stage before
 *                         "every remaining slot" (three stages instead of two; Wiki10-31K's beam of 20); 0: two stages
 *   "leaf_fuse"           1 (default): the FIRST stage of a bound-pruned tile-format layer is one launch where K1T serves it with 32 lanes per item, every
 *                         parent is one tile (<= 128 children) and k <= 20 -- the kernel derives its item from the beam (beams of up to 32 parents; no
 *                         k0_prolongate launch), ranks the candidates in its epilogue and sets the done flags (no k2_topk launch); 2: ... but the
 *                         items still come from a k0_prolongate launch; 0: three launches (K0 -> K1 -> K2)
 *   "leaf_tail"           1 (default): bound-pruned tile-format layers of TWO stages (beams of fewer than 16 parents, or prune_mid = 0): the first stage also
 *                         lists the queries it left unfinished, and the later stage's launches walk that list -- k0b_remaining and k2_topk_rest on a small
 *                         fixed grid, K1 on a fixed grid of 6144 workgroups once the pruning feedback's last item count is known and at most an eighth of
 *                         a worst-case grid of >= 2^21 item slots; n >= 2: ... and K1 always on a fixed grid of n workgroups (A/B runs, tests);
 *                         0: launches sized for the whole batch.  Results never depend on it.
 *   "sort_rest"           1 (default): the second phase of a bound-pruned tile-format layer runs on tile-sorted items (counting sort of the
 *                         compacted list by tile: the items of a tile run back to back on one XCD and share its lookup words and entries in
 *                         that XCD's L2); 0: in query order
 *   "sort_rest_min"       32768 (default): ... and only while the later stages of the handle's previous predicts held at least max(this many, 32 per tile
 *                         of the layer) items (the pruning feedback's count): below that the sort's four launches cost more than the locality buys; 0: always sort
 *   "qsort"               1 (default): K1Q, sparse X -- the LAST layer of a run of dense-format layers is launched on its own, on queries counting-sorted
 *                         by the best parent of their beam, every XCD taking a contiguous eighth of the sorted order (queries of one region of the
 *                         tree share (feature, parent) segments in that XCD's L2), when the layer has >= "qsort_min_parents" (64) parents and the
 *                         row batch >= "qsort_min_rows" (131072) rows; 0: never.  Results do not depend on it (round 5: L2 misses -27 %, time unchanged).
 *   "host_register"       host ABI: 1 = page-lock the caller's X arrays in place for the duration of the call (hipHostRegister) and let
 *                         the copy engine read them directly, instead of staging them through two pinned buffers with host threads
 *   "devices"             MULTI-GPU BEHIND THE DROP-IN ENTRY POINTS: the handle serves c_xlinear_predict_{csr,drm}_f32 from this many
 *                         devices -- its own plus value-1 replicas of the compiled model on the following devices (wrapping around when
 *                         the box has fewer).  A predict then cuts X into nnz-balanced row shards, one host thread + stream + pinned
 *                         staging per device, no inter-GPU traffic, results of all shards into the arrays of the ONE allocator call.
 *                         Only for models loaded from a folder.  c_xlinear_get_int_attr "nr_devices" reads it back.
 *   "prune"               1 (default): EXACT bound pruning -- a layer scores the children of the best beam parent(s) first (tile format: one
 *                         parent; dense row format and the dense-X SGEMM: as many as fill 64 candidates) and skips the other parents
 *                         for every query whose k-th best candidate already reaches the next parent's bound (every post-processor with
 *                         a combiner keeps a child's score <= max(its parent's, 0) resp. <= its parent's, and later candidates lose
 *                         ties by position), so the result is unchanged bit for bit; NaN parent scores and "noop" disable it per
 *                         query / layer; 0: every candidate of every beam parent is scored (what the reference evaluates)
 *   "overlap_min_rows"    split predicts of at least this many rows into two batches on two streams (0 = never)
 *   "reserve_rows"        sizes the host ABI's result buffers (pinned host + device, rows x the model's default top-k) for calls of up to this many rows NOW
 *                         instead of inside the first large call.  (Everything that does not depend on X -- copy threads, streams, the pinned upload
 *                         ring, kernel code objects, both scratch lanes for 65 536-row batches -- is created when a model is loaded from a folder;
 *                         the environment variable XRL_WARM=0 turns that off.)
 *   "host_batch_mb"       12 (default): CSR input of the pipelined host ABI is computed in batches that grow x1.6 from a third of this
 *                         many megabytes of (column id, value) pairs up to three times it (measured on Amazon-670K: 12 -> 10.4 ms per
 *                         call, 24 -> 12.1, 36 -> 13.0)
 *   "host_pipeline"       1 (default): c_xlinear_predict_* cut a large X into nnz-balanced row batches; batch b+1 is staged into
 *                         pinned memory and uploaded on a copy stream while batch b computes; 0: one synchronous upload
 *   "dense_layers"        1 (default): layers that carry the dense row format run the fused query-stationary kernel K1Q
 *                         whenever the beam's candidates fit its registers and, for sparse X, the format moves fewer lines than the
 *                         tile format's row lookup (parents of <= 32 padded columns, or >= 1 weight per (feature, parent) segment);
 *                         2: whenever they fit (tests); 0: tile-format kernels K0 -> K1 -> K2 everywhere
 *   "k1q_fuse"            3 (default): consecutive dense-format layers of <= 3 candidate registers per lane (<= 192 candidates per
 *                         query) run in ONE K1Q launch, the wavefront that owns a query carries its beam through them in LDS;
 *                         1 / 2: only layers of <= 1 / 2 registers share a launch; 0: one launch per layer
 *   "k1g_min_items"       dense X: a dense-format layer runs the tiled, k-ordered SGEMM K1G (tile-sorted items, weight and query
 *                         panels staged in LDS) once a parent serves this many queries on average (default 16; 0 = never: K1Q)
 *   "k1g_variant"         1: the alternative register-tile / panel shapes of K1G (A/B, tests; results identical)
 *   "k1g_first"           K1G layers under bound pruning: beam parents scored in the first stage (0 = default: about one candidate register,
 *                         64 / children per parent)
 *   "tile_rows"           tile-format layers that carry densely held tile rows, sparse X: 1 (default) = launches on items in query order run
 *                         K1T, 2 = every launch, 0 = always the entry-list kernel K1
 *   "k2_big_min_k"        > 0: top-k sizes from this value on take the segmented-sort K2 that otherwise serves k > 20 480 (tests); 0 (default)
 *   "k1_wpb", "k1_lds_pad", "k1_ablate"   debug: wavefronts per K1 workgroup, extra LDS per wavefront, phase ablation
 * Environment read at model load: XRL_LOOKUP=bitmap|bitmap64|bucket (force the row
 * lookup structure; default per layer: bucket table if rank-bitmaps would take more than a quarter of the free HBM, else
 * 64-feature words carrying the first row's extent on sparse tiles, else 32-feature words),
 * XRL_ROW_ALIGN=0 (keep tile rows packed instead of line-aligned), XRL_MAX_TILE_ENTRIES (lower the tile splitter's
 * limit; tests), XRL_DENSE=0 (never build the dense row format), XRL_DENSE_MAX_MB (cap of one layer's dense matrix;
 * default 65536, and never more than a quarter of the free HBM). */
int xrl_set_option(void* model, const char* key, int64_t value);

/* Debug: with option k1_ablate bit 6 set, K1 accumulates per-phase shader cycles
 * [prologue, fill, D1, D3, epilogue, #waves, -, -]; this reads (and optionally resets) them. */
void xrl_debug_k1_phases(unsigned long long* out8, int reset);

/* Single-layer API (c_xlinear_single_layer_predict*): compiled one-layer handles are cached by the identity of the caller's
 * W / C value arrays (pointers, shapes, nnz, bias) plus a 64-bit hash of EVERY byte of all their arrays (an in-place edit is seen on
 * the next call), at most 8 entries, least recently used evicted.  stats: cumulative hits / misses and live entries (tests). */
void xrl_single_layer_cache_clear(void);
void xrl_single_layer_cache_stats(uint64_t* hits, uint64_t* misses, uint64_t* entries);

/* Device layout of one layer: out[0..12) = {row lookup of the tile format (0 = 32-feature rank-bitmap, 1 = bucket table,
 * 2 = 64-feature words with the first row's extent), bucket search levels, carries the dense row format (0/1), padded dense
 * tile width, padded columns per dense row, tiles, weights (entries), bytes of the dense matrix, W.rows, children kept,
 * widest tile, bytes of HBM}.  Returns the number of values available. */
uint32_t xrl_layer_info(void* model, uint32_t layer, uint64_t* out, uint32_t cap);

/* Bytes of HBM held by the compiled model. */
uint64_t xrl_model_device_bytes(void* model);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* XRL_ABI_H */
