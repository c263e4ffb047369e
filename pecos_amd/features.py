"""Query-side hand-offs for callers that produce X on the GPU or in pieces.

* :func:`concat_features` -- host mirror of ``TransformerMatcher.concat_features``
  (pecos/xmc/xtransformer/matcher.py:864-890): [numerical features | (row-normalised) embeddings], the matrix
  XR-Transformer's ``concat_model`` predicts on (pecos/xmc/xtransformer/model.py:589-603).
* :func:`tfidf_weight` / :func:`predict_tfidf_from_torch` -- the weighting half of the reference's TF-IDF vectorizer
  (``BaseVectorizer::get_sorted_feature``, pecos/core/utils/tfidf.hpp:798-822): term counts -> tf -> x idf -> l1/l2 norm, as a host
  mirror (numpy float32, sequential like the reference) and as a device kernel feeding the beam search without a host round trip.
* :func:`predict_from_torch` -- X already in HBM as torch tensors (a GPU TF-IDF featurizer's CSR -- the reference's
  ``c_tfidf_predict`` produces that CSR on the host, pecos/core/libpecos.cpp:427-445 -- optionally with a dense embedding block to
  append on the device): no host round trip of X, results stay on the device.
* :func:`predict_selected_from_torch` -- ``predict_on_selected_outputs`` with the queries and the labels to score in HBM (K7 + K4): re-scores
  one model's candidates with another without a host round trip.
* :func:`ensemble_device` -- the results of several models merged on the device (K6) like ``CsrEnsembler.average`` / ``rank_average`` /
  ``Text2Text.predict``'s tail; :func:`predict_text` and :class:`Text2Text` use it for ensembles that share a device.  ``sigmoid_average``,
  ``softmax_average``, ``round_robin`` and ``only_topk`` go through ``xrl_ensemble_methods_device``; :func:`ensemble_prediction_device` is
  ``TransformerMatcher.ensemble_prediction`` on two device results, :func:`ensemble_host` the same methods on scipy matrices.
* :func:`sparse_matmul_device` / :class:`DeviceMatrix` / :func:`result_to_csr_device` -- the reference's ``clib.sparse_matmul`` with operands and
  product in HBM (K10): a result triple times ``C^T`` (XR-Transformer's descent) or ``C`` (a roll-up of labels to clusters), bit for bit.
* :func:`metrics_device` / :func:`metrics_sums_device` / :class:`Metrics` -- ``smat_util.Metrics.generate`` (precision and recall at
  1 .. topk) from a result in HBM (K8): 2 x topk numbers come back instead of the result.
"""
import collections
import contextlib

import numpy as np
import scipy.sparse as smat

from .core import clib


def concat_features(X_feat, X_emb, normalize_emb=True):
    """matcher.py:864-890 on the host, same operations in the same order (sklearn's ``normalize``, ``dense_to_csr``, ``hstack_csr``)."""
    if normalize_emb:
        from sklearn.preprocessing import normalize as sk_normalize
        X_cat = sk_normalize(X_emb)
    else:
        X_cat = X_emb
    if isinstance(X_feat, smat.csr_matrix):
        # smat_util.dense_to_csr keeps EVERY cell of the dense block as a stored entry (zeros included) and hstack_csr appends
        # it after the row's sparse features (pinned on the reference's outputs, tests/golden/concat/)
        X_cat = np.ascontiguousarray(X_cat, dtype=np.float32)
        n, H = X_cat.shape
        E = smat.csr_matrix((X_cat.ravel(), np.tile(np.arange(H, dtype=np.int64), n), np.arange(n + 1, dtype=np.int64) * H), shape=(n, H))
        X_cat = smat.hstack([X_feat.astype(np.float32), E], format="csr", dtype=np.float32)
    elif isinstance(X_feat, np.ndarray):
        X_cat = np.hstack([X_feat, X_cat])
    elif X_feat is None:
        pass
    else:
        raise TypeError(f"Expected CSR or ndarray, got {type(X_feat)}")
    return X_cat


def result_buffers(rows, k, device, sync=False):
    """The zeroed result triple (labels int32 [rows, k], scores float32 [rows, k], counts int32 [rows]) on ``device``.

    Outputs first: their zero-fills run on torch's current stream, and a predict on any other stream may start only when they (like the
    inputs, produced on that stream) are complete -- ``sync=True`` waits for torch's current stream.  A predict on the current stream
    itself is ordered behind the fills and needs no wait."""
    import torch
    idx = torch.zeros((rows, k), dtype=torch.int32, device=device)
    sc = torch.zeros((rows, k), dtype=torch.float32, device=device)
    cnt = torch.zeros((rows,), dtype=torch.int32, device=device)
    if sync:
        torch.cuda.current_stream().synchronize()
    return idx, sc, cnt


@contextlib.contextmanager
def _device_csr_queries(h, crow, col, val, n_cols, emb, normalize_emb, out_cols):
    """A CSR that is already in HBM (and, with ``emb``, the dense block to append on the device) as a query handle of model handle ``h``,
    with the result triple for ``out_cols`` entries per row: yields ``(q, rows, (idx, sc, cnt))`` and frees ``q`` on exit.  The triple is
    made here because its place is fixed: after the inputs' ``contiguous()`` copies, before the wait that lets the concatenation (which
    runs on the model's stream) read them."""
    import torch
    assert crow.is_cuda and col.is_cuda and val.is_cuda and crow.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
    crow, col, val = crow.contiguous(), col.contiguous(), val.contiguous()
    rows = crow.numel() - 1
    nnz = int(val.numel())
    out = result_buffers(rows, out_cols, val.device, sync=True)
    if emb is not None:
        assert emb.is_cuda and emb.dtype == torch.float32 and emb.shape[0] == rows
        emb = emb.contiguous()
        q = clib.queries_concat_device(h, rows, n_cols, crow.data_ptr(), col.data_ptr(), val.data_ptr(), nnz, emb.shape[1], emb.data_ptr(),
                                       normalize_emb=normalize_emb)
    else:
        q = clib.queries_from_device_csr(h, rows, n_cols, crow.data_ptr(), col.data_ptr(), val.data_ptr(), nnz)
    with clib.freeing(q):
        yield q, rows, out


def predict_from_torch(model, crow, col, val, n_cols, beam_size=None, only_topk=None, post_processor=None, emb=None, stream=None,
                       normalize_emb=False):
    """Beam search on queries that are already on the GPU.

    crow: int64 [rows+1], col: int32 [nnz] (sorted inside every row), val: float32 [nnz] -- CUDA tensors of a CSR with
    ``n_cols`` columns; emb: optional float32 [rows, H] CUDA tensor appended as columns n_cols .. n_cols+H-1 on the device
    (``normalize_emb=True`` l2-normalises its rows on the device first, like the reference's concat_features).  Returns CUDA tensors
    (labels int32 [rows, k], scores float32 [rows, k], counts int32 [rows]); row r holds counts[r] valid entries, best first."""
    import torch
    h = model.model.model_chain
    k = clib.effective_topk(h, only_topk)
    with _device_csr_queries(h, crow, col, val, n_cols, emb, normalize_emb, k) as (q, rows, (idx, sc, cnt)):
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        if rows:
            clib.predict_device(h, q, beam_size, post_processor, only_topk, idx.data_ptr(), sc.data_ptr(), cnt.data_ptr(), k,
                                stream=s or None, sync=True)
    return idx, sc, cnt


def predict_selected_from_torch(model, crow, col, val, n_cols, sel_idx, sel_cnt=None, post_processor=None, emb=None, normalize_emb=False,
                                stream=None):
    """``predict_on_selected_outputs`` with queries AND labels already on the GPU (K7 + K4): the scores of the labels ``sel_idx`` names per row.

    crow / col / val / n_cols / emb / normalize_emb: the queries, as for :func:`predict_from_torch`.  sel_idx: int32 [rows, stride] CUDA tensor
    (stride <= 1024), sel_cnt: int32 [rows] or None (= stride labels in every row) -- the form :func:`predict_from_torch` returns; the order
    of the labels inside a row does not matter.  Returns CUDA tensors (labels int32 [rows, stride], scores float32 [rows, stride], counts
    int32 [rows]): row r holds counts[r] pairs in the order the reference's ``predict_on_selected_outputs`` returns that set, with its scores
    bit for bit.  Raises RuntimeError with the library's message when a row holds a label twice, one out of range or one without a parent.

    The device pieces compose without a host visit: ``predict_from_torch`` of model A (candidates), ``predict_selected_from_torch`` of
    model B on A's ``(labels, counts)`` (re-scoring), then ``ensemble_device([a, b], mode="finish")`` for a score-sorted result."""
    import torch
    h = model.model.model_chain
    assert sel_idx.is_cuda and sel_idx.dtype == torch.int32 and sel_idx.dim() == 2
    sel_idx = sel_idx.contiguous()
    rows, stride = sel_idx.shape
    assert crow.numel() - 1 == rows
    if sel_cnt is not None:
        assert sel_cnt.is_cuda and sel_cnt.dtype == torch.int32 and sel_cnt.shape == (rows,)
        sel_cnt = sel_cnt.contiguous()
    with _device_csr_queries(h, crow, col, val, n_cols, emb, normalize_emb, stride) as (q, rows, (idx, sc, cnt)):
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        if rows and stride:
            clib.predict_selected_device(h, q, post_processor, sel_idx.data_ptr(), sel_cnt.data_ptr() if sel_cnt is not None else None, stride,
                                         idx.data_ptr(), sc.data_ptr(), cnt.data_ptr(), stride, stream=s or None, sync=True)
    return idx, sc, cnt


def tfidf_weight(counts, idf=None, binary=False, sublinear_tf=False, norm="l2"):
    """Host mirror of tfidf.hpp:798-822 for a CSR of term counts (sorted column ids): float32, the norm accumulated
    sequentially in ascending feature order, exactly the reference's operations (pinned on its outputs, tests/golden/tfidf/)."""
    C = smat.csr_matrix(counts, dtype=np.float32)
    C.sort_indices()
    out = np.empty(C.nnz, dtype=np.float32)
    f32 = np.float32
    for r in range(C.shape[0]):
        b, e = C.indptr[r], C.indptr[r + 1]
        v = np.ones(e - b, f32) if binary else C.data[b:e].astype(f32)
        if sublinear_tf:
            v = (np.log(v.astype(np.float64)) + 1.0).astype(f32)          # :801: the DOUBLE log, one rounding
        if idf is not None:
            v = (v * np.asarray(idf, f32)[C.indices[b:e]]).astype(f32)
        denom = f32(0.0)
        for x in v:
            denom = f32(denom + (f32(abs(x)) if norm == "l1" else f32(x * x)))
        if abs(denom) < np.finfo(np.float32).eps:
            denom = f32(1.0)
        elif norm == "l2":
            denom = f32(np.sqrt(denom))
        out[b:e] = (v / denom).astype(f32)
    return smat.csr_matrix((out, C.indices.copy(), C.indptr.copy()), shape=C.shape)


def predict_tfidf_from_torch(model, crow, col, count, n_cols, idf=None, binary=False, sublinear_tf=False, norm="l2", beam_size=None,
                             only_topk=None, post_processor=None, stream=None):
    """Term-count CSR already on the GPU (crow int64 [rows+1], col int32, count float32; idf float32 [n_cols] CUDA tensor or None)
    -> tf-idf weighting on the device -> beam search; returns (labels, scores, counts) CUDA tensors like predict_from_torch."""
    import torch
    h = model.model.model_chain
    assert crow.is_cuda and col.is_cuda and count.is_cuda and crow.dtype == torch.int64 and col.dtype == torch.int32 and count.dtype == torch.float32
    crow, col, count = crow.contiguous(), col.contiguous(), count.contiguous()
    rows = crow.numel() - 1
    k = clib.effective_topk(h, only_topk)
    idx, sc, cnt = result_buffers(rows, k, count.device, sync=True)
    q = clib.queries_tfidf_device(h, rows, n_cols, crow.data_ptr(), col.data_ptr(), count.data_ptr(), int(count.numel()),
                                  idf.data_ptr() if idf is not None else None, binary, sublinear_tf, 1 if norm == "l1" else 2)
    with clib.freeing(q):
        s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        if rows:
            clib.predict_device(h, q, beam_size, post_processor, only_topk, idx.data_ptr(), sc.data_ptr(), cnt.data_ptr(), k, stream=s or None, sync=True)
    return idx, sc, cnt


def _device_text(text_u8, doc_off, doc_len):
    """The device tokenizer's inputs checked and made contiguous: ``(text uint8, offsets int64, lengths int64, text_addr, n)`` -- CUDA tensors
    on one device (the int64 tensors hold the u64 values; keep them alive over the call), the address to pass for the text and the number
    of documents.  The copies, if any, run on torch's current stream, which is then synchronised: K9 runs on the model's stream."""
    import torch
    assert text_u8.is_cuda and doc_off.is_cuda and doc_len.is_cuda and text_u8.device == doc_off.device == doc_len.device
    assert text_u8.dtype == torch.uint8 and doc_off.dtype == torch.int64 and doc_len.dtype == torch.int64
    assert text_u8.dim() == 1 and doc_off.dim() == 1 and doc_off.shape == doc_len.shape
    if text_u8.stride(0) != 1:
        text_u8 = text_u8.contiguous()
    doc_off, doc_len = doc_off.contiguous(), doc_len.contiguous()
    torch.cuda.current_stream(text_u8.device).synchronize()
    # (an empty tensor has no address: the library wants one for every array of a non-empty corpus)
    text_addr = text_u8.data_ptr() if text_u8.numel() else doc_len.data_ptr()
    return text_u8, doc_off, doc_len, text_addr, int(doc_len.numel())


def _status_addr(status, doc_len):
    """The address of the optional per-document ``status`` tensor (int32 [n], CUDA, contiguous), or None."""
    import torch
    if status is None:
        return None
    assert status.is_cuda and status.dtype == torch.int32 and status.shape == doc_len.shape and status.is_contiguous()
    return status.data_ptr()


def _tfidf_of(vectorizer):
    """The :class:`Tfidf` behind a :class:`Preprocessor`, or the :class:`Tfidf` itself."""
    return vectorizer.vectorizer if isinstance(vectorizer, Preprocessor) else vectorizer


def tfidf_counts_device(vectorizer, model, text_u8, doc_off, doc_len, status=None, stream=None):
    """Term counts of documents whose bytes are already in HBM (K9): ``text_u8`` uint8 [bytes] (any alignment: a slice of a larger tensor is
    fine), ``doc_off`` / ``doc_len`` int64 [n] CUDA tensors on ``model``'s device; document i is ``text_u8[doc_off[i] : doc_off[i] + doc_len[i]]``
    (gaps, overlaps and any order are fine).  Returns a query handle (``clib.freeing`` / ``clib.queries_download``) holding the hstacked CSR
    of term COUNTS, equal to ``clib.tfidf_counts`` of the same documents.  ``status``: optional int32 [n] CUDA tensor that takes each
    document's status (0 fine; 1 / 2: not decodable in parallel, row left empty) instead of a RuntimeError."""
    text_u8, doc_off, doc_len, text_addr, n = _device_text(text_u8, doc_off, doc_len)
    return clib.tfidf_counts_device(_tfidf_of(vectorizer).model, model.model.model_chain, text_addr, doc_off.data_ptr(), doc_len.data_ptr(), n,
                                    _status_addr(status, doc_len), stream=stream)


def predict_text_from_torch(vectorizer, model, text_u8, doc_off, doc_len, beam_size=None, only_topk=None, post_processor=None, stream=None):
    """Text that is already in HBM (tensors as for :func:`tfidf_counts_device`) -> term counts (K9) -> tf-idf weighting (K5) -> beam search,
    with no host copy of the text, of X or of the result: returns (labels, scores, counts) CUDA tensors like :func:`predict_from_torch`."""
    import torch
    h = model.model.model_chain
    text_u8, doc_off, doc_len, text_addr, rows = _device_text(text_u8, doc_off, doc_len)
    k = clib.effective_topk(h, only_topk)
    idx, sc, cnt = result_buffers(rows, k, doc_len.device, sync=True)
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    q = clib.tfidf_predict_device_text(_tfidf_of(vectorizer).model, h, text_addr, doc_off.data_ptr(), doc_len.data_ptr(), rows, stream=s or None)
    with clib.freeing(q):
        if rows:
            clib.predict_device(h, q, beam_size, post_processor, only_topk, idx.data_ptr(), sc.data_ptr(), cnt.data_ptr(), k, stream=s or None, sync=True)
    return idx, sc, cnt


def tfidf_train_device(text_u8, doc_off, doc_len, config, device=None, stream=None):
    """Train a :class:`Tfidf` on documents whose bytes are already in HBM (K15; tensors as for :func:`tfidf_counts_device`): the text never
    visits the host.  ``config`` as for :meth:`Tfidf.train`; ``device`` defaults to the tensors' device."""
    text_u8, doc_off, doc_len, text_addr, n = _device_text(text_u8, doc_off, doc_len)
    dev = text_u8.device.index if device is None else int(device)
    assert dev == text_u8.device.index, "the text must live on the training device"
    return Tfidf(clib.tfidf_train_device(dev, text_addr, doc_off.data_ptr(), doc_len.data_ptr(), n, Tfidf._full_config(config), stream=stream))


def tfidf_transform_device(vectorizer, text_u8, doc_off, doc_len, status=None, stream=None):
    """Text in HBM -> the weighted X as a :class:`DeviceMatrix` on the text's device (K9 + the weighting tail): what ``Tfidf.predict``
    returns, resident, with no XR-Linear model needed -- the X of a training pipeline.  ``status`` as for :func:`tfidf_counts_device`."""
    text_u8, doc_off, doc_len, text_addr, n = _device_text(text_u8, doc_off, doc_len)
    return DeviceMatrix(clib.tfidf_transform_device(_tfidf_of(vectorizer).model, text_u8.device.index, text_addr, doc_off.data_ptr(), doc_len.data_ptr(), n,
                                                    _status_addr(status, doc_len), stream=stream))


class Tfidf:
    """The reference's ``pecos.utils.featurization.text.vectorizers.Tfidf`` (vectorizers.py:163-308): ``load`` a folder the reference
    saved, ``predict`` a list of strings to a scipy CSR -- same names, arguments and result -- with the tokenizer on host threads and
    the weighting / normalisation on the device; ``predict_device``, which leaves X in HBM; ``train`` on the device (K15) and ``save``
    in the reference's layout."""

    def __init__(self, model=None):
        self.model = model

    def __del__(self):
        try:
            clib.tfidf_destruct(self.model)
        except Exception:
            pass

    @classmethod
    def load(cls, load_dir):
        import os
        if not os.path.exists(load_dir):
            raise ValueError(f"tfidf model not exist at {load_dir}")
        return cls(clib.tfidf_load(load_dir))

    # the defaults of the reference's Tfidf.train (vectorizers.py:243-268)
    DEFAULTS = {"ngram_range": (1, 1), "truncate_length": -1, "max_feature": 0, "min_df_ratio": 0.0, "max_df_ratio": 1.0, "min_df_cnt": 0,
                "max_df_cnt": -1, "binary": False, "use_idf": True, "smooth_idf": True, "add_one_idf": False, "sublinear_tf": False,
                "keep_frequent_feature": True, "norm": "l2", "analyzer": "word", "buffer_size": 0, "threads": -1}
    DEFAULTS_META = {"norm_p": 2, "buffer_size": 0, "threads": -1, "base_vect_configs": [DEFAULTS]}

    @classmethod
    def _full_config(cls, config):
        """The caller's config over the defaults; a key the reference does not know raises its ``Unknown argument``."""
        def base(c):
            unknown = [k for k in c if k not in cls.DEFAULTS]
            if unknown:
                raise ValueError(f"Unknown argument: {unknown}")
            return {**cls.DEFAULTS, **c}
        config = {} if config is None else config
        if "base_vect_configs" not in config:
            return base(config)
        config = dict(config, base_vect_configs=[base(c) for c in config["base_vect_configs"]])
        return {**cls.DEFAULTS_META, **config}

    @classmethod
    def train(cls, trn_corpus, config=None, dtype=np.float32):
        """The reference's ``Tfidf.train`` (vectorizers.py:175-289) for a list of strings, trained on the device (K15).  The model is the
        reference's: the same vocabulary, feature ids and idf."""
        if dtype != np.float32:
            raise NotImplementedError("Tfidf.train: only dtype=np.float32 is offered")
        return cls(clib.tfidf_train(trn_corpus, cls._full_config(config)))

    def save(self, save_dir):
        import os
        os.makedirs(save_dir, exist_ok=True)
        clib.tfidf_save(self.model, save_dir)

    @property
    def nr_features(self):
        return clib.tfidf_nr_features(self.model)

    def predict(self, corpus, **kwargs):
        return clib.tfidf_predict(self.model, corpus, buffer_size=kwargs.get("buffer_size", 0), threads=kwargs.get("threads", -1))

    def predict_device(self, xlinear_model, corpus, threads=-1, tokenizer="host"):
        """Texts -> X resident on ``xlinear_model``'s GPU: a query handle (to be freed: ``clib.freeing``) for ``clib.predict_device``.
        ``tokenizer="host"`` counts the terms on host threads and uploads the counts; ``"device"`` uploads the text and counts on the GPU (K9)."""
        extra = {} if tokenizer == "host" else {"tokenizer": tokenizer}      # (the default call stays the call as it always was)
        return clib.tfidf_predict_device(self.model, xlinear_model.model.model_chain, corpus, threads, **extra)


class Preprocessor:
    """The PREDICT half of ``pecos.utils.featurization.text.preprocess.Preprocessor`` (preprocess.py:22-88), the object ``Text2Text`` keeps as
    ``self.preprocessor``: ``load`` the folder its ``save`` wrote (``config.json`` = {"type": ..., "kwargs": ...} beside the vectorizer's own
    files; a folder without it is a tfidf one, vectorizers.py:75-79) and ``predict`` texts.  Only the ``tfidf`` type has a device path; ``hashing``
    and ``sklearntfidf`` folders raise -- they stay the reference's."""

    def __init__(self, vectorizer=None, config=None):
        self.vectorizer = vectorizer
        self.config = config

    @classmethod
    def load(cls, preprocessor_folder):
        import json
        import os
        cfg_path = os.path.join(preprocessor_folder, "config.json")
        config = {"type": "tfidf", "kwargs": {}}
        if os.path.exists(cfg_path):
            with open(cfg_path, "r", encoding="utf-8") as fin:
                config = json.loads(fin.read())
        vtype = config.get("type", None)
        if vtype is None:
            raise ValueError(f"{preprocessor_folder} is not a valid vectorizer folder")
        if vtype != "tfidf":
            raise NotImplementedError(f"vectorizer type {vtype!r}: only 'tfidf' has a device-resident predict path; use the reference's Preprocessor")
        return cls(Tfidf.load(preprocessor_folder), config)

    @classmethod
    def train(cls, vectorizer_config, trn_corpus, dtype=np.float32):
        """``Preprocessor.train`` (preprocess.py) for {"type": "tfidf", "kwargs": {...}}: the vectorizer is trained on the device."""
        vtype = vectorizer_config.get("type", None)
        if vtype != "tfidf":
            raise NotImplementedError(f"vectorizer type {vtype!r}: only 'tfidf' is trained by pecos_amd; use the reference's Preprocessor")
        config = {"type": "tfidf", "kwargs": vectorizer_config.get("kwargs", {})}
        return cls(Tfidf.train(trn_corpus, dict(config["kwargs"]), dtype=dtype), config)

    def save(self, preprocessor_folder):
        import json
        import os
        os.makedirs(preprocessor_folder, exist_ok=True)
        with open(os.path.join(preprocessor_folder, "config.json"), "w", encoding="utf-8") as fout:
            fout.write(json.dumps(self.config or {"type": "tfidf", "kwargs": {}}))
        self.vectorizer.save(preprocessor_folder)

    @property
    def nr_features(self):
        return self.vectorizer.nr_features

    def predict(self, corpus, **kwargs):
        """Texts -> scipy CSR (the reference's result, bit for bit)."""
        if isinstance(corpus, str):
            raise NotImplementedError("predict from a corpus FILE is not offered by pecos_amd: read the lines and pass a list")
        return self.vectorizer.predict(corpus, **kwargs)

    def predict_device(self, xlinear_model, corpus, threads=-1, tokenizer="host"):
        return self.vectorizer.predict_device(xlinear_model, corpus, threads=threads, tokenizer=tokenizer)


def _predict_handle_to_csr(model, q, rows, beam_size=None, only_topk=None, post_processor=None):
    import torch
    from .distributed import rows_to_csr
    h = model.model.model_chain
    k = clib.effective_topk(h, only_topk)
    dev = torch.device("cuda", clib.xlinear_get_int_attr(h, "device"))
    idx, sc, cnt = result_buffers(rows, k, dev)
    torch.cuda.synchronize(dev)
    if rows:
        clib.predict_device(h, q, beam_size, post_processor, only_topk, idx.data_ptr(), sc.data_ptr(), cnt.data_ptr(), k, stream=None, sync=True)
    return rows_to_csr(idx.cpu().numpy().view(np.uint32), sc.cpu().numpy(), cnt.cpu().numpy(), model.nr_pred_cols)


ENSEMBLE_MAX_MODELS = 8          # capacity of the device merge (K6, xrl_ensemble_device): models, and entries of one row over all models
ENSEMBLE_MAX_TOTAL = 1024


def ensemble_device(results, mode="average", threshold=None, only_topk=None, stream=None, sync=True):
    """The results of several models over the same rows merged ON THE DEVICE (K6): ``results`` is a list of ``(labels, scores, counts)``
    CUDA tensors as :func:`predict_from_torch` returns them (int32 [rows, k_m], float32 [rows, k_m], int32 [rows]); the return value has
    the same form, its rows ordered and valued like the host code's: ``mode="average"`` = :func:`ensemble_average`
    (``CsrEnsembler.average``), ``"finish"`` = :meth:`Text2Text.finish` (average, ``threshold``, ``sorted_csr(only_topk)``),
    ``"rank_average"`` = ``CsrEnsembler.rank_average``.  ``"sigmoid_average"``, ``"softmax_average"`` and ``"round_robin"`` are
    ``CsrEnsembler``'s methods of those names (see :func:`ensemble_host` for their rules); with them, and with ``"average"`` /
    ``"rank_average"``, ``only_topk`` ranks the merged rows again by their fp32 value and cuts them, as
    ``TransformerMatcher.ensemble_prediction`` does.  Runs on ``stream`` (a raw HIP stream; default: torch's current one); inputs and
    outputs must be ordered on it."""
    import torch
    if mode not in clib.ENSEMBLE_METHODS:
        raise ValueError(f"ensemble mode {mode!r}: expected one of {sorted(clib.ENSEMBLE_METHODS)}")
    methods = mode not in clib.ENSEMBLE_MODES or (mode != "finish" and bool(only_topk))     # xrl_ensemble_methods_device's part; everything else is xrl_ensemble_device's
    if methods and threshold is not None:
        raise ValueError(f"ensemble mode {mode!r}: a threshold belongs to mode 'finish'")
    if not results:
        raise ValueError("ensemble_device: no results given")
    dev = results[0][0].device
    rows = results[0][0].shape[0]
    res = []
    for idx, sc, cnt in results:
        assert idx.is_cuda and idx.device == dev and sc.device == dev and cnt.device == dev, "ensemble_device: results on different devices"
        assert idx.dtype == torch.int32 and sc.dtype == torch.float32 and cnt.dtype == torch.int32
        assert idx.dim() == 2 and idx.shape == sc.shape and idx.shape[0] == rows and cnt.shape == (rows,)
        res.append((idx.contiguous(), sc.contiguous(), cnt.contiguous()))
    total = sum(r[0].shape[1] for r in res)
    out_stride = min(total, only_topk) if ((mode == "finish" or methods) and only_topk) else total
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        # (allocated on torch's current stream; with another `stream` nothing is queued on the buffers ahead of the kernel: no fill)
        o_idx = torch.empty((rows, out_stride), dtype=torch.int32, device=dev)
        o_sc = torch.empty((rows, out_stride), dtype=torch.float32, device=dev)
        o_cnt = torch.empty((rows,), dtype=torch.int32, device=dev)
        if rows and out_stride:
            ins = (dev.index, rows, [r[0].data_ptr() for r in res], [r[1].data_ptr() for r in res], [r[2].data_ptr() for r in res],
                   [r[0].shape[1] for r in res])
            outs = (o_idx.data_ptr(), o_sc.data_ptr(), o_cnt.data_ptr(), out_stride)
            if methods:
                clib.ensemble_methods_device(*ins, mode, only_topk, *outs, stream=s or None, sync=sync)
            else:
                clib.ensemble_device(*ins, mode, threshold, only_topk, *outs, stream=s or None, sync=sync)
        else:
            o_cnt.zero_()
    return o_idx, o_sc, o_cnt


class DeviceMatrix:
    """A CSR in HBM behind a matrix handle of the library (``xrl_smat_*``): uploaded, wrapped around torch tensors (which it keeps
    alive), compacted from a fixed-stride result, or the product of two others.  Freed with the object."""

    def __init__(self, handle, keep=()):
        self.handle, self._keep = handle, keep

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            clib.smat_free(h)

    @property
    def info(self):
        return clib.smat_info(self.handle)

    @property
    def shape(self):
        i = self.info
        return i["rows"], i["cols"]

    @classmethod
    def upload(cls, X, device=0):
        """A scipy sparse matrix (any format; float32 CSR as it is, stored order kept) copied to ``device``."""
        X = X if isinstance(X, smat.csr_matrix) else smat.csr_matrix(X)
        return cls(clib.smat_upload_csr(device, X if X.dtype == np.float32 else X.astype(np.float32)))

    @classmethod
    def from_torch(cls, crow, col, val, shape):
        """Wraps CUDA tensors crow int64 [rows + 1], col int32 [nnz], val float32 [nnz] of a CSR of ``shape`` (no copy of contiguous ones)."""
        import torch
        assert crow.is_cuda and col.device == crow.device and val.device == crow.device
        assert crow.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
        crow, col, val = crow.contiguous(), col.contiguous(), val.contiguous()
        rows, cols = shape
        assert crow.numel() == rows + 1 and col.numel() == val.numel()
        return cls(clib.smat_from_device_csr(crow.device.index, rows, cols, crow.data_ptr(), col.data_ptr(), val.data_ptr(), val.numel()), keep=(crow, col, val))

    @classmethod
    def from_result(cls, result, n_cols, stream=None):
        """A result triple ``(labels int32 [rows, k], scores float32 [rows, k], counts int32 [rows] or None)`` as a rows x ``n_cols`` CSR, rows best first."""
        import torch
        idx, sc, cnt = result
        assert idx.is_cuda and idx.dtype == torch.int32 and sc.dtype == torch.float32 and idx.dim() == 2 and idx.shape == sc.shape and sc.device == idx.device
        idx, sc = idx.contiguous(), sc.contiguous()
        rows, stride = idx.shape
        if cnt is not None:
            assert cnt.device == idx.device and cnt.dtype == torch.int32 and cnt.shape == (rows,)
            cnt = cnt.contiguous()
        with torch.cuda.device(idx.device):
            s = torch.cuda.current_stream().cuda_stream if stream is None else stream
            return cls(clib.smat_from_device_result(idx.device.index, rows, n_cols, idx.data_ptr(), sc.data_ptr(), None if cnt is None else cnt.data_ptr(),
                                                    stride, stream=s or None))

    def to_torch(self, stream=None):
        """``(crow int64, col int32, val float32, (rows, cols))``: CUDA tensors copied out of the handle."""
        import torch
        i = self.info
        dev = torch.device("cuda", i["device"])
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream().cuda_stream if stream is None else stream
            crow = torch.empty(i["rows"] + 1, dtype=torch.int64, device=dev)
            col = torch.empty(i["nnz"], dtype=torch.int32, device=dev)
            val = torch.empty(i["nnz"], dtype=torch.float32, device=dev)
            clib.smat_copy_device(self.handle, crow.data_ptr(), col.data_ptr(), val.data_ptr(), stream=s or None)
        return crow, col, val, (i["rows"], i["cols"])

    def download(self):
        """scipy CSR copy on the host, stored order and explicit zeros kept."""
        return clib.smat_download(self.handle)

    def multiply(self, other, eliminate_zeros=False, sorted_indices=True, stream=None):
        """``self * other`` as a new :class:`DeviceMatrix` (K10; the rule is stated at ``xrl_sparse_matmul_device``)."""
        return DeviceMatrix(clib.sparse_matmul_device(self.handle, other.handle, eliminate_zeros, sorted_indices, stream=stream))


    def transpose(self, stream=None):
        """The transpose as a new :class:`DeviceMatrix`, rows in scipy's ``.T.tocsr()`` order (K12; rule R2 at ``xrl_label_embedding_device``)."""
        return DeviceMatrix(clib.smat_transpose_device(self.handle, stream=stream))

    def normalize_rows(self, in_place=False, stream=None, norm="l2"):
        """Rows scaled to unit ``norm`` (``l2``, ``l1`` or ``max``) in sklearn's arithmetic (K12; rules R1, R1a, R1b).  ``in_place``
        rewrites this matrix's values -- the wrapped tensor's, for :meth:`from_torch` -- and returns ``self``; otherwise a new
        :class:`DeviceMatrix`.  ``max`` refuses a row whose column ids are not strictly ascending."""
        h = clib.smat_normalize_rows_device(self.handle, in_place, stream=stream, norm=norm)
        return self if in_place else DeviceMatrix(h)

    @staticmethod
    def check_relevance(Y, R, by_columns=True, stream=None):
        """ValueError, in :func:`pecos_amd.xlinear.check_relevance`'s words, unless ``R`` stores exactly the entries of ``Y`` and no
        negative value: both :class:`DeviceMatrix` of one shape, compared where they are (K14's check kernel; rule C).  The host check
        reads both column-major, so ``by_columns`` compares the device transposes -- which of ``indptr`` and ``indices`` the message names
        is then the host's; False compares the rows as stored."""
        if Y.shape != R.shape:
            raise ValueError(f"Invalid relevance matrix: R has shape {R.shape}, Y has {Y.shape}")
        if by_columns:
            Y, R = Y.transpose(stream=stream), R.transpose(stream=stream)
        code, _ = clib.smat_check_relevance_device(Y.handle, R.handle, stream=stream)
        if code in (1, 2):
            raise ValueError(f"Invalid relevance matrix: Y.{'indptr' if code == 1 else 'indices'} != R.{'indptr' if code == 1 else 'indices'}")
        if code == 3:
            raise ValueError("Invalid relevance matrix: got value < 0")

    @classmethod
    def hstack(cls, mats, stream=None):
        """``[M0 M1 ...]`` of :class:`DeviceMatrix` with one row count on one device, as a new one (stored order kept inside each part)."""
        mats = list(mats)
        return cls(clib.smat_hstack_device([m.handle for m in mats], stream=stream))

    @classmethod
    def pattern_union(cls, mats, stream=None):
        """A new :class:`DeviceMatrix` that stores a 1 wherever one of ``mats`` (one shape, one device) stores an entry -- explicit zeros
        and NaN count, values are never read --, every row ascending (K14; rule U at ``xrl_smat_pattern_union_device``)."""
        mats = list(mats)
        return cls(clib.smat_pattern_union_device([m.handle for m in mats], stream=stream))


def result_to_csr_device(result, n_cols=0, stream=None):
    """A result triple (:func:`result_buffers`' form; counts may be None = full rows) as CSR tensors on its device: ``(crow int64 [rows + 1],
    col int32 [nnz], val float32 [nnz])``, every row best first as the result stores it."""
    return DeviceMatrix.from_result(result, n_cols, stream).to_torch(stream)[:3]


def _as_device_matrix(M, device, n_cols, stream):
    """An operand of :func:`sparse_matmul_device` as a :class:`DeviceMatrix`."""
    if isinstance(M, DeviceMatrix):
        return M
    if smat.issparse(M):
        return DeviceMatrix.upload(M, device)
    if isinstance(M, (tuple, list)) and len(M) == 4 and isinstance(M[3], (tuple, list)):
        return DeviceMatrix.from_torch(*M)
    if isinstance(M, (tuple, list)) and len(M) in (3, 4):
        if len(M) == 4:
            n_cols = M[3]
        if n_cols is None:
            raise ValueError("sparse_matmul_device: a result triple as the right operand needs its column count: pass (labels, scores, counts, n_cols)")
        return DeviceMatrix.from_result(tuple(M[:3]), n_cols, stream)
    raise TypeError(f"sparse_matmul_device: operand of type {type(M)}")


def _operand_device(M):
    if isinstance(M, DeviceMatrix):
        return M.info["device"]
    if isinstance(M, (tuple, list)):
        return M[0].device.index
    return None


def sparse_matmul_device(A, B, eliminate_zeros=False, sorted_indices=True, stream=None):
    """``A * B`` of two sparse matrices ON THE DEVICE (K10), by the reference's ``clib.sparse_matmul`` rule bit for bit (stored order of
    the left rows = order of the additions; see ``xrl_sparse_matmul_device``).  An operand is a :class:`DeviceMatrix`; a scipy sparse matrix
    (uploaded to the other operand's device); CSR tensors ``(crow, col, val, (rows, cols))``; or a result triple ``(labels, scores, counts)``
    as :func:`predict_from_torch` / :func:`ensemble_device` return it, one row per query and one column per label -- as the left operand its
    column count is the right operand's row count, as the right operand it is given as a fourth element.  Returns CSR tensors ``(crow int64,
    col int32, val float32, (rows, cols))`` on that device, which can be an operand again.  Runs on ``stream`` (a raw HIP stream; default:
    torch's current one), which it synchronises."""
    dev = _operand_device(A)
    if dev is None:
        dev = _operand_device(B)
    if dev is None:
        dev = 0
    b = _as_device_matrix(B, dev, None, stream)
    a = _as_device_matrix(A, dev, b.shape[0], stream)
    return a.multiply(b, eliminate_zeros, sorted_indices, stream=_stream_or_current(dev, stream)).to_torch(stream)


def _stream_or_current(device, stream):
    import torch
    if stream is not None:
        return stream
    with torch.cuda.device(device):
        return torch.cuda.current_stream().cuda_stream or None


class Metrics(collections.namedtuple("Metrics", ["prec", "recall"])):
    """Precision and recall at 1 .. topk, the pair ``smat_util.Metrics`` holds (smat_util.py:950-997); prints like it: one line per
    field, the values as percentages with two decimals."""

    __slots__ = ()

    def __str__(self):
        lines = []
        for name in self._fields:
            shown = " ".join("{:4.2f}".format(100 * v) for v in getattr(self, name))
            lines.append("{:7}= {}".format(name, shown))
        return "\n".join(lines)

    @classmethod
    def from_sums(cls, matched, recall_sum, rows):
        """The metrics of ``rows`` rows from their sums (:func:`metrics_sums_device`, added over batches or ranks): the reference's own last
        two operations in numpy fp64 -- ``total_matched / rows / arange(1, topk + 1)`` and ``recall / rows``."""
        matched = np.asarray(matched).astype(np.uint64)          # (int64 tensors hold the u64 bits)
        recall_sum = np.asarray(recall_sum, dtype=np.float64)
        rows = int(rows)
        prec = matched / rows / np.arange(1, len(matched) + 1)
        return cls(prec=prec, recall=recall_sum / rows)


def _true_pattern_device(Y_true, rows, dev, n_cols):
    """The pattern of the true labels on ``dev``: (crow int64 [rows+1], col int32 [nnz >= 1]) CUDA tensors, ascending inside every row."""
    import torch
    if isinstance(Y_true, smat.csr_matrix):
        if Y_true.shape[0] != rows:
            raise ValueError(f"Y_true has {Y_true.shape[0]} rows, the result {rows}")
        if n_cols is not None and Y_true.shape[1] != n_cols:
            raise ValueError(f"Y_true has {Y_true.shape[1]} columns, expected {n_cols}")
        if not Y_true.has_sorted_indices:
            Y_true = Y_true.sorted_indices()                     # a copy: the caller's matrix stays as it is
        crow = torch.from_numpy(Y_true.indptr.astype(np.int64)).to(dev)
        col = torch.from_numpy(Y_true.indices.astype(np.uint32).view(np.int32)).to(dev)
    else:
        crow, col = Y_true
        assert crow.is_cuda and col.is_cuda and crow.device == dev and col.device == dev, "metrics: Y_true on another device than the result"
        assert crow.dtype == torch.int64 and col.dtype == torch.int32 and crow.shape == (rows + 1,)
        crow, col = crow.contiguous(), col.contiguous()
    if col.numel() == 0:                                         # (no true label at all: the library still wants an address)
        col = torch.zeros(1, dtype=torch.int32, device=dev)
    return crow, col


def metrics_sums_device(result, Y_true, topk=10, stream=None, sync=True, n_cols=None):
    """The sums behind ``smat_util.Metrics.generate(Y_true, Y_pred, topk)`` computed ON THE DEVICE (K8) from a result that is already there.

    result: the ``(labels, scores, counts)`` CUDA triple of :func:`predict_from_torch` / :func:`ensemble_device` (int32 [rows, k], float32
    [rows, k], int32 [rows]); the labels of a row are distinct, their stored order does not matter (rows are ranked by score descending, NaN
    last, ties by label ascending, as the reference's ``sorted_csr`` does).  Y_true: a scipy ``csr_matrix`` (checked for its rows and, with
    ``n_cols``, its columns; indices sorted into a copy when they are not; only the pattern is uploaded) or a ``(crow int64 [rows+1],
    col int32)`` pair of CUDA tensors on the result's device, ascending inside every row.  Returns CUDA tensors ``(matched int64 [topk] --
    the u64 bits --, recall_sum float64 [topk])``: additive over row batches and ranks, :meth:`Metrics.from_sums` turns them into the
    metrics.  Runs on ``stream`` (a raw HIP stream; default: torch's current one); inputs must be ordered on it.  topk and k in 1..1024."""
    import torch
    idx, sc, cnt = result
    dev = idx.device
    assert idx.is_cuda and sc.device == dev and cnt.device == dev, "metrics: result on different devices"
    assert idx.dtype == torch.int32 and sc.dtype == torch.float32 and cnt.dtype == torch.int32
    assert idx.dim() == 2 and idx.shape == sc.shape and cnt.shape == (idx.shape[0],)
    rows, stride = idx.shape
    topk = int(topk)
    for name, v in (("stride", stride), ("topk", topk)):
        if not 1 <= v <= clib.METRICS_MAX:                          # (the library's own check and words; made here too, since no rows = no call)
            raise ValueError(f"xrl_metrics_device: {name} must be 1..{clib.METRICS_MAX}, got {v}")
    idx, sc, cnt = idx.contiguous(), sc.contiguous(), cnt.contiguous()
    with torch.cuda.device(dev):
        crow, col = _true_pattern_device(Y_true, rows, dev, n_cols)
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        if stream is not None:
            torch.cuda.current_stream().synchronize()            # the upload and the contiguous() copies ran on torch's current stream
        if rows == 0:
            return torch.zeros(topk, dtype=torch.int64, device=dev), torch.zeros(topk, dtype=torch.float64, device=dev)
        matched = torch.empty(topk, dtype=torch.int64, device=dev)
        recall_sum = torch.empty(topk, dtype=torch.float64, device=dev)
        clib.metrics_device(dev.index, rows, idx.data_ptr(), sc.data_ptr(), cnt.data_ptr(), stride, crow.data_ptr(), col.data_ptr(), topk,
                            matched.data_ptr(), recall_sum.data_ptr(), stream=s or None, sync=sync)
    return matched, recall_sum


def metrics_device(result, Y_true, topk=10, stream=None, n_cols=None):
    """``smat_util.Metrics.generate(Y_true, Y_pred, topk)`` for a result in HBM: :func:`metrics_sums_device`, one copy back of 2 x topk
    numbers, :meth:`Metrics.from_sums`.  ``prec`` is the reference's bit for bit; ``recall`` too up to 64 rows, beyond that within the
    rounding of a differently ordered fp64 sum (include/xrl_abi.h)."""
    matched, recall_sum = metrics_sums_device(result, Y_true, topk=topk, stream=stream, sync=True, n_cols=n_cols)
    return Metrics.from_sums(matched.cpu().numpy(), recall_sum.cpu().numpy(), result[0].shape[0])


def _ensemble_on_device(models, ensemble, only_topk, finish=None):
    """Whether the ensemble of ``models`` merges on the device: one device, one feature count and one label count, within K6's capacity."""
    if ensemble not in ("auto", "device", "host"):
        raise ValueError(f"ensemble={ensemble!r}: expected 'auto', 'device' or 'host'")
    if ensemble == "host":
        return False
    hs = [m.model.model_chain for m in models]
    why = None
    if len(models) > ENSEMBLE_MAX_MODELS:
        why = f"{len(models)} models, more than {ENSEMBLE_MAX_MODELS}"
    elif len({clib.xlinear_get_int_attr(h, "device") for h in hs}) != 1:
        why = "the models live on different devices"
    elif len({clib.xlinear_get_int_attr(h, "nr_features") for h in hs}) != 1:
        why = "the models differ in nr_features: one X cannot serve them all"
    elif len({m.nr_pred_cols for m in models}) != 1:
        why = "the models differ in their label count"
    elif sum(clib.effective_topk(h, only_topk) for h in hs) > ENSEMBLE_MAX_TOTAL:
        why = f"the models' top-k sum to more than {ENSEMBLE_MAX_TOTAL} entries per row"
    elif finish is not None and finish[1] is not None and finish[1] < 1:
        why = "a final only_topk below 1 (sorted_csr then keeps nothing; K6 reads 0 as 'all')"
    if why is not None and ensemble == "device":
        raise ValueError(f"ensemble='device': {why}")
    return why is None


_ensemble_streams = {}


@contextlib.contextmanager
def _text_queries(vectorizer, model, corpus, X_emb, normalize_emb, threads, tokenizer="host"):
    """Texts -> the query handle to search, on ``model``'s device: the tf-idf X, or with ``X_emb`` (float32 [rows, H] CUDA tensor) the
    concatenation [X | X_emb] made from it on the device.  Both handles are freed on exit."""
    extra = {} if tokenizer == "host" else {"tokenizer": tokenizer}          # (a vectorizer object without the option still serves the default)
    q = vectorizer.predict_device(model, corpus, threads=threads, **extra)
    with clib.freeing(q):
        if X_emb is None:
            yield q
            return
        import torch
        assert X_emb.is_cuda and X_emb.dtype == torch.float32 and X_emb.shape[0] == len(corpus)
        X_emb = X_emb.contiguous()
        torch.cuda.current_stream().synchronize()
        q2 = clib.queries_concat_handle(model.model.model_chain, q, X_emb.shape[1], X_emb.data_ptr(), normalize_emb=normalize_emb)
        with clib.freeing(q2):
            yield q2


def _predict_text_ensemble_device(vectorizer, models, corpus, X_emb, normalize_emb, threads, beam_size, only_topk, post_processor, finish,
                                  tokenizer="host", method="average"):
    """predict_text's ensemble on the device: ONE tokenisation and upload (and one concatenation with X_emb), every model's beam search on
    that handle, the merge (K6) and nothing else on one stream, one synchronisation, one copy back, one CSR."""
    import torch
    from .distributed import rows_to_csr
    hs = [m.model.model_chain for m in models]
    dev = torch.device("cuda", clib.xlinear_get_int_attr(hs[0], "device"))
    rows = len(corpus)
    with _text_queries(vectorizer, models[0], corpus, X_emb, normalize_emb, threads, tokenizer) as q:
        try:
            s = _ensemble_streams.get(dev.index)
            if s is None:
                s = _ensemble_streams[dev.index] = torch.cuda.Stream(device=dev)
            mode, thr, topk = (method, None, None) if finish is None else ("finish", finish[0], finish[1])
            with torch.cuda.stream(s):
                res = []
                for h in hs:
                    k = clib.effective_topk(h, only_topk)
                    idx, sc, cnt = result_buffers(rows, k, dev)          # (filled on `s`, the stream of the predict)
                    if rows:
                        clib.predict_device(h, q, beam_size, post_processor, only_topk, idx.data_ptr(), sc.data_ptr(), cnt.data_ptr(), k,
                                            stream=s.cuda_stream, sync=False)
                    res.append((idx, sc, cnt))
                o_idx, o_sc, o_cnt = ensemble_device(res, mode=mode, threshold=thr, only_topk=topk, stream=s.cuda_stream, sync=False)
                s.synchronize()
                return rows_to_csr(o_idx.cpu().numpy().view(np.uint32), o_sc.cpu().numpy(), o_cnt.cpu().numpy(), models[0].nr_pred_cols)
        finally:
            torch.cuda.synchronize(dev)            # (also on an error: nothing may still read X when its handle goes)


def predict_text(vectorizer, models, corpus, X_emb=None, normalize_emb=True, threads=-1, ensemble="auto", finish=None, tokenizer="host",
                 ensemble_method="average", **kwargs):
    """The reference's text call sites with X DEVICE-RESIDENT end to end:

    * ``Text2Text.predict`` (pecos/apps/text2text/model.py:416-422): ``X = preprocessor.predict(corpus); Y = [m.predict(X) ...]`` --
      here the texts are tokenised on the host, their term counts uploaded once, weighted on the GPU, and every model of ``models``
      (one XLinearModel or a list: the ensemble is averaged like ``CsrEnsembler.average``) searches that X in place;
    * ``XTransformer.predict`` (pecos/xmc/xtransformer/model.py:589-603): with ``X_emb`` (float32 [rows, H] CUDA tensor, the encoder's
      output) the concat model's input ``[X_feat | normalize(X_emb)]`` is assembled on the device as well.

    Several models: ``ensemble="auto"`` (default) merges their results on the device (K6) -- one tokenisation and upload, one copy back --
    where they share a device, ``nr_features`` and label count and their top-k sum to at most 1024 entries per row, and on the host
    otherwise; ``"device"`` raises where "auto" would take the host path; ``"host"`` is the host path (one tokenisation, upload and copy
    back per model, scipy's merge).  The result is the same bit for bit.  ``finish=(threshold, only_topk)`` also applies
    :meth:`Text2Text.finish`'s threshold and cut to the merged rows (on whichever path).  ``ensemble_method``: any method of
    ``CsrEnsembler`` (:data:`ENSEMBLE_METHOD_NAMES`; default ``"average"``) -- merged on the device (K6) where ``ensemble`` allows it, by
    :func:`ensemble_host` otherwise, values as float32 either way; ``finish`` goes with ``"average"`` only.

    ``tokenizer="host"`` (default) counts the terms on host threads; ``"device"`` uploads the text once and counts on the GPU (K9) -- the same
    counts, hence the same labels and score bits.

    kwargs: beam_size, only_topk, post_processor.  Returns the predicted label matrix as scipy CSR (rows score-sorted)."""
    if tokenizer not in clib.TOKENIZERS:
        raise ValueError(f"tokenizer={tokenizer!r}: expected 'host' or 'device'")
    models = list(models) if isinstance(models, (list, tuple)) else [models]
    if ensemble_method not in ENSEMBLE_METHOD_NAMES:
        raise ValueError(f"ensemble_method={ensemble_method!r}: expected one of {list(ENSEMBLE_METHOD_NAMES)}")
    if ensemble_method != "average" and finish is not None:
        raise ValueError(f"ensemble_method={ensemble_method!r}: finish=(threshold, only_topk) goes with 'average' only")
    if isinstance(vectorizer, Preprocessor):
        vectorizer = vectorizer.vectorizer
    if len(models) > 1 and _ensemble_on_device(models, ensemble, kwargs.get("only_topk"), finish):
        return _predict_text_ensemble_device(vectorizer, models, corpus, X_emb, normalize_emb, threads, kwargs.get("beam_size"),
                                             kwargs.get("only_topk"), kwargs.get("post_processor"), finish, tokenizer, ensemble_method)
    elif ensemble not in ("auto", "device", "host"):
        raise ValueError(f"ensemble={ensemble!r}: expected 'auto', 'device' or 'host'")
    outs = []
    for m in models:
        with _text_queries(vectorizer, m, corpus, X_emb, normalize_emb, threads, tokenizer) as q:
            outs.append(_predict_handle_to_csr(m, q, len(corpus), kwargs.get("beam_size"), kwargs.get("only_topk"), kwargs.get("post_processor")))
    if finish is not None:
        return Text2Text.finish(outs, threshold=finish[0], only_topk=finish[1])
    if ensemble_method != "average":
        Y = ensemble_host(outs, ensemble_method)      # rank_average and round_robin: float64 in the reference; float32 here, as the device
        return smat.csr_matrix((Y.data.astype(np.float32), Y.indices, Y.indptr), shape=Y.shape)     # (scipy's astype would sort the columns)
    if len(outs) == 1:
        return outs[0]
    return ensemble_average(outs)               # CsrEnsembler.average (smat_util.py:828-842): sum, sorted_csr, divide -- rows score-sorted like the reference's


def sorted_csr(csr, only_topk=None):
    """``pecos.utils.smat_util.sorted_csr`` (smat_util.py:174-272): every row ordered by value, descending, ties by ascending column (the
    reference sorts the columns, then mergesorts -value: stable), optionally cut to the first ``only_topk``; duplicates summed like its
    ``csr_matrix((val, (row, col)))``.  One lexsort instead of the reference's Python loop over rows."""
    if not isinstance(csr, smat.csr_matrix):
        raise ValueError("the input matrix must be a csr_matrix.")
    c = smat.csr_matrix(csr, copy=True)
    c.sum_duplicates()                                       # (also sorts the columns inside every row)
    n = c.shape[0]
    counts = np.diff(c.indptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), counts)
    order = np.lexsort((c.indices, -c.data, rows))           # by row, then -value, then column; NaN last like argsort
    idx, val = c.indices[order], c.data[order]
    indptr = c.indptr.astype(np.int64)
    if only_topk is not None:
        assert isinstance(only_topk, int), f"Wrong type: type(only_topk) = {type(only_topk)}"
        only_topk = max(min(1, only_topk), only_topk)        # (the reference's own expression, smat_util.py:198)
        keep = (np.arange(len(val), dtype=np.int64) - indptr[rows]) < only_topk
        idx, val = idx[keep], val[keep]
        indptr = np.concatenate([[0], np.cumsum(np.minimum(counts, only_topk))]).astype(np.int64)
    return smat.csr_matrix((val, idx.astype(np.int64), indptr), shape=c.shape)


def ensemble_average(mats):
    """``CsrEnsembler.average`` (smat_util.py:828-842): sum, ``sorted_csr``, divide by the number of matrices."""
    assert all(m.shape == mats[0].shape for m in mats)
    ret = sorted_csr(sum(mats).tocsr())
    ret.data /= len(mats)
    return ret


ENSEMBLE_METHOD_NAMES = ("average", "rank_average", "sigmoid_average", "softmax_average", "round_robin")     # CsrEnsembler's methods


def _relevance_csr(csr, mm):
    """``get_relevance_csr`` (smat_util.py:638-659): position p of a row scores ``mm - p``, float64."""
    counts = np.diff(csr.indptr)
    rows = np.repeat(np.arange(csr.shape[0], dtype=np.int64), counts)
    rel = (mm - (np.arange(len(csr.data), dtype=np.int64) - csr.indptr[rows])).astype(np.float64)
    return smat.csr_matrix((rel, csr.indices.copy(), csr.indptr.copy()), shape=csr.shape)


def _exp_f32(x):
    """exp of a float32 array taken in float64 and rounded to float32 (the device's ``ref_expf``)."""
    return np.exp(x.astype(np.float64)).astype(np.float32)


def _sigmoid_csr(csr):
    """``sigmoid_average``'s transform in fp32 steps: 1 / (1 + exp(-z)).  Returns a new matrix (the reference overwrites its argument)."""
    one = np.float32(1)
    with np.errstate(over="ignore", invalid="ignore"):
        data = one / (one + _exp_f32(-csr.data.astype(np.float32)))
    return smat.csr_matrix((data, csr.indices.copy(), csr.indptr.copy()), shape=csr.shape)


def _softmax_csrs(mats):
    """``csr_row_softmax`` of every matrix by the device's rule (include/xrl_abi.h, method 4): per row and matrix x_max = amax, e = exp(x -
    x_max) rounded to fp32, denominator = the fp64 sum of e in the kernel's order -- entry j of the row's model-ordered list belongs to lane
    j % 64, a lane adds its entries in ascending j, the lanes meet in six exchange steps -- rounded once to fp32.  An empty row of a matrix
    contributes nothing."""
    out = [smat.csr_matrix((m.data.astype(np.float32), m.indices.copy(), m.indptr.copy()), shape=m.shape) for m in mats]
    lanes = np.arange(64)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(out[0].shape[0]):
            pre = 0
            for m in out:
                a, b = int(m.indptr[r]), int(m.indptr[r + 1])
                if b > a:
                    x = m.data[a:b]
                    e = _exp_f32(x - np.amax(x))
                    s = np.zeros(64, dtype=np.float64)
                    np.add.at(s, (pre + np.arange(b - a)) % 64, e.astype(np.float64))      # (unbuffered: in ascending j per lane)
                    for d in (1, 2, 4, 8, 16, 32):
                        s = s + s[lanes ^ d]
                    m.data[a:b] = e / np.float32(s[0])
                pre += b - a
    return out


def ensemble_host(mats, method="average", only_topk=None):
    """The methods of ``CsrEnsembler`` (smat_util.py:814-923) on the host, written against scipy by the rules the device merge follows
    (include/xrl_abi.h): ``average``; ``rank_average``; ``sigmoid_average`` (1 / (1 + exp(-z)) in fp32 steps, then average);
    ``softmax_average`` (softmax over the stored entries of every row of every matrix, then average; an empty row contributes nothing, where
    the reference raises); ``round_robin`` (fp64 relevance ``mm - p + (M - m) / (M + 1)``, maximum over the holders).  The exponentials are
    taken in float64 and rounded to float32.  Rows must be stored best first; the inputs are left as they are.  ``only_topk``:
    ``TransformerMatcher.ensemble_prediction``'s last line, ``sorted_csr(ret.astype(float32), only_topk)``.  rank_average and round_robin
    return float64 like the reference."""
    if method not in ENSEMBLE_METHOD_NAMES:
        raise ValueError(f"ensemble method {method!r}: expected one of {list(ENSEMBLE_METHOD_NAMES)}")
    mats = [m.tocsr() for m in mats]
    assert all(m.shape == mats[0].shape for m in mats)
    M = len(mats)
    if method in ("rank_average", "round_robin"):
        mm = max(int(np.diff(m.indptr).max(initial=0)) for m in mats)
        if method == "rank_average":
            ret = sum(_relevance_csr(m, mm) for m in mats).tocsr()
        else:
            base = 1.0 / (M + 1.0)
            ret = None
            for i, m in enumerate(mats):
                rel = _relevance_csr(m, mm)
                rel.data += (M - i) * base
                ret = rel if ret is None else ret.maximum(rel)
        ret = sorted_csr(ret.tocsr())
        ret.data /= M
    else:
        if method == "sigmoid_average":
            mats = [_sigmoid_csr(m) for m in mats]
        elif method == "softmax_average":
            mats = _softmax_csrs(mats)
        ret = ensemble_average(mats)
    if only_topk is not None:
        ret = sorted_csr(ret.astype(np.float32), only_topk=only_topk)
    return ret


def ensemble_prediction_device(transformer_pred, concat_pred, only_topk, ens_method):
    """``TransformerMatcher.ensemble_prediction`` (pecos/xmc/xtransformer/matcher.py:535-579) on two ``(labels, scores, counts)`` device
    triples: ``ens_method`` is ``"concat-only"``, ``"transformer-only"``, ``"average"``, ``"rank_average"`` or ``"round_robin"``; the merged
    rows are ranked by their fp32 value (ties by label) and cut to ``only_topk`` (``None``: all), as its last line does.  Returns a triple.

    Precondition: the rows of both inputs are stored in ``sorted_csr`` order -- score descending, ties by ascending label.  The reference
    re-sorts its inputs that way before rank_average and round_robin look at the positions; a predict stores ties by candidate position, so
    rows with tied scores may need that sort first (average, concat-only and transformer-only do not depend on the stored order)."""
    if transformer_pred[0].shape[0] != concat_pred[0].shape[0]:
        raise ValueError(f"Transformer/concat prediction mismatch: {tuple(transformer_pred[0].shape)} and {tuple(concat_pred[0].shape)}")
    if ens_method == "concat-only":
        results, mode = [concat_pred], "average"                  # (one model: nothing summed or dropped, value / 1)
    elif ens_method == "transformer-only":
        results, mode = [transformer_pred], "average"
    elif ens_method in ("average", "rank_average", "round_robin"):
        results, mode = [transformer_pred, concat_pred], ens_method
    else:
        raise ValueError(f"Unknown ensemble method {ens_method}")
    total = sum(r[0].shape[1] for r in results)
    return ensemble_device(results, mode=mode, only_topk=only_topk if only_topk is not None else max(total, 1))


class Text2Text:
    """The PREDICT half of ``pecos.apps.text2text.model.Text2Text`` (model.py:136-190 load, :389-427 predict) over the device-resident
    pipeline: ``load`` the folder its ``save`` wrote (``preprocessor/``, ``xlinear_ensemble/{config.json, 0, 1, ...}``, ``output_items.json``),
    ``predict`` a list of strings -- texts -> term counts (host threads) -> X in HBM -> beam search in place, per model; ensemble average,
    threshold and the final ``sorted_csr(only_topk)`` as the reference does them.  ``set_output_constraint`` restricts every model of the
    ensemble to a set of output items, on the loaded handles (the constrained route of the beam search).  Training and saving stay the
    reference's."""

    def __init__(self, preprocessor, xlinear_models, output_items):
        self.preprocessor = preprocessor
        self.xlinear_models = xlinear_models
        self.output_items = output_items

    @classmethod
    def load(cls, model_folder, is_predict_only=True, **kwargs):
        import json
        import os
        from .xlinear import XLinearModel
        preprocessor = Preprocessor.load(os.path.join(model_folder, "preprocessor"))
        xlinear_folder = os.path.join(model_folder, "xlinear_ensemble")
        with open(os.path.join(xlinear_folder, "config.json"), "r", encoding="utf-8") as fin:
            ensemble_config = json.loads(fin.read())
        xlinear_models = []
        for i, model_kwargs in enumerate(ensemble_config["kwargs"]):
            xlinear_models += [(XLinearModel.load(os.path.join(xlinear_folder, str(i)), is_predict_only, **kwargs), model_kwargs)]
        with open(os.path.join(model_folder, "output_items.json"), "r", encoding="utf-8") as fin:
            output_items = json.load(fin)
        if not output_items:
            raise ValueError("Could not read output items saved in json format")
        return cls(preprocessor, xlinear_models, output_items)

    @staticmethod
    def finish(Y_pred, threshold=None, only_topk=None):
        """model.py:418-427 after the per-model predictions: ensemble average, threshold, ``sorted_csr``."""
        Y = ensemble_average(Y_pred) if len(Y_pred) > 1 else Y_pred[0].tocsr()
        if threshold is not None:
            Y = Y.copy()
            Y.data[Y.data <= threshold] = 0
            Y.eliminate_zeros()
        return sorted_csr(Y, only_topk=only_topk)

    def predict(self, corpus, threshold=None, **kwargs):
        """Same arguments and result as the reference's ``Text2Text.predict`` (``threads`` applies to the tokenizer's host threads;
        ``tokenizer="device"`` counts the terms on the GPU instead, see :func:`predict_text`)."""
        threads = kwargs.pop("threads", -1)
        tokenizer = kwargs.pop("tokenizer", "host")
        # (an ensemble: one tokenisation and upload, the merge, threshold and cut on the device where predict_text finds that possible)
        return predict_text(self.preprocessor, [m for m, _ in self.xlinear_models], corpus, threads=threads, tokenizer=tokenizer,
                            finish=(threshold, kwargs.get("only_topk", None)), **kwargs)

    def set_output_constraint(self, output_items_to_keep):
        """Restrict predict() to the given output items (model.py:430-444): strings that are no output item are ignored, every model of
        the ensemble gets the set.  ``None`` clears the constraint."""
        if output_items_to_keep is None:
            for model, _ in self.xlinear_models:
                model.set_output_constraint(None)
            return
        index = {item: i for i, item in enumerate(self.output_items)}      # (an item listed twice answers to its last position)
        keep = {index[item] for item in output_items_to_keep if item in index}
        for model, _ in self.xlinear_models:
            model.set_output_constraint(keep)

    def get_output_item(self, output_id):
        return self.output_items[output_id]
