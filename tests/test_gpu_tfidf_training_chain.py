"""TF-IDF training on the device (K15), second part: the generators of the tokenizer tests (tests/tfidf_cases.py) and tokens with control
bytes through xrl_tfidf_export; caller-owned text, offsets and lengths carved out of larger tensors (tests/device_views.py) with
vocabulary bytes between the documents, documents in any order and aliased, on a side stream; the trained handle through
predict_text with both tokenizers; text -> X -> label embedding -> clustering -> XLinearModel.train_device -> save -> load ->
predict_text end to end against the same chain fed from the recorded reference vectorizer's X; table memory freed at c_tfidf_destruct."""
import numpy as np
import pytest
import scipy.sparse as smat

import device_views as dv
import ranker_training_rule as rr
import tfidf_cases as tc
import tfidf_training_rule as tr
from test_gpu_tfidf_training import clib, env, golden, same_as_statement, train  # noqa: F401  (two fixtures and three helpers)

pytestmark = pytest.mark.gpu
F32 = np.float32


def tensors(docs):
    """(text uint8, offsets int64, lengths int64) CUDA tensors of documents stored back to back."""
    import torch
    lens = [len(d) for d in docs]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if docs else np.zeros(0, np.int64)
    buf = b"".join(docs) or b"\0"
    return (torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda(), torch.from_numpy(off).cuda(), torch.tensor(lens, dtype=torch.int64).cuda())


def same_bits(a, b):
    return np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data.view(np.uint32), b.data.view(np.uint32))


def test_tokenizer_generators_and_control_bytes(clib):
    rng = np.random.default_rng(3)
    # word documents: tokens ending at, starting at and straddling every 64-byte step, runs of spaces, every length of LENGTHS (4097 bytes:
    # the global form), and tokens holding \t, \n, \r and \0 -- compared through the export, since vocab.txt cannot hold a newline
    corpus = tc.word_boundary_docs() + tc.space_docs() + tc.length_docs(rng) + [b"a\tb \n x\ny \t a\tb", b"\n \n\n x\ny \t\n", b"\t"]
    for bases in ([tr.base(ngram_range=(1, 2))], [tr.base(ngram_range=(2, 3), max_length=5)], [tr.base(ngram_range=(1, 1), max_length=33)]):
        m = train(corpus, bases)
        want = same_as_statement(clib, m.h, corpus, bases, "word generators")
        for t in (b"\n", b"\t", b"a\tb", b"x\ny", b"\n\n", b"\t\n", b"z\0z", b"a\rb"):
            assert t in want["vocab"], t
        f = clib.tfidf_train_forms(m.h)
        assert f["df_global_segments"] == (1 if bases[0]["max_length"] < 0 else 0), f
        m.close()
    # character documents: 1-, 2-, 3- and 4-byte characters across the steps, and documents cut inside their last character
    chars = tc.char_docs_wellformed(rng)
    for bases in ([tr.base(tok_type=20, ngram_range=(1, 3))], [tr.base(tok_type=20, ngram_range=(2, 2), max_length=10)]):
        m = train(chars, bases)
        same_as_statement(clib, m.h, chars, bases, "char generators")
        m.close()
    for doc, status, _ in tc.char_docs_status():
        bad = tr.Trained(tr.OURS, "xrl_", [b"ok", doc, b"fine"], [tr.base(tok_type=20)])
        assert not bad.h and "document 1" in bad.error, (doc, bad.error)
        assert ("not utf-8 encoded" in bad.error) if status == 1 else ("too few continuation bytes" in bad.error), (doc, status, bad.error)


def test_caller_owned_text_between_vocabulary_bytes(clib):
    import torch
    from pecos_amd.features import tfidf_train_device, tfidf_transform_device
    docs = [d for d in tr.word_docs(41, 40) if d][:24] + tr.long_token_docs()[:2]
    band = b" poison zz never_a_token \xfe\xfe "             # vocabulary bytes: tokens that enter the model if a kernel reads outside a document
    order = np.random.default_rng(5).permutation(len(docs))
    buf, off, ln = bytearray(b"\x01" + band), [0] * len(docs), [len(d) for d in docs]
    for i in order:                                           # any address order, a band between every two documents
        off[i] = len(buf)
        buf += docs[i] + band
    # aliased documents: one stored document named three times, and one that overlaps another (its tail from a token start on)
    cut = docs[3].index(b" ") + 1 if b" " in docs[3] else 0
    off += [off[0], off[0], off[3] + cut]
    ln += [ln[0], ln[0], ln[3] - cut]
    corpus = [bytes(buf[o:o + n]) for o, n in zip(off, ln)]
    assert corpus[-3] == docs[0] and all(b"poison" not in d for d in corpus)
    dev = torch.device("cuda", 0)
    whole_text = torch.from_numpy(np.frombuffer(bytes(buf), dtype=np.uint8).copy()).to(dev)
    text = whole_text[1:]                                     # an odd address
    off_w, off_p = dv.banded(np.array(off, np.int64) - 1, 1, dv.BAND, np.int64(1), dev)          # band: a valid offset (inside the first poison band)
    len_w, len_p = dv.banded(np.array(ln, np.int64), 3, dv.BAND, np.int64(6), dev)               # band: a valid length ("poison")
    bases = [tr.base(ngram_range=(1, 2)), tr.base(ngram_range=(2, 2), max_length=4)]
    cfg = {"base_vect_configs": [{"ngram_range": (1, 2)}, {"ngram_range": (2, 2), "truncate_length": 4}], "norm_p": 2}
    side = torch.cuda.Stream(device=dev)
    vec = tfidf_train_device(text, off_p, len_p, cfg, stream=side.cuda_stream)
    want = same_as_statement(clib, vec.model, corpus, bases, "banded text")
    assert b"poison" not in clib.tfidf_export(vec.model, 0)[0] and b"\xfe\xfe" not in clib.tfidf_export(vec.model, 0)[0]
    f = clib.tfidf_train_forms(vec.model)
    assert f["vocab_docs"] == len(corpus) and f["df_lds_segments"] + f["df_global_segments"] == 2 * len(corpus)
    X = tfidf_transform_device(vec, text, off_p, len_p, stream=side.cuda_stream).download()
    with env(XRL_TFIDF_HOST_DOCS=0):
        assert same_bits(X, vec.predict(corpus))
    assert same_bits(X[len(docs)], X[0]) and same_bits(X[len(docs) + 1], X[0])
    dv.assert_bands_intact(off_w, off_p, np.int64(1), "offsets")
    dv.assert_bands_intact(len_w, len_p, np.int64(6), "lengths")
    assert bytes(whole_text.cpu().numpy().tobytes()) == bytes(buf), "the caller's text was written"


def test_trained_handle_through_predict_text_with_both_tokenizers(clib, tmp_path):
    import xrl_synth
    from pecos_amd import XLinearModel
    from pecos_amd.features import Tfidf, predict_text
    corpus, bases, _ = tr.cases()["word_bi_cut"]
    vec = Tfidf.train(corpus, {"ngram_range": (1, 2), "truncate_length": 7})
    mdir = str(tmp_path / "x")
    xrl_synth.make_model(mdir, vec.nr_features, 300, [60, 30, 12], seed=61, shape=[5, 30, 300])
    m = XLinearModel.load(mdir)
    h = predict_text(vec, m, corpus, beam_size=5, only_topk=6, tokenizer="host")
    d = predict_text(vec, m, corpus, beam_size=5, only_topk=6, tokenizer="device")
    assert h.nnz > 0 and same_bits(h, d)
    with env(XRL_TFIDF_HOST_DOCS=0):
        assert same_bits(m.predict(vec.predict(corpus), beam_size=5, only_topk=6), h)


def test_end_to_end_text_to_labels(clib, golden, tmp_path):
    import pecos_amd
    from pecos_amd import DeviceMatrix, XLinearModel
    from pecos_amd.features import predict_text, tfidf_train_device, tfidf_transform_device
    docs, Y = tr.e2e_corpus()
    text, off, lens = tensors(docs)
    vec = tfidf_train_device(text, off, lens, {"ngram_range": (1, 2), "min_df_cnt": 2})
    Xd = tfidf_transform_device(vec, text, off, lens)
    X_ref = smat.csr_matrix((golden["e2e/data_bits"].view(F32), golden["e2e/indices"].astype(np.int32), golden["e2e/indptr"]), shape=(len(docs), vec.nr_features))
    Xh = Xd.download()
    assert X_ref.nnz > 1000 and same_bits(Xh, X_ref), "the X of the trained vectorizer is not the recorded reference's"
    L, depth = Y.shape[1], 3
    kw = dict(rr.E2E_KW, negative_sampling_scheme="tfn+man")

    def chain(X_dev, X_host, folder):
        E = pecos_amd.label_embedding_device(Y, X_dev)
        codes = pecos_amd.run_clustering_device(E, depth, seed=0).cpu().numpy().view(np.uint32)
        C = smat.csc_matrix((np.ones(L, F32), (np.arange(L), codes)), shape=(L, 1 << depth), dtype=F32)
        XLinearModel.train_device(X_host, smat.csc_matrix(Y), C=C, **kw).save(folder)
        model = XLinearModel.load(folder)
        return codes, predict_text(vec, model, docs, tokenizer="device"), predict_text(vec, model, docs, tokenizer="host")

    codes_a, pa_dev, pa_host = chain(Xd, Xh, str(tmp_path / "ours"))
    codes_b, pb_dev, pb_host = chain(DeviceMatrix.upload(X_ref, 0), X_ref, str(tmp_path / "ref"))
    assert np.array_equal(codes_a, codes_b) and len(set(codes_a.tolist())) == 1 << depth
    assert pa_dev.nnz >= len(docs) and same_bits(pa_dev, pb_dev) and same_bits(pa_host, pb_host) and same_bits(pa_dev, pa_host)


def test_destruct_frees_the_tables_of_a_trained_handle(clib):
    import torch
    # a vocabulary of 200 k tokens: the short-token table alone is 8 MiB
    corpus = [b" ".join(b"w%d" % i for i in range(j, 200000, 40)) for j in range(40)]
    text, off, lens = tensors(corpus)
    probe = tensors([b"w0 w40 w5", b"w199999"])

    def trained():
        h = clib.tfidf_train_device(0, text.data_ptr(), off.data_ptr(), lens.data_ptr(), len(corpus), {"max_df_ratio": 1.0})
        assert clib.tfidf_device_bytes(h, 0) == 0              # training leaves nothing on the device
        q = clib.tfidf_transform_device(h, 0, probe[0].data_ptr(), probe[1].data_ptr(), probe[2].data_ptr(), 2)
        clib.smat_free(q)
        return h

    h = trained()
    size = clib.tfidf_device_bytes(h, 0)
    assert size >= 8 << 20 and clib.tfidf_train_forms(h)["distinct_tokens"] == 200000
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(8):                                          # eight more handles leave the free memory where it was (a leak would take eight tables' worth)
        clib.tfidf_destruct(trained())
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 2 * size
    clib.tfidf_destruct(h)
