"""TF-IDF training on the device (K15, pecos_amd/csrc/xrl_tfidf_train.hip): xrl_tfidf_train, xrl_tfidf_train_device and Tfidf.train
against the statement of the rule (tests/tfidf_training_rule.py), the recording of the compiled reference
(tests/golden/tfidf_training_ref.npz) and, where it is built, the live reference.  Compared exactly: token -> id and n-gram -> id maps
and idf bits (through xrl_tfidf_export), saved folders as parsed content, predict bits of the trained handle."""
import glob
import os
import tempfile

import numpy as np
import pytest

import tfidf_training_rule as tr
from tfidf_cases import CAP

pytestmark = pytest.mark.gpu
F32 = np.float32
CASES = tr.cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(tr.GOLDEN)


@pytest.fixture(scope="module")
def clib():
    from pecos_amd import clib
    clib.set_device(0)
    return clib


class env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update({k: str(v) for k, v in self.kw.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same_as_statement(clib, handle, corpus, bases, what=""):
    for b, p in enumerate(bases):
        want = tr.statement(corpus, p)
        vocab, ngrams, idf = clib.tfidf_export(handle, b)
        assert vocab == want["vocab"], f"{what}: base {b}: token ids differ"
        assert ngrams == want["ngrams"], f"{what}: base {b}: feature ids differ"
        assert np.array_equal(idf.view(np.uint32), want["idf"].view(np.uint32)), f"{what}: base {b}: idf bits differ"
    return want


def train(corpus, bases, norm_p=None, threads=1):
    m = tr.Trained(tr.OURS, "xrl_", corpus, bases, norm_p, threads=threads)
    assert m.error is None and m.h, m.error
    return m


@pytest.mark.parametrize("name", sorted(CASES))
def test_train_equals_statement_recording_and_folder(name, golden, clib):
    corpus, bases, norm_p = CASES[name]
    m = train(corpus, bases, norm_p)
    same_as_statement(clib, m.h, corpus, bases, name)
    with tempfile.TemporaryDirectory() as d:
        assert m.save(d) is None
        assert tr.canon_model(*tr.parse_folder(d)) == tr.canon_model(*tr.statement_as_parsed(corpus, bases, norm_p)), name
        assert tr.digest(tr.canon_model(*tr.parse_folder(d))) == str(golden[name + "/digest"]), name
        loaded = tr.Trained.loaded(tr.OURS, d)
        assert loaded.error is None, loaded.error
    probe = tr.probe_of(bases)
    try:
        # the trained handle predicts the bits the reference's in-memory trained model does
        with env(XRL_TFIDF_HOST_DOCS=0):
            X = clib.tfidf_predict(m.h, probe)
        assert np.array_equal(X.indptr, golden[name + "/indptr"]) and np.array_equal(X.indices, golden[name + "/indices"]), name
        assert np.array_equal(X.data.view(np.uint32), golden[name + "/data_bits"]), name
        # train -> save -> load (this library) -> predict == the reference's train -> save -> load -> predict (the idf is the %f text by then)
        if os.path.exists(tr.REF):
            ref = tr.Trained(tr.REF, "c_", corpus, bases, norm_p, threads=1)
            with tempfile.TemporaryDirectory() as d:
                assert ref.save(d) is None
                ref_loaded = tr.Trained.loaded(tr.REF, d)
            want = ref_loaded.predict(probe)
            with env(XRL_TFIDF_HOST_DOCS=0):
                got = loaded.predict(probe)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), name
            ref.close()
            ref_loaded.close()
    finally:
        loaded.close()
        m.close()


def test_nothing_kept_gives_empty_rows(clib):
    corpus, bases, _ = CASES["word_nothing_kept"]
    m = train(corpus, bases)
    assert clib.tfidf_nr_features(m.h) == 0
    X = clib.tfidf_predict(m.h, [b"a b", b"c", b"", b"d", b"e"])
    assert X.shape == (5, 0) and X.nnz == 0
    m.close()


def _uni_docs(T):
    """T one-byte tokens over five letters: 2T - 1 bytes."""
    return b" ".join(bytes([97 + i % 5]) for i in range(T))


def test_cap_boundaries_and_forms(clib):
    # a document of T one-byte tokens has 2T - 1 bytes and a token bound of T: CAP - 1 and CAP are served by the LDS form, CAP + 1 by the global one
    for T, glob_segments in ((CAP - 1, 0), (CAP, 0), (CAP + 1, 1)):
        corpus = [_uni_docs(T), b"a b", b"c"]
        bases = [tr.base(ngram_range=(1, 2))]
        m = train(corpus, bases)
        f = clib.tfidf_train_forms(m.h)
        assert (f["df_global_segments"], f["df_lds_segments"]) == (glob_segments, 3 - glob_segments), (T, f)
        assert f["vocab_docs"] == 3 and f["distinct_tokens"] == 5
        same_as_statement(clib, m.h, corpus, bases, f"T={T}")
        m.close()
    # max_length on both sides of T and of a 64-byte step, on a long document
    doc = _uni_docs(CAP + 40)
    for cut in (31, 32, 33, CAP - 1, CAP, CAP + 1, CAP + 39, CAP + 40, CAP + 41):
        corpus, bases = [doc, b"a b c", doc[:300]], [tr.base(ngram_range=(2, 3), max_length=cut)]
        m = train(corpus, bases)
        same_as_statement(clib, m.h, corpus, bases, f"cut={cut}")
        m.close()


def test_batches_table_growth_and_truncated_hash(clib):
    # (600 distinct tokens in one document: more than half of the 1024 slots the vocabulary table starts with under this budget)
    corpus = tr.word_docs(7, 64, vocab=150) + tr.long_token_docs() + [_uni_docs(CAP + 5), b" ".join(b"u%d" % i for i in range(600))]
    bases = [tr.base(ngram_range=(1, 2)), tr.base(ngram_range=(2, 3), max_length=9)]
    with env(XRL_TFIDF_TRAIN_SCRATCH_ENTRIES=700):
        m = train(corpus, bases)
    f = clib.tfidf_train_forms(m.h)
    assert f["batches"] >= 6 and f["table_grows"] >= 1 and f["df_global_segments"] >= 1 and f["df_lds_segments"] >= 1, f
    assert f["long_compares"] > 0
    same_as_statement(clib, m.h, corpus, bases, "small scratch")
    m.close()
    for bits in (2, 4):
        with env(XRL_TFIDF_TRAIN_HASH_BITS=bits):
            m = train(corpus, bases)
        same_as_statement(clib, m.h, corpus, bases, f"hash cut to {bits} bits")
        m.close()


def test_document_counts(clib):
    for n in (1, 2, 63, 64, 65):
        corpus, bases = tr.word_docs(11, n), [tr.base(ngram_range=(1, 2), max_df_ratio=1.0)]
        m = train(corpus, bases)
        same_as_statement(clib, m.h, corpus, bases, f"nr_doc={n}")
        m.close()
    corpus, bases = tr.word_docs(12, 5000, vocab=300, max_len=9), [tr.base(ngram_range=(1, 2), min_df_cnt=2, max_feature=400)]
    m = train(corpus, bases, threads=4)
    same_as_statement(clib, m.h, corpus, bases, "5000 documents")
    m.close()


def test_key_width_refusal_and_char_statuses(clib):
    alpha = tr.ALPHA17
    corpus = ["".join(alpha).encode() * 2]
    m = tr.Trained(tr.OURS, "xrl_", corpus, [tr.base(tok_type=20, ngram_range=(26, 26))])          # 17 characters: 5 bits, 26 * 5 = 130
    assert not m.h and "26 tokens at 5 bits" in m.error and "largest n that fits is 25" in m.error, m.error
    m = tr.Trained(tr.OURS, "xrl_", [b"ab", b"a\x80b", b"c"], [tr.base(tok_type=20)])                # a stray continuation byte: status 1
    assert not m.h and "not utf-8 encoded" in m.error and "document 1" in m.error, m.error
    m = tr.Trained(tr.OURS, "xrl_", [b"ab", b"c", b"x\xe2\x82y"], [tr.base(tok_type=20, max_length=1)])  # a short sequence past the cut: status 2
    assert not m.h and "document 2" in m.error and "too few continuation bytes" in m.error, m.error
    m = train([b"ab", b"a\x80b", b"x\xe2\x82y"], [tr.base()])                                       # the word tokenizer takes any bytes
    m.close()


def test_resident_form_python_layer_and_transform(clib, golden):
    import torch
    import pecos_amd
    from pecos_amd.features import Tfidf, tfidf_train_device, tfidf_transform_device
    name = "word_bi_cut"
    corpus, bases, _ = CASES[name]
    cfg = {"ngram_range": (1, 2), "truncate_length": 7}
    # caller-owned text: three bytes of padding in front, documents stored in reverse order with a gap byte between them, on a side stream
    order = list(range(len(corpus)))[::-1]
    buf, off = bytearray(b"\xffzz"), [0] * len(corpus)
    for i in order:
        off[i] = len(buf)
        buf += corpus[i] + b"#"
    dev = torch.device("cuda", 0)
    text = torch.tensor(list(buf), dtype=torch.uint8, device=dev)
    d_off = torch.tensor(off, dtype=torch.int64, device=dev)
    d_len = torch.tensor([len(d) for d in corpus], dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    vec = tfidf_train_device(text, d_off, d_len, cfg, stream=side.cuda_stream)
    same_as_statement(clib, vec.model, corpus, bases, "resident form")
    vec2 = Tfidf.train(corpus, dict(cfg))
    same_as_statement(clib, vec2.model, corpus, bases, "Tfidf.train")
    with pytest.raises(ValueError, match="Unknown argument"):
        Tfidf.train(corpus, {"ngrams": 2})
    # transform: the weighted X in HBM with no XR-Linear model == Tfidf.predict of the same documents (host tokenizer)
    probe = tr.PROBE_WORD
    pbuf = b"".join(probe)
    p_text = torch.tensor(list(pbuf), dtype=torch.uint8, device=dev)
    lens = [len(d) for d in probe]
    p_off = torch.tensor(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), device=dev)
    p_len = torch.tensor(lens, dtype=torch.int64, device=dev)
    before = clib.tfidf_device_bytes(vec.model, 0)
    Xd = tfidf_transform_device(vec, p_text, p_off, p_len).download()
    assert before == 0 and clib.tfidf_device_bytes(vec.model, 0) > 0
    with env(XRL_TFIDF_HOST_DOCS=0):
        Xh = vec.predict(probe)
    for X in (Xd, Xh):
        assert np.array_equal(X.indptr, golden[name + "/indptr"]) and np.array_equal(X.indices, golden[name + "/indices"])
        assert np.array_equal(X.data.view(np.uint32), golden[name + "/data_bits"])
    # Preprocessor.train / save / load
    with tempfile.TemporaryDirectory() as d:
        pre = pecos_amd.Preprocessor.train({"type": "tfidf", "kwargs": cfg}, corpus)
        pre.save(d)
        back = pecos_amd.Preprocessor.load(d)
        assert back.nr_features == vec.nr_features
        want = tr.statement(corpus, bases[0])            # (a loaded handle's idf is the folder's %f text: the maps are compared)
        vocab, ngrams, idf = clib.tfidf_export(back.vectorizer.model, 0)
        assert (vocab, ngrams) == (want["vocab"], want["ngrams"]) and ["%f" % v for v in idf] == ["%f" % v for v in want["idf"]]


def test_load_then_save_keeps_every_golden_folder(clib):
    folders = [f for f in sorted(glob.glob(os.path.join(tr.REPO, "tests", "golden", "tfidf_models", "*", "model"))) if os.path.isdir(f) and "charwb_bigram" not in f]
    assert folders
    for f in folders:
        # (a folder saved from one BaseVectorizer holds the base's files directly; the saved one always has the ensemble layout)
        want = tr.parse_folder(f)[1] if os.path.exists(os.path.join(f, "meta.json")) else [tr.parse_base(f)]
        h = clib.tfidf_load(f)
        with tempfile.TemporaryDirectory() as d:
            clib.tfidf_save(h, d)
            meta, got = tr.parse_folder(d)
        clib.tfidf_destruct(h)
        assert meta["kwargs"]["num_base_vect"] == len(want), f
        for g, w in zip(got, want):
            assert (g["vocab"], g["ngrams"], g["idf_text"], g["tok_config"]) == (w["vocab"], w["ngrams"], w["idf_text"], w["tok_config"]), f
            assert g["config"]["type"] == w["config"]["type"]
            for k, v in w["config"]["kwargs"].items():          # every parameter the folder states is stated again (older folders lack some)
                assert g["config"]["kwargs"][k] == v, (f, k)


@pytest.mark.skipif(not os.path.exists(tr.REF), reason="the compiled reference is not built")
def test_against_the_live_reference(clib):
    corpus = tr.word_docs(21, 80, vocab=60) + tr.long_token_docs()
    bases = [tr.base(ngram_range=(1, 3), min_df_cnt=2, max_df_ratio=0.9, max_feature=120, add_one_idf=True), tr.base(ngram_range=(2, 2), norm_p=1, smooth_idf=False)]
    ours, ref = train(corpus, bases, norm_p=2), tr.Trained(tr.REF, "c_", corpus, bases, 2, threads=8)
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        assert ours.save(a) is None and ref.save(b) is None
        assert tr.canon_model(*tr.parse_folder(a)) == tr.canon_model(*tr.parse_folder(b))
    probe = corpus[:6] + tr.PROBE_WORD
    with env(XRL_TFIDF_HOST_DOCS=0):
        got = ours.predict(probe)
    want = ref.predict(probe)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    ours.close()
    ref.close()
