"""The device tokenizer (K9, xrl_tfidf_counts_device / xrl_tfidf_predict_device_text / tokenizer="device") against the host tokenizer
(clib.tfidf_counts): term counts are integers, so every comparison is exact -- indptr, feature ids and counts."""
import os

import numpy as np
import pytest

import tfidf_cases as tc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tfidf_models")
GOLDEN_NAMES = sorted(os.listdir(GOLDEN))


@pytest.fixture(scope="module")
def xmodel(tmp_path_factory):
    """Any loaded XLinearModel: the device tokenizer takes its device and stream from it."""
    import xrl_synth
    from pecos_amd import XLinearModel, clib
    clib.set_device(0)
    d = str(tmp_path_factory.mktemp("k9_model"))
    xrl_synth.make_model(d, 500, 800, [150, 90, 25], seed=21, shape=[4, 28, 800])
    return XLinearModel.load(d)


def _tensors(docs, layout=None):
    """(text uint8, offsets int64, lengths int64) CUDA tensors of byte documents; layout: a function (docs) -> (buffer, offsets, lengths)."""
    import torch
    from pecos_amd import clib
    buf, off, lens = layout(docs) if layout else clib.corpus_packed(docs)
    text = torch.from_numpy(np.frombuffer(bytes(buf) or b"\0", dtype=np.uint8).copy()).cuda()
    return text, torch.from_numpy(np.asarray(off, dtype=np.uint64).view(np.int64).copy()).cuda(), torch.from_numpy(np.asarray(lens, dtype=np.uint64).view(np.int64).copy()).cuda()


def _device_counts(vec, xmodel, docs, layout=None, status=None, stream=None, tensors=None):
    from pecos_amd import clib
    from pecos_amd.features import tfidf_counts_device
    text, off, lens = tensors if tensors is not None else _tensors(docs, layout)
    q = tfidf_counts_device(vec, xmodel, text, off, lens, status=status, stream=stream)
    with clib.freeing(q):
        return clib.queries_download(q)


def _same(a, b, what=""):
    assert a.shape == b.shape, what
    assert np.array_equal(a.indptr, b.indptr), f"{what}: row lengths differ"
    assert np.array_equal(a.indices, b.indices), f"{what}: feature ids differ"
    assert np.array_equal(a.data.view(np.uint32), b.data.view(np.uint32)), f"{what}: counts differ"


def _check(vec, xmodel, docs, what="", **kw):
    from pecos_amd import clib
    got = _device_counts(vec, xmodel, docs, **kw)
    _same(got, clib.tfidf_counts(vec.model, docs, threads=2), what)
    return got


def _load(folder):
    from pecos_amd.features import Tfidf
    return Tfidf.load(folder)


GRAMS = [(0,), (1,), (2,), (3,), (4,), (5,), (6,), (7,), (8,), (9,), (77,), (5000000,), (0, 1), (1, 0), (3, 4), (77, 0), (0, 1, 2), (2, 1, 0), (0, 0, 0, 0), (1, 2, 3, 4, 5),
         (9, 10, 11), (0, 1)]
NEG_GRAMS = [(0, -1), (-1,), (-1, -1, 2)]


def _word_model(folder, ngram_range=(1, 5), max_length=-1, far=True, negative=False, **over):
    """The words of tfidf_cases.WORDS as tokens 0..11, "dup" listed twice (the last index, 77, wins), with `far` a token index far outside the
    vocabulary (its unigram lives in `packed`, and 3-grams no longer pack: `gen`); n-grams up to 5 tokens, (0, 1) listed twice (the last
    feature id wins); with `negative` n-grams that name the unknown token -1."""
    vocab = [(i, w) for i, w in enumerate(tc.WORDS)] + [(12, b"dup"), (77, b"dup")] + ([(5000000, b"far")] if far else [])
    grams = [g for g in GRAMS if far or 5000000 not in g] + (NEG_GRAMS if negative else [])
    feats = [(i, 1.0 + 0.25 * i, g) for i, g in enumerate(grams)]
    return tc.write_base(folder, 10, vocab, feats, ngram_range=ngram_range, max_length=max_length, **over)


@pytest.fixture(scope="module")
def word_vec(tmp_path_factory):
    return _load(_word_model(str(tmp_path_factory.mktemp("k9_word") / "m")))


def test_document_lengths(word_vec, xmodel, tmp_path):
    rng = np.random.default_rng(1)
    docs = tc.length_docs(rng)
    assert [len(d) for d in docs] == list(tc.LENGTHS)
    _check(word_vec, xmodel, docs, "word")
    chars = [c.encode() for c in tc.CHARS]
    vocab, feats = tc.model_of_pieces([chars], max_n=2)
    cvec = _load(tc.write_base(str(tmp_path / "c"), 20, vocab, feats, ngram_range=(1, 2)))
    cdocs = [(b"ab " * (n // 3 + 1))[:n] for n in tc.LENGTHS]
    _check(cvec, xmodel, cdocs, "char")


def test_token_boundaries_spaces_and_separators(word_vec, xmodel):
    docs = tc.word_boundary_docs() + tc.space_docs() + [b"z\0z t\tb a\nb z\0z", b"a\tbb a\0bb a\nbb a bb"]
    got = _check(word_vec, xmodel, docs)
    assert got.nnz > 0 and got[len(tc.word_boundary_docs()) + 1].nnz == 0          # (a document of spaces only holds nothing)
    # the 9-byte token whose first 8 bytes are another token is its own feature; \0 and \t do not separate
    rows = tc.rows_of(_check(word_vec, xmodel, [b"12345678X", b"12345678", b"z\0z", b"z z"]))
    assert rows[0] == [(6, 1)] and rows[1] == [(4, 1)] and rows[2] == [] and rows[3] == []     # (z\0z is token 11, which no n-gram names)


@pytest.mark.parametrize("max_length", [-1, 31, 32, 33, 39, 40, 41])
def test_max_length_cut(xmodel, tmp_path, max_length):
    # T = 40 one-byte tokens; token 32 starts at byte 64: the cut falls before, at and after the step boundary, and at T - 1, T, T + 1
    vec = _load(_word_model(str(tmp_path / "m"), ngram_range=(1, 3), max_length=max_length))
    docs = [b"a bb " * 20, b"a " * 40, (b"a " * 40)[:-1], b" " + b"a " * 40, b"a " * 31 + b"ccc ccc a a a a a a a", b"a"]
    assert len(tc.host_word(docs[1])) == 40 and docs[1][64:65] == b"a"
    _check(vec, xmodel, docs, f"max_length {max_length}")


def test_unigram_homes_and_ngram_ranges(xmodel, tmp_path):
    # inside uni (token 0), beyond uni = packed (token 5000000), unknown; min_ngram 2 with one token: nothing; max_ngram above the model's max_n
    vec = _load(_word_model(str(tmp_path / "a"), ngram_range=(1, 9)))
    rows = tc.rows_of(_check(vec, xmodel, [b"a", b"far", b"unk", b"far a far", b"a bb ccc 1234567 12345678 123456789 a"]))
    assert rows[0] == [(0, 1)] and rows[1] == [(11, 1)] and rows[2] == [] and rows[3] == [(0, 1), (11, 2)]
    vec2 = _load(_word_model(str(tmp_path / "b"), ngram_range=(2, 3)))
    rows = tc.rows_of(_check(vec2, xmodel, [b"a", b"a bb", b"", b"a bb ccc"]))
    assert rows[0] == [] and rows[1] == [(21, 1)]                                  # (0, 1) is listed twice: the last id, 21, wins


@pytest.mark.parametrize("far,negative", [(False, False), (True, False), (True, True), (False, True)])
def test_ngram_tables(xmodel, tmp_path, far, negative):
    # without the far token every n-gram packs into one u64; with it 3-grams and longer live in `gen`; with `negative` the model names the
    # unknown token, so an unknown token inside a run is looked up too (unigram and bigram through `gen`)
    vec = _load(_word_model(str(tmp_path / "m"), far=far, negative=negative))
    rng = np.random.default_rng(3)
    pool = tc.WORDS + [b"dup", b"far", b"unk", b"another-unknown-token"]
    docs = [b" ".join(pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(0, 40)))) for _ in range(300)]
    docs += [b"a bb ccc", b"a a a a a a a a", b"unk ccc", b"unk unk ccc", b"a unk", b"dup a", b"far", b"a bb ccc unk a bb ccc", b"bb ccc 1234567 12345678 123456789",
             b"ccc bb a", b"t\tb z\0z", "日本語 t\tb z\0z".encode()]
    rows = tc.rows_of(_check(vec, xmodel, docs, f"far={far} negative={negative}"))
    if negative:
        base = len(GRAMS) - (0 if far else 1)
        assert (base + 1, 1) in rows[302] and (base, 1) in rows[304] and (base + 2, 1) in rows[303]     # (-1,), (0, -1), (-1, -1, 2)


def _forms(vec):
    from pecos_amd import clib
    return clib.tfidf_device_forms(vec.model)


def test_counting_and_form_selection(xmodel, tmp_path):
    # unigrams only: a document of T one-byte tokens has exactly T occurrences, and its bound is T -- CAP - 1 and CAP go through the LDS
    # form, CAP + 1 and 5000 through the global one; in one call both forms serve a neighbour
    vec = _load(_word_model(str(tmp_path / "m"), ngram_range=(1, 1)))
    def doc(T):
        return b" ".join([b"a", b"bb", b"a", b"ccc", b"a"][i % 5] for i in range(T))
    f0 = _forms(vec)
    rows = tc.rows_of(_check(vec, xmodel, [b"a " * 1000]))
    assert rows == [[(0, 1000)]]
    f1 = _forms(vec)
    assert (f1["lds_segments"] - f0["lds_segments"], f1["global_segments"] - f0["global_segments"]) == (1, 0)
    sizes = [tc.CAP - 1, tc.CAP, tc.CAP + 1, 5000, 3, tc.CAP + 1, tc.CAP]
    docs = [b"a " * (T - 1) + b"a" for T in sizes]
    assert [tc.is_big(10, -1, 1, 1, 1, len(d)) for d in docs] == [False, False, True, True, False, True, False]
    both = _check(vec, xmodel, docs)
    f2 = _forms(vec)
    assert (f2["lds_segments"] - f1["lds_segments"], f2["global_segments"] - f1["global_segments"]) == (4, 3)
    assert tc.rows_of(both) == [[(0, T)] for T in sizes]
    # mixed words, and the mixed batch equal to one call per form
    docs = [doc(T) for T in sizes] + [b"", b"unk"]
    both = _check(vec, xmodel, docs)
    small = [d for d in docs if not tc.is_big(10, -1, 1, 1, 1, len(d))]
    large = [d for d in docs if tc.is_big(10, -1, 1, 1, 1, len(d))]
    f3 = _forms(vec)
    a, b = _device_counts(vec, xmodel, small), _device_counts(vec, xmodel, large)
    f4 = _forms(vec)
    assert (f4["lds_segments"] - f3["lds_segments"], f4["global_segments"] - f3["global_segments"]) == (len(small), len(large))
    ia = ib = 0
    for r, d in enumerate(docs):
        if tc.is_big(10, -1, 1, 1, 1, len(d)):
            part = b[ib]; ib += 1
        else:
            part = a[ia]; ia += 1
        assert np.array_equal(both[r].indices, part.indices) and np.array_equal(both[r].data.view(np.uint32), part.data.view(np.uint32)), r
    # bigrams: the bound counts n-gram positions, 2T - 1
    vec2 = _load(_word_model(str(tmp_path / "m2"), ngram_range=(1, 2)))
    docs = [b"a " * (T - 1) + b"a" for T in (512, 513, 2000)] + [doc(300), doc(2000)]
    assert [tc.is_big(10, -1, 1, 2, 5, len(d)) for d in docs] == [False, True, True, False, True]
    _check(vec2, xmodel, docs, "bigrams")


def test_batches(xmodel, tmp_path, monkeypatch):
    # a scratch budget of 600 entries cuts the corpus into batches: documents above it are batches of their own, both forms occur in one
    # batch and across batches, a bad document's row stays empty, and the pieces come back side by side
    import torch
    from pecos_amd import clib
    vec = _load(tc.write_ensemble(str(tmp_path / "e"), [
        dict(tok_type=10, vocab=[(i, w) for i, w in enumerate(tc.WORDS)], features=[(i, 1.0, g) for i, g in enumerate([(0,), (1,), (2,), (0, 1), (1, 2)])], ngram_range=(1, 2)),
        dict(tok_type=20, vocab=[(0, b"a"), (1, b"b"), (2, b" ")], features=[(0, 1.0, (0,)), (1, 1.0, (1, 1)), (2, 1.0, (2,))], ngram_range=(1, 2), max_length=50)]))
    rng = np.random.default_rng(7)
    docs = tc.fuzz_word_corpus(rng, tc.WORDS[:4], 120, 30) + [b"a bb " * 300, b"", b"a bb ccc " * 500, b"bb"] + tc.fuzz_word_corpus(rng, tc.WORDS[:4], 40, 60)
    one = _check(vec, xmodel, docs, "one batch")
    f0 = _forms(vec)
    monkeypatch.setenv("XRL_TOK_SCRATCH_ENTRIES", "600")
    many = _check(vec, xmodel, docs, "batches")
    f1 = _forms(vec)
    assert f1["batches"] - f0["batches"] > 10 and f1["global_segments"] - f0["global_segments"] == 2
    _same(many, one, "batches against one batch")
    bad = list(docs)
    bad[5] = b"ab\x80"; bad[150] = b"\x80"
    st = torch.full((len(bad),), -1, dtype=torch.int32, device="cuda")
    got = _device_counts(vec, xmodel, bad, status=st)
    want = clib.tfidf_counts(vec.model, [b"" if i in (5, 150) else d for i, d in enumerate(bad)])
    _same(got, want, "batches with bad documents")
    assert [i for i, v in enumerate(st.cpu().tolist()) if v] == [5, 150]
    q = clib.tfidf_predict_device(vec.model, xmodel.model.model_chain, docs, threads=2, tokenizer="device")
    monkeypatch.delenv("XRL_TOK_SCRATCH_ENTRIES")
    q1 = clib.tfidf_predict_device(vec.model, xmodel.model.model_chain, docs, threads=2)
    with clib.freeing(q, q1):
        _same(clib.queries_download(q), clib.queries_download(q1), "weighted X over batches")


def test_char_modes(xmodel, tmp_path):
    import torch
    from pecos_amd import clib
    rng = np.random.default_rng(12)
    docs = tc.char_docs_wellformed(rng) + ["".join(tc.CHARS[int(i)] for i in rng.integers(0, len(tc.CHARS), size=1500)).encode()]
    pieces = [tc.host_char(d)[0] for d in docs]
    cases = tc.char_docs_status()
    for d, _, _ in cases:
        pieces += [[d[b:e] for b, e in tc.char_rule(d)[0]], tc.host_char(d)[0]]
    vocab, feats = tc.model_of_pieces(pieces, max_n=3)
    for tok_type, max_length in ((20, -1), (30, -1), (20, 64), (20, 65), (20, 3)):
        vec = _load(tc.write_base(str(tmp_path / f"c{tok_type}_{max_length}"), tok_type, vocab, feats, ngram_range=(1, 3), max_length=max_length))
        _check(vec, xmodel, docs, f"char {tok_type} max_length {max_length}")
    # status 1: the call fails in the host's words; with a status tensor only that row is empty and the others are served
    vec = _load(tc.write_base(str(tmp_path / "status"), 20, vocab, feats))          # unigrams, no max_length cut: every position is checked
    good = [b"abc", "日本".encode()]
    for d, status, host_does in cases:
        batch = [good[0], d, good[1]]
        st = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        got = _device_counts(vec, xmodel, batch, status=st)
        assert st.cpu().tolist() == [0, status, 0], d
        want = clib.tfidf_counts(vec.model, [good[0], b"", good[1]])
        _same(got, want, "rows beside a bad document")
        if host_does == "fails":
            with pytest.raises(RuntimeError, match=r"the string is not utf-8 encoded! \(document 1\)"):
                _device_counts(vec, xmodel, batch)
            with pytest.raises(RuntimeError, match="the string is not utf-8 encoded!"):
                clib.tfidf_counts(vec.model, batch)
        else:
            # status 2: refused, and the refusal is needed -- the host's own answer is not the parallel rule's
            with pytest.raises(RuntimeError, match="document 1 .*use the host tokenizer"):
                _device_counts(vec, xmodel, batch)
            host_row = tc.rows_of(clib.tfidf_counts(vec.model, [d]))[0]
            assert host_row != tc.counts_of_pieces([d[b:e] for b, e in tc.char_rule(d)[0]], vocab, feats, (1, 1))
    # the lowest bad document is the one named
    with pytest.raises(RuntimeError, match=r"\(document 2\)"):
        _device_counts(vec, xmodel, [good[0], good[1], cases[0][0], cases[1][0]])


def test_ensemble_of_word_and_char(xmodel, tmp_path):
    chars = [c.encode() for c in tc.CHARS]
    cvocab, cfeats = tc.model_of_pieces([chars + chars[::-1]], max_n=2)
    wvocab = [(i, w) for i, w in enumerate(tc.WORDS)]
    wfeats = [(i, 1.0 + i, g) for i, g in enumerate([(0,), (1,), (2,), (0, 1), (1, 2), (9,)])]
    folder = tc.write_ensemble(str(tmp_path / "e"), [
        dict(tok_type=10, vocab=wvocab, features=wfeats, ngram_range=(1, 2)),
        dict(tok_type=20, vocab=cvocab, features=cfeats, ngram_range=(1, 2), max_length=70),
        dict(tok_type=10, vocab=wvocab, features=wfeats, ngram_range=(2, 2), max_length=3)])
    vec = _load(folder)
    rng = np.random.default_rng(5)
    docs = ["a bb ccc 日本語 é", "", " ", "a" * 200, "日本語 " * 30, "bb ccc " * 700] + [" ".join(["a", "bb", "ccc", "日本語", "ü😀"][int(i)] for i in rng.integers(0, 5, size=int(n)))
                                                                                  for n in rng.integers(0, 60, size=80)]
    docs = [d.encode() for d in docs]
    got = _check(vec, xmodel, docs, "ensemble")
    nf = [len(wfeats), len(cfeats), len(wfeats)]
    assert got.shape[1] == sum(nf) and got[0].indices.min() < nf[0] <= got[0].indices[got[0].indices >= nf[0]].min() < nf[0] + nf[1] <= got[0].indices.max()
    f = _forms(vec)
    assert f["global_segments"] > 0 and f["lds_segments"] > 0          # ("bb ccc" * 700 is big for the first base, small for the cut third one)


def test_caller_buffers(word_vec, xmodel):
    import torch
    from pecos_amd import clib
    rng = np.random.default_rng(9)
    docs = tc.fuzz_word_corpus(rng, tc.WORDS, 60, 30) + [b"a bb ccc", b"", b"a"]
    want = clib.tfidf_counts(word_vec.model, docs, threads=2)
    # d_text at odd byte offsets: a slice of a larger tensor
    for shift in (1, 3, 5):
        text, off, lens = _tensors(docs)
        big = torch.zeros(text.numel() + 8, dtype=torch.uint8, device="cuda")
        big[shift:shift + text.numel()] = text
        _same(_device_counts(word_vec, xmodel, None, tensors=(big[shift:shift + text.numel()], off, lens)), want, f"offset {shift}")
    # documents separated by bands of bytes that are vocabulary tokens: a read past a document's end would count them
    band = b"a bb ccc a"
    def banded(ds):
        buf, off, at = b"", [], 0
        for d in ds:
            buf += band; at += len(band)
            off.append(at); buf += d; at += len(d)
        return buf + band, np.array(off, dtype=np.uint64), np.array([len(d) for d in ds], dtype=np.uint64)
    _same(_device_counts(word_vec, xmodel, docs, layout=banded), want, "banded")
    over = clib.tfidf_counts(word_vec.model, [d + band for d in docs], threads=2)
    assert not np.array_equal(over.data, want.data) or not np.array_equal(over.indices, want.indices)      # (the over-read would have shown)
    # documents out of address order, and two documents aliasing the same bytes
    def reversed_layout(ds):
        buf, off, at = b"", [0] * len(ds), 0
        for i in reversed(range(len(ds))):
            off[i] = at; buf += ds[i]; at += len(ds[i])
        return buf, np.array(off, dtype=np.uint64), np.array([len(d) for d in ds], dtype=np.uint64)
    _same(_device_counts(word_vec, xmodel, docs, layout=reversed_layout), want, "out of order")
    def aliased(ds):
        return ds[0], np.zeros(len(ds), dtype=np.uint64), np.array([len(ds[0])] * len(ds), dtype=np.uint64)
    three = [b"a bb ccc a bb"] * 3
    _same(_device_counts(word_vec, xmodel, three, layout=aliased), clib.tfidf_counts(word_vec.model, three), "aliased")
    # a side stream
    side = torch.cuda.Stream()
    _same(_device_counts(word_vec, xmodel, docs, stream=side.cuda_stream), want, "side stream")
    # nr_doc 0 and 1
    got0 = _device_counts(word_vec, xmodel, [])
    assert got0.shape == (0, word_vec.nr_features) and got0.nnz == 0
    _same(_device_counts(word_vec, xmodel, docs[:1]), clib.tfidf_counts(word_vec.model, docs[:1]), "one document")


def _golden(name):
    import json
    folder = os.path.join(GOLDEN, name, "model")
    return folder, json.load(open(os.path.join(GOLDEN, name, "corpus.json")))


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_vectorizers(name, xmodel, tmp_path):
    import torch
    import xrl_synth
    from oracle.tfidf_oracle import TfidfOracle
    from pecos_amd import XLinearModel, clib
    from pecos_amd.features import predict_text
    folder, corpus = _golden(name)
    vec = _load(folder)
    docs = [c.encode("utf-8") for c in corpus]
    got = _check(vec, xmodel, docs, name)
    O = TfidfOracle(folder)
    indptr, idx, val = O.counts(docs)
    assert np.array_equal(got.indptr, indptr.astype(np.int64)) and np.array_equal(got.indices, idx.astype(np.int64)) and np.array_equal(got.data, val)
    # a 2000-document fuzz corpus over the model's own tokens
    rng = np.random.default_rng(23)
    toks = sorted(set().union(*[set(b.vocab) for b in O.base]))
    if O.base[0].tok_type != 10:
        toks = [b"".join(toks[int(i)] for i in rng.integers(0, len(toks), size=int(rng.integers(1, 9)))) for _ in range(200)]
    fuzz = [b" ".join(toks[int(i)] for i in rng.integers(0, len(toks), size=int(n))) for n in rng.integers(0, 90, size=2000)]
    fuzz[7] = b" ".join(toks[int(i)] for i in rng.integers(0, min(len(toks), 12), size=3000))           # one long row: the global form
    _check(vec, xmodel, fuzz, name + " fuzz")
    # the weighted X: same counts, same K5 -> the host-tokenizer handle's bits
    text, off, lens = _tensors(fuzz)
    mc = xmodel.model.model_chain
    q_dev = clib.tfidf_predict_device_text(vec.model, mc, text.data_ptr(), off.data_ptr(), lens.data_ptr(), len(fuzz))
    q_tok = clib.tfidf_predict_device(vec.model, mc, fuzz, threads=2, tokenizer="device")
    q_host = clib.tfidf_predict_device(vec.model, mc, fuzz, threads=2)
    with clib.freeing(q_dev, q_tok, q_host):
        a, b, c = clib.queries_download(q_dev), clib.queries_download(q_tok), clib.queries_download(q_host)
    _same(a, c, name + " weighted X")
    _same(b, c, name + " weighted X from a host corpus")
    # text -> labels
    D = vec.nr_features
    mdirs = []
    for i, seed in enumerate((61, 62)):
        mdirs.append(str(tmp_path / f"x{i}"))
        xrl_synth.make_model(mdirs[-1], D, 300, [60, 30, 12], seed=seed, shape=[5, 30, 300])
    ms = [XLinearModel.load(d) for d in mdirs]
    for models in (ms[0], ms):
        h = predict_text(vec, models, corpus, beam_size=5, only_topk=6, tokenizer="host")
        d = predict_text(vec, models, corpus, beam_size=5, only_topk=6, tokenizer="device")
        assert np.array_equal(h.indptr, d.indptr) and np.array_equal(h.indices, d.indices) and np.array_equal(h.data.view(np.uint32), d.data.view(np.uint32))
    torch.cuda.synchronize()


def test_predict_text_from_torch(xmodel, tmp_path):
    import xrl_synth
    from pecos_amd import XLinearModel
    from pecos_amd.distributed import rows_to_csr
    from pecos_amd.features import predict_text, predict_text_from_torch
    folder, corpus = _golden("word_default")
    vec = _load(folder)
    mdir = str(tmp_path / "x")
    xrl_synth.make_model(mdir, vec.nr_features, 300, [60, 30, 12], seed=63, shape=[5, 30, 300])
    m = XLinearModel.load(mdir)
    text, off, lens = _tensors([c.encode("utf-8") for c in corpus])
    idx, sc, cnt = predict_text_from_torch(vec, m, text, off, lens, beam_size=5, only_topk=6)
    got = rows_to_csr(idx.cpu().numpy().view(np.uint32), sc.cpu().numpy(), cnt.cpu().numpy(), m.nr_pred_cols)
    want = predict_text(vec, m, corpus, beam_size=5, only_topk=6)
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices) and np.array_equal(got.data.view(np.uint32), want.data.view(np.uint32))


def test_table_memory(xmodel, tmp_path):
    import torch
    from pecos_amd import clib
    # a vocabulary of 200 k tokens: the short-token table alone is 8 MiB
    vocab = [(i, b"w%d" % i) for i in range(200000)]
    feats = [(i, 1.0, (i * 1000,)) for i in range(200)]
    folder = tc.write_base(str(tmp_path / "m"), 10, vocab, feats)
    docs = [b"w0 w1000 w5 w1000", b"w199000"]
    vec = _load(folder)
    assert clib.tfidf_device_bytes(vec.model, 0) == 0
    _check(vec, xmodel, docs)
    size = clib.tfidf_device_bytes(vec.model, 0)
    assert size >= 8 << 20
    for _ in range(3):
        _check(vec, xmodel, docs)
        assert clib.tfidf_device_bytes(vec.model, 0) == size            # no new table memory
    assert clib.tfidf_device_bytes(vec.model, 1) == 0
    # destruct frees the tables: four more handles leave the device's free memory where it was (a leak would take four tables' worth)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(4):
        v = _load(folder)
        _check(v, xmodel, docs)
        clib.tfidf_destruct(v.model); v.model = None
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 2 * size
