"""The device tokenizer's rule and plumbing, as far as they go without a GPU: the parallel token rule (tests/tfidf_cases.py) against the host
tokenizer, the corpus packer, the exported symbols and their refusals."""
import ctypes
import os

import numpy as np
import pytest

import tfidf_cases as tc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_rows(clib, folder, docs):
    h = clib.tfidf_load(folder)
    try:
        return tc.rows_of(clib.tfidf_counts(h, docs, threads=2))
    finally:
        clib.tfidf_destruct(h)


def _word_docs():
    rng = np.random.default_rng(11)
    return (tc.word_boundary_docs() + tc.space_docs() + tc.length_docs(rng) + tc.fuzz_word_corpus(rng, tc.WORDS, 150, 40))


@pytest.mark.parametrize("max_length", [-1, 1, 3, 33])
def test_word_rule_gives_the_host_tokens(tmp_path, max_length):
    # the rule's pieces are the sequential split's, and the host tokenizer counts exactly them: under a model in which every piece is a
    # token and every unigram / bigram of pieces a feature, the host's term counts are those of the rule's token sequence
    from pecos_amd import clib
    docs = _word_docs()
    pieces = [[d[b:e] for b, e in tc.word_rule(d, max_length)] for d in docs]
    for d, p in zip(docs, pieces):
        assert p == tc.host_word(d, max_length), d
    vocab, feats = tc.model_of_pieces([tc.host_word(d) for d in docs])
    folder = tc.write_base(str(tmp_path / "m"), 10, vocab, feats, ngram_range=(1, 2), max_length=max_length)
    want = [tc.counts_of_pieces(p, vocab, feats, (1, 2)) for p in pieces]
    assert _host_rows(clib, folder, docs) == want


@pytest.mark.parametrize("max_length", [-1, 2, 64, 65])
def test_char_rule_gives_the_host_tokens_on_wellformed_text(tmp_path, max_length):
    from pecos_amd import clib
    docs = tc.char_docs_wellformed(np.random.default_rng(12))
    pieces = []
    for d in docs:
        toks, status = tc.char_rule(d, max_length)
        assert status == 0, d
        host, failed = tc.host_char(d, max_length)
        assert not failed and [d[b:e] for b, e in toks] == host, d
        pieces.append(host)
    vocab, feats = tc.model_of_pieces(pieces, max_n=3)
    for tok_type in (20, 30):
        folder = tc.write_base(str(tmp_path / f"m{tok_type}"), tok_type, vocab, feats, ngram_range=(1, 3), max_length=max_length)
        assert _host_rows(clib, folder, docs) == [tc.counts_of_pieces(p, vocab, feats, (1, 3)) for p in pieces]


def test_char_rule_status_is_where_the_host_fails_or_diverges(tmp_path):
    from pecos_amd import clib
    cases = tc.char_docs_status()
    seqs = []
    for d, _, _ in cases:
        seqs.append([d[b:e] for b, e in tc.char_rule(d)[0]])
        seqs.append(tc.host_char(d)[0])
    vocab, feats = tc.model_of_pieces(seqs, max_n=1)
    folder = tc.write_base(str(tmp_path / "m"), 20, vocab, feats)
    h = clib.tfidf_load(folder)
    try:
        for d, status, host_does in cases:
            toks, got = tc.char_rule(d)
            assert got == status, d
            pieces, failed = tc.host_char(d)
            if host_does == "fails":
                assert failed
                with pytest.raises(RuntimeError, match="the string is not utf-8 encoded!"):
                    clib.tfidf_counts(h, [d])
            else:
                assert not failed
                host_row = tc.rows_of(clib.tfidf_counts(h, [d]))[0]
                assert host_row == tc.counts_of_pieces(pieces, vocab, feats, (1, 1))                       # the restated sequential decode is the host's
                assert host_row != tc.counts_of_pieces([d[b:e] for b, e in toks], vocab, feats, (1, 1))   # ... and the parallel rule's answer is another
        # the cut: a violation past max_length tokens is not looked at, by the rule and by the host alike
        d = b"abc" + b"\x80"
        assert tc.char_rule(d, 2) == ([(0, 1), (1, 2)], 0) and tc.host_char(d, 2) == ([b"a", b"b"], False)
        # ... but the byte where the first dropped character would start is: the host looks at it before it applies the cut
        d = b"ab" + b"\x80"
        assert tc.char_rule(d, 2)[1] == 1 and tc.host_char(d, 2)[1]
    finally:
        clib.tfidf_destruct(h)


def test_bounds_decide_the_form_from_the_length_alone():
    # a word document of T one-byte tokens is 2T - 1 bytes: unigrams only, its bound is T
    for T, big in ((tc.CAP - 1, False), (tc.CAP, False), (tc.CAP + 1, True)):
        assert tc.is_big(10, -1, 1, 1, 1, 2 * T - 1) is big
    assert tc.is_big(10, -1, 1, 2, 2, 2 * 513 - 1) is True and tc.is_big(10, -1, 1, 2, 2, 2 * 512 - 1) is False      # 2T - 1 positions
    assert tc.is_big(10, 16, 1, 2, 2, 1 << 20) is False                                                              # max_length bounds it
    assert tc.is_big(20, -1, 1, 1, 1, tc.CAP) is False and tc.is_big(20, -1, 1, 1, 1, tc.CAP + 1) is True


def test_corpus_packer_against_corpus_arrays():
    from pecos_amd import clib
    corpora = [["a b", "", "ccc"], ["é日", "ab", ""], [b"raw \xff bytes", "str", b""], [""], ["x" * 300, "y"]]
    for corpus in corpora:
        buf, off, lens = clib.corpus_packed(corpus)
        arr, lens2, n = clib._corpus_arrays(corpus)
        assert n == len(corpus) == len(off) == len(lens) and off.dtype == np.uint64 and lens.dtype == np.uint64
        assert np.array_equal(lens, lens2[:n])
        enc = [d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in corpus]
        assert buf == b"".join(enc)
        ptrs = np.ctypeslib.as_array(ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint64)), shape=(n,))
        assert np.array_equal(ptrs - ptrs[0], off)                      # the same joined buffer: the pointer table is base + offsets
        for i, e in enumerate(enc):
            assert buf[int(off[i]):int(off[i] + lens[i])] == e
    buf, off, lens = clib.corpus_packed([])
    assert buf == b"" and len(off) == 0 and len(lens) == 0 and off.dtype == np.uint64


def test_new_symbols_are_exported_and_refuse_null_arguments(tmp_path):
    from pecos_amd import clib
    lib = clib.clib_float32
    for name in ("xrl_tfidf_counts_device", "xrl_tfidf_predict_device_text", "xrl_tfidf_predict_device_tok", "xrl_tfidf_device_bytes",
                 "xrl_debug_tfidf_device_forms"):
        assert name in clib.SIGNATURES and getattr(lib, name) is not None
        assert name in open(os.path.join(REPO, "include", "xrl_abi.h")).read()

    def refused(match):
        with pytest.raises(RuntimeError, match=match):
            clib._check()

    vocab, feats = tc.model_of_pieces([[b"a"]])
    h = clib.tfidf_load(tc.write_base(str(tmp_path / "m"), 10, vocab, feats))
    try:
        word = ctypes.create_string_buffer(64)
        p = ctypes.addressof(word)                                      # a non-null address: no call below gets as far as reading it
        assert lib.xrl_tfidf_counts_device(None, p, p, p, p, 1, None, None) is None
        refused("null vectorizer handle")
        assert lib.xrl_tfidf_counts_device(h, None, p, p, p, 1, None, None) is None
        refused("null model handle")
        for args in ((None, p, p), (p, None, p), (p, p, None)):
            assert lib.xrl_tfidf_counts_device(h, p, *args, 1, None, None) is None
            refused("null text, offsets or lengths")
            assert lib.xrl_tfidf_predict_device_text(h, p, *args, 1, None) is None
            refused("null text, offsets or lengths")
        assert lib.xrl_tfidf_predict_device_text(None, p, p, p, p, 1, None) is None
        refused("null vectorizer handle")
        assert lib.xrl_tfidf_counts_device(h, p, p, p, p, 1 << 32, None, None) is None
        refused("too many documents")
        lens = (ctypes.c_uint64 * 1)(1)
        assert lib.xrl_tfidf_predict_device_tok(None, p, p, lens, 1, 1, 1) is None
        refused("null vectorizer handle")
        assert lib.xrl_tfidf_predict_device_tok(h, None, p, lens, 1, 1, 1) is None
        refused("null model handle")
        assert lib.xrl_tfidf_predict_device_tok(h, p, None, lens, 1, 1, 1) is None
        refused("null corpus")
        assert lib.xrl_tfidf_predict_device_tok(h, p, p, lens, 1, 2, 1) is None
        refused("tokenizer must be 0")
        assert lib.xrl_tfidf_device_bytes(None, 0) == 0
        refused("null vectorizer handle")
        assert clib.tfidf_device_bytes(h, 0) == 0                       # no device-tokenizer call yet: no tables
        assert clib.tfidf_device_forms(h) == dict(lds_segments=0, global_segments=0, batches=0, calls=0)
    finally:
        clib.tfidf_destruct(h)


def test_tokenizer_argument_is_checked_before_any_work():
    from pecos_amd import clib
    from pecos_amd.features import predict_text
    with pytest.raises(ValueError, match="tokenizer="):
        clib.tfidf_predict_device(None, None, ["a"], tokenizer="gpu")
    with pytest.raises(ValueError, match="tokenizer="):
        predict_text(None, [], ["a"], tokenizer="gpu")
