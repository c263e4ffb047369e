"""TEST INFRASTRUCTURE for the device tokenizer (K9, pecos_amd/csrc/xrl_tokenize.hip): the parallel token rule restated in numpy, a writer of
hand-made base-vectorizer folders, and case generators.  Each generator states what it assumes of the host's output; the CPU tests check
those assumptions against the host tokenizer itself (``clib.tfidf_counts``), the GPU tests compare the device with it.

The parallel rule (64 bytes per step, one lane per byte):
  word (token_type 10)    ``sp`` = ballot of the bytes equal to ' ' (bytes past the end count as ' '); a token starts at a non-space byte
                          whose predecessor is a space or the document start (one carry bit between steps); its ordinal = starts seen so far +
                          starts below the lane; ordinals >= token_bound are dropped; its end = the next set bit of ``sp`` at or above the
                          lane, or, when the step holds none, the first ' ' (or the end) found by walking on
  char (20, 30)           a token starts at every byte that is not 10xxxxxx and has the size its lead byte names, cut at the buffer end.
                          Equal to the host's sequential decode only where every lead byte is followed by exactly the continuation bytes it
                          names; per kept token (ordinal < token_bound) the lane checks: the byte after the character is a continuation
                          byte -> 1 (the host's next character starts there: it fails); else a byte inside the character is none -> 2 (the
                          host skips a byte that starts a character by this rule).  A continuation byte at position 0 -> 1.  The document's
                          status is that of the LOWEST position that has one.
"""
import json
import os

import numpy as np

STEP = 64
M64 = (1 << 64) - 1
CAP = 1024            # kTokCap (csrc/xrl_tokenize.h): the most tokens / n-gram positions of a segment the LDS form serves

KW = dict(ngram_range=[1, 1], max_length=-1, binary=False, use_idf=True, sublinear_tf=False, norm_p="l2", min_df_ratio=0.0, max_df_ratio=1.0,
          min_df_cnt=0, max_df_cnt=-1, add_one_idf=False, keep_frequent_feature=True, smooth_idf=True, max_feature=0)


def token_bound(tok_type, max_length, n):
    by_len = (n + 1) // 2 if tok_type == 10 else n
    return min(max_length, by_len) if max_length > 0 else by_len


def occurrence_bound(T, n_lo, n_hi):
    return sum(T - n + 1 for n in range(n_lo, n_hi + 1))


def is_big(tok_type, max_length, n_lo, max_ngram, max_n, n):
    """Whether the global form serves a document of n bytes (tok_segment_is_big)."""
    tb = token_bound(tok_type, max_length, n)
    return tb > CAP or occurrence_bound(tb, n_lo, min(max_ngram, max_n, tb)) > CAP


def _mask(bits):
    return int(np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little").view(np.uint64)[0])


def _popc(x):
    return bin(x).count("1")


def _ctz(x):
    return (x & -x).bit_length() - 1


def word_rule(doc, max_length=-1):
    """[(begin, end)] of the tokens the parallel word rule keeps."""
    a = np.frombuffer(doc, dtype=np.uint8)
    n, tb = len(doc), token_bound(10, max_length, len(doc))
    toks, count, carry = [], 0, 1
    for p0 in range(0, n, STEP):
        if count >= tb:
            break
        bits = np.ones(STEP, dtype=bool)
        chunk = a[p0:p0 + STEP]
        bits[:len(chunk)] = chunk == 0x20
        sp = _mask(bits)
        starts = ~sp & ((sp << 1) | carry) & M64
        carry = sp >> 63
        for lane in range(STEP):
            if not (starts >> lane) & 1:
                continue
            if count + _popc(starts & ((1 << lane) - 1)) >= tb:
                continue
            m = sp >> lane
            if m:
                end = p0 + lane + _ctz(m)
            else:
                end = p0 + STEP
                while end < n and doc[end] != 0x20:
                    end += 1
            toks.append((p0 + lane, end))
        count += _popc(starts)
    return toks


def char_rule(doc, max_length=-1):
    """([(begin, end)], status) of the parallel character rule."""
    a = np.frombuffer(doc, dtype=np.uint8)
    n, tb = len(doc), token_bound(20, max_length, len(doc))
    cont = (a & 0xC0) == 0x80
    toks, count, status = [], 0, 0
    for p0 in range(0, n, STEP):
        if count >= tb:
            break
        bits = np.zeros(STEP, dtype=bool)
        m = min(STEP, n - p0)
        bits[:m] = ~cont[p0:p0 + m]
        starts = _mask(bits)
        viol = {}
        for lane in range(m):
            pos = p0 + lane
            if (starts >> lane) & 1:
                if count + _popc(starts & ((1 << lane) - 1)) >= tb:
                    continue
                c = int(a[pos])
                cs = 4 if c >= 0xF0 else 3 if c >= 0xE0 else 2 if c >= 0xC0 else 1
                k = min(cs, n - pos)
                inner = all(cont[pos + i] for i in range(1, k))
                if pos + cs < n and cont[pos + cs]:
                    viol[lane] = 1
                elif not inner:
                    viol[lane] = 2
                toks.append((pos, pos + k))
            elif pos == 0:
                viol[lane] = 1
        if viol and not status:
            status = viol[min(viol)]
        count += _popc(starts)
    return toks, status


def host_word(doc, max_length=-1):
    """The host's sequential word split (pieces)."""
    pieces = [p for p in doc.split(b" ") if p]
    return pieces[:max_length] if max_length > 0 else pieces


def host_char(doc, max_length=-1):
    """The host's sequential decode: (pieces, failed).  It jumps the size the lead byte names whatever follows, cuts the last character at
    the buffer end, and looks at the byte where the next character starts BEFORE it applies the max_length cut."""
    pieces, p, n = [], 0, len(doc)
    tb = token_bound(20, max_length, n)
    while p < n:
        c = doc[p]
        if 0x80 <= c < 0xC0:
            return pieces, True
        if len(pieces) >= tb:
            break
        cs = 4 if c >= 0xF0 else 3 if c >= 0xE0 else 2 if c >= 0xC0 else 1
        pieces.append(doc[p:min(p + cs, n)])
        p += cs
    return pieces, False


# ----------------------------------------------------------------------------------------------------------------------------- model folders
def write_base(folder, tok_type, vocab, features, ngram_range=(1, 1), max_length=-1, **over):
    """One BaseVectorizer folder.  vocab: [(token index, token bytes)] in file order (a repeated token keeps the last index);
    features: [(feature id, idf, (token index, ...))] in file order (a repeated n-gram keeps the last id)."""
    os.makedirs(os.path.join(folder, "tokenizer")); os.makedirs(os.path.join(folder, "vectorizer"))
    json.dump({"token_type": tok_type}, open(os.path.join(folder, "tokenizer", "config.json"), "w"))
    with open(os.path.join(folder, "tokenizer", "vocab.txt"), "wb") as f:
        f.write(f"{len(vocab)}\n".encode())
        for idx, tok in vocab:
            f.write(f"{idx}\t".encode() + tok + b"\n")
    kw = dict(KW, ngram_range=list(ngram_range), max_length=max_length, **over)
    json.dump({"type": "tfidf", "kwargs": kw}, open(os.path.join(folder, "vectorizer", "config.json"), "w"))
    with open(os.path.join(folder, "vectorizer", "tfidf-model.txt"), "w") as f:
        f.write(f"{len(features)}\n")
        for fid, idf, toks in features:
            f.write(f"{fid} {idf!r} {len(toks)}" + "".join(f" {t}" for t in toks) + "\n")
    return folder


def write_ensemble(folder, bases, norm_p=2):
    """bases: [dict of write_base's arguments after the folder]."""
    os.makedirs(folder)
    json.dump({"type": "tfidf", "kwargs": {"norm_p": norm_p, "num_base_vect": len(bases)}}, open(os.path.join(folder, "meta.json"), "w"))
    for i, b in enumerate(bases):
        write_base(os.path.join(folder, f"{i}.base"), **b)
    return folder


def model_of_pieces(piece_lists, max_n=2):
    """(vocab, features) in which every distinct piece of the given token sequences is a token (vocab.txt cannot hold a token with a newline:
    such a piece stays unknown) and every distinct n-gram of known tokens up to max_n a feature: the term counts then tell the token
    sequences apart."""
    index = {}
    for pieces in piece_lists:
        for p in pieces:
            if b"\n" not in p and p not in index:
                index[p] = len(index)
    grams = {}
    for pieces in piece_lists:
        t = [index.get(p, -1) for p in pieces]
        for n in range(1, max_n + 1):
            for i in range(len(t) - n + 1):
                g = tuple(t[i:i + n])
                if min(g) >= 0 and g not in grams:
                    grams[g] = len(grams)
    vocab = [(i, p) for p, i in index.items()]
    features = [(f, 1.0 + 0.125 * (f % 7), g) for g, f in grams.items()]
    return vocab, features


def counts_of_pieces(pieces, vocab, features, ngram_range):
    """[(feature id, count)] ascending of a token sequence under write_base's vocab / features (the reference's get_sorted_feature)."""
    index = {}
    for i, p in vocab:
        index[p] = i
    fmap = {}
    for f, _, g in features:
        fmap[tuple(g)] = f
    t = [index.get(p, -1) for p in pieces]
    c = {}
    for n in range(ngram_range[0], min(ngram_range[1], len(t)) + 1):
        for i in range(len(t) - n + 1):
            f = fmap.get(tuple(t[i:i + n]))
            if f is not None:
                c[f] = c.get(f, 0) + 1
    return sorted(c.items())


def rows_of(csr):
    """A count CSR as [[(feature id, count)]] per row, in stored order."""
    return [list(zip(csr.indices[csr.indptr[r]:csr.indptr[r + 1]].tolist(), csr.data[csr.indptr[r]:csr.indptr[r + 1]].astype(np.int64).tolist()))
            for r in range(csr.shape[0])]


# ----------------------------------------------------------------------------------------------------------------------------- documents
WORDS = [b"a", b"bb", b"ccc", b"1234567", b"12345678", b"123456789", b"12345678X", b"x" * 65, b"y" * 300, "日本語".encode(), b"t\tb", b"z\0z"]


def word_boundary_docs():
    """Word documents whose tokens end at, start at and straddle every 64-byte step boundary of a 200-byte document; tokens of 8 and 9 bytes
    there; a 9-byte token whose first 8 bytes are another token; 65- and 300-byte tokens, known and unknown.  Precondition: only ' '
    separates (the pieces hold \\0 and \\t, never \\n -- vocab.txt could not name such a token)."""
    docs = []
    for edge in (64, 128):
        for tok in (b"a", b"12345678", b"123456789", b"12345678X", b"x" * 65, b"u" * 65):
            for shift in range(-len(tok) - 1, 2):
                begin = edge + shift
                if begin < 0:
                    continue
                fill = (b"bb " * 80)[:begin]
                if fill and fill[-1:] != b" ":
                    fill = fill[:-1] + b" "
                docs.append(fill + tok + b" ccc a")
    docs += [b"y" * 300, b"q" * 300, b"a " + b"y" * 300 + b" bb", b"x" * 65 + b" " + b"u" * 66, b"z\0z t\tb a\rb", b"12345678 123456789 12345678X 1234567"]
    return docs


def space_docs():
    return [b"", b" ", b"   ", b" " * 64, b" " * 65, b" " * 200, b" a", b"a ", b"  a  bb   ccc    ", b" " * 63 + b"a", b" " * 64 + b"a", b"a" + b" " * 63 + b"bb",
            b"a" + b" " * 64 + b"bb", b"a" + b" " * 130 + b"bb "]


LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 4097)


def length_docs(rng, words=WORDS[:6]):
    """One document of every length in LENGTHS: random words, cut (the cut may fall inside a word -- it is then another, maybe unknown, token)."""
    docs = []
    for n in LENGTHS:
        d = b" ".join(words[int(i)] for i in rng.integers(0, len(words), size=n // 2 + 2))
        docs.append(d[:n])
    return docs


CHARS = ["a", "b", "é", "ü", "日", "本", "語", "😀", "🎉", " "]


def char_docs_wellformed(rng):
    """Well-formed UTF-8 with 1-, 2-, 3- and 4-byte characters across the step boundaries; then documents cut inside their last character
    (the host takes what is left as the token).  Precondition: every lead byte is followed by exactly its continuation bytes or the end."""
    docs = []
    for lead in range(0, 5):
        s = "a" * lead + "".join(CHARS[int(i)] for i in rng.integers(0, len(CHARS), size=90))
        docs.append(s.encode())
    docs += ["é".encode() * 40, "日".encode() * 50, "😀".encode() * 40, b"a" * 63 + "😀".encode(), b"a" * 62 + "日".encode() + b"b", b""]
    docs += ["ab日".encode()[:-1], "ab😀".encode()[:-2], "é".encode()[:1], b"a" * 63 + "😀".encode()[:3], b"a" * 61 + "😀".encode()[:3]]
    return docs


def char_docs_status():
    """[(document, status the parallel rule gives, what the host does: "fails" / "differs")]."""
    e, j = "é".encode(), "日".encode()
    return [
        (b"ab" + b"\x80" + b"cd", 1, "fails"),                 # a stray continuation byte after an ASCII character
        (b"\x80abc", 1, "fails"),                              # ... at the document start
        (e + b"\xa9" + b"ab", 1, "fails"),                     # one continuation byte too many
        (b"a" * 63 + e + b"\xa9", 1, "fails"),                 # ... across a step boundary
        (b"ab" + e[:1] + b"ab" + b"ab", 2, "differs"),         # a 2-byte lead followed by ASCII: the host swallows the 'a'
        (b"a" * 63 + j[:1] + b"ab" + b"ab", 2, "differs"),     # a 3-byte lead at a step boundary followed by ASCII
        (j[:2] + b"abab", 2, "differs"),                       # a 3-byte lead with one continuation byte
    ]


def fuzz_word_corpus(rng, toks, n_docs, max_tokens, unknown=(b"unk", b"another-unknown-token")):
    pool = list(toks) + list(unknown)
    docs = []
    for _ in range(n_docs):
        k = int(rng.integers(0, max_tokens + 1))
        seps = [b" " * int(s) for s in rng.choice([1, 1, 1, 2, 5], size=k + 1)]
        words = [pool[int(i)] for i in rng.integers(0, len(pool), size=k)]
        docs.append(b"".join(s + w for s, w in zip(seps, words)) + (b" " if rng.random() < 0.2 else b""))
    return docs
