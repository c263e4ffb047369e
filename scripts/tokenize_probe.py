#!/usr/bin/env python3
"""Texts -> X in HBM: the host tokenizer (xrl_tfidf_predict_device, threads=16: host threads count, the counts are uploaded) against the device
tokenizer (K9) with the upload of the text (xrl_tfidf_predict_device_tok, tokenizer 1) and without it (xrl_tfidf_predict_device_text on
text that is resident), in documents/s, on three corpora:

  bench     the corpus bench.py's extra.text_to_labels builds (Amazon-670K shape: 135 000 words, one unigram feature each, ~76 tokens a document)
  bigram    a Zipf corpus over 20 000 words, unigrams + the bigrams of a sample as features
  long      documents of ~3000 tokens (every one above CAP: the global form)

    timeout 900 python scripts/tokenize_probe.py [--docs 100000] [--threads 16] [--out FILE.md]

One process.  The native calls are timed on pre-packed arguments (the Python packing of the corpus is the same work for every route and is
reported apart); 2 warm-ups, the median of 5; every call ends in a stream synchronise.  Every timed output is compared bit for bit with
the host route's X (same K5 on the same counts), and the device counts once per corpus with the host counts."""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))


def median_of(fn, check, warm=2, reps=5):
    for _ in range(warm):
        check(fn())
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); h = fn(); ts.append(time.perf_counter() - t0)
        check(h)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import n4_producer_bench as N4
    import xrl_synth
    from pecos_amd import XLinearModel, clib
    from pecos_amd.features import Tfidf
    if clib.device_count() < 1:
        raise RuntimeError("tokenize_probe: no HIP device visible")
    clib.set_device(0)
    lib = clib.clib_float32
    tmp = tempfile.mkdtemp(prefix="k9probe_")
    mdir = os.path.join(tmp, "x")
    xrl_synth.make_model(mdir, 500, 800, [150, 90, 25], seed=21, shape=[4, 28, 800])
    xm = XLinearModel.load(mdir)                       # (the vectorizer calls take their device and stream from a model handle)
    mc = xm.model.model_chain
    rng = np.random.default_rng(5)

    corpora = []
    D = 135000
    X = xrl_synth.make_queries(args.docs, D, 76, seed=1)
    words = np.array([f"t{i:x}" for i in range(D)])
    tok = words[X.indices]
    corpus = [" ".join(tok[X.indptr[i]:X.indptr[i + 1]]) for i in range(args.docs)]
    corpora.append(("bench", corpus, list(words), [(i,) for i in range(D)]))
    w2 = [f"w{i:x}" for i in range(20000)]
    corpus2, ids, lens = N4.zipf_corpus(rng, w2, args.docs, 60)
    sample = ids[: min(len(ids), 400000)]
    grams = [(i,) for i in range(len(w2))] + sorted({(int(a), int(b)) for a, b in zip(sample[:-1], sample[1:])})
    corpora.append(("bigram", corpus2, w2, grams))
    corpus3, _, _ = N4.zipf_corpus(rng, w2, max(1, args.docs // 50), 3000)
    corpora.append(("long", corpus3, w2, [(i,) for i in range(len(w2))]))

    lines = ["| corpus | documents | bytes | route | ms (median of 5) | min .. max ms | M documents/s |", "|---|---|---|---|---|---|---|"]
    for name, corpus, words, grams in corpora:
        vdir = os.path.join(tmp, name)
        os.makedirs(vdir)
        N4.write_vectorizer(vdir, words, grams, rng)
        vec = Tfidf.load(vdir)
        t0 = time.perf_counter(); arr, lens, n = clib._corpus_arrays(corpus); t_pack = time.perf_counter() - t0
        lp = lens.ctypes.data_as(C.POINTER(C.c_uint64))
        buf, off, ln = clib.corpus_packed(corpus)
        text = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
        off_t = torch.from_numpy(off.view(np.int64).copy()).cuda(); len_t = torch.from_numpy(ln.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()

        def host():
            h = lib.xrl_tfidf_predict_device(vec.model, mc, arr, lp, n, args.threads); clib._check(); return h

        def dev_upload():
            h = lib.xrl_tfidf_predict_device_tok(vec.model, mc, arr, lp, n, 1, args.threads); clib._check(); return h

        def dev_resident():
            h = lib.xrl_tfidf_predict_device_text(vec.model, mc, text.data_ptr(), off_t.data_ptr(), len_t.data_ptr(), n, None); clib._check(); return h

        h0 = host()
        want = clib.queries_download(h0); clib.queries_free(h0)

        def check(h):
            got = clib.queries_download(h); clib.queries_free(h)
            assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), name
            assert np.array_equal(got.data.view(np.uint32), want.data.view(np.uint32)), name

        q = clib.tfidf_counts_device(vec.model, mc, text.data_ptr(), off_t.data_ptr(), len_t.data_ptr(), n)
        cd = clib.queries_download(q); clib.queries_free(q)
        ch = clib.tfidf_counts(vec.model, corpus, threads=args.threads)
        assert np.array_equal(cd.indptr, ch.indptr) and np.array_equal(cd.indices, ch.indices) and np.array_equal(cd.data, ch.data), name
        f0 = clib.tfidf_device_forms(vec.model)
        for route, fn in (("host tokenizer, threads=%d" % args.threads, host), ("device tokenizer + upload of the text", dev_upload),
                          ("device tokenizer, text resident", dev_resident)):
            med, lo, hi = median_of(fn, check)
            lines.append(f"| {name} | {n} | {len(buf)} | {route} | {med * 1e3:.2f} | {lo * 1e3:.2f} .. {hi * 1e3:.2f} | {n / med / 1e6:.3f} |")
            print(lines[-1], flush=True)
        f1 = clib.tfidf_device_forms(vec.model)
        calls = max(1, f1["calls"] - f0["calls"])
        lines.append(f"| {name} | | | per device call: {(f1['lds_segments'] - f0['lds_segments']) // calls} LDS-form segments, "
                     f"{(f1['global_segments'] - f0['global_segments']) // calls} global-form segments, {(f1['batches'] - f0['batches']) // calls} batches; "
                     f"tables {clib.tfidf_device_bytes(vec.model, 0)} bytes; Python packing of the corpus {t_pack * 1e3:.1f} ms (every route) | | | |")
        print(lines[-1], flush=True)
        del vec
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
