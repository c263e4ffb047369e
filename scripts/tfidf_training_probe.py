#!/usr/bin/env python3
"""First timings of TF-IDF training on the device (K15): xrl_tfidf_train_device (text resident in HBM) and xrl_tfidf_train (host
corpus: packing + upload + training) against the compiled reference's c_tfidf_train (oracle/_ref/libpecos_float32.so) at 1 and 16
threads, on the three corpora scripts/tokenize_probe.py uses:

  bench     the corpus bench.py's extra.text_to_labels builds (135 000 words, ~76 tokens a document), ngram_range (1, 1)
  bigram    a Zipf corpus over 20 000 words, ngram_range (1, 2)
  long      documents of ~3000 tokens (every one above CAP: the global form), ngram_range (1, 1)

    timeout 900 python scripts/tfidf_training_probe.py [--docs 50000] [--out FILE.md]

One process.  The native calls are timed on pre-packed arguments; ours: 1 warm-up, the median of 3; the reference: one run per thread
count (it is seconds long).  Every call ends synchronised.  The trained models are compared once per corpus: ours against the
reference's saved folder, by parsed content.  The per-pass split and the form counters are xrl_debug_tfidf_train_forms of the last
resident run."""
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
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=50000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import n4_producer_bench as N4
    import tfidf_training_rule as tr
    import xrl_synth
    from pecos_amd import clib
    from pecos_amd.core import TfidfVectorizerParam
    from pecos_amd.features import Tfidf
    if clib.device_count() < 1:
        raise RuntimeError("tfidf_training_probe: no HIP device visible")
    clib.set_device(0)
    lib = clib.clib_float32
    rng = np.random.default_rng(5)
    corpora = []
    D = 135000
    X = xrl_synth.make_queries(args.docs, D, 76, seed=1)
    words = np.array([f"t{i:x}" for i in range(D)])
    tok = words[X.indices]
    corpora.append(("bench", [" ".join(tok[X.indptr[i]:X.indptr[i + 1]]) for i in range(args.docs)], {"ngram_range": (1, 1)}))
    w2 = [f"w{i:x}" for i in range(20000)]
    corpora.append(("bigram", N4.zipf_corpus(rng, w2, args.docs, 60)[0], {"ngram_range": (1, 2)}))
    corpora.append(("long", N4.zipf_corpus(rng, w2, max(1, args.docs // 50), 3000)[0], {"ngram_range": (1, 1)}))
    ref = C.CDLL(tr.REF) if os.path.exists(tr.REF) else None

    lines = ["| corpus | documents | bytes | route | ms | min .. max ms | M documents/s |", "|---|---|---|---|---|---|---|"]
    for name, corpus, cfg in corpora:
        full = Tfidf._full_config(dict(cfg))
        arr, lens, n = clib._corpus_arrays(corpus)
        lp = lens.ctypes.data_as(C.POINTER(C.c_uint64))
        buf, off, ln = clib.corpus_packed(corpus)
        text = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
        off_t = torch.from_numpy(off.view(np.int64).copy()).cuda(); len_t = torch.from_numpy(ln.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        params = TfidfVectorizerParam.from_config(dict(full))

        def resident():
            h = lib.xrl_tfidf_train_device(0, text.data_ptr(), off_t.data_ptr(), len_t.data_ptr(), n, C.byref(params), None); clib._check(); return h

        def host_corpus():
            h = lib.xrl_tfidf_train(arr, lp, n, C.byref(params), 16); clib._check(); return h

        forms = None
        for route, fn in (("xrl_tfidf_train_device, text resident", resident), ("xrl_tfidf_train, host corpus, threads=16", host_corpus)):
            clib.tfidf_destruct(fn())
            ts = []
            for _ in range(3):
                t0 = time.perf_counter(); h = fn(); ts.append(time.perf_counter() - t0)
                if fn is resident:
                    forms = clib.tfidf_train_forms(h)
                    with tempfile.TemporaryDirectory() as d:
                        clib.tfidf_save(h, d)
                        ours_model = tr.canon_model(*tr.parse_folder(d))
                clib.tfidf_destruct(h)
            med = float(np.median(ts))
            lines.append(f"| {name} | {n} | {len(buf)} | {route} | {med * 1e3:.1f} | {min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f} | {n / med / 1e6:.3f} |")
            print(lines[-1], flush=True)
        if ref is not None:
            ref.c_tfidf_train.restype = C.c_void_p
            ref.c_tfidf_train.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64, C.c_void_p, C.c_int]
            ref.c_tfidf_save.argtypes, ref.c_tfidf_destruct.argtypes = [C.c_void_p, C.c_char_p], [C.c_void_p]
            for threads in (1, 16):
                t0 = time.perf_counter(); h = ref.c_tfidf_train(arr, lp, n, C.byref(params), threads); t = time.perf_counter() - t0
                if threads == 1:
                    with tempfile.TemporaryDirectory() as d:
                        ref.c_tfidf_save(h, d.encode())
                        assert tr.canon_model(*tr.parse_folder(d)) == ours_model, f"{name}: the trained model differs from the reference's"
                ref.c_tfidf_destruct(h)
                lines.append(f"| {name} | {n} | {len(buf)} | reference c_tfidf_train, threads={threads} (one run) | {t * 1e3:.1f} | | {n / t / 1e6:.3f} |")
                print(lines[-1], flush=True)
        lines.append(f"| {name} | | | resident run: vocabulary passes {forms['us_vocab'] / 1e3:.1f} ms, df batches {forms['us_df'] / 1e3:.1f} ms, merge + filter + order "
                     f"{forms['us_order'] / 1e3:.1f} ms; {forms['df_lds_segments']} LDS-form and {forms['df_global_segments']} global-form segments, {forms['batches']} batches, "
                     f"{forms['distinct_tokens']} distinct tokens, {forms['distinct_ngrams']} distinct n-grams, {forms['long_compares']} long-token comparisons, "
                     f"{forms['table_grows']} table reruns | | | |")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
