"""Ensemble leg of text -> labels on the GPU box (profiles/ensemble_device.md): documents/s of `features.predict_text` on THREE models, and
where the time goes.

Workload: synthetic documents over the unigram vectorizer bench.py's text_to_labels writes (one word per feature), three Eurlex-4K-shape
models (xrl_synth.CONFIGS["eurlex-4k"], seeds 0..2), beam 10, top-10.  The end-to-end number uses only the public `predict_text`, so the
script also runs on a tree that predates the device merge (it passes `ensemble=` only where the argument exists).  Where
`features.ensemble_device` exists it adds the stage times of both paths (tokenise, upload + weighting, the three beam searches, merge,
D2H + CSR), and K6 alone between two events for (M, k) = (3, 10) and (3, 100) beside ONE model's xrl_predict_device on the same rows.

Usage: python scripts/ensemble_bench.py [--docs 100000] [--out FILE.json]   (the result is printed as one JSON line; --out also saves it)"""
import argparse
import inspect
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))


def med(f, n=5):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import n4_producer_bench as N4
    import xrl_synth
    from pecos_amd import XLinearModel, clib, features
    from pecos_amd.distributed import rows_to_csr

    cfg = xrl_synth.CONFIGS["eurlex-4k"]
    D, n = cfg["D"], args.docs
    tmp = tempfile.mkdtemp(prefix="ensb_")
    models = []
    for seed in range(3):
        xrl_synth.make_model(os.path.join(tmp, f"m{seed}"), D, cfg["L"], cfg["w_nnz"], seed=seed)
        models.append(XLinearModel.load(os.path.join(tmp, f"m{seed}")))
    X = xrl_synth.make_queries(n, D, cfg["x_nnz"], seed=7)
    words = np.array([f"t{i:x}" for i in range(D)])
    tok = words[X.indices]
    corpus = [" ".join(tok[X.indptr[i]:X.indptr[i + 1]]) for i in range(n)]
    rng = np.random.default_rng(5)
    N4.write_vectorizer(os.path.join(tmp, "vec"), list(words), [(i,) for i in range(D)], rng)
    vec = features.Tfidf.load(os.path.join(tmp, "vec"))
    kw = dict(beam_size=cfg["beam"], only_topk=10)
    has_arg = "ensemble" in inspect.signature(features.predict_text).parameters
    res = dict(docs=n, tokens_per_doc=round(X.nnz / n, 1), models=3, only_topk=10, has_ensemble_argument=has_arg)

    def e2e(**extra):
        features.predict_text(vec, models, corpus[:4096], **kw, **extra)                     # warm-up
        t, Y = med(lambda: features.predict_text(vec, models, corpus, **kw, **extra))
        return t, Y
    paths = {"default": {}}
    if has_arg:
        paths = {"device": dict(ensemble="device"), "host": dict(ensemble="host")}
    Ys = {}
    for name, extra in paths.items():
        t, Ys[name] = e2e(**extra)
        res[f"e2e_{name}"] = dict(ms=round(t * 1e3, 2), docs_per_s=round(n / t, 1))
        print(f"predict_text, 3 models, path {name}: {t * 1e3:.1f} ms = {n / t:.0f} documents/s", flush=True)
    if len(Ys) == 2:
        a, b = Ys["device"], Ys["host"]
        res["device_equals_host"] = bool(np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
                                         and np.array_equal(a.data.view(np.uint32), b.data.view(np.uint32)))
        print("device == host, bit for bit:", res["device_equals_host"], flush=True)

    # ---- stages (synchronised after each, so their sum exceeds the pipelined call a little)
    hs = [m.model.model_chain for m in models]
    st = {}
    st["tokenise_host_half"], _ = med(lambda: clib.tfidf_counts(vec.model, corpus), 3)
    def produce():
        q = vec.predict_device(models[0], corpus); clib.queries_free(q)
    st["tokenise_upload_weight"], _ = med(produce, 3)
    q = vec.predict_device(models[0], corpus)
    outs = [(torch.zeros((n, 10), dtype=torch.int32, device="cuda"), torch.zeros((n, 10), dtype=torch.float32, device="cuda"),
             torch.zeros((n,), dtype=torch.int32, device="cuda")) for _ in hs]
    torch.cuda.synchronize()
    def predicts():
        for h, (i, s, c) in zip(hs, outs):
            clib.predict_device(h, q, kw["beam_size"], None, 10, i.data_ptr(), s.data_ptr(), c.data_ptr(), 10, stream=None, sync=True)
    predicts()
    st["three_predicts"], _ = med(predicts)
    to_csr = lambda i, s, c: rows_to_csr(i.cpu().numpy().view(np.uint32), s.cpu().numpy(), c.cpu().numpy(), models[0].nr_pred_cols)   # noqa: E731
    st["host_path_three_d2h_csr"], mats = med(lambda: [to_csr(*o) for o in outs], 3)
    st["host_path_merge_scipy"], _ = med(lambda: features.ensemble_average(mats), 3)
    if hasattr(features, "ensemble_device"):
        features.ensemble_device(outs)
        def merge():
            o = features.ensemble_device(outs); torch.cuda.synchronize(); return o
        st["device_path_merge_k6"], merged = med(merge)
        st["device_path_one_d2h_csr"], _ = med(lambda: to_csr(*merged), 3)
    res["stages_ms"] = {k: round(v * 1e3, 3) for k, v in st.items()}
    print(json.dumps(res["stages_ms"], indent=1), flush=True)

    # ---- K6 alone between events, beside one model's predict on the same rows
    if hasattr(features, "ensemble_device"):
        res["k6"] = []
        for k in (10, 100):
            o3 = [(torch.zeros((n, k), dtype=torch.int32, device="cuda"), torch.zeros((n, k), dtype=torch.float32, device="cuda"),
                   torch.zeros((n,), dtype=torch.int32, device="cuda")) for _ in hs]
            s = torch.cuda.Stream()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            t_pred, t_k6 = [], []
            for rep in range(4):
                with torch.cuda.stream(s):
                    for j, (h, (i, sc, c)) in enumerate(zip(hs, o3)):
                        if j == 0:
                            ev[0].record(s)
                        clib.predict_device(h, q, max(kw["beam_size"], k), None, k, i.data_ptr(), sc.data_ptr(), c.data_ptr(), k, stream=s.cuda_stream, sync=False)
                        if j == 0:
                            ev[1].record(s)
                    ev[2].record(s)
                    out = features.ensemble_device(o3, stream=s.cuda_stream, sync=False)
                    ev[3].record(s)
                    s.synchronize()
                if rep:
                    t_pred.append(ev[0].elapsed_time(ev[1])); t_k6.append(ev[2].elapsed_time(ev[3]))
            cnt_in = sum(int(c.sum().item()) for _, _, c in o3)
            cnt_out = int(out[2].sum().item())
            moved = 8 * (cnt_in + cnt_out) + 4 * n * 4
            ms = float(np.median(t_k6))
            res["k6"].append(dict(M=3, k=k, rows=n, k6_ms=round(ms, 4), one_predict_ms=round(float(np.median(t_pred)), 4), entries_in=cnt_in,
                                  entries_out=cnt_out, bytes_moved=moved, gb_per_s=round(moved / ms / 1e6, 1)))
            print(res["k6"][-1], flush=True)
    clib.queries_free(q)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
