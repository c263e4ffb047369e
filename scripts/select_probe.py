#!/usr/bin/env python3
"""Selected outputs: the host route (m.predict(X, selected_outputs_csr=S): pattern walk on one host thread, three uploads and one
synchronisation per layer, K4) against the device form (xrl_predict_selected_device: K7 plans the walk, K4 scores it, everything resident),
on a bench workload's model, for patterns equal to the model's own top-k.

    timeout 900 python scripts/select_probe.py --config eurlex-4k [--rows 100000] [--topk 10,100] [--cache /tmp/xrl_bench] [--out FILE.md]

One process.  Per pattern: 2 warm-ups, the median of 5 for both routes, every timed device output compared bit for bit (labels, order, score
bits) with the host route's, and the device route's per-kernel split from the profile (a separate, untimed call)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as smat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def workload(name, cache):
    import xrl_synth
    folder = os.path.join(cache, f"{name}_1.0")
    if not os.path.exists(os.path.join(folder, ".done")):
        os.makedirs(folder, exist_ok=True)
        ks, X, cfg = xrl_synth.make_config(name, folder, scale=1.0)
        smat.save_npz(os.path.join(folder, "X.npz"), X, compressed=False)
        json.dump({"ks": ks, "cfg": cfg}, open(os.path.join(folder, "meta.json"), "w"))
        open(os.path.join(folder, ".done"), "w").write("ok")
    X = smat.load_npz(os.path.join(folder, "X.npz")).tocsr().astype(np.float32)
    X.sort_indices()
    return folder, X


def median_ms(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="eurlex-4k")
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--topk", default="10,100")
    ap.add_argument("--cache", default=os.environ.get("XRL_BENCH_CACHE", "/tmp/xrl_bench"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pecos_amd import XLinearModel, clib
    folder, X = workload(a.config, a.cache)
    pick = np.arange(a.rows) % X.shape[0]
    X = X[pick].tocsr(); X.sort_indices()
    m = XLinearModel.load(folder)
    h = m.model.model_chain
    depth = clib.xlinear_get_int_attr(h, "depth")
    q = clib.queries_upload(h, X)
    lines = [f"## {a.config}: {a.rows} rows, depth {depth}, {m.nr_pred_cols} labels", "",
             "| pattern | host route ms (median of 5) | device form ms (median of 5) | ratio | device split (ms) |", "|---|---|---|---|---|"]
    try:
        for k in [int(v) for v in a.topk.split(",")]:
            k = min(k, 1024, m.nr_pred_cols)
            idx = torch.zeros((a.rows, k), dtype=torch.int32, device="cuda"); val = torch.zeros((a.rows, k), dtype=torch.float32, device="cuda")
            cnt = torch.zeros((a.rows,), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            clib.predict_device(h, q, max(k, 10), None, k, idx.data_ptr(), val.data_ptr(), cnt.data_ptr(), k)
            hi, hc = idx.cpu().numpy().view(np.uint32), cnt.cpu().numpy().astype(np.int64)
            mask = np.arange(k)[None, :] < hc[:, None]
            S = smat.csr_matrix((np.ones(int(mask.sum()), np.float32), hi[mask].astype(np.int64), np.concatenate([[0], np.cumsum(hc)])),
                                shape=(a.rows, m.nr_pred_cols))
            S.sort_indices()
            host = {}
            host_ms, _ = median_ms(lambda: host.__setitem__("P", m.predict(X, selected_outputs_csr=S)))
            o = (torch.zeros_like(idx), torch.zeros_like(val), torch.zeros_like(cnt))
            torch.cuda.synchronize()

            def dev():
                clib.predict_selected_device(h, q, None, idx.data_ptr(), cnt.data_ptr(), k, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), k)
            dev_ms, _ = median_ms(dev)
            P = host["P"]
            oi, ov, oc = o[0].cpu().numpy().view(np.uint32), o[1].cpu().numpy(), o[2].cpu().numpy().astype(np.int64)
            same = (np.array_equal(np.concatenate([[0], np.cumsum(oc)]), P.indptr) and np.array_equal(oi[mask], P.indices.astype(np.uint32))
                    and np.array_equal(ov[mask].view(np.uint32), P.data.astype(np.float32).view(np.uint32)))
            if not same:
                raise SystemExit(f"top-{k}: the device form's output differs from the host route's")
            clib.profile_enable(h, True); clib.profile_reset(h)
            dev()
            prof = clib.profile_get(h)
            clib.profile_reset(h); clib.profile_enable(h, False)
            split = ", ".join(f"{p['name']}[{p['layer']}] {p['ms']:.3f}" for p in prof)
            lines.append(f"| own top-{k} ({int(mask.sum())} pairs) | {host_ms:.2f} | {dev_ms:.3f} | {host_ms / dev_ms:.1f}x | {split} |")
            print(lines[-1], flush=True)
    finally:
        clib.queries_free(q)
    text = "\n".join(lines) + "\n\nEvery timed device output equals the host route's bit for bit (labels, order, score bits).\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
