#!/usr/bin/env python3
"""Output constraint: what xrl_set_output_constraint costs and what a constrained predict costs, on a bench workload's model.

    timeout 1500 python scripts/constraint_probe.py --config amazon-670k [--rows 100000] [--fractions 0.001,0.01,0.1,0.5] [--cache /tmp/xrl_bench] [--out FILE.md]

One process.  Per kept fraction (a random subset of the labels): the set time of the host-list and of the device-list form (median of 5),
the constrained predict (xrl_predict_device, 2 warm-ups, median of 5) beside the unconstrained step, the route's per-kernel split from the
profile (a separate, untimed call), and every timed output compared bit for bit with this library loaded from the folder rewritten by the
reference's rule (tests/constraint_view.py), which takes the fast kernels."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))


def median_ms(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="amazon-670k")
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--fractions", default="0.001,0.01,0.1,0.5")
    ap.add_argument("--cache", default=os.environ.get("XRL_BENCH_CACHE", "/tmp/xrl_bench"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import constraint_view as cv
    from select_probe import workload
    from pecos_amd import XLinearModel, clib
    folder, X = workload(a.config, a.cache)
    pick = np.arange(a.rows) % X.shape[0]
    X = X[pick].tocsr(); X.sort_indices()
    m = XLinearModel.load(folder)
    h = m.model.model_chain
    L = m.nr_pred_cols
    k = clib.effective_topk(h, None)
    q = clib.queries_upload(h, X)

    def buffers():
        return (torch.zeros((a.rows, k), dtype=torch.int32, device="cuda"), torch.zeros((a.rows, k), dtype=torch.float32, device="cuda"),
                torch.zeros((a.rows,), dtype=torch.int32, device="cuda"))

    def predict(handle, queries, o):
        clib.predict_device(handle, queries, None, None, None, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), k)

    o = buffers()
    torch.cuda.synchronize()
    plain_ms = median_ms(lambda: predict(h, q, o))
    lines = [f"## {a.config}: {a.rows} rows, {L} labels, top-{k}; unconstrained step {plain_ms:.2f} ms", "",
             "| kept | set, host list ms | set, device list ms | constrained predict ms | x unconstrained | kept children per layer | split (ms) |",
             "|---|---|---|---|---|---|---|"]
    rng = np.random.default_rng(1)
    try:
        for frac in [float(v) for v in a.fractions.split(",")]:
            labels = np.sort(rng.choice(L, max(1, int(round(frac * L))), replace=False)).astype(np.uint32)
            d_labels = torch.from_numpy(labels.view(np.int32)).cuda()
            torch.cuda.synchronize()
            host_ms = median_ms(lambda: clib.set_output_constraint(h, labels), warm=1)
            dev_ms = median_ms(lambda: clib.set_output_constraint_device(h, d_labels.data_ptr(), labels.size), warm=1)
            kept = clib.output_constraint_info(h)[1]
            ms = median_ms(lambda: predict(h, q, o))
            clib.profile_enable(h, True); clib.profile_reset(h)
            predict(h, q, o)
            prof = clib.profile_get(h)
            clib.profile_reset(h); clib.profile_enable(h, False)
            split = ", ".join(f"{p['name']}[{p['layer']}] {p['ms']:.3f}" for p in prof)
            # the same answer from the rewritten folder through the fast kernels
            tmp = tempfile.mkdtemp(prefix="xrl_constraint_")
            try:
                pruned = cv.prune_folder(folder, os.path.join(tmp, "m"), labels)
                m2 = XLinearModel.load(pruned)
                h2 = m2.model.model_chain
                q2 = clib.queries_upload(h2, X)
                with clib.freeing(q2):
                    o2 = buffers()
                    torch.cuda.synchronize()
                    predict(h2, q2, o2)
                    cnt = o[2].cpu().numpy().astype(np.int64)
                    mask = np.arange(k)[None, :] < cnt[:, None]
                    same = (np.array_equal(cnt, o2[2].cpu().numpy()) and np.array_equal(o[0].cpu().numpy()[mask], o2[0].cpu().numpy()[mask])
                            and np.array_equal(o[1].cpu().numpy().view(np.uint32)[mask], o2[1].cpu().numpy().view(np.uint32)[mask]))
                del m2
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
            if not same:
                raise SystemExit(f"kept {frac}: the constrained output differs from the rewritten folder's")
            lines.append(f"| {frac:g} ({labels.size}) | {host_ms:.2f} | {dev_ms:.2f} | {ms:.2f} | {ms / plain_ms:.2f} | {kept} | {split} |")
            print(lines[-1], flush=True)
            clib.clear_output_constraint(h)
    finally:
        clib.queries_free(q)
    text = "\n".join(lines) + "\n\nEvery timed constrained output equals the library loaded from the rewritten folder bit for bit (labels, order, score bits, counts).\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
