"""The ensemble methods on the GPU box (profiles/ensemble_methods.md): the time of every method of `features.ensemble_device` next to
`average` in ONE process, at the shape of scripts/ensemble_bench.py -- the top-k of three Eurlex-4K-shape models (seeds 0-2) over 100 000
rows, k = 10 and k = 100 -- between events on one stream, median of 5 launches after a warm-up.  `average` is timed through
xrl_ensemble_device and, with only_topk, through xrl_ensemble_methods_device; `finish` is xrl_ensemble_device's cut.

Usage: python scripts/ensemble_methods_bench.py [--rows 100000] [--out FILE.json]   (the result is printed as one JSON line)"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import xrl_synth
    from pecos_amd import XLinearModel, features

    cfg = xrl_synth.CONFIGS["eurlex-4k"]
    D, n = cfg["D"], args.rows
    tmp = tempfile.mkdtemp(prefix="ensm_")
    models = []
    for seed in range(3):
        xrl_synth.make_model(os.path.join(tmp, f"m{seed}"), D, cfg["L"], cfg["w_nnz"], seed=seed)
        models.append(XLinearModel.load(os.path.join(tmp, f"m{seed}")))
    X = xrl_synth.make_queries(n, D, cfg["x_nnz"], seed=7)
    dev = torch.device("cuda", 0)
    crow, col, val = (torch.from_numpy(X.indptr.astype(np.int64)).to(dev), torch.from_numpy(X.indices.astype(np.int32)).to(dev),
                      torch.from_numpy(X.data.astype(np.float32)).to(dev))
    res = dict(rows=n, models=3, runs=[])
    for k in (10, 100):
        outs = [features.predict_from_torch(m, crow, col, val, D, beam_size=max(cfg["beam"], k), only_topk=k) for m in models]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        for mode, topk in (("average", None), ("average", k), ("finish", k), ("rank_average", None), ("sigmoid_average", None), ("softmax_average", None),
                           ("round_robin", None), ("round_robin", k)):
            ts = []
            for rep in range(6):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(s):
                    a.record(s)
                    out = features.ensemble_device(outs, mode=mode, only_topk=topk, stream=s.cuda_stream, sync=False)
                    b.record(s)
                    s.synchronize()
                if rep:
                    ts.append(a.elapsed_time(b))
            run = dict(k=k, mode=mode, only_topk=topk, ms=round(float(np.median(ts)), 4), entries_out=int(out[2].sum().item()))
            res["runs"].append(run)
            print(run, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
