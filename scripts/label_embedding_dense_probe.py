#!/usr/bin/env python3
"""Label embeddings over dense features on the device (K12D) at synthetic shapes, Y (samples x labels, 5 labels per sample, label
popularity ~ 1 / (rank + 10) with the ranks dealt to the ids at random: long-tailed label rows anywhere), X (samples x 768, dense) -> E (labels x 768, dense):

  eurlex-like        15 449 samples,     3 956 labels
  dense-768 / 4     250 000 samples,   750 000 labels
  dense-768       1 000 000 samples, 3 000 000 labels   (device only: the host route needs minutes and 12 GB)

Timed per shape, PIFA with normalized_Y: (a) label_embedding_dense_device on a resident Y handle and a resident X, E left in HBM, at
several thresholds of the long form (xrl_debug_embed_dense_long; "never" = no row takes it); (b) where --host names the shape, the host
route: X copied back from HBM, sklearn normalize, scipy .T.tocsr(), YT.dot(X), sklearn normalize of the dense product (as the reference
does), and E copied to HBM.  Host clocks around calls that end in a device synchronise; warm-ups and the median of --reps.  The device
E is compared with the host route's in ulps (the two normalisations differ: DESIGN.md section 9).

    timeout 900 python scripts/label_embedding_dense_probe.py [--shapes eurlex,quarter,full] [--host eurlex,quarter] [--reps 3] [--out FILE.md]

One process, one GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SHAPES = {"eurlex": (15449, 3956), "quarter": (250000, 750000), "full": (1000000, 3000000)}
COLS, PER_SAMPLE = 768, 5
THRESHOLDS = (64, 256, 512, 2048, 8192, 2 ** 31)


def label_matrix(samples, labels, seed):
    import scipy.sparse as smat
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(labels) + 10.0)
    col = rng.permutation(labels)[rng.choice(labels, size=(samples, PER_SAMPLE), p=p / p.sum())].astype(np.int64)     # popular labels at any id
    m = smat.csr_matrix((samples, labels), dtype=np.float32)
    m.indptr, m.indices, m.data = np.arange(samples + 1, dtype=np.int64) * PER_SAMPLE, col.reshape(-1), np.ones(samples * PER_SAMPLE, np.float32)
    return m


def timed(fn, reps, warm):
    for _ in range(warm):
        out = fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)), float(min(t)), float(max(t))], out


def measure(args):
    import torch
    import pecos_amd
    import dense_embedding_rule as der
    from pecos_amd import DeviceMatrix, clib
    assert clib.device_count() >= 1, "no GPU: nothing is measured"
    res = dict(build=clib.clib_float32.xrl_version().decode(), device=torch.cuda.get_device_name(0), reps=args.reps, warm=args.warm, shapes={})
    for name in args.shapes.split(","):
        samples, labels = SHAPES[name]
        Y = label_matrix(samples, labels, seed=len(name))
        lens = np.bincount(Y.indices, minlength=labels)
        row = dict(samples=samples, labels=labels, cols=COLS, nnz_Y=int(Y.nnz), longest_row=int(lens.max()), rows_512_and_more=int((lens >= 512).sum()))
        print(name, row, flush=True)
        y = DeviceMatrix.upload(Y)
        X = torch.randn((samples, COLS), dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
        E = torch.empty((labels, COLS), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        row["device_ms"] = {}
        for t in THRESHOLDS:
            clib.debug_embed_dense_long(t)
            row["device_ms"][str(t)], _ = timed(lambda: pecos_amd.label_embedding_dense_device(y, X, out=E), args.reps, args.warm)
            print(" long form from", t, "entries:", row["device_ms"][str(t)], flush=True)
        clib.debug_embed_dense_long(0)
        pecos_amd.label_embedding_dense_device(y, X, out=E)
        if name in args.host.split(","):
            from sklearn.preprocessing import normalize

            def host_route():
                Xh = X.cpu().numpy()
                P = np.ascontiguousarray(normalize(Y, axis=1, norm="l2").T.tocsr().dot(Xh))
                return torch.from_numpy(normalize(P, axis=1, norm="l2", copy=False)).cuda()
            row["host_route_ms"], Eh = timed(host_route, args.reps, args.warm)
            row["max_ulp_to_host_route"] = int(der.ulps(E.cpu().numpy(), Eh.cpu().numpy()).max())
            print(" host route", row["host_route_ms"], "max ulp", row["max_ulp_to_host_route"], flush=True)
            del Eh
        res["shapes"][name] = row
        del y, X, E
    return res


def render(res):
    f = lambda m: "not measured" if m is None else f"{m[0]:.1f} ({m[1]:.1f} .. {m[2]:.1f})"      # noqa: E731
    L = ["## First timings", "",
         f"Build `{res['build']}`, device {res['device']}.  `scripts/label_embedding_dense_probe.py`: synthetic label matrices (5 labels per sample, values 1, label popularity "
         f"~ 1 / (rank + 10)) and a random dense X of 768 columns, PIFA with `normalized_Y`, Y and X resident, E left in HBM.  {res['warm']} warm-up, median (min .. max) of "
         f"{res['reps']} in milliseconds, host clock around calls that end in a device synchronise.  The host route is X copied back, sklearn `normalize`, scipy `.T.tocsr()` and "
         "`YT.dot(X)`, sklearn `normalize` of the dense product, and E copied to HBM.  No target is set: these are the first numbers for this code.", "",
         "| shape | samples x labels | longest label row / rows of 512 entries and more | " + " | ".join(f"long form from {t}" if t < 2 ** 31 else "long form never" for t in THRESHOLDS)
         + " | host route | max ulp to the host route |", "|---|---|---|" + "---|" * (len(THRESHOLDS) + 2)]
    for name, r in res["shapes"].items():
        L.append(f"| {name} | {r['samples']} x {r['labels']} | {r['longest_row']} / {r['rows_512_and_more']} | " + " | ".join(f(r["device_ms"][str(t)]) for t in THRESHOLDS)
                 + f" | {f(r.get('host_route_ms'))} | {r.get('max_ulp_to_host_route', 'not measured')} |")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="eurlex,quarter,full")
    ap.add_argument("--host", default="eurlex,quarter")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--render")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "label_embedding_dense_timings.md"))
    args = ap.parse_args()
    if args.render:
        res = json.load(open(args.render))
    else:
        res = measure(args)
        json.dump(res, open(args.out + ".json", "w"), indent=1)
    open(args.out, "w").write(render(res))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
