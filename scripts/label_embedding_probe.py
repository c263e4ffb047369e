#!/usr/bin/env python3
"""Label embeddings on the device (K12 + K10) at two synthetic shapes, Y (samples x labels), X (samples x features) -> E (labels x features):

  eurlex-like   15 449 samples, 3 956 labels (5 per sample), 186 104 features (240 per sample)
  amazon-670k-like   490 449 samples, 670 091 labels (5 per sample), 135 909 features (75 per sample)

Timed per shape, PIFA with normalized_Y: (a) the resident form label_embedding_device on uploaded handles, result left in HBM, and its
stages one by one (normalise Y, transpose, product, normalise E); (b) copy-back plus the host route: download Y and X from HBM, sklearn
normalize, scipy .T.tocsr(), the compiled reference's c_sparse_matmul_csr_f32 (oracle/_ref) at 1 and at 16 threads, sklearn normalize --
each part only where it exists on the machine, said so otherwise.  Host clocks around calls that end in a device synchronise; warm-ups
and the median of --reps.  The device embedding is compared with the host route's bit for bit.

    timeout 900 python scripts/label_embedding_probe.py [--shapes eurlex,amazon] [--reps 3] [--commit ID] [--out FILE.md]

One process, one GPU."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SHAPES = {"eurlex": (15449, 3956, 5, 186104, 240), "amazon": (490449, 670091, 5, 135909, 75)}   # samples, labels, labels per sample, features, features per sample


def rows_of(rows, cols, per_row, seed, ones=False):
    """rows x cols CSR, per_row distinct ascending columns in every row; values 1 or |N(0, 1)|"""
    import scipy.sparse as smat
    rng = np.random.default_rng(seed)
    col = np.sort(rng.integers(0, cols - per_row, size=(rows, per_row), dtype=np.int64), axis=1) + np.arange(per_row)
    val = np.ones((rows, per_row), np.float32) if ones else np.abs(rng.standard_normal((rows, per_row))).astype(np.float32)
    m = smat.csr_matrix((rows, cols), dtype=np.float32)
    m.indptr, m.indices, m.data = np.arange(rows + 1, dtype=np.int64) * per_row, col.reshape(-1), val.reshape(-1)
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
    import sparse_matmul_rule as smr
    from oracle import xrl_oracle
    from pecos_amd import DeviceMatrix, clib
    assert clib.device_count() >= 1, "no GPU: nothing is measured"
    try:
        from sklearn.preprocessing import normalize
    except Exception:
        normalize = None
    ref = smr.ref_lib() if xrl_oracle.ref_available() else None
    so = open(clib.so_path, "rb").read()
    res = dict(build=clib.clib_float32.xrl_version().decode(), so_sha256_16=hashlib.sha256(so).hexdigest()[:16], device=torch.cuda.get_device_name(0),
               commit=args.commit, reps=args.reps, warm=args.warm, sklearn=normalize is not None, reference=ref is not None, shapes={})
    for name in args.shapes.split(","):
        n, labels, lps, feats, fps = SHAPES[name]
        Y, X = rows_of(n, labels, lps, seed=len(name), ones=True), rows_of(n, feats, fps, seed=7 + len(name))
        row = dict(samples=n, labels=labels, features=feats, nnz_Y=int(Y.nnz), nnz_X=int(X.nnz))
        print(name, row, flush=True)
        y, x = DeviceMatrix.upload(Y), DeviceMatrix.upload(X)
        torch.cuda.synchronize()
        f0 = clib.debug_embed_forms()
        row["resident_ms"], E = timed(lambda: pecos_amd.label_embedding_device(y, x), args.reps, args.warm)
        f1 = clib.debug_embed_forms()
        row["nnz_E"] = E.info["nnz"]
        row["forms_per_call"] = {k: (f1[k] - f0[k]) // (args.reps + args.warm) for k in ("t_lds", "t_big", "n_lane", "n_wave")}
        print(" resident", row["resident_ms"], row["forms_per_call"], flush=True)
        row["normalize_Y_ms"], yn = timed(lambda: y.normalize_rows(), args.reps, args.warm)
        row["transpose_ms"], yt = timed(lambda: yn.transpose(), args.reps, args.warm)
        row["product_ms"], p = timed(lambda: yt.multiply(x, False, True), args.reps, args.warm)
        row["normalize_E_ms"], _ = timed(lambda: p.normalize_rows(), args.reps, args.warm)
        print(" stages", row["normalize_Y_ms"], row["transpose_ms"], row["product_ms"], row["normalize_E_ms"], flush=True)
        row["copy_back_ms"], (Yh, Xh) = timed(lambda: (y.download(), x.download()), args.reps, args.warm)
        if normalize is not None:
            def host_front():
                return normalize(Yh, axis=1, norm="l2").T.tocsr()
            row["host_normalize_transpose_ms"], YT = timed(host_front, args.reps, args.warm)
            if ref is not None:
                A, B = smr.from_scipy(YT), smr.from_scipy(Xh)
                for threads in (16, 1):
                    t0 = time.perf_counter()
                    P, _ = smr.native_matmul(ref, A, B, "csr", False, True, threads=threads)
                    row[f"reference_matmul_t{threads}_ms"] = (time.perf_counter() - t0) * 1e3          # ONE run each
                import scipy.sparse as smat
                Ph = smat.csr_matrix((labels, feats), dtype=np.float32)
                pl = smr.logical(P)
                Ph.indptr, Ph.indices, Ph.data = pl[0].astype(np.int64), pl[1].astype(np.int64), pl[2].copy()
                row["host_normalize_E_ms"], Eh = timed(lambda: normalize(Ph, axis=1, norm="l2"), args.reps, args.warm)
                Ed = E.download()
                row["equal_host_route"] = bool(smr.same((Ed.indptr, Ed.indices, Ed.data), (Eh.indptr, Eh.indices, Eh.data)))
                print(" host route equal:", row["equal_host_route"], flush=True)
        res["shapes"][name] = row
        del y, x, yn, yt, p, E
    return res


def render(res):
    f = lambda m: "not measured" if m is None else f"{m[0]:.1f} ({m[1]:.1f} .. {m[2]:.1f})"      # noqa: E731
    g = lambda v: "not measured" if v is None else f"{v:.0f}"                                     # noqa: E731
    L = ["# Label embeddings on the device (K12 + K10): first measurements", "",
         f"Build: `{res['build']}`, libxrl_amd.so sha256 `{res['so_sha256_16']}`, commit: {res['commit']}; device: {res['device']}.  `scripts/label_embedding_probe.py`: synthetic "
         f"label matrices (5 labels per sample, values 1) and features, PIFA with `normalized_Y`.  {res['warm']} warm-up, median (min .. max) of {res['reps']} in milliseconds, host clock "
         "around calls that end in a device synchronise; the reference's product is ONE run per thread count.  The parent commit has no such path, so no speed target is set: these are "
         "the first numbers for this code, and nobody has tuned it."
         + ("" if res["sklearn"] else "  sklearn is not on this machine: the host route was not measured.")
         + ("" if res["reference"] else "  The compiled reference is not on this machine: its product was not measured."), "",
         "| shape | samples x labels x features | nnz Y / X / E | resident `label_embedding_device` | copy-back of Y and X | host normalize + transpose | reference product, 16 threads | "
         "reference product, 1 thread | host normalize of E | device == host route |", "|---|---|---|---|---|---|---|---|---|---|"]
    for name, r in res["shapes"].items():
        L.append(f"| {name} | {r['samples']} x {r['labels']} x {r['features']} | {r['nnz_Y']} / {r['nnz_X']} / {r['nnz_E']} | {f(r['resident_ms'])} | {f(r['copy_back_ms'])} | "
                 f"{f(r.get('host_normalize_transpose_ms'))} | {g(r.get('reference_matmul_t16_ms'))} | {g(r.get('reference_matmul_t1_ms'))} | {f(r.get('host_normalize_E_ms'))} | "
                 f"{r.get('equal_host_route', 'not measured')} |")
    L += ["", "Stages of the resident form, each as a call of its own on resident operands (each ends in a synchronise and allocates its result):", "",
          "| shape | normalise Y | transpose | product (K10) | normalise E | transposed rows in LDS / big form | normalised rows per lane / per wavefront |", "|---|---|---|---|---|---|---|"]
    for name, r in res["shapes"].items():
        fm = r["forms_per_call"]
        L.append(f"| {name} | {f(r['normalize_Y_ms'])} | {f(r['transpose_ms'])} | {f(r['product_ms'])} | {f(r['normalize_E_ms'])} | {fm['t_lds']} / {fm['t_big']} | "
                 f"{fm['n_lane']} / {fm['n_wave']} |")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="eurlex,amazon")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--commit", default="not given")
    ap.add_argument("--render")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "label_embedding.md"))
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
