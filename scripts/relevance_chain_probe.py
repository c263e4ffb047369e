#!/usr/bin/env python3
"""The relevance and matching chains of cost-sensitive / user-negative training at two synthetic shapes, label matrix Y (samples x labels, 5
labels per sample), a relevance R over Y's pattern, a user-supplied matching matrix M (3 labels per sample) and a chain of nr_splits 16:

  eurlex-like        15 449 samples,   3 956 labels, 256 leaf clusters    (1 <- 16 <- 256 <- labels)
  amazon-670k-like  490 449 samples, 670 091 labels, 4 096 leaf clusters  (1 <- 16 <- 256 <- 4 096 <- labels)

Timed per shape: (a) the resident builders relevance_chain_device({0: R}, chain, norm, induce=True) per norm and
matching_chain_device({0: M}, chain) on operands that are in HBM already, results left in HBM; (b) the same chains on the host -- levels
by clib.sparse_matmul (this library's host entry point: upload, product, download per call), sklearn's normalize, scipy's sum of binarized
patterns -- followed by the uploads the training loop then needs.  Host clocks around calls that end in a device synchronise; warm-ups and
the median of --reps.  Every resident level is compared with the host route's: values bit for bit, matching levels by pattern.

    timeout 900 python scripts/relevance_chain_probe.py [--shapes eurlex,amazon] [--reps 3] [--commit ID] [--out FILE.md]

One process, one GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as smat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"eurlex": (15449, 3956, 256), "amazon": (490449, 670091, 4096)}     # samples, labels, leaf clusters
NORMS = ("l1", "l2", "max", "no-norm")


def rows_of(rows, cols, per_row, seed, ones=False):
    """rows x cols CSR, per_row distinct ascending columns in every row; values 1 or uniform in (0.1, 2)"""
    rng = np.random.default_rng(seed)
    col = np.sort(rng.integers(0, cols - per_row, size=(rows, per_row), dtype=np.int64), axis=1) + np.arange(per_row)
    val = np.ones((rows, per_row), np.float32) if ones else rng.uniform(0.1, 2.0, (rows, per_row)).astype(np.float32)
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


def same(a, b, values):
    a, b = smat.csr_matrix(a), smat.csr_matrix(b)
    a.sort_indices(); b.sort_indices()
    ok = np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    return bool(ok and (not values or np.array_equal(a.data.view(np.uint32), b.data.view(np.uint32))))


def host_relevance(clib, normalize, R, chain, norm, upload):
    levels = [R]
    for i in range(1, len(chain) + 1):
        levels.append(clib.sparse_matmul(levels[-1], chain[-i]))
    levels.reverse()
    if norm != "no-norm":
        levels = [normalize(m.tocsr(), norm=norm) for m in levels]
    return [upload(m) for m in levels[1:]], levels[1:]


def host_matching(clib, M, chain, upload):
    def binarized(A):
        A = smat.csc_matrix(A, dtype=np.float32, copy=True)
        A.data[:] = 1
        return A
    levels = [binarized(M)]
    for i in range(1, len(chain) + 1):
        levels.append(smat.csc_matrix(clib.sparse_matmul(levels[-1], chain[-i])).sorted_indices())
    levels.reverse()
    return [upload(m) for m in levels[:-1]], levels[:-1]


def measure(args):
    import torch
    from sklearn.preprocessing import normalize
    from pecos_amd import ClusterChain, DeviceMatrix, clib, matching_chain_device, relevance_chain_device
    assert clib.device_count() >= 1, "no GPU: nothing is measured"
    res = dict(build=clib.clib_float32.xrl_version().decode(), device=torch.cuda.get_device_name(0), commit=args.commit, reps=args.reps, warm=args.warm, shapes={})
    for name in args.shapes.split(","):
        n, labels, leaves = SHAPES[name]
        R = rows_of(n, labels, 5, seed=len(name))
        M = rows_of(n, labels, 3, seed=11 + len(name), ones=True)
        C = smat.csc_matrix((np.ones(labels, np.float32), (np.arange(labels), np.arange(labels) * leaves // labels)), shape=(labels, leaves))
        chain = list(ClusterChain.from_partial_chain(C, nr_splits=16))
        row = dict(samples=n, labels=labels, chain=[list(c.shape) for c in chain], nnz_R=int(R.nnz), nnz_M=int(M.nnz))
        print(name, row, flush=True)
        row["upload_ms"], (r, m, cs) = timed(lambda: (DeviceMatrix.upload(R), DeviceMatrix.upload(M), [DeviceMatrix.upload(c) for c in chain]), args.reps, args.warm)
        torch.cuda.synchronize()
        for norm in NORMS:
            row[f"resident_{norm}_ms"], dev = timed(lambda: relevance_chain_device({0: r}, cs, norm, True), args.reps, args.warm)
            row[f"host_{norm}_ms"], (_, host) = timed(lambda: host_relevance(clib, normalize, R, chain, norm, DeviceMatrix.upload), args.reps, args.warm)
            row[f"equal_{norm}"] = all(same(d.download(), h, True) for d, h in zip(dev, host))
            row["nnz_levels"] = [int(d.info["nnz"]) for d in dev]
            print(" relevance", norm, row[f"resident_{norm}_ms"], row[f"host_{norm}_ms"], row[f"equal_{norm}"], flush=True)
        row["resident_matching_ms"], dev = timed(lambda: matching_chain_device({0: m}, cs), args.reps, args.warm)
        row["host_matching_ms"], (_, host) = timed(lambda: host_matching(clib, M, chain, DeviceMatrix.upload), args.reps, args.warm)
        row["equal_matching"] = all(same(d.download(), h, False) for d, h in zip(dev, host))
        print(" matching", row["resident_matching_ms"], row["host_matching_ms"], row["equal_matching"], flush=True)
        res["shapes"][name] = row
        del r, m, cs, dev
    return res


def render(res):
    f = lambda m: "not measured" if m is None else f"{m[0]:.1f} ({m[1]:.1f} .. {m[2]:.1f})"      # noqa: E731
    L = ["# Relevance and matching chains on the device (K10 + K12 + K14): first measurements", "",
         f"Build: `{res['build']}`, commit: {res['commit']}; device: {res['device']}.  `scripts/relevance_chain_probe.py`: synthetic label matrices (5 labels per sample), a "
         "relevance over their pattern, a user-supplied matching matrix of 3 labels per sample and chains of `nr_splits = 16`.  `resident`: `relevance_chain_device({0: R}, chain, "
         "norm, induce=True)` / `matching_chain_device({0: M}, chain)` on operands that are in HBM, results left there.  `host`: the same chains by `clib.sparse_matmul` per level "
         f"(upload, product and download per call), sklearn's `normalize` and scipy, then the upload of every level the training loop needs.  {res['warm']} warm-up, median (min .. "
         f"max) of {res['reps']} in milliseconds, host clock around calls that end in a device synchronise.  The parent commit has no such path, so no speed target is set: these are "
         "the first numbers for this code, and nobody has tuned it.", ""]
    for name, r in res["shapes"].items():
        L += [f"## {name}: {r['samples']} samples x {r['labels']} labels, chain {' <- '.join(str(c[1]) for c in r['chain'])} <- {r['labels']}", "",
              f"nnz R {r['nnz_R']}, nnz M {r['nnz_M']}; entries of the induced relevance levels, root side first: {r['nnz_levels']}.  Upload of R, M and the chain, once: "
              f"{f(r['upload_ms'])} (not in `resident`).", "", "| chain | resident | host + uploads | resident == host |", "|---|---|---|---|"]
        for norm in NORMS:
            L.append(f"| relevance, `{norm}` | {f(r[f'resident_{norm}_ms'])} | {f(r[f'host_{norm}_ms'])} | {r[f'equal_{norm}']} (value bits) |")
        L += [f"| matching | {f(r['resident_matching_ms'])} | {f(r['host_matching_ms'])} | {r['equal_matching']} (pattern) |", ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="eurlex,amazon")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--commit", default="not given")
    ap.add_argument("--render")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "relevance_chains.md"))
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
