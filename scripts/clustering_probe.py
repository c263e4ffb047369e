#!/usr/bin/env python3
"""Label clustering on the device (K11) at two synthetic embedding shapes, against the compiled reference (oracle/_ref):

  eurlex-like   3 956 labels x 186 104 features, depth 6        amazon-670k-like   670 091 labels x 135 909 features, depth 13

Sparse rows of about 100 entries, generated here; SKMEANS, 20 iterations at most, no sampling.  Timed per shape: (a) the host entry point
c_run_clustering_csr_f32 (upload + run + copy back); (b) the resident form xrl_run_clustering_device on an uploaded handle; (c) the
reference at threads = 1 and at 16.  Host clocks around calls that end in a device synchronise; warm-ups and the median of --reps for
the device forms, ONE run each for the reference (it takes minutes at the larger shape; said so in the table).  The device codes are
compared with the reference's at threads = 1.

    timeout 1100 python scripts/clustering_probe.py [--shapes eurlex,amazon] [--reps 3] [--out FILE.md]
    rocprofv3 --kernel-trace -d DIR -o k11 -f csv -- python scripts/clustering_probe.py --device-only --reps 1 --warm 1 --out FILE.md   (kernel times: a run of its own)
    python scripts/clustering_probe.py --render FILE.md.json --kernel-stats TRACE.csv --out profiles/clustering.md                 (no GPU: the tables)

One process, one GPU."""
import argparse
import csv
import hashlib
import json
import os
import re
import sys
import threading
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SHAPES = {"eurlex": (3956, 186104, 6), "amazon": (670091, 135909, 13)}
CHAIN_KERNELS = ("k11_first_centre", "k11_centre", "k11_norm(", "k11_score")      # the serial fp32 chains ("k11_norm(": not k11_norm_keys / _segs)


def embedding(rows, cols, per_row, seed):
    """rows x cols CSR, per_row distinct ascending columns in every row, N(0, 1) values, rows scaled to unit length."""
    import scipy.sparse as smat
    rng = np.random.default_rng(seed)
    col = np.sort(rng.integers(0, cols - per_row, size=(rows, per_row), dtype=np.int64), axis=1) + np.arange(per_row)
    val = rng.standard_normal((rows, per_row)).astype(np.float32)
    val /= np.sqrt((val.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
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


def with_heartbeat(fn, what):
    """Runs fn() while a thread prints a line a minute: a reference run at the larger shape is silent for minutes."""
    stop = threading.Event()

    def beat():
        while not stop.wait(60):
            print(f"  ... {what} still running", flush=True)
    th = threading.Thread(target=beat, daemon=True)
    th.start()
    try:
        return fn()
    finally:
        stop.set()


def measure(args):
    import torch
    import clustering_rule as cr
    import pecos_amd
    from pecos_amd import DeviceMatrix, clib
    assert clib.device_count() >= 1, "no GPU: nothing is measured"
    have_ref = os.path.exists(cr.REF) and not args.device_only
    so = open(clib.so_path, "rb").read()
    res = dict(build=clib.clib_float32.xrl_version().decode(), so_sha256_16=hashlib.sha256(so).hexdigest()[:16], device=torch.cuda.get_device_name(0),
               reps=args.reps, warm=args.warm, per_row=args.per_row, shapes={})
    for name in args.shapes.split(","):
        rows, cols, depth = SHAPES[name]
        X = embedding(rows, cols, args.per_row, seed=len(name))
        kw = dict(algo=cr.SKMEANS, seed=0, max_iter=20)
        row = dict(rows=rows, cols=cols, depth=depth, nnz=int(X.nnz))
        print(name, row, flush=True)
        m = DeviceMatrix.upload(X)
        torch.cuda.synchronize()

        def resident():
            c = pecos_amd.run_clustering_device(m, depth, partition_algo=cr.SKMEANS, seed=0, kmeans_max_iter=20)
            torch.cuda.synchronize()
            return c
        row["resident_ms"], codes = timed(resident, args.reps, args.warm)
        forms = clib.debug_cluster_forms()
        row["forms"] = forms
        print(" resident", row["resident_ms"], forms, flush=True)
        codes = codes.cpu().numpy().view(np.uint32)
        if not args.device_only:
            row["host_entry_ms"], got = timed(lambda: cr.run_library(cr.OURS, X, depth, **kw), args.reps, args.warm)
            assert got[1] is None and np.array_equal(got[0], codes)
            print(" host entry", row["host_entry_ms"], flush=True)
        if have_ref:
            for threads in (16, 1):
                t0 = time.perf_counter()
                ref = with_heartbeat(lambda: cr.reference(X, depth, threads=threads, **kw), f"reference, {threads} threads")
                row[f"reference_t{threads}_ms"] = (time.perf_counter() - t0) * 1e3
                print(f" reference threads={threads}", row[f"reference_t{threads}_ms"], flush=True)
            row["codes_equal_reference_t1"] = bool(np.array_equal(ref, codes))
            print(" codes equal the reference's at threads = 1:", row["codes_equal_reference_t1"], flush=True)
        res["shapes"][name] = row
        del m
    return res


def per_level(stats_csv, res, runs_per_shape):
    """From a --device-only trace (runs_per_shape clusterings per shape, shapes in order): kernel time per level of the LAST run of each shape (a level
    starts at its k11_rowlen launch), and the share of the chain kernels."""
    calls = []
    for r in csv.DictReader(open(stats_csv)):
        m = re.search(r"(k11_\w+(?:<\w+>)?|rocprim\S*?::detail::\w+)", r["Kernel_Name"])
        if m:
            calls.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), m.group(1) + "("))
    calls.sort()
    starts = [i for i, c in enumerate(calls) if c[2].startswith("k11_check")]
    out, at = {}, 0
    for name, row in res["shapes"].items():
        if at + runs_per_shape > len(starts):
            break
        b = starts[at + runs_per_shape - 1]
        e = starts[at + runs_per_shape] if at + runs_per_shape < len(starts) else len(calls)
        at += runs_per_shape
        levels, chain = [], []
        for c in calls[b:e]:
            if c[2].startswith("k11_rowlen"):
                levels.append(0.0); chain.append(0.0)
            if levels:
                levels[-1] += c[1] / 1e6
                if c[2].startswith(CHAIN_KERNELS):
                    chain[-1] += c[1] / 1e6
        kernels = {}
        for c in calls[b:e]:
            kernels[c[2][:-1]] = kernels.get(c[2][:-1], 0.0) + c[1] / 1e6
        out[name] = dict(level_ms=levels, chain_ms=chain, kernels=kernels)
    return out


def render(res, stats_csv, trace_runs=2):
    f = lambda m: "not measured" if m is None else f"{m[0]:.1f} ({m[1]:.1f} .. {m[2]:.1f})"      # noqa: E731
    g = lambda v: "not measured" if v is None else f"{v:.0f}"                                     # noqa: E731
    L = ["# Label clustering on the device (K11): measured", "",
         f"Build: `{res['build']}`, libxrl_amd.so sha256 `{res['so_sha256_16']}`; device: {res['device']}.  `scripts/clustering_probe.py`: synthetic embeddings, "
         f"{res['per_row']} entries per row, SKMEANS, at most 20 iterations, no sampling.  Device forms: {res['warm']} warm-up, median (min .. max) of {res['reps']} "
         "in milliseconds, host clock around calls that end in a device synchronise.  Reference: ONE run each (no warm-up, no spread), 16 host threads available.  "
         "No target is set: these are the first numbers for this code.", "",
         "| shape | labels x features | depth | nnz | resident form | host entry point (upload + run + copy back) | reference, 1 thread | reference, 16 threads | codes == reference at 1 thread |",
         "|---|---|---|---|---|---|---|---|---|"]
    for name, r in res["shapes"].items():
        L.append(f"| {name} | {r['rows']} x {r['cols']} | {r['depth']} | {r['nnz']} | {f(r['resident_ms'])} | {f(r.get('host_entry_ms'))} | {g(r.get('reference_t1_ms'))} | "
                 f"{g(r.get('reference_t16_ms'))} | {r.get('codes_equal_reference_t1', 'not measured')} |")
    L += ["", "| shape | runs served per lane | runs served per wavefront | segmented sorts | norm order switched at level | iterations per level |", "|---|---|---|---|---|---|"]
    for name, r in res["shapes"].items():
        fm = r["forms"]
        L.append(f"| {name} | {fm['lane_runs']} | {fm['wave_runs']} | {fm['seg_sorts']} | {fm['switch_level']} | {fm['iters']} |")
    if stats_csv:
        L += ["", "## Per level (`rocprofv3 --kernel-trace`, a run of its own: resident form only; kernel time of the last run, milliseconds)", "",
              "The serial chains are `k11_first_centre`, `k11_centre`, `k11_norm` and `k11_score`; the rest is sorts, scans and the bookkeeping kernels.", "",
              "| shape | level | all kernels | serial chains | share |", "|---|---|---|---|---|"]
        for name, p in per_level(stats_csv, res, trace_runs).items():
            for d, (a, c) in enumerate(zip(p["level_ms"], p["chain_ms"])):
                L.append(f"| {name} | {d} | {a:.2f} | {c:.2f} | {100 * c / a if a else 0:.0f} % |")
            a, c = sum(p["level_ms"]), sum(p["chain_ms"])
            L.append(f"| {name} | all | {a:.2f} | {c:.2f} | {100 * c / a if a else 0:.0f} % |")
        L += ["", "Kernel time by kernel, the last run of each shape (milliseconds; rocPRIM's kernels are the segmented sorts and the scans):", ""]
        per = per_level(stats_csv, res, trace_runs)
        names = sorted({k for p in per.values() for k in p["kernels"]}, key=lambda k: -sum(p["kernels"].get(k, 0.0) for p in per.values()))
        L += ["| kernel | " + " | ".join(per) + " |", "|---|" + "---|" * len(per)]
        for k in names:
            shown = re.sub(r"rocprim\S*?::detail::", "rocprim ", k)
            L.append(f"| `{shown}` | " + " | ".join(f"{p['kernels'].get(k, 0.0):.2f}" for p in per.values()) + " |")
    else:
        L += ["", "Per-level kernel times and the share of the serial chains: not measured (no kernel trace was given)."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="eurlex,amazon")
    ap.add_argument("--per-row", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--render")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--trace-runs", type=int, default=2, help="clusterings per shape in the traced run (its warm-ups + reps)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clustering.md"))
    args = ap.parse_args()
    if args.render:
        res = json.load(open(args.render))
    else:
        res = measure(args)
        json.dump(res, open(args.out + ".json", "w"), indent=1)
    open(args.out, "w").write(render(res, args.kernel_stats, args.trace_runs))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
