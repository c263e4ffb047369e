#!/usr/bin/env python3
"""Sparse products on the device (K10, xrl_sparse_matmul_device) at the two serving shapes, against what they replace:

  descent   a rows x beam result over the clusters of a leaf layer (Amazon-670K: 65 536 clusters, 670 091 labels) times C^T
  roll-up   a rows x topk result over the labels times the leaf C (one stored entry per label)

Each is timed (a) on the device form: result triple and the other operand resident, the product left in HBM; (b) as the copy back of the
result followed by the compiled reference's c_sparse_matmul_csr_f32 on 16 host threads (oracle/_ref); (c) through this library's host
entry point c_sparse_matmul_csr_f32 (upload, product, copy back).  Host clocks around calls that end in a device synchronise; 2
warm-ups, the median of 5.  The device product is compared bit for bit with the reference's on all rows.

    timeout 900 python scripts/sparse_matmul_probe.py [--rows 490000] [--beam 10] [--out FILE.md]
    rocprofv3 --kernel-trace -d DIR -o k10 -f csv -- python scripts/sparse_matmul_probe.py --device-only --reps 3 --out FILE.md     (kernel times: a run of its own)
    python scripts/sparse_matmul_probe.py --render FILE.md.json --kernel-stats TRACE.csv --out profiles/sparse_matmul.md       (no GPU: the table)

One process, one GPU."""
import argparse
import csv
import ctypes as C
import hashlib
import json
import os
import re
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

LABELS, CLUSTERS = 670091, 65536


def synthetic(rows, stride, n_cols, seed):
    """Rows best first, distinct ids per row."""
    rng = np.random.default_rng(seed)
    step = rng.integers(1, max(2, n_cols // stride), size=(rows, stride), dtype=np.int64)
    ids = (rng.integers(0, n_cols, size=(rows, 1), dtype=np.int64) + np.cumsum(step, axis=1)) % n_cols
    val = -np.sort(-rng.random((rows, stride)).astype(np.float32), axis=1)
    return ids.astype(np.int32), val, np.full(rows, stride, dtype=np.int32)


def leaf_c():
    """labels x clusters, label l under cluster l * CLUSTERS // LABELS (contiguous ranges of 10 or 11), values 1"""
    import scipy.sparse as smat
    lab = np.arange(LABELS, dtype=np.int64)
    return smat.csr_matrix((np.ones(LABELS, np.float32), (lab * CLUSTERS // LABELS), np.arange(LABELS + 1, dtype=np.int64)), shape=(LABELS, CLUSTERS))


def median_ms(fn, reps, warm=2):
    for _ in range(warm):
        out = fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t)), out


def measure(args):
    import torch
    import sparse_matmul_rule as R
    from oracle import xrl_oracle
    from pecos_amd import clib
    from pecos_amd.features import DeviceMatrix
    assert clib.device_count() >= 1, "no GPU: nothing is measured"
    raw = C.CDLL(clib.so_path)
    ref = R.ref_lib() if xrl_oracle.ref_available() and not args.device_only else None
    Cl = leaf_c()
    Ct = Cl.T.tocsr()
    Ct.sort_indices()
    shapes = {"descent": (CLUSTERS, args.beam, Ct, 5), "roll-up": (LABELS, args.topk, Cl, 6)}
    so = open(clib.so_path, "rb").read()
    res = dict(build=clib.clib_float32.xrl_version().decode(), so_sha256_16=hashlib.sha256(so).hexdigest()[:16], device=torch.cuda.get_device_name(0),
               rows=args.rows, reps=args.reps, shapes={})
    for name, (n_cols, stride, Bm, seed) in shapes.items():
        idx, val, cnt = synthetic(args.rows, stride, n_cols, seed)
        t = tuple(torch.from_numpy(a).cuda() for a in (idx, val, cnt))
        Bd = DeviceMatrix.upload(Bm)
        torch.cuda.synchronize()

        def device_form():
            return DeviceMatrix.from_result(t, n_cols).multiply(Bd)
        before = clib.debug_spgemm_forms()
        dev_ms = median_ms(device_form, args.reps)
        after = clib.debug_spgemm_forms()
        Z = dev_ms[3]
        info = Z.info
        row = dict(left=f"{args.rows} x {n_cols}, {stride} per row", right=f"{Bm.shape[0]} x {Bm.shape[1]}, nnz {Bm.nnz}", products=None, nnz=info["nnz"],
                   device_ms=dev_ms[:3], big_rows=after["big_rows"] - before["big_rows"])
        Br = R.from_scipy(Bm)
        row["products"] = int(np.diff(Bm.indptr)[idx.ravel()].sum())
        if not args.device_only:
            def host_copy():
                i, v, n = (x.cpu().numpy() for x in t)
                return R.csr(np.arange(args.rows + 1, dtype=np.uint64) * stride, i.reshape(-1).view(np.uint32), v.reshape(-1), (args.rows, n_cols))

            def ours_host():
                return R.native_matmul(raw, host_copy(), Br, "csr", False, True, 16)[0]
            row["host_entry_ms"] = median_ms(ours_host, args.reps)[:3]
            if ref is not None:
                def reference():
                    return R.native_matmul(ref, host_copy(), Br, "csr", False, True, 16)[0]
                r = median_ms(reference, args.reps)
                row["reference_ms"] = r[:3]
                got = Z.download()
                row["bit_equal_to_reference"] = bool(R.same((got.indptr, got.indices, got.data), R.logical(r[3])))
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        del Z, dev_ms, Bd
    return res


def render(res, stats_csv):
    L = ["# Sparse matrix products on the device (K10): measured", "",
         f"Build: `{res['build']}`, libxrl_amd.so sha256 `{res['so_sha256_16']}`; device: {res['device']}.  `scripts/sparse_matmul_probe.py`, {res['rows']} rows, "
         f"2 warm-ups, median (min .. max) of {res['reps']} in milliseconds; host clock around calls that end in a device synchronise.", "",
         "| shape | left | right | products | nnz of the product | device form | copy back + reference, 16 threads | this library's host entry point | big-form rows |",
         "|---|---|---|---|---|---|---|---|---|"]
    f = lambda m: "not measured" if m is None else f"{m[0]:.1f} ({m[1]:.1f} .. {m[2]:.1f})"      # noqa: E731
    for name, r in res["shapes"].items():
        L.append(f"| {name} | {r['left']} | {r['right']} | {r['products']} | {r['nnz']} | {f(r['device_ms'])} | {f(r.get('reference_ms'))} | {f(r.get('host_entry_ms'))} | {r['big_rows']} |")
    L += ["", "Device form: `xrl_smat_from_device_result` of the resident result + `xrl_sparse_matmul_device` against the resident right operand; the product stays in HBM.  "
          "Reference: the result triple copied to the host, then the compiled reference's `c_sparse_matmul_csr_f32`.  Host entry point: the same host arrays "
          "through this library's `c_sparse_matmul_csr_f32` (upload, product, copy back)."]
    eq = {n: r.get("bit_equal_to_reference") for n, r in res["shapes"].items()}
    L += ["", f"Device product bit-equal to the reference's on all rows: {eq}."]
    if stats_csv:
        # the trace of a --device-only run: per kernel the calls in time order, the first half the descent's, the second the roll-up's
        per = {}
        for r in csv.DictReader(open(stats_csv)):
            m = re.search(r"(k10_\w+(?:<\w+>)?|rocprim\S*?::detail::\w+)", r["Kernel_Name"])
            if m:
                per.setdefault(re.sub(r"rocprim\S*?::detail::", "rocprim ", m.group(1)), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
        L += ["", "## Per kernel (`rocprofv3 --kernel-trace`, a run of its own: device form only, 2 warm-up + 3 timed products per shape; average microseconds per product)", "",
              "| kernel | launches per product | descent | roll-up |", "|---|---|---|---|"]
        tot = [0.0, 0.0]
        for name, calls in sorted(per.items(), key=lambda kv: -sum(c[1] for c in kv[1])):
            calls.sort()
            half = len(calls) // 2
            a, b = (sum(c[1] for c in part) / 5e3 for part in (calls[:half], calls[half:]))
            tot[0] += a; tot[1] += b
            L.append(f"| `{name}` | {half // 5} | {a:.1f} | {b:.1f} |")
        L.append(f"| all kernels | | {tot[0]:.1f} | {tot[1]:.1f} |")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=490000)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--render")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sparse_matmul.md"))
    args = ap.parse_args()
    if args.render:
        res = json.load(open(args.render))
    else:
        res = measure(args)
        json.dump(res, open(args.out + ".json", "w"), indent=1)
    open(args.out, "w").write(render(res, args.kernel_stats))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
