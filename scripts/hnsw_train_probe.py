"""First timings of HNSW graph construction on the device (K19) at two shapes: a label-embedding-like sparse set and a dense set.

    python scripts/hnsw_train_probe.py [--out profiles/hnsw_train.md] [--small]

The parent never opens the GPU.  It makes the items, times the compiled reference's train (oracle/_ref) at 1 and at 16 threads, keeps the
folder of the single-thread run, and then runs this library's host entry point and its resident form in one child process under a time limit.
The child checks the folder it saves against the reference's single-thread folder byte for byte and reports the counters.  No timing target
exists; the numbers are written down with how they were taken."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import scipy.sparse as smat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))
import hnsw_rule as hr  # noqa: E402
from hnsw_probe import make  # noqa: E402

M, EFC = 32, 100
FILES = ("c_model/index.mmap_store", "c_model/config.json")


def shapes(small):
    if small:
        return {"sparse-embedding": ("csr", 1000, 20000), "dense-128": ("drm", 1000, 128)}
    return {"sparse-embedding": ("csr", 10000, 100000), "dense-128": ("drm", 10000, 128)}


def child(folder):
    import torch
    import pecos_amd
    from pecos_amd import clib
    kind = json.load(open(os.path.join(folder, "ref1", "param.json")))["data_type"]
    X = np.load(os.path.join(folder, "X.npy")) if kind == "drm" else smat.load_npz(os.path.join(folder, "X.npz")).tocsr()
    params = dict(M=M, efC=EFC, metric_type="ip")
    cls = pecos_amd.hnsw.HNSW
    cls.train(X[:64], params)                                          # warm-up: the code object is loaded
    out = {}
    clib.debug_hnsw_train_counters(reset=True)
    t0 = time.perf_counter()
    m = cls.train(X, params)
    out["host_s"] = time.perf_counter() - t0
    out["counters"] = clib.debug_hnsw_train_counters()
    t0 = time.perf_counter()
    m.save(os.path.join(folder, "ours"))
    out["save_s"] = time.perf_counter() - t0
    out["same_bytes"] = all(open(os.path.join(folder, "ours", f), "rb").read() == open(os.path.join(folder, "ref1", f), "rb").read() for f in FILES)
    Xd = torch.from_numpy(X).cuda() if kind == "drm" else pecos_amd.DeviceMatrix.upload(X)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cls.train_device(Xd, params)
    torch.cuda.synchronize()
    out["device_s"] = time.perf_counter() - t0
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if not hr.have_reference():
        sys.exit("oracle/_ref/libpecos_float32.so is missing: build() makes it where the reference's sources are")
    lines = ["# HNSW graph construction on the device (K19): first timings", "",
             "One MI355X; host: %d CPUs visible to the process, avx512f %s.  Written by `scripts/hnsw_train_probe.py%s`: one timed call each, `time.perf_counter` around the "
             "call, after a warm-up call on 64 rows; the reference is timed first, in the parent, which never opens the GPU; this library runs in a child process.  "
             "M = %d, efC = %d, ip.  Nobody has tuned this kernel and no timing target exists." % (
                 len(os.sched_getaffinity(0)), "yes" if hr.host_has_avx512f() else "no", " --small" if a.small else "", M, EFC), "",
             "| items | reference 1 thread | reference 16 threads | host entry point | resident form | save | bytes equal to the reference at 1 thread | dist evals: search / select / reverse | lists rewritten | sorted by rank / by replay |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, (kind, n, dim) in shapes(a.small).items():
        with tempfile.TemporaryDirectory() as d:
            X = make(kind, n, dim, 0, 7)[0]
            ref_s = {}
            for threads in (1, 16):
                t0 = time.perf_counter()
                hr.train_reference(X, os.path.join(d, "ref%d" % threads), metric="ip", M=M, efC=EFC, threads=threads)
                ref_s[threads] = time.perf_counter() - t0              # (train and save)
            if kind == "drm":
                np.save(os.path.join(d, "X.npy"), X)
            else:
                smat.save_npz(os.path.join(d, "X.npz"), X)
            limit = max(240.0, 400.0 * ref_s[1])
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", d], capture_output=True, text=True, timeout=limit)
                got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                r = json.loads(got[-1][7:]) if got else {"error": "exit %d: %s" % (p.returncode, p.stderr[-300:])}
            except subprocess.TimeoutExpired:
                r = {"error": "time limit of %.0f s" % limit}
            head = "| %s: %d x %d, %s | %.2f s | %.2f s |" % (name, n, dim, kind, ref_s[1], ref_s[16])
            if "error" in r:
                lines.append(head + " failed: %s | - | - | - | - | - | - |" % r["error"])
                break                                                  # nothing more is started on the GPU after a failure
            c = r["counters"]
            lines.append(head + " %.2f s | %.2f s | %.2f s | %s | %d / %d / %d | %d | %d / %d |" % (
                r["host_s"], r["device_s"], r["save_s"], r["same_bytes"], c["dist_search"], c["dist_select"], c["dist_reverse"], c["rewritten"], c["sort_rank"], c["sort_replay"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
