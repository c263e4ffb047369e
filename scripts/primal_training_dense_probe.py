"""Timings of the primal L2-loss SVC over dense features (K16D) beside the route it replaces, on the two layers of
scripts/primal_training_probe.py with a dense N x 768 X: the resident K16D call (xrl_train_layer_newton_dense_device on a tensor in HBM)
against K16 over the CSR of all rows * cols entries (xrl_train_layer_newton_device), and the host entry point
xrl_single_layer_train_newton_drm_f32 on both routes (XRL_TRAIN_DRM_CSR=1 in the environment is the route of the CSR of all entries).
Each form runs in a child process of its own under a time limit: a warm-up on a small layer, then the median of --repeat runs.  The probe
stops at the first child that fails or runs out of time; the forms' weights are compared bit for bit through a digest.

    python scripts/primal_training_dense_probe.py [--problem eurlex|amazon|both] [--labels L] [--repeat 3] [--limit SECONDS] [--out FILE.json]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as smat

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))
import primal_training_probe as pp  # noqa: E402
import primal_training_rule as pr  # noqa: E402

COLS = 768
STEPS = ("k16d_resident", "k16_csr_resident", "host_k16d", "host_csr")


def dense_layer(name, labels):
    """The layer's Y, C and M with a dense unit-norm N x 768 X in place of its sparse one."""
    X, Y, C, M = pp.problem(name, labels)
    D = np.random.RandomState(7).standard_normal((X.shape[0], COLS)).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    return D, Y, C, M


def digest(coo):
    rows, cols, vals = pr.canonical(*coo)
    return hashlib.sha256(rows.tobytes() + cols.tobytes() + np.ascontiguousarray(vals).tobytes()).hexdigest()


def step(name, labels, which, repeat):
    """A child's work: one form, timed after a warm-up -> one JSON line."""
    import torch
    from pecos_amd import DeviceMatrix, clib
    D, Y, C, M = dense_layer(name, labels)
    N = D.shape[0]
    kw = dict(threshold=pp.KW["threshold"], solver_type=pr.L2_PRIMAL, eps=pp.KW["eps"])
    if which.startswith("host"):
        if which == "host_csr":
            os.environ["XRL_TRAIN_DRM_CSR"] = "1"

        def run():
            got, err = pr.run_newton(pr.OURS, D, Y, C, M, **pp.KW)
            assert err is None, err
            return got["rows"], got["cols"], got["vals"]
    else:
        yt, ct, mt = (DeviceMatrix.upload(pr.as_stored_transpose(A)) for A in (Y, C, M))
        if which == "k16d_resident":
            Xd = torch.from_numpy(D).cuda()
            call = lambda: clib.train_layer_newton_dense_device(0, Xd.data_ptr(), N, COLS, COLS, yt.handle, ct.handle, mt.handle, **kw)      # noqa: E731
        else:
            full = smat.csr_matrix((N, COLS), dtype=np.float32)
            full.indptr, full.indices, full.data = np.arange(N + 1, dtype=np.int64) * COLS, np.tile(np.arange(COLS, dtype=np.int32), N), D.ravel()
            xh = DeviceMatrix.upload(full)
            call = lambda: clib.train_layer_device(xh.handle, yt.handle, ct.handle, mt.handle, **kw)      # noqa: E731

        def run():
            out = DeviceMatrix(call())
            torch.cuda.synchronize()
            return out

    Xw, Yw, Cw, Mw = pr.problem(200, 50, 8, 2, 5, 6, 1)
    pr.run_newton(pr.OURS, np.ascontiguousarray(Xw.toarray()), Yw, Cw, Mw, **pp.KW)                      # module load, allocator
    before = clib.debug_newton_dense_forms()
    times, out = [], None
    for _ in range(repeat):
        t = time.perf_counter()
        out = run()
        times.append(time.perf_counter() - t)
    after = clib.debug_newton_dense_forms()
    coo = out if which.startswith("host") else pr.wt_as_coo(out.download())
    r = dict(seconds=statistics.median(times), runs=times, w_nnz=int(len(coo[2])), digest=digest(coo), counters=clib.newton_counters(),
             k16d_jobs={k: after[k] - before[k] for k in ("lds_jobs", "scratch_jobs")}, N=N, d=COLS, labels=Y.shape[1], jobs=int(C.nnz))
    print("STEP " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", default="both", choices=["eurlex", "amazon", "both"])
    ap.add_argument("--labels", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--limit", type=int, default=600, help="seconds a child may run")
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=STEPS)
    a = ap.parse_args()
    if a.step:
        return step(a.problem, a.labels, a.step, a.repeat)
    results = {}
    for name in (("eurlex", "amazon") if a.problem == "both" else (a.problem,)):
        r = {}
        for which in a.steps.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--problem", name, "--labels", str(a.labels), "--repeat", str(a.repeat), "--step", which]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"{name} {which}: no result within {a.limit} s; the probe stops here")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("STEP ")]
            if p.returncode != 0 or not line:
                sys.exit(f"{name} {which}: exit status {p.returncode}; the probe stops here\n{p.stderr[-2000:]}")
            r[which] = json.loads(line[-1][5:])
            print(name, which, json.dumps(r[which]), flush=True)
            assert r[which]["digest"] == next(iter(r.values()))["digest"], f"{name}: {which} differs from the first form"
        if "k16d_resident" in r and "k16_csr_resident" in r:
            r["resident_ratio"] = r["k16_csr_resident"]["seconds"] / r["k16d_resident"]["seconds"]
        if "host_k16d" in r and "host_csr" in r:
            r["host_ratio"] = r["host_csr"]["seconds"] / r["host_k16d"]["seconds"]
        results[name] = r
        print(name, json.dumps({k: v for k, v in r.items() if k.endswith("ratio")}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(results, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
