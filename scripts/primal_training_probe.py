"""First timings of the primal L2-loss SVC solver on the device (K16) beside the compiled reference on the same box, on the layers of
scripts/ranker_training_probe.py: an Eurlex-like layer and a slice of an Amazon-670K-like leaf layer.  The reference (oracle/_ref) runs
first, at 1 and 16 threads; then the resident form (xrl_train_layer_newton_device over handles already in HBM) and the host entry point
(upload, train, copy back), EACH IN A CHILD PROCESS UNDER ITS OWN `timeout -k 10`, sized from the reference's time on the same slice
(nobody has measured this solver on a GPU: a job is a long serial chain, and a step that takes 30 times the reference's single thread
is ended rather than waited for).  A step that fails or is ended stops the probe: nothing more is started on the GPU.  Results are checked
against the reference (canonical COO, bit for bit).

    python scripts/primal_training_probe.py [--problem eurlex|amazon|both] [--labels L] [--limit-cap SECONDS] [--out FILE.json]

--labels keeps the first L labels of a problem (and the clusters that hold them), for a shorter run: the first labels are the frequent
ones, whose jobs list the most instances.  --limit-cap bounds a GPU step's time limit from above."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as smat

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))
import primal_training_rule as pr  # noqa: E402
from ranker_training_probe import PROBLEMS  # noqa: E402

KW = dict(threshold=0.1, eps=0.01)                       # newton_eps, the stop the reference's python passes


def problem(name, labels):
    X, Y, C, M = PROBLEMS[name]()
    if labels and labels < Y.shape[1]:
        Y = smat.csc_matrix(Y[:, :labels])
        C = smat.csc_matrix(C[:labels])
        keep = np.flatnonzero(np.diff(C.indptr) > 0)
        C, M = smat.csc_matrix(C[:, keep]), smat.csc_matrix(M[:, keep])
        for A in (Y, C, M):
            A.sort_indices()
    return X, Y, C, M


def step(name, labels, which):
    """A child's work: one GPU form, timed after a warm-up on a small layer (module load, allocator) -> one JSON line."""
    import torch
    from pecos_amd import DeviceMatrix, clib
    X, Y, C, M = problem(name, labels)
    Xw, Yw, Cw, Mw = pr.problem(200, 50, 8, 2, 5, 6, 1)
    pr.run_newton(pr.OURS, Xw, Yw, Cw, Mw, **KW)
    r = {}
    if which == "resident":
        hs = [DeviceMatrix.upload(X)] + [DeviceMatrix.upload(pr.as_stored_transpose(A)) for A in (Y, C, M)]
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = DeviceMatrix(clib.train_layer_device(*(h.handle for h in hs), threshold=KW["threshold"], solver_type=pr.L2_PRIMAL, eps=KW["eps"]))
        torch.cuda.synchronize()
        r["seconds"] = time.perf_counter() - t
        Wt = out.download()
        got = dict(zip(("rows", "cols", "vals"), pr.wt_as_coo(Wt)))
    else:
        t = time.perf_counter()
        got, err = pr.run_newton(pr.OURS, X, Y, C, M, **KW)
        r["seconds"] = time.perf_counter() - t
        assert err is None, err
    r["counters"] = clib.newton_counters()
    ref = pr.reference(X, Y, C, M, threads=16, **KW)
    r["equals_reference"] = bool(pr.same_coo(got, ref, canon=True))
    r["w_nnz"] = int(len(got["vals"]))
    print("STEP " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", default="both", choices=["eurlex", "amazon", "both"])
    ap.add_argument("--labels", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit-cap", type=int, default=900, help="the most seconds a GPU step may get, whatever the reference took")
    ap.add_argument("--step", default=None, choices=["resident", "host"])
    a = ap.parse_args()
    if a.step:
        return step(a.problem, a.labels, a.step)
    assert os.path.exists(pr.REF), "the compiled reference sizes the time limits: build oracle/_ref first"
    results = {}
    for name in (("eurlex", "amazon") if a.problem == "both" else (a.problem,)):
        X, Y, C, M = problem(name, a.labels)
        r = dict(N=X.shape[0], d=X.shape[1], labels=Y.shape[1], clusters=C.shape[1], x_nnz=int(X.nnz), y_nnz=int(Y.nnz), m_nnz=int(M.nnz))
        for threads in (16, 1):
            t = time.perf_counter()
            pr.reference(X, Y, C, M, threads=threads, **KW)
            r[f"reference_{threads}_threads_s"] = time.perf_counter() - t
        print(name, "reference", json.dumps(r), flush=True)
        limit = int(min(a.limit_cap, max(120, 30 * r["reference_1_threads_s"])))
        for which in ("resident", "host"):
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--problem", name, "--labels", str(a.labels), "--step", which]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("STEP ")]
            if p.returncode != 0 or not lines:
                r[which] = dict(failed=True, returncode=p.returncode, limit_s=limit, tail=p.stdout[-400:])
                results[name] = r
                print(name, json.dumps(r), flush=True)
                if a.out:
                    json.dump(results, open(a.out, "w"), indent=1)
                sys.exit(f"{name}: the {which} step ended with status {p.returncode} (limit {limit} s): nothing more is started on the GPU")
            r[which] = dict(json.loads(lines[-1][5:]), limit_s=limit)
        results[name] = r
        print(name, json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(results, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
