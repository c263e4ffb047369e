"""First timings of ranker training on the device (K13) beside the compiled reference on the same box: the resident form
(xrl_train_layer_device over handles that are already in HBM), the host entry point (upload, train, copy back) and, where oracle/_ref is
built, the reference at 1 and 16 threads -- on an Eurlex-like layer and on a slice of an Amazon-670K-like leaf layer.  Results are
checked against the reference (canonical COO, bit for bit) where it ran.

    python scripts/ranker_training_probe.py [--problem eurlex|amazon|both] [--once] [--out FILE.json]

--once runs each problem's resident form a single time and nothing else: the run to put under a kernel trace for the per-kernel split."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as smat

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import ranker_training_rule as rr  # noqa: E402


def fast_csr(rows, cols, per_row, seed):
    """Sparse rows of about per_row distinct sorted columns with tf-idf-like positive values, unit L2 norm."""
    rs = np.random.RandomState(seed)
    idx = np.sort(rs.randint(0, cols, (rows, per_row)), axis=1)
    keep = np.ones_like(idx, dtype=bool)
    keep[:, 1:] = idx[:, 1:] != idx[:, :-1]
    val = rs.gamma(2.0, 1.0, idx.shape).astype(np.float32)
    m = smat.csr_matrix((rows, cols), dtype=np.float32)
    m.indptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    m.indices, m.data = idx[keep].astype(np.int64), val[keep]
    norm = np.sqrt(np.asarray(m.multiply(m).sum(1))).ravel()
    m.data /= np.repeat(norm, np.diff(m.indptr)).astype(np.float32)
    return m


def layer(N, d, L, K, per_row, per_inst, seed):
    """X, Y (per_inst labels per instance, power-law label frequencies), C (label l under cluster l * K // L), M = pattern of Y * C."""
    rs = np.random.RandomState(seed)
    X = fast_csr(N, d, per_row, seed + 1)
    lab = np.minimum((L * rs.power(0.6, (N, per_inst))).astype(np.int64), L - 1)
    Y = smat.csr_matrix((np.ones(N * per_inst, np.float32), (np.repeat(np.arange(N), per_inst), lab.ravel())), shape=(N, L))
    Y.sum_duplicates()
    Y.data[:] = 1
    Y = Y.tocsc()
    Y.sort_indices()
    code = (np.arange(L) * K) // L
    C = smat.csc_matrix((np.ones(L, np.float32), (np.arange(L), code)), shape=(L, K))
    M = (Y.tocsr() * C.tocsr()).tocsc().astype(np.float32)
    M.sort_indices()
    return X, Y, C, M


PROBLEMS = {
    # Eurlex-4K's leaf layer: 15 449 x 5 000 tf-idf rows, 3 956 labels, ~5 labels per instance, clusters of ~16 labels
    "eurlex": lambda: layer(15000, 5000, 3956, 256, 230, 5, 1),
    # a slice of Amazon-670K's leaf layer: 135 909 features, ~75 per row, 20 000 of the labels under 200 clusters of 100
    "amazon": lambda: layer(100000, 135909, 20000, 200, 75, 5, 2),
}
KW = dict(solver=rr.L2_DUAL, threshold=0.1, max_iter=100)


def timed(fn, repeat):
    best = None
    for _ in range(repeat):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", default="both", choices=["eurlex", "amazon", "both"])
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pecos_amd import DeviceMatrix, clib
    have_ref = os.path.exists(rr.REF) and not a.once
    results = {}
    for name in (("eurlex", "amazon") if a.problem == "both" else (a.problem,)):
        X, Y, C, M = PROBLEMS[name]()
        r = dict(N=X.shape[0], d=X.shape[1], labels=Y.shape[1], clusters=C.shape[1], x_nnz=int(X.nnz), y_nnz=int(Y.nnz), m_nnz=int(M.nnz))
        t = lambda A: smat.csr_matrix((A.data, A.indices, A.indptr), shape=(A.shape[1], A.shape[0]))      # noqa: E731  the CSC arrays as the transpose's CSR
        hs = [DeviceMatrix.upload(X)] + [DeviceMatrix.upload(t(A)) for A in (Y, C, M)]

        def resident():
            out = DeviceMatrix(clib.train_layer_device(*(h.handle for h in hs), threshold=KW["threshold"], solver_type=KW["solver"], max_iter=KW["max_iter"]))
            torch.cuda.synchronize()
            return out

        if a.once:
            resident()
            results[name] = dict(r, counters=clib.debug_train_counters())
            continue
        resident()                                                        # warm-up: module load, allocator
        wt, r["resident_s"] = timed(resident, 3)
        r["counters"] = clib.debug_train_counters()
        (got, err), r["host_entry_s"] = timed(lambda: rr.run_library(rr.OURS, X, Y, C, M, **KW), 2)
        assert err is None, err
        Wt = wt.download()
        r["w_nnz"] = int(Wt.nnz)
        assert rr.same_coo((Wt.indices.astype(np.uint64), np.repeat(np.arange(Wt.shape[0]), np.diff(Wt.indptr)).astype(np.uint64), Wt.data), got, canon=True)
        if have_ref:
            for threads in (1, 16):
                ref, r[f"reference_{threads}_threads_s"] = timed(lambda: rr.reference(X, Y, C, M, threads=threads, **KW), 1)
                assert rr.same_coo(got, ref, canon=True), f"{name}: differs from the reference at {threads} threads"
            r["equals_reference"] = True
        results[name] = r
        print(name, json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(results, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
