"""Timings of ranker training over dense features (K13D) beside the route it replaces, on the two layers of scripts/ranker_training_probe.py
with a dense N x 768 X: the resident K13D call (xrl_train_layer_dense_device on a tensor in HBM) against K13 over the CSR of all rows * cols
entries (xrl_train_layer_device; the index build on the host and the upload of 8 bytes per entry are reported separately), and the host entry
point xrl_single_layer_train_drm_f32 on both routes (XRL_TRAIN_DRM_CSR=1 in the environment is the route of the CSR of all entries).
Medians of --repeat runs after a warm-up; peak device memory of a route is the drop of hipMemGetInfo's free bytes at its lowest, polled
from a thread.  The two routes' weights are compared bit for bit.

    python scripts/ranker_training_dense_probe.py [--problem eurlex|amazon|both] [--repeat 5] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np
import scipy.sparse as smat

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))
import ranker_training_probe as rp  # noqa: E402
import ranker_training_rule as rr  # noqa: E402

COLS = 768


def dense_layer(name):
    """The layer's Y, C and M with a dense unit-norm N x 768 X in place of its sparse one."""
    X, Y, C, M = rp.PROBLEMS[name]()
    D = np.random.RandomState(7).standard_normal((X.shape[0], COLS)).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    return D, Y, C, M


def median_of(fn, repeat):
    fn()                                                                  # warm-up
    times, out = [], None
    for _ in range(repeat):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return out, statistics.median(times)


def peak_of(fn):
    """fn's result and the most device memory in use during it, above what was in use before (bytes)."""
    import torch
    free0 = torch.cuda.mem_get_info()[0]
    low, stop = [free0], threading.Event()

    def poll():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
            time.sleep(0.002)

    th = threading.Thread(target=poll)
    th.start()
    try:
        out = fn()
    finally:
        stop.set()
        th.join()
    return out, free0 - low[0]


def coo_of(Wt):
    return Wt.indices.astype(np.uint64), np.repeat(np.arange(Wt.shape[0]), np.diff(Wt.indptr)).astype(np.uint64), Wt.data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", default="both", choices=["eurlex", "amazon", "both"])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pecos_amd import DeviceMatrix, clib
    kw = dict(threshold=rp.KW["threshold"], solver_type=rp.KW["solver"], max_iter=rp.KW["max_iter"])
    results = {}
    for name in (("eurlex", "amazon") if a.problem == "both" else (a.problem,)):
        D, Y, C, M = dense_layer(name)
        N = D.shape[0]
        r = dict(N=N, d=COLS, labels=Y.shape[1], clusters=C.shape[1], y_nnz=int(Y.nnz), m_nnz=int(M.nnz))
        t = lambda A: smat.csr_matrix((A.data, A.indices, A.indptr), shape=(A.shape[1], A.shape[0]))      # noqa: E731
        yt, ct, mt = (DeviceMatrix.upload(t(A)) for A in (Y, C, M))
        torch.cuda.empty_cache()

        # ---- K13D, resident
        Xd = torch.from_numpy(D).cuda()

        def dense():
            out = DeviceMatrix(clib.train_layer_dense_device(0, Xd.data_ptr(), N, COLS, COLS, yt.handle, ct.handle, mt.handle, **kw))
            torch.cuda.synchronize()
            return out

        before = clib.debug_train_dense_forms()
        wt, r["k13d_resident_s"] = median_of(dense, a.repeat)
        after = clib.debug_train_dense_forms()
        r["k13d_forms"] = {k: after[k] - before[k] for k in ("reg_jobs", "lds_jobs")}
        r["k13d_counters"] = clib.debug_train_counters()
        _, peak = peak_of(dense)
        r["k13d_peak_bytes"] = int(peak + Xd.numel() * 4)
        got = coo_of(wt.download())
        r["w_nnz"] = int(len(got[2]))
        del wt
        print(name, "k13d", json.dumps(r), flush=True)

        # ---- the parent's route: the index arrays on the host, 8 bytes per entry up, K13 over the CSR of all entries
        t0 = time.perf_counter()
        full = smat.csr_matrix((N, COLS), dtype=np.float32)
        full.indptr, full.indices, full.data = np.arange(N + 1, dtype=np.int64) * COLS, np.tile(np.arange(COLS, dtype=np.int32), N), D.ravel()
        r["csr_index_build_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        xh = DeviceMatrix.upload(full)
        torch.cuda.synchronize()
        r["csr_upload_s"] = time.perf_counter() - t0

        def sparse():
            out = DeviceMatrix(clib.train_layer_device(xh.handle, yt.handle, ct.handle, mt.handle, **kw))
            torch.cuda.synchronize()
            return out

        wt, r["k13_csr_resident_s"] = median_of(sparse, a.repeat)
        r["k13_counters"] = clib.debug_train_counters()
        _, peak = peak_of(sparse)
        r["k13_csr_peak_bytes"] = int(peak + full.nnz * 8 + (N + 1) * 8)
        assert rr.same_coo(coo_of(wt.download()), got, canon=True), f"{name}: the two routes differ"
        del wt, xh, full
        print(name, "k13", json.dumps(r), flush=True)

        # ---- the host entry point on both routes
        for key, env in (("host_entry_k13d_s", None), ("host_entry_csr_s", "1")):
            if env:
                os.environ["XRL_TRAIN_DRM_CSR"] = env
            else:
                os.environ.pop("XRL_TRAIN_DRM_CSR", None)
            (h, err), r[key] = median_of(lambda: rr.run_library(rr.OURS, D, Y, C, M, **rp.KW), max(1, a.repeat // 2))
            assert err is None, err
            assert rr.same_coo(h, got, canon=True), f"{name}: {key} differs from the resident form"
        os.environ.pop("XRL_TRAIN_DRM_CSR", None)
        results[name] = r
        print(name, json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(results, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
