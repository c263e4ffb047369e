"""First timings of PairwiseANN on the device (K18) for profiles/pairwise_ann.md: batches of 1024 pairs through the resident form and the host
entry point, against the compiled reference (oracle/_ref) at 1 and 16 searchers, on a dense 768-wide index and a sparse tf-idf-like index with a
skewed label distribution.  Prints one JSON line per index.  Each figure is the median of --reps timed calls after --warmup untimed ones; the
device calls end with their own stream synchronisation, so wall time around the call is the latency a caller sees."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as smat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def skewed_columns(n_rows, n_label, longest, rs):
    """Column lengths ~ longest / rank (Zipf), at least 1: a few long columns, many short ones."""
    lengths = np.maximum(1, (longest / np.arange(1, n_label + 1)).astype(int))
    ind = np.concatenate([rs.choice(n_rows, size=n, replace=False) for n in lengths]).astype(np.int32)
    return smat.csc_matrix((rs.rand(len(ind)).astype(np.float32), ind, np.concatenate([[0], np.cumsum(lengths)])), shape=(n_rows, n_label)), lengths


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--labels", type=int, default=2000)
    ap.add_argument("--longest", type=int, default=20000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    import test_pairwise_cpu as pc
    from pecos_amd import DeviceMatrix, clib, pairwise_predict_device
    from pecos_amd.pairwise import PairwiseANN
    rs = np.random.RandomState(0)
    Yc, lengths = skewed_columns(a.rows, a.labels, a.longest, rs)
    keys = rs.choice(a.labels, size=a.batch, p=lengths / lengths.sum()).astype(np.uint32)          # a pair's label is drawn by its frequency
    for kind, dim in (("drm", 768), ("csr", 100000)):
        if kind == "drm":
            X, Q = rs.randn(a.rows, dim).astype(np.float32), rs.randn(a.batch, dim).astype(np.float32)
        else:
            X, Q = (smat.random(n, dim, density=60.0 / dim, format="csr", dtype=np.float32, random_state=rs) for n in (a.rows, a.batch))
            X.sort_indices(), Q.sort_indices()
        model = PairwiseANN.train(X, Yc)
        s = model.searchers_create(model.PredParams(batch_size=a.batch, only_topk=a.topk), num_searcher=2048)
        dev = torch.device("cuda", 0)
        dQ = DeviceMatrix.upload(Q) if kind == "csr" else torch.from_numpy(Q).to(dev)
        dkeys = torch.from_numpy(keys.view(np.int32)).to(dev)
        clib.debug_pairwise_counters(reset=True)
        got = [m.copy() for m in model.predict(Q, keys, s)]
        c = clib.debug_pairwise_counters()
        out = dict(index=kind, rows=a.rows, labels=a.labels, feat_dim=dim, batch=a.batch, only_topk=a.topk, longest_column=int(lengths.max()),
                   pairs_by_form={f: c[f] for f in ("sorted", "stream", "replay")}, second_passes=c["second_pass"], distance_evaluations=c["dist"])
        out["device_resident_ms"] = timed(lambda: pairwise_predict_device(model, dQ, dkeys, only_topk=a.topk, searchers=s), a.warmup, a.reps)
        out["device_host_entry_ms"] = timed(lambda: model.predict(Q, keys, s), a.warmup, a.reps)
        if pc.can_witness(kind):
            ref = pc.Reference(kind, X, Yc)
            out["equal_to_reference"] = pc.same_outputs(ref.predict(Q, keys, a.topk), got)
            for threads in (1, 16):
                out["reference_%d_threads_ms" % threads] = timed(lambda: ref.predict(Q, keys, a.topk, searchers=threads), 1, 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
