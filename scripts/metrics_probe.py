#!/usr/bin/env python3
"""Metrics at k: the device call (xrl_metrics_device, K8: result and true labels resident, 2 x topk numbers come back) against what it replaces
-- the copy back of the result triple followed by the numpy restatement of smat_util.Metrics.generate (tests/metrics_cases.py), and the
reference's own python loop where oracle/_ref/refpy is built (--reference: one run, it takes tens of seconds) -- on a synthetic result of
the Amazon-670K shape.

    timeout 900 python scripts/metrics_probe.py [--rows 490000] [--stride 10] [--topk 10] [--labels 670091] [--reference] [--out FILE.md]

One process.  2 warm-ups, the median of 5 for every route; every timed device output is compared bit for bit (integers and fp64 sums) with the
restatement of all rows, and a 10 000-row prefix (a call of its own, by row count) with the restatement of that prefix."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def synthetic(rows, stride, labels, seed=3):
    """Rows best first with ties (scores in hundredths), distinct labels per row, 1-7 true labels per row, about half of them predicted."""
    rng = np.random.default_rng(seed)
    step = rng.integers(1, max(2, labels // stride), size=(rows, stride), dtype=np.int64)
    lab = (rng.integers(0, labels, size=(rows, 1), dtype=np.int64) + np.cumsum(step, axis=1)) % labels      # distinct: the steps sum to < labels
    idx = rng.permuted(lab, axis=1).astype(np.uint32)
    val = -np.sort(-np.round(rng.random((rows, stride)), 2).astype(np.float32), axis=1)
    cnt = np.full(rows, stride, dtype=np.uint32)
    cnt[rng.random(rows) < 0.01] = 0
    n_true = rng.integers(1, 8, size=rows)
    tptr = np.concatenate([[0], np.cumsum(n_true)]).astype(np.uint64)
    row = np.repeat(np.arange(rows), n_true)
    pos = np.arange(int(tptr[-1])) - np.repeat(tptr[:-1].astype(np.int64), n_true)
    own = idx[row, (pos * 3) % stride].astype(np.int64)
    t = np.where(pos % 2 == 0, own, rng.integers(0, labels, size=len(row)))
    order = np.lexsort((t, row))                                         # ascending inside rows (a label drawn twice stays twice)
    return dict(idx=idx, val=val, cnt=cnt, tptr=tptr, tidx=t[order].astype(np.uint32), topk=0, n_cols=labels)


def median_ms(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=490000)
    ap.add_argument("--stride", type=int, default=10)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--labels", type=int, default=670091)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import metrics_cases as mc
    from pecos_amd import clib
    if clib.device_count() < 1:
        raise SystemExit("metrics_probe: no HIP device visible; nothing is measured without one")
    c = synthetic(a.rows, a.stride, a.labels)
    c["topk"] = a.topk
    want = mc.metric_sums(c)
    prefix = min(10000, a.rows)
    p = dict(c, idx=c["idx"][:prefix], val=c["val"][:prefix], cnt=c["cnt"][:prefix], tptr=c["tptr"][:prefix + 1])
    want_prefix = mc.metric_sums(p)
    dev = torch.device("cuda", 0)
    idx, val, cnt = (torch.from_numpy(x).to(dev) for x in (c["idx"].view(np.int32), c["val"], c["cnt"].view(np.int32)))
    tptr, tidx = torch.from_numpy(c["tptr"].view(np.int64)).to(dev), torch.from_numpy(c["tidx"].view(np.int32)).to(dev)
    matched = torch.empty(a.topk, dtype=torch.int64, device=dev); recall = torch.empty(a.topk, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def same(w, what):
        if not (np.array_equal(matched.cpu().numpy().view(np.uint64), w[0]) and np.array_equal(recall.cpu().numpy().view(np.uint64), w[1].view(np.uint64))):
            raise SystemExit(f"{what}: the device sums differ from the restatement")

    def device(rows=a.rows):
        clib.metrics_device(0, rows, idx.data_ptr(), val.data_ptr(), cnt.data_ptr(), a.stride, tptr.data_ptr(), tidx.data_ptr(), a.topk,
                            matched.data_ptr(), recall.data_ptr(), sync=True)

    def device_checked():
        device(); same(want, "all rows")

    dev_ms, _ = median_ms(device)                                        # (the timed call alone ...)
    median_ms(device_checked, warm=0)                                    # (... and five more, each compared)
    device(prefix); same(want_prefix, f"{prefix}-row prefix")
    host = {}

    def copy_back():
        host["t"] = (idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy())
    copy_ms, _ = median_ms(copy_back)
    numpy_ms, _ = median_ms(lambda: mc.metric_sums(c))
    lines = [f"## {a.rows} rows, stride {a.stride}, topk {a.topk}, {a.labels} labels, 1-7 true labels per row", "",
             "| route | ms (median of 5 after 2 warm-ups) |", "|---|---|",
             f"| device call (K8, synchronised) | {dev_ms:.3f} |",
             f"| copy back of the result triple | {copy_ms:.2f} |",
             f"| numpy restatement on the host (vectorised) | {numpy_ms:.1f} |"]
    refpy = os.path.join(REPO, "oracle", "_ref", "refpy")
    if a.reference and os.path.isdir(refpy):
        sys.path.insert(0, refpy)
        from pecos.utils import smat_util
        tY, pY = mc.true_csr(c), mc.pred_csr(c)
        t0 = time.perf_counter(); m = smat_util.Metrics.generate(tY, pY, topk=a.topk); ref_ms = (time.perf_counter() - t0) * 1e3
        pr = mc.from_sums(*want, a.rows)
        if not np.array_equal(np.asarray(m.prec).view(np.uint64), pr[0].view(np.uint64)):
            raise SystemExit("the reference's prec differs from the restatement's")
        lines.append(f"| the reference's Metrics.generate (one run; prec equal bit for bit) | {ref_ms:.0f} |")
    text = "\n".join(lines) + "\n\nEvery timed device output equals the restatement bit for bit (u64 counts, fp64 sums), on all rows and on the " \
        f"{prefix}-row prefix.\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
