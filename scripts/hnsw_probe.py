"""First timings of HNSW search on the device (K17) at two shapes: a dense-768 index and a sparse tf-idf-like index.

    python scripts/hnsw_probe.py [--out profiles/hnsw_predict.md] [--small]

The parent never opens the GPU.  It makes the data, trains both indexes with the compiled reference (oracle/_ref, 16 threads), times the
reference's predict at 1 and at 16 threads first, and then runs the host entry point and the resident form each in a child process of its
own under a time limit sized from the reference's single-thread time.  A child checks its answer against the reference's (ids; distance
bits where the contract gives them: sparse always, dense when this host has avx512f), times `--reps` calls after one warm-up, and reports
the counters.  No timing target exists; the numbers are written down with how they were taken."""
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
import hnsw_rule as hr  # noqa: E402

SETTINGS = ((100, 10), (400, 100))


def shapes(small):
    if small:
        return {"dense-768": ("drm", 2000, 768, 200), "sparse-tfidf": ("csr", 2000, 20000, 200)}
    return {"dense-768": ("drm", 20000, 768, 2000), "sparse-tfidf": ("csr", 20000, 100000, 2000)}


def make(kind, n, dim, nq, seed):
    if kind == "drm":
        X = hr.dense_items(n + nq, dim, seed)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        return X[:n], X[n:]
    rs = np.random.RandomState(seed)                      # Zipf-like column popularity, about 60 entries a row, l2-normalised rows
    rows = []
    p = 1.0 / np.arange(1, dim + 1) ** 0.8
    p /= p.sum()
    for _ in range(n + nq):
        ids = np.unique(rs.choice(dim, size=60, p=p))
        v = rs.rand(len(ids)).astype(np.float32) + 0.1
        rows.append((ids, v / np.linalg.norm(v)))
    ptr = np.cumsum([0] + [len(r[0]) for r in rows])
    X = smat.csr_matrix((np.concatenate([r[1] for r in rows]).astype(np.float32), np.concatenate([r[0] for r in rows]).astype(np.int32), ptr), shape=(n + nq, dim))
    return X[:n].tocsr(), X[n:].tocsr()


def median_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts))


def child(mode, folder, reps):
    import torch
    import pecos_amd
    from pecos_amd import clib
    kind = json.load(open(os.path.join(folder, "param.json")))["data_type"]
    Q = np.load(os.path.join(folder, "Q.npy")) if kind == "drm" else smat.load_npz(os.path.join(folder, "Q.npz")).tocsr()
    t0 = time.perf_counter()
    m = pecos_amd.HNSW.load(folder)
    out = {"mode": mode, "load_s": time.perf_counter() - t0, "device_bytes": m.info["device_bytes"], "runs": []}
    exact = kind == "csr" or hr.host_has_avx512f()
    for efS, topk in SETTINGS:
        ref = np.load(os.path.join(folder, "ref_%d_%d.npz" % (efS, topk)))
        pp = m.PredParams(efS=efS, topk=topk)
        if mode == "host":
            run = lambda: m.predict(Q, pred_params=pp, ret_csr=False)
            got = run()
        else:
            dev = "cuda:0"
            Xd = torch.from_numpy(Q).to(dev) if kind == "drm" else pecos_amd.DeviceMatrix.upload(Q)
            if kind == "csr":
                Xd = tuple(Xd.to_torch()[:3])
            s = m.searchers_create(2048)

            def run():
                r = pecos_amd.hnsw_predict_device(m, Xd, efS=efS, topk=topk, searchers=s)
                torch.cuda.synchronize()
                return r
            r = run()
            got = (r[0].cpu().numpy().view(np.uint32), r[1].cpu().numpy())
        same_ids = bool(np.array_equal(got[0], ref["idx"]))
        same_bits = bool(np.array_equal(got[1].view(np.uint32), ref["bits"]))
        clib.debug_hnsw_counters(reset=True)
        run()
        c = clib.debug_hnsw_counters()
        med, best = median_time(run, reps)
        out["runs"].append({"efS": efS, "topk": topk, "median_s": med, "min_s": best, "same_ids": same_ids, "same_bits": same_bits, "bits_in_contract": exact, "counters": c})
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.reps)
    if not hr.have_reference():
        sys.exit("oracle/_ref/libpecos_float32.so is missing: build() makes it where the reference's sources are")
    lines = ["# HNSW search on the device (K17): first timings", "",
             "One MI355X; host: %d CPUs visible to the process, avx512f %s.  Written by `scripts/hnsw_probe.py%s`: median of %d timed calls after one warm-up call, "
             "`time.perf_counter` around the call (the resident form ends with a device synchronisation); the reference is timed first, in the parent, which never "
             "opens the GPU; each of this library's two forms runs in a child process of its own.  Indexes are trained by the reference with 16 threads, M = 32, efC = 100.  "
             "Nobody has tuned this kernel and no timing target exists." % (len(os.sched_getaffinity(0)), "yes" if hr.host_has_avx512f() else "no", " --small" if a.small else "", a.reps), ""]
    failed = False
    for name, (kind, n, dim, nq) in shapes(a.small).items():
        if failed:
            break                                          # nothing more is started on the GPU after a failure
        with tempfile.TemporaryDirectory() as d:
            X, Q = make(kind, n, dim, nq, 7)
            t0 = time.perf_counter()
            hr.train_reference(X, d, metric="ip", M=32, efC=100, threads=16)
            train_s = time.perf_counter() - t0
            if kind == "drm":
                np.save(os.path.join(d, "Q.npy"), Q)
            else:
                smat.save_npz(os.path.join(d, "Q.npz"), Q)
            info = hr.check_folder(d)[0]
            lines += ["## %s: %d items x %d, %d queries, %s / ip (max_level %d; trained by the reference in %.1f s)" % (name, n, dim, nq, kind, info[5], train_s), "",
                      "| efS | topk | reference 1 thread | reference 16 threads | host entry point | resident form | ids / bits equal | dist evals | pops | admissions | passes | max cand | rerun | heap form |",
                      "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
            ref_t, ref = {}, hr.Reference(d)              # loaded once: only predict is timed
            for efS, topk in SETTINGS:
                idx, dist = ref.predict(Q, efS, topk, threads=1)
                np.savez(os.path.join(d, "ref_%d_%d.npz" % (efS, topk)), idx=idx, bits=dist.view(np.uint32))
                ref_t[(efS, topk)] = (median_time(lambda: ref.predict(Q, efS, topk, threads=1), 3)[0], median_time(lambda: ref.predict(Q, efS, topk, threads=16), 3)[0])
            ref.close()
            limit = max(120.0, 40.0 * sum(t[0] for t in ref_t.values()))
            res = {}
            for mode in ("host", "device"):
                try:
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, d, "--reps", str(a.reps)], capture_output=True, text=True, timeout=limit)
                    got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                    res[mode] = json.loads(got[-1][7:]) if got else {"error": "exit %d: %s" % (p.returncode, p.stderr[-300:])}
                except subprocess.TimeoutExpired:
                    res[mode] = {"error": "time limit of %.0f s" % limit}
                if "error" in res[mode]:
                    lines += ["", "%s form failed: %s" % (mode, res[mode]["error"]), ""]
                    failed = True
                    break
            for k, (efS, topk) in enumerate(SETTINGS):
                def cell(mode):
                    r = res.get(mode, {})
                    return "%.1f ms" % (1e3 * r["runs"][k]["median_s"]) if "runs" in r else "-"
                r = (res.get("device") or {}).get("runs") or (res.get("host") or {}).get("runs")
                c = r[k]["counters"] if r else {}
                eq = "-" if not r else "%s / %s%s" % (r[k]["same_ids"], r[k]["same_bits"], "" if r[k]["bits_in_contract"] else " (bits outside the contract on this host)")
                lines.append("| %d | %d | %.1f ms | %.1f ms | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (
                    efS, topk, 1e3 * ref_t[(efS, topk)][0], 1e3 * ref_t[(efS, topk)][1], cell("host"), cell("device"), eq, c.get("dist", "-"), c.get("pops", "-"),
                    c.get("admissions", "-"), c.get("passes", "-"), c.get("max_cand", "-"), c.get("rerun", "-"), "HBM" if c.get("hbm_queries") else "LDS"))
            if "runs" in res.get("host", {}):
                lines += ["", "Load (read, check, split, upload): %.2f s; %.1f MB held in HBM." % (res["host"]["load_s"], res["host"]["device_bytes"] / 1e6), ""]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
