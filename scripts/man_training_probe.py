"""First timings of training under matcher-aware negatives (tfn+man) on the device beside the same loop through the host entry points and
the compiled reference on the same box: the layer chains above the Eurlex-like leaf layer and the slice of an Amazon-670K-like leaf layer
that scripts/ranker_training_probe.py generates (clusters grouped 16 to a parent up to a single root).

    python scripts/man_training_probe.py [--problem eurlex|amazon|both] [--no-reference] [--only-train] [--runs N] [--out FILE.json]

resident      pecos_amd.train_chain_device: X, Y, the label chain, the matching matrices, the predictions and the weights stay in HBM
host loop     the reference's loop in scipy (tests/matching_rule.chain_loop) over this library's HOST entry points: per layer an upload of
              X and the operands, the weights and the prediction copied back, the union on the host -- what residency is measured against
reference     the same loop over the compiled reference (oracle/_ref), 16 threads and 1 thread, one run each
train         HierarchicalMLModel.train under tfn with every operand on the host, as a user calls it: uploads, the loop, the download of
              the weights and the model built from them; on the Eurlex-like chain, or with --only-train (nothing else, so the same file times any revision
              that has train) on the problem asked for
split         the resident loop once more, step by step, with stream events around each step: per layer the predict of the layer above,
              the union (with the wrap of the prediction as a CSR), the transposes, K13; the median of the timed runs
Results are compared with the host loop's (and the reference's where it ran): every layer's weights, bit for bit."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as smat

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "scripts"))
import matching_rule as mr  # noqa: E402
import ranker_training_probe as rp  # noqa: E402

TRAIN_KW = dict(threshold=0.1, max_iter=100, solver_type="L2R_L2LOSS_SVC_DUAL")
BEAM, POST = 10, "l3-hinge"
RUNS = 5


def split_loop(x, y, chain_dev, pps, events):
    """train_chain_device's steps under tfn+man, one at a time; events(name, t) -> a context that times one step of layer t on the stream."""
    from pecos_amd.training import _label_chain, _union_of_sources, _predict_transposed, _train_transposed
    depth = len(chain_dev)
    with events("label_chain", 0):
        labels_of = _label_chain(y, chain_dev, None)
    weights, m_pred = [], None
    cts = []
    for t in range(depth):
        with events("transposes", t):
            cts.append(chain_dev[t].transpose())
        if t > 0:
            with events("predict", t):
                m_pred = _predict_transposed(x, weights[t - 1], cts[t - 1], m_pred, pps[t - 1][0], pps[t - 1][1], 1.0, None)
        with events("union", t):
            m = _union_of_sources(t, "tfn+man", labels_of, chain_dev[t], None, m_pred, None)
        with events("transposes", t):
            yt = labels_of[t].transpose()
            mt = None if m is None else m.transpose()
        with events("k13", t):
            weights.append(_train_transposed(x, yt, cts[t] if m is not None else None, mt, None, None, bias=1.0, **TRAIN_KW))
    return weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", default="both", choices=["eurlex", "amazon", "both"])
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--runs", type=int, default=RUNS)
    ap.add_argument("--only-train", action="store_true", help="time HierarchicalMLModel.train alone (runs on any revision that has it)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    runs_n = a.runs
    import contextlib
    import torch
    import pecos_amd
    from pecos_amd import DeviceMatrix, HierarchicalMLModel, MLModel, clib
    from pecos_amd.xlinear import MLProblem
    from pecos_amd.indexer import chain_from_partial
    have_ref = mr.refpy_available() and not a.no_reference
    results = {}

    def report(name, r):
        results[name] = r
        print(name, json.dumps(r), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(results, open(a.out, "w"), indent=1)

    for name in (("eurlex", "amazon") if a.problem == "both" else (a.problem,)):
        X, Y, C, _ = rp.PROBLEMS[name]()
        chain = chain_from_partial(C, nr_splits=16)
        depth = len(chain)
        pps = [(POST, BEAM)] * depth
        pred_params = [MLModel.PredParams(only_topk=BEAM, post_processor=POST) for _ in range(depth)]
        r = dict(N=X.shape[0], d=X.shape[1], labels=Y.shape[1], chain=[list(c.shape) for c in chain], x_nnz=int(X.nnz), y_nnz=int(Y.nnz), beam=BEAM, post_processor=POST)

        # HierarchicalMLModel.train under tfn as a user calls it: every operand on the host, the model built at the end
        def train():
            model = HierarchicalMLModel.train(MLProblem(X, Y), clustering=chain, negative_sampling_scheme="tfn", **TRAIN_KW)
            torch.cuda.synchronize()
            return model

        if a.only_train or name == "eurlex":                             # (the Amazon-like slice only when asked for: about a minute per run)
            train()                                                       # warm-up: module load, allocator
            times = []
            for _ in range(runs_n):
                t0 = time.perf_counter()
                model = train()
                times.append(time.perf_counter() - t0)
            r["train_tfn_s"] = statistics.median(times)
            r["train_tfn_runs_s"] = times
            r["train_tfn_w_nnz"] = [int(layer.W.nnz) for layer in model.layers]
            del model
        if a.only_train:
            report(name, r)
            continue
        t0 = time.perf_counter()
        x, y, chain_dev = DeviceMatrix.upload(X), DeviceMatrix.upload(smat.csr_matrix(Y)), [DeviceMatrix.upload(c) for c in chain]
        torch.cuda.synchronize()
        r["upload_s"] = time.perf_counter() - t0

        def resident():
            out = pecos_amd.train_chain_device(x, y, chain_dev, "tfn+man", train_params=TRAIN_KW, pred_params=pred_params, return_matching=True)
            torch.cuda.synchronize()
            return out

        resident()                                                        # warm-up: module load, allocator
        before = clib.debug_match_forms()
        times = []
        for _ in range(runs_n):
            t0 = time.perf_counter()
            weights, matchings, _ = resident()
            times.append(time.perf_counter() - t0)
        after = clib.debug_match_forms()
        r["resident_s"] = statistics.median(times)
        r["resident_runs_s"] = times
        r["match_forms_per_run"] = {k: (after[k] - before[k]) // runs_n for k in ("lds_rows", "big_rows", "read", "written")}
        r["m_nnz"] = [None if m is None else int(m.info["nnz"]) for m in matchings]
        r["w_nnz"] = [int(w.info["nnz"]) for w in weights]
        got = [mr.wt_to_w(w.download()) for w in weights]

        # the per-layer split, from stream events
        cur, runs, bounds = {}, [], []

        @contextlib.contextmanager
        def events(step, t):
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record()
            yield
            e.record()
            e.synchronize()
            cur[f"{step}[{t}]"] = cur.get(f"{step}[{t}]", 0.0) + b.elapsed_time(e) / 1e3      # (a layer's transposes are two steps of one name)
            if step == "predict":
                bounds.append(clib.debug_match_forms()["last_bound"])

        split_loop(x, y, chain_dev, pps, events)                          # warm-up
        cur.clear(); bounds.clear()
        for _ in range(runs_n):
            split = split_loop(x, y, chain_dev, pps, events)
            runs.append(dict(cur))
            cur.clear()
        r["split_s"] = {k: statistics.median(run[k] for run in runs) for k in runs[0]}
        r["largest_candidate_bound"] = int(max(bounds)) if bounds else 0
        for t in range(depth):
            assert mr.same_bits(mr.wt_to_w(split[t].download()), got[t]), f"{name}: the split loop's layer {t} differs"

        # the same loop through the host entry points
        t0 = time.perf_counter()
        host = mr.chain_loop(X, Y, chain, ["tfn+man"] * depth, *mr.ours_host_backend(TRAIN_KW), pps)
        r["host_loop_s"] = time.perf_counter() - t0
        for t in range(depth):
            assert mr.same_bits(got[t], host["W"][t]), f"{name}: layer {t} differs from the host loop's"
        r["equals_host_loop"] = True
        if have_ref:
            for threads in (16, 1):
                t0 = time.perf_counter()
                ref = mr.chain_loop(X, Y, chain, ["tfn+man"] * depth, *mr.reference_backend(threads, TRAIN_KW), pps)
                r[f"reference_{threads}_threads_s"] = time.perf_counter() - t0
                for t in range(depth):
                    assert mr.same_bits(got[t], ref["W"][t]), f"{name}: layer {t} differs from the reference at {threads} threads"
            r["equals_reference"] = True
        report(name, r)


if __name__ == "__main__":
    main()
