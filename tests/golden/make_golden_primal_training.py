"""Records tests/golden/primal_training_ref.npz from the compiled reference (threads = 1): per case of primal_training_rule.cases() and of
its seeded search the (rows, cols, value bits) of c_xlinear_single_layer_train_* with L2R_L2LOSS_SVC_PRIMAL, and through the reference's
own python package (oracle/_ref/refpy) on relevance_rule.fixture_problem() (200 x 48 labels) the per-layer weights of XLinearModel.train
per configuration of primal_training_rule.E2E_CONFIGS, with the predictions of the first.  Inputs and outputs only.  Run from the
repository root where the reference is built."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import matching_rule as mr  # noqa: E402
import primal_training_rule as pr  # noqa: E402


def record(path):
    out = {}
    cases = dict(pr.cases())
    cases.update({"search_" + k: v for k, v in pr.search_cases().items()})
    for name, (X, Y, C, M, R, kw) in cases.items():
        ref = pr.reference(X, Y, C, M, R, **kw)
        cols, rows, bits = pr.canonical(ref["rows"], ref["cols"], ref["vals"]) if kw.get("max_nonzeros") else (ref["cols"], ref["rows"], ref["vals"].view(np.uint32))
        out[f"case__{name}__rows"], out[f"case__{name}__cols"], out[f"case__{name}__bits"] = rows.astype(np.uint32), cols.astype(np.uint32), bits
    mr.import_refpy()
    from pecos.xmc.xlinear.model import XLinearModel
    stored = {}
    for name in pr.E2E_CONFIGS:
        X, Y, C, R, kw = pr.e2e_kwargs(name)
        model = XLinearModel.train(X, Y, C=C, R=R, threads=1, **kw)
        out[f"e2e__{name}__depth"] = np.array([len(model.model.model_chain)])
        for t, layer in enumerate(model.model.model_chain):
            W = layer.W.tocsc()
            W.sort_indices()
            mr.put_sparse(out, f"e2e__{name}__W{t}", W, stored)
        if name == pr.E2E_PREDICTED:
            P = model.predict(X[:pr.E2E_QUERIES], threads=1, **pr.E2E_PREDICT_KW).tocsr()
            P.sort_indices()
            mr.put_sparse(out, f"e2e__{name}__pred", P)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 * 1024, f"{path}: {size} bytes"
    print(path, size, "bytes")


if __name__ == "__main__":
    record(pr.FIXTURE)
