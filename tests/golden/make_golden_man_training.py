"""Records tests/golden/man_training_ref.npz from the compiled reference through its own python package (oracle/_ref/refpy, threads = 1):
HierarchicalMLModel.train on ranker_training_rule.e2e_problem() with E2E_KW under the schemes of matching_rule.SCHEMES (tfn+man, man,
usn+tfn+man with a small random matching_chain, and the per-layer list tfn, tfn, tfn+man), each under l3-hinge and under noop -- per
layer the weights W (sorted CSC), the pattern of the matching matrix M the layer's MLProblem was built with (MLProblem.__init__ wrapped as
a recorder) and the prediction M_pred that entered it (MLModel.predict wrapped as a recorder; indptr, indices, value bits) -- and the
chain itself.  Inputs and outputs only.  Run from the repository root where the reference is built."""
import os
import sys

import numpy as np
import scipy.sparse as smat

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import matching_rule as mr  # noqa: E402
import ranker_training_rule as rr  # noqa: E402


def record(path):
    mr.import_refpy()
    from pecos.xmc import HierarchicalMLModel, MLModel, MLProblem
    from pecos.xmc.base import ClusterChain
    X, Y, C = rr.e2e_problem()
    chain = [smat.csc_matrix(c, dtype=np.float32) for c in ClusterChain.from_partial_chain(C, min_codes=rr.E2E_KW["min_codes"], nr_splits=rr.E2E_KW["nr_splits"])]
    out = {"depth": np.array([len(chain)])}
    for t, c in enumerate(chain):
        c.sort_indices()
        mr.put_sparse(out, f"chain__{t}", c)
    usn = mr.usn_chain()
    seen, stored = {"M": [], "P": []}, {}
    init, predict = MLProblem.__init__, MLModel.predict

    def init_recorder(self, *a, **kw):
        init(self, *a, **kw)
        if kw.get("C") is not None:                          # the layers' problems (the outer problem comes without C)
            seen["M"].append(None if kw.get("M") is None else self.M.copy())

    def predict_recorder(self, *a, **kw):
        got = predict(self, *a, **kw)
        seen["P"].append(got.copy())
        return got

    MLProblem.__init__, MLModel.predict = init_recorder, predict_recorder
    try:
        for name, scheme in mr.SCHEMES.items():
            for post in mr.POST:
                seen["M"].clear(); seen["P"].clear()
                tp = HierarchicalMLModel.TrainParams(neg_mining_chain=scheme, model_chain=MLModel.TrainParams(threads=1, **mr.TRAIN_KW))
                pp = HierarchicalMLModel.PredParams(model_chain=[MLModel.PredParams(only_topk=k, post_processor=p) for p, k in mr.layer_pred_params(post)])
                model = HierarchicalMLModel.train(MLProblem(X, Y), clustering=chain, matching_chain=usn if "usn" in name else None, train_params=tp, pred_params=pp)
                key = mr.config_key(name, post)
                assert len(seen["M"]) == len(chain) and len(seen["P"]) == len(chain) - 1      # every scheme here names man at layer 2 at the latest: a prediction before layer 1 and before layer 2
                preds = [None] + list(seen["P"])
                for t, layer in enumerate(model.model_chain):
                    W = layer.W.tocsc()
                    W.sort_indices()
                    mr.put_sparse(out, f"{key}__W{t}", W, stored)
                    if seen["M"][t] is not None:
                        M = smat.csc_matrix(seen["M"][t])
                        M.sort_indices()
                        mr.put_sparse(out, f"{key}__M{t}", M, stored)
                    if preds[t] is not None:
                        mr.put_sparse(out, f"{key}__P{t}", smat.csr_matrix(preds[t]), stored)
    finally:
        MLProblem.__init__, MLModel.predict = init, predict
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 * 1024, f"{path}: {size} bytes"
    print(path, size, "bytes")


if __name__ == "__main__":
    record(os.path.join(HERE, "man_training_ref.npz"))
