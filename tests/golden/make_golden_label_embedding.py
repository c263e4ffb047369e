"""Records tests/golden/label_embedding_ref.npz from the live reference (oracle/_ref/refpy, threads = 1): LabelEmbeddingFactory.create
for pifa, pifa_lf_concat and pii, with and without normalized_Y, on the 400 x 260 Y, 400 x 150 X and 260 x 40 Z of
tests/label_embedding_rule.golden_inputs(), and the chain of the reference's HierarchicalKMeans.gen on the pifa embedding.
Run from the repository root where the reference is built."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import clustering_rule as cr  # noqa: E402
import label_embedding_rule as ler  # noqa: E402


def record(path):
    sys.path.insert(0, os.path.join(cr.REPO, "oracle", "_ref", "refpy"))
    from pecos.xmc.base import HierarchicalKMeans, LabelEmbeddingFactory
    Y, X, Z = ler.golden_inputs()
    out = {}
    for method in ler.METHODS:
        for normalized_Y in (True, False):
            kw = {} if method == "pii" else dict(threads=1, normalized_Y=normalized_Y)
            if method == "pifa_lf_concat":
                kw["Z"] = Z.copy()
            E = LabelEmbeddingFactory.create(Y.copy(), X.copy(), method=method, **kw).tocsr()
            key = ler.golden_key(method, normalized_Y)
            out[key + "__shape"] = np.array(E.shape)
            out[key + "__indptr"] = E.indptr.astype(np.uint64)
            out[key + "__indices"] = E.indices.astype(np.uint32)
            out[key + "__data"] = E.data.astype(np.float32)
            if method == "pifa" and normalized_Y:
                chain = HierarchicalKMeans.gen(E, train_params=HierarchicalKMeans.TrainParams.from_dict(ler.GOLDEN_CHAIN))
                out["chain__levels"] = np.array([len(chain)])
                for i, C in enumerate(chain):
                    C = C.tocsc()
                    C.sort_indices()
                    out[f"chain__{i}__shape"] = np.array(C.shape)
                    out[f"chain__{i}__indptr"] = C.indptr.astype(np.int64)
                    out[f"chain__{i}__indices"] = C.indices.astype(np.int64)
                    out[f"chain__{i}__data"] = C.data.astype(np.float32)
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    record(os.path.join(HERE, "label_embedding_ref.npz"))
