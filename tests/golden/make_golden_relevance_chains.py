"""Records tests/golden/relevance_chains_ref.npz from the compiled reference through its own python package (oracle/_ref/refpy, threads =
1) on relevance_rule.fixture_problem(): the chain of ClusterChain.from_partial_chain (nr_splits 4); ClusterChain.generate_relevance_chain
over the key sets, norm types and both values of induce of relevance_rule; generate_matching_chain over the key sets; and per
configuration of relevance_rule.TRAIN_CONFIGS the layers' W of XLinearModel.train.  Every matrix is kept as a CSR (W: CSC) with ascending
ids, no entry summed or dropped: row pointer, ids, value bits.  Inputs and outputs only.  Run from the repository root where the
reference is built."""
import os
import sys

import numpy as np
import scipy.sparse as smat

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import matching_rule as mr  # noqa: E402
import relevance_rule as rl  # noqa: E402


def record(path):
    mr.import_refpy()
    from pecos.utils.cluster_util import ClusterChain
    from pecos.xmc.xlinear.model import XLinearModel
    X, Y, C, R = rl.fixture_problem()
    chain = ClusterChain.from_partial_chain(C, min_codes=rl.NR_SPLITS, nr_splits=rl.NR_SPLITS)
    out, stored = {"depth": np.array([len(chain)])}, {}
    for t, c in enumerate(chain):
        c = smat.csc_matrix(c, dtype=np.float32)
        c.sort_indices()
        mr.put_sparse(out, f"chain__{t}", c)
    for ks, keys in rl.KEYSETS.items():
        for norm in rl.NORM_TYPES:
            for induce in (True, False):
                got = chain.generate_relevance_chain(rl.partial_dict(keys, "R"), norm_type=norm, induce=induce)
                got = got[-len(chain):] if keys else got[:len(chain)]           # (nothing given: the reference hands back one None more)
                for t, m in enumerate(got):
                    if m is not None:
                        mr.put_sparse(out, f"rel__{ks}__{norm}__{int(induce)}__{t}", rl.canonical_csr(m), stored)
        got = chain.generate_matching_chain(rl.partial_dict(keys, "M"))[:len(chain)]
        for t, m in enumerate(got):
            if m is not None:
                mr.put_sparse(out, f"match__{ks}__{t}", rl.canonical_csr(m), stored)
    for name in rl.TRAIN_CONFIGS:
        X, Yc, C, Rn, usn, kw = rl.train_kwargs(name)
        model = XLinearModel.train(X, Yc, C=C, R=Rn, user_supplied_negatives=usn, threads=1, **kw)
        out[f"train__{name}__depth"] = np.array([len(model.model.model_chain)])
        for t, layer in enumerate(model.model.model_chain):
            W = layer.W.tocsc()
            W.sort_indices()
            mr.put_sparse(out, f"train__{name}__W{t}", W, stored)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 * 1024, f"{path}: {size} bytes"
    print(path, size, "bytes")


if __name__ == "__main__":
    record(rl.FIXTURE)
