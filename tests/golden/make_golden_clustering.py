"""Records tests/golden/clustering_ref.npz and clustering_chains.npz from the compiled reference (oracle/_ref, threads = 1):
the reference's codes of every case of tests/clustering_rule.py (CSR, and dense where the case is small), and the chains of the
reference's HierarchicalKMeans.gen for a handful of parameter sets.  ``--search`` looks for near-duplicate seeds on which the order
preconditions hold (tests/test_clustering_cpu.py asserts them).  ``range_edges`` writes clustering_range_edges.npz alone: the reference's
codes of clustering_rule.range_edge_cases() and of the widest-ids case renumbered into 2^24 columns, each run twice and required equal.
Run from the repository root where the reference is built."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import clustering_rule as cr  # noqa: E402


def gen_cases():
    """{name: (feature matrix, TrainParams keywords)} of the recorded chains."""
    X = cr.random_csr(700, 200, 8, 31)
    small = dict(max_leaf_size=10, threads=1)
    return {
        "default": (X, dict(small)),
        "splits4_min2": (X, dict(small, nr_splits=4, min_codes=2)),
        "splits2_min16": (X, dict(small, nr_splits=2, min_codes=16)),
        "min1": (X, dict(small, nr_splits=4, min_codes=1)),
        "kmeans": (X, dict(small, spherical=False, seed=3)),
        "sampled": (X, dict(small, do_sample=True, max_sample_rate=0.9, min_sample_rate=0.2, warmup_ratio=0.3)),
        "dense": (np.ascontiguousarray(X[:300, :40].toarray()), dict(small, kmeans_max_iter=5)),
        "one_leaf": (X, dict(max_leaf_size=700, threads=1)),
        "leaf100": (X, dict(threads=1)),
    }


def record_codes(path):
    out = {}
    for name, (X, depth, kw) in cr.cases().items():
        out[name + "__csr"] = cr.reference(X, depth, **kw)
        if cr.dense_ok(X):
            out[name + "__drm"] = cr.reference(X.toarray(), depth, **kw)
    np.savez_compressed(path, **out)


def record_chains(path):
    sys.path.insert(0, os.path.join(cr.REPO, "oracle", "_ref", "refpy"))
    from pecos.xmc.base import HierarchicalKMeans
    out = {}
    for name, (X, kw) in gen_cases().items():
        chain = HierarchicalKMeans.gen(X, train_params=HierarchicalKMeans.TrainParams.from_dict(kw))
        out[name + "__levels"] = np.array([len(chain)])
        for i, C in enumerate(chain):
            C = C.tocsc()
            C.sort_indices()
            out[f"{name}__{i}__shape"] = np.array(C.shape)
            out[f"{name}__{i}__indptr"] = C.indptr.astype(np.int64)
            out[f"{name}__{i}__indices"] = C.indices.astype(np.int64)
            out[f"{name}__{i}__data"] = C.data.astype(np.float32)
    np.savez_compressed(path, **out)


def record_range_edges(path):
    out = {}

    def twice(X, depth, kw):
        a, b = cr.reference(X, depth, **kw), cr.reference(X, depth, **kw)
        assert np.array_equal(a, b), "the reference answered differently the second time"
        return a
    for name, (X, depth, kw) in cr.range_edge_cases().items():
        out[name + "__csr"] = twice(X, depth, kw)
        if cr.dense_ok(X):
            out[name + "__drm"] = twice(X.toarray(), depth, kw)
    out["wide_ids_2p24__csr"] = twice(cr.wide_ids(1 << 24), cr.WIDE_IDS_DEPTH, cr.WIDE_IDS_KW)
    np.savez_compressed(path, **out)


def search(algo, seeds=range(0, 40)):
    for s in seeds:
        X = cr.near_duplicate(seed=s)
        kw = dict(algo=algo, seed=s)
        ref = cr.reference(X, 6, **kw)
        n = [int((cr.statement(X, 6, variant=v, **kw)["codes"] != ref).sum()) for v in ("reverse_walk", "ascending_norm")]
        t8 = int((cr.reference(X, 6, threads=8, **kw) != ref).sum())
        print("algo", algo, "seed", s, "reverse_walk", n[0], "ascending_norm", n[1], "8 threads", t8, flush=True)
        if n[0] and t8 and (n[1] or algo == cr.KMEANS):
            return s
    return None


if __name__ == "__main__":
    if "--search" in sys.argv:
        print({a: search(a) for a in (cr.SKMEANS, cr.KMEANS)})
    elif "range_edges" in sys.argv:
        record_range_edges(os.path.join(HERE, "clustering_range_edges.npz"))
    else:
        record_codes(os.path.join(HERE, "clustering_ref.npz"))
        record_chains(os.path.join(HERE, "clustering_chains.npz"))
