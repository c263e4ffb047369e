"""The CPU half of the label clustering (K11): the numpy statement of the rule (tests/clustering_rule.py) against the compiled reference at
threads = 1 on every case of the GPU half, sampled ones included; the host plan (xrl_debug_cluster_plan) against the statement's draws;
the order preconditions of the near-duplicate cases, without which those cases pin nothing; every refusal that needs no GPU;
TrainParams, depth inference and the chain builder against the recorded goldens; the reference's link_clustering prototypes."""
import ctypes
import os
import sys

import numpy as np
import pytest
import scipy.sparse as smat

import clustering_rule as cr
from conftest import GOLDEN, REPO

CASES = cr.cases()
RECORDED = np.load(os.path.join(GOLDEN, "clustering_ref.npz"))
CHAINS = np.load(os.path.join(GOLDEN, "clustering_chains.npz"))
HAVE_REF = os.path.exists(cr.REF)
_truth = {}


def truth(name):
    if name not in _truth:
        X, depth, kw = CASES[name]
        _truth[name] = cr.statement(X, depth, **kw)
    return _truth[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_statement_equals_the_reference(name):
    X, depth, kw = CASES[name]
    assert np.array_equal(truth(name)["codes"], RECORDED[name + "__csr"]), "the statement differs from the recorded reference"
    if HAVE_REF:
        assert np.array_equal(truth(name)["codes"], cr.reference(X, depth, **kw)), "the statement differs from the live reference"


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if cr.dense_ok(c[0]) and c[0].shape[0] * c[0].shape[1] <= 200_000))
def test_statement_equals_the_reference_dense(name):
    X, depth, kw = CASES[name]
    D = np.ascontiguousarray(X.toarray())
    got = cr.statement(cr.as_full_csr(D), depth, **kw)["codes"]
    assert np.array_equal(got, RECORDED[name + "__drm"])
    if HAVE_REF:
        assert np.array_equal(got, cr.reference(D, depth, **kw))


def test_reference_is_deterministic():
    if not HAVE_REF:
        pytest.skip("oracle/_ref not built")
    for name in ("sample_warm_sk", "rand300_km_s1"):
        X, depth, kw = CASES[name]
        for threads in (1, 8):
            assert np.array_equal(cr.reference(X, depth, threads=threads, **kw), cr.reference(X, depth, threads=threads, **kw))


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_equals_the_statements_draws(name):
    from pecos_amd import clib
    from pecos_amd.core import ClusteringParam
    X, depth, kw = CASES[name]
    t = truth(name)
    p = ClusteringParam(partition_algo=kw.get("algo", cr.SKMEANS), seed=kw.get("seed", 0), kmeans_max_iter=kw.get("max_iter", 20), threads=1,
                        max_sample_rate=kw.get("max_rate", 1.0), min_sample_rate=kw.get("min_rate", 1.0), warmup_ratio=kw.get("warmup", 1.0))
    plan = clib.debug_cluster_plan(X.shape[0], X.shape[1], X.nnz, depth, p)
    assert np.array_equal(plan["node_seed"], t["node_seed"])
    assert np.array_equal(plan["perm"], t["perm"])
    assert plan["level_info"][:, 1].astype(bool).tolist() == t["first_touch"]
    for nid, w in t["work"].items():
        assert tuple(int(v) for v in plan["work"][nid]) == w, f"node {nid}"


@pytest.mark.parametrize("tag,algo", [("sk", cr.SKMEANS), ("km", cr.KMEANS)])
def test_near_duplicate_cases_pin_the_order(tag, algo):
    """On these cases the order of the additions decides codes: a reversed walk of update_center changes some, the SKMEANS norm in
    ascending feature order changes some, and the reference itself answers differently with 8 threads.  A case on which one of these
    fails pins nothing and is worthless: regenerate it (tests/golden/make_golden_clustering.py --search)."""
    X, depth, kw = CASES[f"near_duplicate_{tag}"]
    want = truth(f"near_duplicate_{tag}")["codes"]
    changed = int((cr.statement(X, depth, variant="reverse_walk", **kw)["codes"] != want).sum())
    assert changed >= 1, "worthless case: the reversed walk changes no code"
    if algo == cr.SKMEANS:
        changed = int((cr.statement(X, depth, variant="ascending_norm", **kw)["codes"] != want).sum())
        assert changed >= 1, "worthless case: the ascending-feature norm changes no code"
    if HAVE_REF:
        assert not np.array_equal(cr.reference(X, depth, threads=8, **kw), want), "worthless case: the reference at 8 threads gives the same codes"


def test_plain_random_data_pins_no_order():
    X, depth, kw = CASES["rand300_sk_s0"]
    assert np.array_equal(cr.statement(X, depth, variant="reverse_walk", **kw)["codes"], truth("rand300_sk_s0")["codes"])


# ------------------------------------------------------------------------------------------------ refusals, before a GPU is needed
def _call(fn_name, view, depth, param, codes):
    lib = cr.load(cr.OURS)
    fn = getattr(lib, fn_name)
    fn.restype, fn.argtypes = None, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    fn(view, depth, param, codes)
    return cr.last_error(lib)


REFUSALS = {
    "depth_above_rows": (dict(depth=7), "2^depth"),
    "depth_31": (dict(depth=31), "above 30"),
    "algo": (dict(algo=3), "partition_algo"),
    "min_rate_zero": (dict(min_rate=0.0), "expect 0 < min_sample_rate <= 1.0"),
    "min_rate_above_1": (dict(min_rate=1.5, max_rate=1.0), "expect 0 < min_sample_rate <= 1.0"),
    "max_rate_zero": (dict(max_rate=0.0, min_rate=0.5), "expect 0 < max_sample_rate <= 1.0"),
    "max_rate_above_1": (dict(max_rate=1.5, min_rate=0.5), "expect 0 < max_sample_rate <= 1.0"),
    "min_above_max": (dict(min_rate=0.9, max_rate=0.5), "expect min_sample_rate <= max_sample_rate"),
    "warmup_negative": (dict(warmup=-0.1), "expect 0 <= warmup_ratio <= 1.0"),
    "warmup_above_1": (dict(warmup=1.1), "expect 0 <= warmup_ratio <= 1.0"),
    "sampled_node_below_2": (dict(min_rate=0.01, max_rate=0.01, warmup=0.0), "samples"),
}


@pytest.mark.parametrize("fn", ["c_run_clustering_csr_f32", "c_run_clustering_drm_f32"])
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(fn, name):
    kw, needle = REFUSALS[name]
    kw = dict(kw)
    depth = kw.pop("depth", 3)
    X = cr.random_csr(100, 12, 4, 60)
    got, err = cr.run_library(cr.OURS, X if fn.endswith("csr_f32") else X.toarray(), depth, **kw)
    assert err and err.startswith(fn + ": ") and needle in err, err
    assert np.all(got == 0xFFFFFFFF)


@pytest.mark.parametrize("fn", ["c_run_clustering_csr_f32", "c_run_clustering_drm_f32"])
def test_null_pointers_are_refused(fn):
    X = cr.random_csr(20, 6, 3, 61)
    ptr, idx, val = X.indptr.astype(np.uint64), X.indices.astype(np.uint32), X.data
    dense = np.ascontiguousarray(X.toarray())
    csr = fn.endswith("csr_f32")
    view = cr.CsrView(20, 6, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data) if csr else cr.DrmView(20, 6, dense.ctypes.data)
    param, codes = cr.make_param(), np.zeros(20, np.uint32)
    assert _call(fn, None, 2, ctypes.byref(param), codes.ctypes.data).startswith(fn + ": null")
    assert _call(fn, ctypes.byref(view), 2, None, codes.ctypes.data).startswith(fn + ": null")
    assert _call(fn, ctypes.byref(view), 2, ctypes.byref(param), None).startswith(fn + ": null")
    bad = cr.CsrView(20, 6, ptr.ctypes.data, None, val.ctypes.data) if csr else cr.DrmView(20, 6, None)
    assert _call(fn, ctypes.byref(bad), 2, ctypes.byref(param), codes.ctypes.data).startswith(fn + ": null")


def test_resident_form_refuses_before_a_gpu():
    lib = cr.load(cr.OURS)
    fn = lib.xrl_run_clustering_device
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    param = cr.make_param()
    assert fn(None, 2, ctypes.byref(param), 16, None, None) == -1
    assert cr.last_error(lib).startswith("xrl_run_clustering_device: null")
    # a handle that wraps device addresses makes no GPU call: the plan's refusals come first
    mk = lib.xrl_smat_from_device_csr
    mk.restype, mk.argtypes = ctypes.c_void_p, [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    h = mk(0, 10, 4, 256, 256, 256, 12)
    assert h and cr.last_error(lib) is None
    try:
        assert fn(h, 2, None, 16, None, None) == -1 and cr.last_error(lib).startswith("xrl_run_clustering_device: null")
        assert fn(h, 2, ctypes.byref(param), None, None, None) == -1 and cr.last_error(lib).startswith("xrl_run_clustering_device: null")
        assert fn(h, 4, ctypes.byref(param), 16, None, None) == -1 and "2^depth" in cr.last_error(lib)
        bad = cr.make_param(algo=1)
        assert fn(h, 2, ctypes.byref(bad), 16, None, None) == -1 and "partition_algo" in cr.last_error(lib)
    finally:
        lib.xrl_smat_free.argtypes = [ctypes.c_void_p]
        lib.xrl_smat_free(h)


def test_param_layout_is_the_references():
    from pecos_amd.core import ClusteringParam
    assert ctypes.sizeof(ClusteringParam) == ctypes.sizeof(cr.Param) == 40
    assert [(n, t) for n, t in ClusteringParam._fields_] == [(n, t) for n, t in cr.Param._fields_]
    for name, _ in cr.Param._fields_:
        assert getattr(ClusteringParam, name).offset == getattr(cr.Param, name).offset


# ------------------------------------------------------------------------------------------------ the Python surface
def test_train_params_defaults_and_depth():
    from pecos_amd import HierarchicalKMeans
    p = HierarchicalKMeans.TrainParams()
    assert (p.nr_splits, p.min_codes, p.max_leaf_size, p.spherical, p.seed, p.kmeans_max_iter, p.threads) == (16, None, 100, True, 0, 20, -1)
    assert (p.do_sample, p.max_sample_rate, p.min_sample_rate, p.warmup_ratio) == (False, 1.0, 0.1, 0.4)
    assert (HierarchicalKMeans.KMEANS, HierarchicalKMeans.SKMEANS) == (0, 5)
    assert [p.infer_binary_tree_depth(n) for n in (101, 200, 201, 1000, 6400, 6401)] == [1, 1, 2, 4, 6, 7]
    q = HierarchicalKMeans.TrainParams(max_leaf_size=1)
    assert q.infer_binary_tree_depth(64) == 6
    with pytest.raises(ValueError):
        HierarchicalKMeans.TrainParams(max_leaf_size=1).infer_binary_tree_depth(65)
    assert HierarchicalKMeans.TrainParams.from_dict(dict(nr_splits=4, unknown=1)).nr_splits == 4
    r = HierarchicalKMeans.TrainParams(do_sample=True)
    assert [r.get_layer_sample_rate(d, 5) for d in range(5)] == pytest.approx([0.1, 0.1, 0.4, 0.7, 1.0])


def _recorded_chain(name):
    out = []
    for i in range(int(CHAINS[name + "__levels"][0])):
        out.append(smat.csc_matrix((CHAINS[f"{name}__{i}__data"], CHAINS[f"{name}__{i}__indices"], CHAINS[f"{name}__{i}__indptr"]),
                                   shape=tuple(CHAINS[f"{name}__{i}__shape"])))
    return out


def _same_chain(a, b):
    assert len(a) == len(b)
    for A, B in zip(a, b):
        A, B = A.tocsc(), B.tocsc()
        A.sort_indices(); B.sort_indices()
        assert A.shape == B.shape and A.dtype == np.float32
        assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)


@pytest.mark.parametrize("name,kw", [("default", {}), ("splits4_min2", dict(nr_splits=4, min_codes=2)), ("splits2_min16", dict(nr_splits=2, min_codes=16)),
                                     ("min1", dict(nr_splits=4, min_codes=1))])
def test_chain_builder_against_the_recorded_chains(name, kw):
    """The recorded bottom matrix (the reference's codes) through this project's chain builder gives the recorded chain."""
    from pecos_amd.indexer import chain_from_partial, codes_to_csc
    want = _recorded_chain(name)
    bottom = want[-1]
    codes = np.zeros(bottom.shape[0], dtype=np.uint32)
    codes[bottom.indices] = np.repeat(np.arange(bottom.shape[1]), np.diff(bottom.indptr))
    depth = int(np.log2(bottom.shape[1]))
    _same_chain(chain_from_partial(codes_to_csc(codes, depth), **kw), want)


def test_max_leaf_size_shortcut_needs_no_gpu():
    from pecos_amd import HierarchicalKMeans
    X = cr.random_csr(700, 200, 8, 31)
    _same_chain(HierarchicalKMeans.gen(X, train_params=dict(max_leaf_size=700)), _recorded_chain("one_leaf"))


def test_reference_link_clustering_binds_to_this_library():
    refpy = os.path.join(REPO, "oracle", "_ref", "refpy")
    if not os.path.isdir(os.path.join(refpy, "pecos")):
        pytest.skip("oracle/_ref/refpy (the reference's python package) is not built")
    if refpy not in sys.path:
        sys.path.insert(0, refpy)
    import pecos.core.base as pcb
    ours = ctypes.CDLL(cr.OURS)
    lib = pcb.corelib.__new__(pcb.corelib)
    lib.clib_float32 = ours
    lib.link_clustering()
    assert ours.c_run_clustering_csr_f32.argtypes[2]._type_ is pcb.ClusteringParam
    assert ctypes.sizeof(pcb.ClusteringParam) == ctypes.sizeof(cr.Param)
    # a refusal travels through the reference's own binding and structures
    X = cr.random_csr(10, 5, 2, 62)

    class P:
        partition_algo, seed, kmeans_max_iter, threads, max_sample_rate, min_sample_rate, warmup_ratio, depth = 5, 0, 20, 1, 1.0, 1.0, 1.0, 6
    lib.run_clustering(pcb.ScipyCsrF32.init_from(X), P())
    assert cr.last_error(ours).startswith("c_run_clustering_csr_f32: 2^depth")
