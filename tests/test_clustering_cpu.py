"""The CPU half of the label clustering (K11): the numpy statement of the rule (tests/clustering_rule.py) against the compiled reference at
threads = 1 on every case of the GPU half, sampled ones included; the host plan (xrl_debug_cluster_plan) against the statement's draws;
the order preconditions of the near-duplicate cases, without which those cases pin nothing; the range-edge cases (statement against the
recording, what each claims, no NaN in any iteration, the unscaled-centre variant changes their codes) and the widest column ids
renumbered into 2^24 columns at the reference; every refusal that needs no GPU;
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


# ------------------------------------------------------------------------------------------------ the range edges
EDGES = cr.range_edge_cases()
EDGES_RECORDED = np.load(os.path.join(GOLDEN, "clustering_range_edges.npz"))
FLT_MIN = float(np.finfo(np.float32).tiny)
_edge_truth = {}


def edge_truth(name):
    if name not in _edge_truth:
        X, depth, kw = EDGES[name]
        _edge_truth[name] = cr.statement(X, depth, trace=True, **kw)
    return _edge_truth[name]


def test_range_edge_cases_are_small():
    for name, (X, depth, kw) in EDGES.items():
        assert X.shape[0] <= 128 and depth <= 4, name
        assert np.all(np.isfinite(X.data)), name


@pytest.mark.parametrize("name", sorted(EDGES))
def test_range_edge_statement_equals_the_reference(name):
    X, depth, kw = EDGES[name]
    assert np.array_equal(edge_truth(name)["codes"], EDGES_RECORDED[name + "__csr"]), "the statement differs from the recorded reference"
    if HAVE_REF:
        assert np.array_equal(edge_truth(name)["codes"], cr.reference(X, depth, **kw)), "the statement differs from the live reference"


@pytest.mark.parametrize("name", sorted(n for n, c in EDGES.items() if cr.dense_ok(c[0]) and c[0].shape[0] * c[0].shape[1] <= 200_000))
def test_range_edge_statement_equals_the_reference_dense(name):
    X, depth, kw = EDGES[name]
    D = np.ascontiguousarray(X.toarray())
    got = cr.statement(cr.as_full_csr(D), depth, **kw)["codes"]
    assert np.array_equal(got, EDGES_RECORDED[name + "__drm"])
    if HAVE_REF:
        assert np.array_equal(got, cr.reference(D, depth, **kw))


@pytest.mark.parametrize("name", sorted(EDGES))
def test_range_edge_cases_meet_no_nan(name):
    """The contract's condition, a property of the inputs: no centre entry, no norm and no score of any iteration of any node is a NaN.
    A case that fails this is outside the contract: redraw it."""
    bad = {k: v["nans"] for k, v in edge_truth(name)["trace"].items() if v["nans"]}
    assert not bad, f"{name}: NaNs at (node, iteration) {bad}"


def _level(nid):
    return nid.bit_length() - 1


def _scored(t, key):
    s, we, _, _ = t["work"][key[0]]
    return we - s


@pytest.mark.parametrize("name", sorted(EDGES))
def test_range_edge_cases_hold_what_they_claim(name):
    """Every case meets, somewhere in the statement's trace, the edge it is named after.  Under KMEANS there is no norm: the cases named
    after one run the same inputs, and the claim is where their scores sit in fp32's range."""
    X, depth, kw = EDGES[name]
    t = edge_truth(name)
    tr = t["trace"]
    sk = kw["algo"] == cr.SKMEANS
    kind = name.rsplit("_", 1)[0]
    finite = np.abs(t["scores"][np.isfinite(t["scores"])]).astype(np.float64)
    both = [k for k, v in tr.items() if v["inf_sides"] == "RL"]
    if "first_touch" in kind:
        assert all(t["first_touch"]), "not in first-touch order from the root"
    elif "dense" in kind:
        assert not any(t["first_touch"]), "the norm order switches"
    if not sk and kind in ("collapse_dense", "collapse_first_touch", "one_half", "one_half_first_touch", "late_dense", "late_first_touch"):
        assert finite.max() > 1e35 and not any(v["inf_scores"] for v in tr.values())
        return
    if not sk and kind in ("subnormal_norm", "zero_norm"):
        assert 0 < finite[finite > 0].min() < FLT_MIN or (kind == "zero_norm" and (t["scores"] == 0).any())
        return
    if kind in ("collapse_dense", "collapse_first_touch", "all_but_first_centre"):
        assert both and sum(v["zeroed"] for v in tr.values()) >= 2 * len(both)
        assert not any(v["inf_scores"] for v in tr.values())
    elif kind in ("inf_scores_dense", "inf_scores_first_touch"):
        assert sum(v["inf_scores"] for v in tr.values()) > 0
        assert not sk or both
    elif kind in ("one_half", "one_half_first_touch"):
        assert [k for k, v in tr.items() if v["inf_sides"] == "R"] and [k for k, v in tr.items() if v["inf_sides"] == "L"]
        assert tr[(1, 1)]["inf_norms"] == 1, "the root's first split is not the block against the rest"
        for d in (1, 2):        # the scale is per node and side: some nodes of the level overflow and some do not
            per_node = {nid: sum(v["inf_norms"] for k, v in tr.items() if k[0] == nid) for nid in range(1 << d, 2 << d)}
            assert any(per_node.values()) and not all(per_node.values()), f"level {d}: {per_node}"
    elif kind in ("late_dense", "late_first_touch"):
        late = [k for k, v in tr.items() if v["runs"] >= 64 and any(a is not None and a >= 64 for a in v["inf_at"])]
        assert late, "no norm overflows past the 64th term of its chain"
    elif kind == "inf_ties":
        assert [k for k, v in tr.items() if v["id_decides"] and v["pos_inf"] and v["neg_inf"]], "no node with +inf and -inf and the id deciding"
        if not sk:
            assert [k for k, v in tr.items() if v["pos_inf"] == _scored(t, k)], "no node whose scores are all +inf"
            assert [k for k, v in tr.items() if v["neg_inf"] == _scored(t, k)], "no node whose scores are all -inf"
            assert np.all(np.isinf(t["scores"]))
    elif kind == "subnormal_norm":
        sub = [a for v in tr.values() if v["norms"] for a in v["norms"] if 0 < a < FLT_MIN]
        assert sub and max(1.0 / np.sqrt(np.float64(a)) for a in sub) > 1e20
    elif kind == "zero_norm":
        assert [k for k, v in tr.items() if v.get("zero_norm_sides")]
    elif kind == "sampled":
        whole = [k for k in tr if k[1] == "whole"]
        assert len(whole) == (1 << depth) - 1, "a level is not sampled"
        assert all(_scored(t, k) == (X.shape[0] >> _level(k[0])) // 2 for k in whole), "a node does not work on half of its range"
        if sk:
            assert sum(v["zeroed"] for v in tr.values()) > 0
        else:
            assert sum(v["inf_scores"] for v in tr.values()) > 0 and sum(tr[k]["inf_scores"] for k in whole) > 0
    else:
        raise AssertionError(f"{name}: a case without a claim")


@pytest.mark.parametrize("name", sorted(n for n, c in EDGES.items() if c[2]["algo"] == cr.SKMEANS
                                        and n.rsplit("_", 1)[0] not in ("subnormal_norm", "zero_norm")))
def test_unscaled_on_inf_changes_the_codes(name):
    """Keeping the summed centre of a half whose norm is infinite, where the rule zeroes it, changes codes on every SKMEANS case that
    meets an infinite norm: a device that does so cannot pass them."""
    X, depth, kw = EDGES[name]
    assert sum(v["zeroed"] for v in edge_truth(name)["trace"].values()) > 0, "no centre is zeroed by an infinite norm"
    changed = int((cr.statement(X, depth, variant="unscaled_on_inf", **kw)["codes"] != edge_truth(name)["codes"]).sum())
    assert changed >= 1, "worthless case: the unscaled centre changes no code"


def test_trace_and_variant_leave_plain_data_alone():
    X, depth, kw = CASES["rand300_sk_s0"]
    t = cr.statement(X, depth, trace=True, variant="unscaled_on_inf", **kw)
    assert np.array_equal(t["codes"], truth("rand300_sk_s0")["codes"]) and np.array_equal(t["scores"], truth("rand300_sk_s0")["scores"])
    assert not any(v["inf_norms"] or v["inf_scores"] or v["nans"] or v["zeroed"] for v in t["trace"].values())


def test_widest_ids_renumbering_leaves_the_codes():
    """The column ids enter the rule through their order and the first-touch switch only: the compact matrix under a strictly increasing
    renumbering into 2^24 columns has, at the reference, the codes the statement gives the compact matrix in first-touch order from
    the root (nnz=0).  The reference cannot hold a centre of 2^32 - 1 columns; the device is compared with the same statement."""
    from pecos_amd import clib
    from pecos_amd.core import ClusteringParam
    compact, depth, kw = cr.wide_ids(), cr.WIDE_IDS_DEPTH, cr.WIDE_IDS_KW
    t = cr.statement(compact, depth, nnz=0, **kw)
    assert all(t["first_touch"])
    other = cr.statement(compact, depth, nnz=0, variant="ascending_norm", **kw)
    assert not np.array_equal(t["codes"], other["codes"]), "the norm order changes no code: the case pins no order"
    assert np.array_equal(t["codes"], EDGES_RECORDED["wide_ids_2p24__csr"])
    if HAVE_REF:
        assert np.array_equal(cr.reference(cr.wide_ids(1 << 24), depth, **kw), t["codes"])
    wide = cr.wide_ids(0xFFFFFFFF)
    assert wide.shape == (600, 0xFFFFFFFF) and wide.indices.max() == 0xFFFFFFFE and wide.indices.min() == 0
    assert np.array_equal(np.argsort(wide.indices, kind="stable"), np.argsort(compact.indices, kind="stable")), "the renumbering is not increasing"
    plan = clib.debug_cluster_plan(wide.shape[0], wide.shape[1], wide.nnz, depth, ClusteringParam(partition_algo=cr.SKMEANS, seed=kw["seed"], kmeans_max_iter=20, threads=1,
                                                                                                  max_sample_rate=1.0, min_sample_rate=1.0, warmup_ratio=1.0))
    assert plan["level_info"][:, 1].astype(bool).tolist() == [True] * depth
    assert np.array_equal(plan["node_seed"], t["node_seed"])


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
