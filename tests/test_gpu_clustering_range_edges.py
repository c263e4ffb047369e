"""Label clustering on the device (K11) where norms, centres and scores leave fp32's range: the cases of clustering_rule.range_edge_cases()
(finite inputs; no NaN in any centre or score of any iteration, which tests/test_clustering_cpu.py checks on the statement's trace) through
c_run_clustering_csr_f32, c_run_clustering_drm_f32 and the resident form.  Codes against the numpy statement and the recorded reference
(tests/golden/clustering_range_edges.npz), scores against the statement bit for bit, +-inf and zeros included, iterations per level from
the form counters.  And the widest column ids: a matrix of 2^32 - 1 columns with the top id present, against the statement on its compact
renumbering."""
import os

import numpy as np
import pytest

import clustering_rule as cr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = cr.range_edge_cases()
RECORDED = np.load(os.path.join(GOLDEN, "clustering_range_edges.npz"))
HAVE_REF = os.path.exists(cr.REF)
_truth = {}


def truth(name, dense=False):
    """The statement's answer for a case, computed once."""
    key = (name, dense)
    if key not in _truth:
        X, depth, kw = CASES[name]
        _truth[key] = cr.statement(cr.as_full_csr(X.toarray()) if dense else X, depth, **kw)
    return _truth[key]


def check_codes(name, form, got, err, X, depth, kw):
    assert err is None, err
    want = truth(name, form == "drm")["codes"]
    assert np.array_equal(got, want), f"{name} ({form}): codes differ from the statement at elements {np.flatnonzero(got != want)[:8]}: " \
                                      f"got {got[got != want][:8]}, wanted {want[got != want][:8]}"
    assert np.array_equal(got, RECORDED[f"{name}__{form}"]), f"{name} ({form}): codes differ from the recorded reference"
    if HAVE_REF:
        assert np.array_equal(got, cr.reference(X, depth, **kw)), f"{name} ({form}): codes differ from the live reference"


@pytest.mark.parametrize("name", sorted(CASES))
def test_csr_entry_point(name):
    X, depth, kw = CASES[name]
    got, err = cr.run_library(cr.OURS, X, depth, **kw)
    check_codes(name, "csr", got, err, X, depth, kw)


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if cr.dense_ok(c[0])))
def test_drm_entry_point(name):
    X, depth, kw = CASES[name]
    D = np.ascontiguousarray(X.toarray())
    got, err = cr.run_library(cr.OURS, D, depth, **kw)
    check_codes(name, "drm", got, err, D, depth, kw)


def device_kw(kw):
    return dict(partition_algo=kw.get("algo", cr.SKMEANS), seed=kw.get("seed", 0), kmeans_max_iter=kw.get("max_iter", 20),
                max_sample_rate=kw.get("max_rate", 1.0), min_sample_rate=kw.get("min_rate", 1.0), warmup_ratio=kw.get("warmup", 1.0))


def check_resident(name, X, depth, kw, t, recorded):
    import pecos_amd
    from pecos_amd import clib
    codes, scores = pecos_amd.run_clustering_device(X, depth, return_scores=True, **device_kw(kw))
    codes, scores = codes.cpu().numpy().view(np.uint32), scores.cpu().numpy()
    forms = clib.debug_cluster_forms()
    bad = np.argwhere(scores.view(np.uint32) != t["scores"].view(np.uint32))
    where = f"first at (level, element) {tuple(bad[0])}: got {scores[tuple(bad[0])]!r}, wanted {t['scores'][tuple(bad[0])]!r}" if len(bad) else ""
    print(f"{name}: {int((codes != t['codes']).sum())} codes and {len(bad)} scores differ from the statement; iterations {forms['iters']}  {where}")
    assert np.array_equal(codes, t["codes"]), f"{name}: {int((codes != t['codes']).sum())} codes differ from the statement"
    if recorded is not None:
        assert np.array_equal(codes, recorded), f"{name}: codes differ from the recorded reference"
    assert len(bad) == 0, f"{name}: {len(bad)} scores differ from the statement, {where}"
    want_iters = [max(k for nid, k in t["iters"].items() if nid.bit_length() - 1 == d) for d in range(depth)]
    assert forms["iters"] == want_iters, f"{name}: iterations per level {forms['iters']}, the statement's nodes need {want_iters}"
    want = t["first_touch"].index(True) if True in t["first_touch"] else None
    assert forms["switch_level"] == (want if kw.get("algo", cr.SKMEANS) == cr.SKMEANS else None)


@pytest.mark.parametrize("name", sorted(CASES))
def test_resident_form(name):
    X, depth, kw = CASES[name]
    check_resident(name, X, depth, kw, truth(name), RECORDED[f"{name}__csr"])


def test_hierarchical_kmeans_gen_on_a_collapsed_centre():
    from pecos_amd import HierarchicalKMeans
    from pecos_amd.indexer import chain_from_partial, codes_to_csc
    X, depth, kw = CASES["collapse_dense_sk"]
    p = HierarchicalKMeans.TrainParams(max_leaf_size=8, threads=1, nr_splits=4)
    assert p.infer_binary_tree_depth(X.shape[0]) == depth
    chain = HierarchicalKMeans.gen(X, train_params=p)
    want = chain_from_partial(codes_to_csc(RECORDED["collapse_dense_sk__csr"], depth), nr_splits=4)
    assert len(chain) == len(want) == 3
    for A, B in zip(chain, want):
        A, B = A.tocsc(), B.tocsc()
        A.sort_indices(); B.sort_indices()
        assert A.shape == B.shape and A.dtype == np.float32
        assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)


# ------------------------------------------------------------------------------------------------ the widest column ids
def wide_truth():
    if "wide" not in _truth:
        _truth["wide"] = cr.statement(cr.wide_ids(), cr.WIDE_IDS_DEPTH, nnz=0, **cr.WIDE_IDS_KW)
    return _truth["wide"]


def test_widest_ids_csr_entry_point():
    """cols = 2^32 - 1 with column 2^32 - 2 stored: the layout's sort reads all 64 key bits.  Neither the reference nor the statement
    can hold a centre that wide; the rule sees the ids through their order and the first-touch switch only (the CPU half shows it on the
    reference at 2^24 columns), so the answer is the statement's on the compact matrix in first-touch order from the root."""
    X = cr.wide_ids(0xFFFFFFFF)
    assert X.shape[1] == 0xFFFFFFFF and X.indices.max() == 0xFFFFFFFE
    got, err = cr.run_library(cr.OURS, X, cr.WIDE_IDS_DEPTH, **cr.WIDE_IDS_KW)
    assert err is None, err
    assert np.array_equal(got, wide_truth()["codes"]), f"{int((got != wide_truth()['codes']).sum())} codes differ from the statement"
    assert np.array_equal(got, RECORDED["wide_ids_2p24__csr"])


def test_widest_ids_resident_form():
    check_resident("wide_ids", cr.wide_ids(0xFFFFFFFF), cr.WIDE_IDS_DEPTH, cr.WIDE_IDS_KW, wide_truth(), RECORDED["wide_ids_2p24__csr"])
