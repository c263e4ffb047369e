"""CPU: the checkers themselves at the edges of the fp32 range (tests/edge_inputs.py).

For every case, every weight layout and sparse / dense X: the case's precondition holds on the reference output (so the GPU test that
reuses the case is not vacuous), and the C restatement (OracleModel) equals the compiled reference (RefModel, when oracle/_ref is built)
bit for bit.  HASH_CHUNKED x dense X is left out: the reference sums in the iteration order of its hash table there.

This file is also the canary for a host process that runs with flush-to-zero / denormals-are-zero set (a library linked with fast-math
sets MXCSR from a static constructor): in such a process the oracle itself would lie, and all_subnormal's precondition fails here first.
"""
import numpy as np
import pytest
import scipy.sparse as smat

import edge_inputs as E


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    root = tmp_path_factory.mktemp("edges")
    made = {}

    def get(model):
        if model not in made:
            made[model] = E.build_model(model, str(root / model))
        return made[model]
    return get


def test_host_process_keeps_denormals():
    tiny = E.FLT_MIN                      # 2^-126: a quarter of it is an exact subnormal
    assert np.float32(tiny * np.float32(0.25)) != 0 and np.float32(tiny * np.float32(0.25)) * np.float32(4.0) == tiny
    a = np.full(64, 3e-39, np.float32)
    assert np.all(a + a == np.float32(2.0) * a) and float(np.sum(a, dtype=np.float32)) > 0.0
    P = smat.csr_matrix((np.array([3e-39, 0.0, -0.0, 1.0, np.inf, np.nan], np.float32), np.arange(6), np.array([0, 6])), shape=(1, 6))
    assert E.describe(P) == dict(n=6, subnormal=1, zero=2, neg_zero=1, normal=1, inf=1, nan=1)


@pytest.mark.parametrize("layout", E.LAYOUTS)
@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_reference_at_the_edges(case, layout, folders, oracle_mod):
    folder = folders(case.model)
    have_ref = oracle_mod.ref_available()
    ref = oracle_mod.RefModel(folder, layout) if have_ref else None
    orc = oracle_mod.OracleModel.load(folder, "HASH_CHUNKED" if layout == "HASH_CHUNKED" else "BINARY_SEARCH_CHUNKED")
    X = case.queries()
    kw = E.case_kw(case)
    checked = 0
    for Xq, xk in ((X, "sparse"), (E.dense_of(X), "dense")):
        if xk == "dense" and (not case.dense or layout == "HASH_CHUNKED"):
            continue
        what = f"{layout} {xk} X"
        want = ref.predict(Xq, **kw) if have_ref else None
        if want is not None:
            E.check_precondition(case, want, what + " (compiled reference)")
            checked += 1
        if layout == "CSC":
            # the restatement has the CSC arithmetic (bias first, dot product summed separately) on a given output pattern only: re-score the
            # reference's own pattern
            if want is None:
                continue
            S = smat.csr_matrix((want.data, want.indices, want.indptr), shape=want.shape)
            got = orc.predict_on_selected_outputs(Xq, S, case.pp)       # (rows come back in the route's own order: compare label by label)
            assert np.array_equal(got.indptr, want.indptr), what
            rows = np.repeat(np.arange(want.shape[0]), np.diff(want.indptr))
            og, ow = np.lexsort((got.indices, rows)), np.lexsort((want.indices, rows))
            assert np.array_equal(got.indices[og], want.indices[ow]), what
            assert np.array_equal(got.data[og].view(np.uint32), want.data[ow].view(np.uint32)), f"{case.name} {what}: restatement (CSC route) != compiled reference"
            continue
        got = orc.predict(Xq, **kw)
        E.check_precondition(case, got, what + " (C restatement)")
        checked += 1
        if want is not None:
            assert got.shape == want.shape and np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), \
                f"{case.name} {what}: restatement and compiled reference return different labels / order"
            assert np.array_equal(got.data.view(np.uint32), want.data.view(np.uint32)), f"{case.name} {what}: scores not bit-identical"
    assert checked > 0 or (layout == "CSC" and not have_ref)
