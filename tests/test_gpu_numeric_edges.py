"""GPU (-m gpu): parity at the edges of the fp32 range.  Every case of tests/edge_inputs.py (subnormal products and accumulators, sums
that cross FLT_MIN, scores that underflow down the tree, signed zeros, products that round to zero, overflow to +inf) runs through every
row of FAMILIES -- one row per kernel family / launch shape an option can select -- against the compiled reference (oracle/_ref) when it
is built, else the C restatement.  The case's precondition is asserted on the reference output first: a case that no longer produces what
it is named for fails, it is never skipped.

noop and the hinge family: label ids, order and fp32 bits identical (the sign of a zero included).  sigmoid / log-sigmoid: every family
is bit-identical to the first family of its (layout, sparse / dense X) group, and that one is within assert_topk_ulps' derived bound of the
reference.  A kernel that flushes subnormals to zero, rounds a double -> float conversion into the subnormal range differently, orders
subnormal keys wrongly in a top-k or breaks ties of exact zeros by anything but candidate position fails here.
"""
import os
from collections import namedtuple

import numpy as np
import pytest
import scipy.sparse as smat

import edge_inputs as E
from conftest import assert_same_topk

pytestmark = pytest.mark.gpu

Family = namedtuple("Family", "name opts fuse01 xkind layout")

OPTION_DEFAULTS = dict(dense_layers=1, presence=1, qsort=1, qsort_min_rows=131072, qsort_min_parents=64, tile_rows=1, leaf_fuse=1, adaptive=1,
                       k1_group=0, sort_min_tiles=0, k2_big_min_k=0, prune=1, k1g_min_items=16, k1g_variant=0)
BSC = "BINARY_SEARCH_CHUNKED"


def _families():
    base = [("defaults", {}, None), ("dense_layers=2", dict(dense_layers=2), None),
            ("XRL_K1Q_FUSE01=0", {}, "0"), ("XRL_K1Q_FUSE01=1", {}, "1"),                       # (unset: every other row)
            ("presence=0", dict(presence=0), None), ("presence=2", dict(presence=2), None),
            ("sorted launch", dict(qsort=1, qsort_min_rows=1, qsort_min_parents=2), None)]
    for tr in (0, 2):
        for lf in (0, 1):
            base.append((f"tile format tile_rows={tr} leaf_fuse={lf}", dict(dense_layers=0, tile_rows=tr, leaf_fuse=lf, adaptive=0), None))
    for g in (1, 64):
        base.append((f"tile format k1_group={g}", dict(dense_layers=0, tile_rows=0, k1_group=g), None))
    base.append(("tile format sort_min_tiles=1", dict(dense_layers=0, sort_min_tiles=1), None))
    base.append(("tile format k2_big_min_k=1", dict(dense_layers=0, k2_big_min_k=1), None))
    fams = []
    for name, opts, fuse in base:                                    # exact bound pruning on / off on each of them
        for pr in (1, 0):
            fams.append(Family(f"{name} prune={pr}", dict(opts, prune=pr), fuse, "sparse", BSC))
    for name, opts in (("dense X", {}), ("dense X k1g_min_items=1 k1g_variant=0", dict(k1g_min_items=1, k1g_variant=0)),
                       ("dense X k1g_min_items=1 k1g_variant=1", dict(k1g_min_items=1, k1g_variant=1)), ("dense X k1g_min_items=0", dict(k1g_min_items=0)),
                       ("dense X tile format", dict(dense_layers=0))):
        for pr in (1, 0):
            fams.append(Family(f"{name} prune={pr}", dict(opts, prune=pr), None, "dense", BSC))
    fams.append(Family("CSC (K1C)", {}, None, "sparse", "CSC"))
    fams.append(Family("CSC (K1C) dense X", {}, None, "dense", "CSC"))
    for dl in (1, 0):
        fams.append(Family(f"HASH_CHUNKED dense_layers={dl}", dict(dense_layers=dl), None, "sparse", "HASH_CHUNKED"))
    return fams


FAMILIES = _families()


def _ordered(v):
    """fp32 bit patterns as integers that count units in the last place across the whole line: -x -> -(bits of x); -0.0 and +0.0 both 0."""
    i = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulp_bound(depth):
    return 3 * depth + 1


def assert_topk_ulps(got, want, depth, what=""):
    """sigmoid / log-sigmoid against the reference, distance measured in units in the last place of the fp32 bit patterns (so that it means
    the same for a subnormal score as for one near 1; no absolute slack).

    The bound is derived, not tuned: DESIGN.md documents the device's expf within 1 ulp of glibc's; e = expf(-v) enters 1 / (1 + e) (or
    -log(1 + e)) in double and the result is cast to float -- the 1-ulp difference of e moves the double result by at most that much relative,
    and the cast may round it the other way: <= 2 ulps of the transformed score per layer.  The combine with the parent's score (a product
    for sigmoid, a sum for log-sigmoid) carries the parent's error over (relative error adds under a product; under a sum of same-signed
    terms it does not grow) and adds one rounding of its own: <= 3 ulps per layer.  One more for a rounding that lands on the other side of
    a binade boundary, where an ulp halves.  Hence 3 * depth + 1.

    Same row lengths; the i-th scores within the bound; a label both sides return within the bound; a label only one side returns must be a
    near-tie of the k-th score: its score (the reference's where the reference returned it) within the bound of the reference's k-th.
    Returns the largest distance seen."""
    bound = ulp_bound(depth)
    assert got.shape == want.shape and np.array_equal(got.indptr, want.indptr), f"{what}: shapes / row lengths differ"
    worst = 0
    for r in range(want.shape[0]):
        lo, hi = want.indptr[r], want.indptr[r + 1]
        if hi == lo:
            continue
        ig, iw = got.indices[lo:hi], want.indices[lo:hi]
        og, ow = _ordered(got.data[lo:hi]), _ordered(want.data[lo:hi])
        d = int(np.max(np.abs(og - ow)))
        worst = max(worst, d)
        assert d <= bound, f"{what}: row {r}: i-th scores differ by {d} ulps (bound {bound})"
        dg, dw = dict(zip(ig.tolist(), og.tolist())), dict(zip(iw.tolist(), ow.tolist()))
        for lab in set(dg) | set(dw):
            if lab in dg and lab in dw:
                d = abs(dg[lab] - dw[lab])
            else:
                d = abs((dw[lab] if lab in dw else dg[lab]) - int(ow[-1]))
            worst = max(worst, d)
            assert d <= bound, f"{what}: row {r} label {lab}: {d} ulps (bound {bound}; one side only: {not (lab in dg and lab in dw)})"
    return worst


@pytest.fixture(scope="module")
def clib():
    from pecos_amd import clib
    assert clib.device_count() > 0, "no GPU visible"
    return clib


@pytest.fixture(scope="module")
def handles(tmp_path_factory, clib):
    """(model name, layout) -> (folder, XLinearModel); only the current model's handles are kept alive (every handle reserves pinned staging)."""
    from pecos_amd import XLinearModel
    root = tmp_path_factory.mktemp("edges")
    state = {"model": None, "folder": None, "h": {}}

    def get(model, layout):
        if state["model"] != model:
            state["h"].clear()
            state["model"], state["folder"] = model, E.build_model(model, str(root / model))
        if layout not in state["h"]:
            state["h"][layout] = XLinearModel.load(state["folder"], weight_matrix_type=layout)
        return state["folder"], state["h"][layout]
    return get


class _Applied:
    """Options of a FAMILIES row set on a handle, restored on exit."""

    def __init__(self, clib, h, fam):
        self.clib, self.h, self.fam = clib, h, fam

    def __enter__(self):
        for o, v in self.fam.opts.items():
            self.clib.set_option(self.h, o, v)
        if self.fam.fuse01 is not None:
            os.environ["XRL_K1Q_FUSE01"] = self.fam.fuse01

    def __exit__(self, *exc):
        os.environ.pop("XRL_K1Q_FUSE01", None)
        for o in self.fam.opts:
            self.clib.set_option(self.h, o, OPTION_DEFAULTS[o])


def _rescore_csc(orc, Xq, got, pp):
    """No whole-model CSC reference here (oracle/_ref not built): the restatement's CSC route re-scores the pattern the library returned."""
    S = smat.csr_matrix((got.data, got.indices, got.indptr), shape=got.shape)
    re = orc.predict_on_selected_outputs(Xq, S, pp)
    rows = np.repeat(np.arange(got.shape[0]), np.diff(got.indptr))
    og, orr = np.lexsort((got.indices, rows)), np.lexsort((re.indices, rows))
    assert np.array_equal(got.indices[og], re.indices[orr])
    return got.data[og], re.data[orr]


@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_edge_case_through_every_family(case, handles, clib, oracle_mod):
    X = case.queries()
    Xs = {"sparse": X, "dense": E.dense_of(X)}
    kw = E.case_kw(case)
    depth = E.model_depth(case.model)
    refs, wants, first, worst, ran = {}, {}, {}, 0, 0
    for fam in FAMILIES:
        if fam.xkind == "dense" and not case.dense:
            continue
        folder, m = handles(case.model, fam.layout)
        h = m.model.model_chain
        Xq = Xs[fam.xkind]
        key = (fam.layout, fam.xkind)
        if key not in wants:
            if fam.layout not in refs:
                refs[fam.layout] = E.CpuReference(oracle_mod, folder, fam.layout)
            wants[key] = refs[fam.layout].predict(Xq, **kw)
            if wants[key] is not None:
                E.check_precondition(case, wants[key], f"{fam.layout} {fam.xkind} X")
        want = wants[key]
        what = f"{case.name} [{fam.name}]"
        with _Applied(clib, h, fam):
            got = m.predict(Xq, **kw)
        ran += 1
        if want is None:
            a, b = _rescore_csc(refs[fam.layout].orc, Xq, got, case.pp)
            if E.is_sigmoid(case):
                d = int(np.max(np.abs(_ordered(a) - _ordered(b)))); worst = max(worst, d)
                assert d <= ulp_bound(depth), f"{what}: {d} ulps from the restated CSC route"
            else:
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: scores differ from the restated CSC route"
        elif not E.is_sigmoid(case):
            assert_same_topk(got, want, exact_scores=True, what=what)
        elif key not in first:
            first[key] = got
            worst = max(worst, assert_topk_ulps(got, want, depth, what))
        else:
            assert_same_topk(got, first[key], exact_scores=True, what=what + " vs the group's first family")
    assert ran == len(FAMILIES) - (0 if case.dense else sum(f.xkind == "dense" for f in FAMILIES))
    if E.is_sigmoid(case):
        print(f"\nULPS {case.name}: worst distance from the reference {worst} (bound {ulp_bound(depth)})")


# ---------------------------------------------------------------------------------------------
# the other entry points on the same data
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,pps", [("all_subnormal", ("noop",)), ("underflow3", ("sigmoid", "l1-hinge", "l3-hinge", "log-l6-hinge"))])
def test_single_layer_predict_at_the_edges(model, pps, handles, clib, oracle_mod):
    from pecos_amd.core import ScipyCompressedSparseAllocator
    folder, _ = handles(model, BSC)
    layers = oracle_mod.load_model_folder(folder)
    X = E._base_queries()
    have_ref = oracle_mod.ref_available()

    def ours(Xq, codes, L, pp, k):
        alloc = ScipyCompressedSparseAllocator()
        clib.xlinear_single_layer_predict(Xq, codes, L["W"], L["C"], pp, k, -1, L["bias"], alloc)
        return alloc.get()

    clib.single_layer_cache_clear()
    seen = dict(n=0, subnormal=0, zero=0)
    for Xq in (X, E.dense_of(X)):
        for pp in pps:
            codes, worst = None, 0
            for l, k in enumerate((5, 10, 20)):
                P = ours(Xq, codes, layers[l], pp, k)
                what = f"{model} single layer {l} {pp} dense={not smat.issparse(Xq)}"
                if have_ref:
                    R = oracle_mod.ref_single_layer_predict(Xq, codes, layers[l]["W"], layers[l]["C"], pp, k, layers[l]["bias"])
                    if "sigmoid" in pp:
                        worst = max(worst, assert_topk_ulps(P, R, 1, what))       # (both sides start from the same codes: one layer's error)
                    else:
                        assert_same_topk(P, R, exact_scores=True, what=what)
                elif l == 0:   # the restatement's CSC route on the returned pattern (one layer, no codes)
                    a, b = _rescore_csc(oracle_mod.OracleModel(layers[:1]), Xq, P, pp)
                    if "sigmoid" in pp:
                        assert int(np.max(np.abs(_ordered(a) - _ordered(b)))) <= ulp_bound(1), what
                    else:
                        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what
                s = E.describe(R if have_ref else P)
                for f in seen:
                    seen[f] += s[f]
                codes = smat.csr_matrix(P, dtype=np.float32)
            if "sigmoid" in pp and have_ref:
                print(f"\nULPS single layer {model} {pp}: worst {worst}")
    clib.single_layer_cache_clear()
    # the entry point did see the range this test is about (CPU reference: all_subnormal 1729 of 1750 per X kind, underflow3 851 subnormal + 596 zero of 7000)
    assert seen["subnormal"] >= 0.05 * seen["n"], seen


@pytest.mark.parametrize("model,pps", [("all_subnormal", ("noop",)), ("underflow3", ("sigmoid", "l1-hinge", "l3-hinge", "log-sigmoid"))])
def test_selected_outputs_at_the_edges(model, pps, handles, clib, oracle_mod):
    folder, m = handles(model, BSC)
    X = E._base_queries()
    om = oracle_mod.OracleModel.load(folder)
    rm = oracle_mod.RefModel(folder, "CSC") if oracle_mod.ref_available() else None
    S = om.predict(X, beam_size=6, only_topk=8, post_processor="noop")
    S = smat.csr_matrix((np.ones_like(S.data), S.indices, S.indptr), shape=(S.shape[0], m.nr_pred_cols))
    seen = dict(n=0, subnormal=0, zero=0)
    for pp in pps:
        for Xq in (X, E.dense_of(X)):
            got = m.predict(Xq, selected_outputs_csr=S, post_processor=pp)
            for ref, name in ((om, "restatement"), (rm, "compiled reference")):
                if ref is None:
                    continue
                want = ref.predict_on_selected_outputs(Xq, S, pp)
                what = f"{model} selected outputs {pp} dense={not smat.issparse(Xq)} vs {name}"
                if "sigmoid" in pp:
                    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), what
                    d = int(np.max(np.abs(_ordered(got.data) - _ordered(want.data))))
                    assert d <= ulp_bound(3), f"{what}: {d} ulps"
                else:
                    assert_same_topk(got, want, exact_scores=True, what=what)
            s = E.describe(om.predict_on_selected_outputs(Xq, S, pp))
            for f in seen:
                seen[f] += s[f]
    assert seen["subnormal"] >= 0.05 * seen["n"], seen       # (restatement: all_subnormal 390 of 400, underflow3 160 subnormal + 765 zero of 1600, per X kind)


def test_sparse_inner_products_subnormal(clib, oracle_mod):
    # values scaled so that every product (~1e-19 x 1e-20) and every sum is subnormal: four layouts, bit for bit
    rng = np.random.default_rng(5)
    A = smat.random(200, 500, density=0.05, format="csr", dtype=np.float32, random_state=6); A.sort_indices()
    B = smat.random(500, 300, density=0.08, format="csc", dtype=np.float32, random_state=7); B.sort_indices()
    A.data = ((A.data - 0.5) * np.float32(1e-19)).astype(np.float32)
    B.data = ((B.data + 0.1) * np.float32(1e-20)).astype(np.float32)
    rr = rng.integers(0, 200, 5000).astype(np.uint32); cc = rng.integers(0, 300, 5000).astype(np.uint32)
    for Aq, Bq in [(A, B), (np.ascontiguousarray(A.toarray()), B), (A, np.asfortranarray(B.toarray())),
                   (np.ascontiguousarray(A.toarray()), np.asfortranarray(B.toarray()))]:
        exp = oracle_mod.sparse_inner_products(Aq, Bq, rr, cc)
        a = np.abs(exp)
        assert np.sum((a > 0) & (a < E.FLT_MIN)) >= 0.5 * len(exp) and np.all(a < E.FLT_MIN), "precondition: subnormal inner products"
        got = clib.sparse_inner_products(Aq, Bq, rr, cc)
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
        if oracle_mod.ref_available():
            assert np.array_equal(got.view(np.uint32), oracle_mod.ref_sparse_inner_products(Aq, Bq, rr, cc).view(np.uint32))
