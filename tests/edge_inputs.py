"""Inputs at the edges of the fp32 range, shared by test_numeric_edges_cpu.py and test_gpu_numeric_edges.py (a plain helper module).

Every generator builds on xrl_synth.make_model / make_queries and then rewrites the weights (and sometimes the query values) so that
products, accumulators or final scores leave fp32's comfortable middle: subnormal products and sums, sums that cross FLT_MIN in both
directions, scores that underflow gradually down the tree, signed zeros, products that round to zero, overflow to +inf.

A case names a MODEL (built once per folder by build_model), a query matrix (queries), predict keywords, and a PRECONDITION on the
reference's output: what the case is there to produce.  The precondition is asserted before any kernel is consulted, so a case can not
go vacuous (a generator change that moves the scores back to the normal range fails the test instead of passing it).

Scales recorded here were tuned on the CPU reference (oracle/_ref and OracleModel agree bit for bit on every case):
  all_subnormal    weights x 3e-39                  -> 980 of 1000 returned scores subnormal
  cross_flt_min    weights x 2e-39, x values x 10^U(-1.5, 1.5) per entry -> 522 of 1000 subnormal (5e-39: 185, 1e-38: 7, 2e-38: 0)
  score_underflow  weights -25 |w|                  -> sigmoid / l1-hinge products underflow through the subnormals to 0 down the tree:
                   3 layers: sigmoid 278 subnormal / 194 zero / 528 normal, l1-hinge 284 / 249 / 467; 4 layers (12 weights per column on every
                   level -- with the 3-layer tree's 60 / 40 per column four products leave < 10 % normal): sigmoid 276 / 211 / 513, l1-hinge 260 / 271 / 469
"""
import os
from collections import namedtuple

import numpy as np
import scipy.sparse as smat

import xrl_synth

FLT_MIN = np.float32(1.17549435e-38)
D = 120
BEAM, TOPK = 10, 20
CROSS_SCALE = 2e-39          # cross_flt_min: tuned on the CPU reference until 20 % .. 80 % of the returned scores are subnormal
LAYOUTS = ("BINARY_SEARCH_CHUNKED", "HASH_CHUNKED", "CSC")

# model name -> (make_model arguments, weight rewrite).  "base" is the 3-layer tree of test_bound_pruning_with_massive_ties.
_TREES = {
    3: dict(L=700, w_nnz=[60, 40, 12], seed=41, shape=[5, 40, 700]),
    4: dict(L=700, w_nnz=[12, 12, 12, 12], seed=41, shape=[4, 16, 96, 700]),
    "guard": dict(L=700, w_nnz=[60, 40, 12], seed=51, shape=[5, 40, 700]),    # the tree of test_bound_pruning_guard_nonfinite
}


def _rewrite(folder, depth, fn):
    for d in range(depth):
        f = os.path.join(folder, "ranker", f"{d}.model", "W.npz")
        W = smat.load_npz(f).tocsc().astype(np.float32)
        fn(W, d)
        smat.save_npz(f, W, compressed=False)


def _w_all_subnormal(W, d):
    W.data *= np.float32(3e-39)


def _w_cross(W, d):
    W.data *= np.float32(CROSS_SCALE)


def _w_underflow(W, d):
    W.data[:] = np.float32(-25.0) * np.abs(W.data)


def _w_neg_zero_half(W, d):
    W.data[::2] = np.float32(-0.0)


def _w_neg_zero_all(W, d):
    W.data[:] = np.float32(-0.0)


def _w_tiny_negative(W, d):
    W.data[:] = np.float32(-1e-30)


def _w_positive(W, d):
    W.data[:] = np.abs(W.data) + np.float32(0.01)


def _w_inf(W, d):
    _w_positive(W, d)
    if d >= 1:
        W.data[np.random.default_rng(11 + d).integers(0, len(W.data), 6)] = np.inf


MODELS = {
    "all_subnormal": (3, _w_all_subnormal),
    "cross_flt_min": (3, _w_cross),
    "underflow3": (3, _w_underflow),
    "underflow4": (4, _w_underflow),
    "neg_zero_half": (3, _w_neg_zero_half),
    "neg_zero_all": (3, _w_neg_zero_all),
    "tiny_negative": (3, _w_tiny_negative),
    "positive": ("guard", _w_positive),
    "w_inf": ("guard", _w_inf),
}


def model_depth(model):
    return len(_TREES[MODELS[model][0]]["shape"])


def build_model(model, folder):
    """Write the named model into `folder`; returns the folder."""
    tree, fn = MODELS[model]
    t = _TREES[tree]
    xrl_synth.make_model(folder, D, t["L"], t["w_nnz"], seed=t["seed"], shape=t["shape"], permute_leaf=True)
    _rewrite(folder, len(t["shape"]), fn)
    return folder


def _base_queries():
    return xrl_synth.make_queries(50, D, 12, seed=43, relabel_seed=41).tocsr()


def _q_plain():
    return _base_queries()


def _q_wide():        # x values spread over three decades, so that a sum's partial sums move across FLT_MIN in both directions (weights have both signs)
    X = _base_queries()
    X.data = (X.data * (10.0 ** np.random.default_rng(47).uniform(-1.5, 1.5, len(X.data)))).astype(np.float32)
    return X


def _q_half_negative():
    X = _base_queries()
    X.data[::2] *= np.float32(-1.0)
    return X


def _q_tiny():
    X = _base_queries()
    X.data = (X.data * np.float32(1e-20)).astype(np.float32)
    return X


def _guard_queries():
    X = xrl_synth.make_queries(64, D, 14, seed=53, relabel_seed=51).tocsr()
    X.data = np.abs(X.data)
    return X


def _q_guard():
    return _guard_queries()


def _q_huge():        # products overflow to +inf (weights are positive: no inf - inf)
    X = _guard_queries()
    rng = np.random.default_rng(11)
    for r in range(0, 64, 3):
        lo, hi = X.indptr[r], X.indptr[r + 1]
        if hi > lo:
            X.data[lo + int(rng.integers(0, hi - lo))] = [3.0e38, np.inf, 1.0e30][(r // 3) % 3]
    return X


def describe(P):
    """Counts over the returned scores of a prediction (CSR): how many are subnormal, exactly zero, negative zero, normal, inf, NaN."""
    v = np.asarray(P.data, dtype=np.float32)
    a = np.abs(v)
    zero = v == 0
    return dict(n=int(v.size), subnormal=int(np.sum((a > 0) & (a < FLT_MIN))), zero=int(np.sum(zero)),
                neg_zero=int(np.sum(zero & np.signbit(v))), normal=int(np.sum((a >= FLT_MIN) & np.isfinite(v))),
                inf=int(np.sum(np.isinf(v))), nan=int(np.sum(np.isnan(v))))


# preconditions: describe(P) -> bool
def _pre_mostly_subnormal(s): return s["n"] > 0 and s["subnormal"] >= 0.9 * s["n"]
def _pre_crossing(s): return s["n"] > 0 and 0.2 * s["n"] <= s["subnormal"] <= 0.8 * s["n"]
def _pre_three_ways(s): return s["n"] > 0 and min(s["subnormal"], s["zero"], s["normal"]) >= 0.1 * s["n"]
def _pre_all_zero(s): return s["n"] > 0 and s["zero"] == s["n"]
def _pre_finite(s): return s["n"] > 0 and s["inf"] == 0 and s["nan"] == 0
def _pre_all_pos_zero(s): return s["n"] > 0 and s["zero"] == s["n"] and s["neg_zero"] == 0
def _pre_no_neg_zero(s): return s["n"] > 0 and s["neg_zero"] == 0 and s["zero"] < s["n"]
def _pre_some_zero(s): return s["n"] > 0 and s["zero"] >= 0.05 * s["n"] and s["neg_zero"] == 0
def _pre_inf_no_nan(s): return s["inf"] >= 1 and s["nan"] == 0


_PRE_TEXT = {
    _pre_mostly_subnormal: ">= 90 % subnormal", _pre_crossing: "20 % .. 80 % subnormal",
    _pre_three_ways: ">= 10 % each of subnormal, exact zero and normal", _pre_all_zero: "100 % exact zeros", _pre_finite: "all finite",
    _pre_all_pos_zero: "every score +0.0, no sign bit", _pre_no_neg_zero: "no negative zero, not all zero",
    _pre_some_zero: ">= 5 % exact zeros, none negative", _pre_inf_no_nan: ">= 1 inf, 0 NaN",
}

# dense: whether a dense copy of X may be compared with the reference too (w_inf: dense X multiplies every chunk row, 0 * inf is a NaN whose place in the
# reference's std::sort is not a defined order -- as in test_bound_pruning_guard_nonfinite)
Case = namedtuple("Case", "name model queries pp pre dense")

CASES = [
    Case("all_subnormal", "all_subnormal", _q_plain, "noop", _pre_mostly_subnormal, True),
    Case("cross_flt_min", "cross_flt_min", _q_wide, "noop", _pre_crossing, True),
]
for _depth in (3, 4):
    for _pp, _pre in (("sigmoid", _pre_three_ways), ("l1-hinge", _pre_three_ways), ("l2-hinge", _pre_all_zero), ("l3-hinge", _pre_all_zero),
                      ("l5-hinge", _pre_all_zero), ("log-sigmoid", _pre_finite), ("log-l6-hinge", _pre_finite)):
        CASES.append(Case(f"score_underflow-{_depth}-{_pp}", f"underflow{_depth}", _q_plain, _pp, _pre, True))
CASES += [
    Case("neg_zero_weights-half", "neg_zero_half", _q_half_negative, "noop", _pre_no_neg_zero, True),
    Case("neg_zero_weights-all", "neg_zero_all", _q_half_negative, "noop", _pre_all_pos_zero, True),
    Case("product_to_zero", "tiny_negative", _q_tiny, "noop", _pre_some_zero, True),
    Case("overflow_no_nan-x_huge", "positive", _q_huge, "noop", _pre_inf_no_nan, True),
    Case("overflow_no_nan-w_inf", "w_inf", _q_guard, "noop", _pre_inf_no_nan, False),
]
CASE_IDS = [c.name for c in CASES]


def case_kw(case):
    return dict(beam_size=BEAM, only_topk=TOPK, post_processor=case.pp)


def is_sigmoid(case):
    return "sigmoid" in case.pp


def check_precondition(case, P, what=""):
    s = describe(P)
    assert case.pre(s), f"{case.name} {what}: precondition '{_PRE_TEXT[case.pre]}' does not hold on the reference output: {s}"
    return s


def dense_of(X):
    return np.ascontiguousarray(X.toarray())


class CpuReference:
    """The checker of one model folder in one layout: RefModel (the compiled reference) when oracle/_ref is built, else the C restatement.
    The restatement has no whole-model CSC arithmetic; for that layout it re-scores a given output pattern (predict_on_selected_outputs is the
    CSC route) -- see selected()."""

    def __init__(self, oracle_mod, folder, layout):
        self.layout = layout
        self.ref = oracle_mod.RefModel(folder, layout) if oracle_mod.ref_available() else None
        self.orc = oracle_mod.OracleModel.load(folder, layout if layout != "CSC" else "BINARY_SEARCH_CHUNKED")

    def predict(self, X, **kw):
        """None when this layout has no whole-model reference here (CSC without oracle/_ref)."""
        if self.ref is not None:
            return self.ref.predict(X, **kw)
        return None if self.layout == "CSC" else self.orc.predict(X, **kw)
