"""Ranker training (K13) at its edges, the half that needs no GPU: the numpy statement of the rule on ranker_training_rule.edge_cases()
-- non-finite, huge, tiny and zero values of X, QD == 0, relevance values away from ordinary costs, row ids stored twice in a column of Y
or M, solver parameters away from ordinary positive numbers -- against the compiled reference as recorded in
tests/golden/ranker_training_edges_ref.npz and, where oracle/_ref is built, live at 1 and 8 threads, bit for bit; what the cases claim to
meet, from the statement's own trace; the wrong variants."""
import os

import numpy as np
import pytest

import ranker_training_rule as rr
from conftest import GOLDEN

CASES = rr.edge_cases()
RECORDED = np.load(os.path.join(GOLDEN, "ranker_training_edges_ref.npz"))
HAVE_REF = os.path.exists(rr.REF)
_truth = {}


def truth(name):
    if name not in _truth:
        X, Y, C, M, R, kw = CASES[name]
        _truth[name] = rr.statement(X, Y, C, M, R, **kw)
    return _truth[name]


def recorded(name):
    return RECORDED[f"case__{name}__rows"].astype(np.uint64), RECORDED[f"case__{name}__cols"].astype(np.uint64), RECORDED[f"case__{name}__vals"]


def test_the_cases_keep_the_sizes_of_the_plain_python_statement():
    assert set(f"case__{n}__vals" for n in CASES) == set(k for k in RECORDED.files if k.endswith("__vals")), "the recording and edge_cases() list the same cases"
    for name, (X, Y, C, M, R, kw) in CASES.items():
        assert X.shape[0] <= 200 and X.shape[1] <= 80 and len(rr.jobs_of(Y, C, M)) <= 8 and kw["max_iter"] <= 30, name


@pytest.mark.parametrize("name", sorted(CASES))
def test_statement_equals_the_recorded_reference(name):
    X, Y, _, _, _, kw = CASES[name]
    assert rr.same_coo(truth(name), recorded(name), canon=bool(kw.get("max_nonzeros")))
    assert tuple(RECORDED[f"case__{name}__shape"]) == (X.shape[1] + (kw.get("bias", 1.0) > 0), Y.shape[1]), "one row more exactly when bias > 0 (a NaN is not)"
    assert rr.digest(truth(name)) == str(RECORDED[f"digest8__{name}"]), "the reference at 8 threads: the same weights in another order"
    assert not np.isnan(truth(name)["vals"]).any(), "a NaN fails every threshold"


@pytest.mark.parametrize("name", sorted(CASES))
def test_statement_equals_the_live_reference_at_1_and_8_threads(name):
    if not HAVE_REF:
        pytest.skip("oracle/_ref not built")
    X, Y, C, M, R, kw = CASES[name]
    assert rr.same_coo(truth(name), rr.reference(X, Y, C, M, R, threads=1, **kw), canon=bool(kw.get("max_nonzeros")))
    assert rr.same_coo(truth(name), rr.reference(X, Y, C, M, R, threads=8, **kw), canon=True)


def test_edge_cases_cover_what_they_claim():
    """Preconditions on the statement's own trace: a case that stops meeting its edge fails here."""
    tr = lambda name: truth(name)["trace"]
    for tag in ("l1", "l2"):
        # values of X: the special value sits in a row the lanes sum (fewer than 64 entries) and in one the wavefront sums, in both of its steps
        for name in ("qnan", "snan", "pinf", "ninf", "both"):
            X = CASES[f"x_{name}_{tag}"][0]
            for r, ks in ((rr.SHORT_ROW, (1,)), (rr.LONG_ROW, (10, 66))):
                assert all(not np.isfinite(X.data[X.indptr[r] + k]) for k in ks) and (X.indptr[r + 1] - X.indptr[r] >= 64) == (r == rr.LONG_ROW)
            assert tr(f"x_{name}_{tag}")["nan_w_setup"] > 0 and tr(f"x_{name}_{tag}")["nan_g_zero"] > 0
        assert CASES[f"x_snan_{tag}"][0].data.view(np.uint32)[CASES[f"x_snan_{tag}"][0].indptr[rr.SHORT_ROW] + 1] == rr.SNAN_BITS, "the payload reaches the library"
        X = CASES[f"x_both_{tag}"][0]
        assert {np.inf, -np.inf} <= set(X.data[X.indptr[rr.LONG_ROW]:X.indptr[rr.LONG_ROW + 1]].tolist())
        X = CASES[f"x_zeros_{tag}"][0]
        z = X.data[X.indptr[rr.LONG_ROW]:X.indptr[rr.LONG_ROW + 1]]
        assert (z == 0).sum() == 3 and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all(), "explicit zeros of both signs"
        assert tr(f"x_scale1e+19_{tag}")["qd_inf"] > 0 and tr(f"x_scale1e+25_{tag}")["qd_inf"] > 0, "x'x overflows: as the chain's sum, and in a single square"
        # an alpha above FLT_MAX in fp64 stored as inf, +-inf weights emitted, a NaN gradient met in every state of alpha
        for name in (f"x_overflow_{tag}", f"x_overflow25_{tag}"):
            t = tr(name)
            assert t["t_overflow"] > 0 and t["alpha_inf"] > 0 and t["qd_subnormal"] > 0 and t["qd_inf"] > 0 and t["dot_nonfinite"] > 0, name
            assert t["nan_g_zero"] > 0 and t["nan_g_between"] > 0, name
            v = truth(name)["vals"]
            assert (v == np.inf).any() and (v == -np.inf).any(), "weights of both infinities are emitted"
        for k in (1, 3):
            t = truth(f"inf_ties_maxnz{k}_{tag}")
            assert np.isinf(t["vals"]).all() and len(t["vals"]) == k and t["trace"]["nan_w_setup"] > 0, "max_nonzeros picks among tied infinities; the NaN is never one"
            assert (t["rows"] < 12).all(), "neither the bias (|b| = inf does not exceed the least kept inf) nor the NaN feature"
        # repeated ids
        for name in ("dups", "dups_R", "dups_R0", "dups_pure_R0"):
            assert tr(f"{name}_{tag}")["dup_in_run"] >= 2 and tr(f"{name}_{tag}")["dup_across_runs"] >= 2
            assert (tr(f"{name}_{tag}")["reappends"] > 0) == name.endswith("R0")
        n_pure = [n for _, _, n in truth(f"dups_pure_R0_{tag}")["per_job"]]
        assert max(n_pure) > CASES[f"dups_pure_R0_{tag}"][0].shape[0], "a pure multi-label job lists more instances than X has rows"
        M = CASES[f"mdup_{tag}"][3]
        for k in (0, 1):
            ids = M.indices[M.indptr[k]:M.indptr[k + 1]].tolist()
            assert len(ids) > len(set(ids))
    assert tr("x_overflow_l2")["nan_g_at_c"] > 0, "alpha == C == inf under the L2 loss"
    # QD: subnormal, and 0 with an update that divides by it and is clipped at C (L1 loss, no bias)
    assert tr("x_scale1e-20_b0_l1")["qd_subnormal"] > 0 and tr("x_scale1e-20_bneg_l1")["qd_subnormal"] > 0
    for name in ("x_scale1e-23_b0_l1", "x_scale1e-30_b0_l1", "x_scale1e-40_b0_l1", "qd0_b0_l1", "qd0_bneg_l1"):
        assert tr(name)["qd0_clipped"] > 0, name
    X = CASES["qd0_b0_l1"][0]
    assert X.indptr[3] == X.indptr[2] and (X.data[X.indptr[4]:X.indptr[5]] == 0).all() and X.indptr[5] - X.indptr[4] == 5, "an empty row and an all-zero one"
    assert truth("qd0_b0_l2")["counters"]["clipped"] == 0
    # the bias row
    for v in rr.PARAM_VALUES["bias"]:
        name = [n for n in CASES if n.startswith("par_bias_") and n.endswith("_l1") and (CASES[n][5]["bias"] == v or (v != v and CASES[n][5]["bias"] != CASES[n][5]["bias"]))]
        assert len(name) == 1 and int(RECORDED[f"case__{name[0]}__shape"][0]) == 30 + (v > 0)


@pytest.mark.parametrize("variant", sorted(rr.EDGE_VARIANT_CASES))
def test_wrong_variants_differ_from_the_reference(variant):
    for name in rr.EDGE_VARIANT_CASES[variant]:
        X, Y, C, M, R, kw = CASES[name]
        assert not rr.same_coo(rr.statement(X, Y, C, M, R, variant=variant, **kw), recorded(name), canon=True), f"{variant} shows no difference on {name}"


def test_fmax_cannot_differ_from_std_max_here():
    """PGmax_new is never a NaN (it starts at -inf and std::max(PGmax_new, PG) never takes a NaN PG), and for a first argument that is no
    NaN, std::max and fmax agree: on every case that meets a NaN PG the "fmax" variant IS the rule.  What a NaN tells apart is the order
    of std::max's arguments ("nan_kept", above)."""
    met = [n for n in sorted(CASES) if truth(n)["trace"]["nan_g_between"]]
    assert met
    for name in met:
        X, Y, C, M, R, kw = CASES[name]
        assert rr.same_coo(rr.statement(X, Y, C, M, R, variant="fmax", **kw), recorded(name), canon=bool(kw.get("max_nonzeros")))
