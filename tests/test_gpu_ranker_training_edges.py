"""Ranker training on the device (K13) at its edges: xrl_single_layer_train_csr_f32, xrl_single_layer_train_drm_f32 and
xrl_train_layer_device on ranker_training_rule.edge_cases() -- non-finite, huge, tiny and zero values of X, QD == 0, relevance values away
from ordinary costs, row ids stored twice in a column of Y or M, solver parameters away from ordinary positive numbers -- against the
numpy statement of the rule and the compiled reference as recorded in tests/golden/ranker_training_edges_ref.npz: rows, cols and value
bits, and the counters of what ran; a slot that served a job full of inf and NaN; the table's end; one plain repeat of the repeated-id
cases."""
import os

import numpy as np
import pytest

import ranker_training_rule as rr
from conftest import GOLDEN
from ranker_training_rule import resident, wt_as_coo

pytestmark = pytest.mark.gpu

CASES = rr.edge_cases()
RECORDED = np.load(os.path.join(GOLDEN, "ranker_training_edges_ref.npz"))
_truth = {}


def truth(name, dense=False):
    """The statement's answer for a case, computed once."""
    key = (name, dense)
    if key not in _truth:
        X, Y, C, M, R, kw = CASES[name]
        _truth[key] = rr.statement(rr.dense_bits(X) if dense else X, Y, C, M, R, **kw)
    return _truth[key]


def recorded(name):
    return RECORDED[f"case__{name}__rows"].astype(np.uint64), RECORDED[f"case__{name}__cols"].astype(np.uint64), RECORDED[f"case__{name}__vals"]


def same_counters(name, dense=False):
    got, want = rr.counters(), truth(name, dense)["counters"]
    assert {k: got[k] for k in want} == want, f"{name}: the counters differ from the statement's"
    return got


def rows_of_the_result(X, kw):
    return X.shape[1] + (kw.get("bias", 1.0) > 0)             # a NaN bias is not > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_csr_entry_point(name):
    X, Y, C, M, R, kw = CASES[name]
    canon = bool(kw.get("max_nonzeros"))
    got, err = rr.run_library(rr.OURS, X, Y, C, M, R, **kw)
    assert err is None, err
    assert got["shape"] == (rows_of_the_result(X, kw), Y.shape[1])
    assert rr.same_coo(got, truth(name), canon=canon), f"{name}: differs from the statement"
    assert rr.same_coo(got, recorded(name), canon=canon), f"{name}: differs from the recorded reference"
    same_counters(name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_resident_form(name):
    X, Y, C, M, R, kw = CASES[name]
    Wt, _ = resident(X, Y, C, M, R, kw)
    assert Wt.shape == (Y.shape[1], rows_of_the_result(X, kw))
    assert rr.same_coo(wt_as_coo(Wt), truth(name), canon=True), f"{name}: differs from the statement"
    assert rr.same_coo(wt_as_coo(Wt), recorded(name), canon=True), f"{name}: differs from the recorded reference"
    same_counters(name)


@pytest.mark.parametrize("name", rr.EDGE_DENSE)
def test_drm_entry_point(name):
    """Every row stores every column: zeros meet a NaN or an infinite w, and every row is summed by the wavefront."""
    X, Y, C, M, R, kw = CASES[name]
    D = rr.dense_bits(X)
    assert D.view(np.uint32)[rr.SHORT_ROW, X.indices[X.indptr[rr.SHORT_ROW] + 1]] == X.data.view(np.uint32)[X.indptr[rr.SHORT_ROW] + 1], "the special value's bits"
    got, err = rr.run_library(rr.OURS, D, Y, C, M, R, **kw)
    assert err is None, err
    assert got["shape"] == (rows_of_the_result(X, kw), Y.shape[1])
    assert rr.same_coo(got, truth(name, dense=True)), f"{name}: differs from the statement"
    c = same_counters(name, dense=True)
    assert c["lane_rows"] == 0 and c["wave_rows"] > 0


def _slot_problem():
    """Two codes of one label each over one X: code 0 lists the rows scaled by 1e-20 and 1e19 and one that stores an inf (its job's alpha,
    w and gradient become inf and NaN), code 1 lists ordinary rows only; both touch the same features."""
    X, _ = rr.overflow_problem()
    X = rr.set_entries(X, {(5, 2): rr.INF})
    N = X.shape[0]
    M = rr.raw_csc((N, 2), [(list(range(0, 10)) + [30, 31, 12, 13], [1] * 14), (list(range(10, 30)) + list(range(32, 40)), [1] * 28)])
    Y = rr.raw_csc((N, 2), [([1, 3, 8, 5, 30], [1] * 5), ([12, 20, 33, 35, 15], [1] * 5)])
    both = rr.raw_csc((2, 2), [([0], [1]), ([1], [1])])
    alone = rr.raw_csc((2, 2), [([], []), ([1], [1])])
    return X, Y, M, both, alone


@pytest.mark.parametrize("threshold", [0.0, 1e-3], ids=["every_feature_swept", "touched_features_swept"])
@pytest.mark.parametrize("solver", [rr.L1_DUAL, rr.L2_DUAL], ids=["l1", "l2"])
def test_a_slot_is_clean_after_a_job_of_inf_and_nan(monkeypatch, solver, threshold):
    X, Y, M, both, alone = _slot_problem()
    kw = dict(solver=solver, threshold=threshold, Cp=1e39, Cn=1e39, bias=0.0, max_iter=6)
    want_both, want_alone = rr.statement(X, Y, both, M, None, **kw), rr.statement(X, Y, alone, M, None, **kw)
    t = want_both["trace"]
    assert t["alpha_inf"] > 0 and t["nan_w_setup"] > 0 and t["nan_g_zero"] + t["nan_g_at_c"] + t["nan_g_between"] > 0, "the first job leaves inf and NaN behind"
    assert not any(want_alone["trace"].values()) and np.isfinite(want_alone["vals"]).all() and len(want_alone["vals"]) > 0, "the second job is ordinary"
    monkeypatch.setenv("XRL_TRAIN_SCRATCH_BYTES", "1")                    # one slot, one job per batch
    got_alone, err = rr.run_library(rr.OURS, X, Y, alone, M, None, **kw)
    assert err is None and rr.same_coo(got_alone, want_alone)
    got_both, err = rr.run_library(rr.OURS, X, Y, both, M, None, **kw)
    assert err is None and rr.same_coo(got_both, want_both)
    c = rr.counters()
    assert (c["jobs"], c["slots"]) == (2, 1)
    second = got_both["cols"] == 1
    assert rr.same_coo((got_both["rows"][second], got_both["cols"][second], got_both["vals"][second]), got_alone), "the job after it trains as it does alone"
    Wt, c = resident(X, Y, both, M, None, kw)
    assert c["slots"] == 1 and rr.same_coo(wt_as_coo(Wt), want_both, canon=True)


@pytest.mark.parametrize("name", ["x_overflow_l2", "dups_R0_l1"])
def test_jobs_cross_the_tables_end(monkeypatch, name):
    """A job that reaches the end of the table of random words cleans its slot and runs again: after inf and NaN, and with repeated ids."""
    X, Y, C, M, R, kw = CASES[name]
    monkeypatch.setenv("XRL_TRAIN_RANDOM_WORDS", "64")
    got, err = rr.run_library(rr.OURS, X, Y, C, M, R, **kw)
    assert err is None, err
    assert rr.same_coo(got, truth(name)) and rr.same_coo(got, recorded(name))
    c = same_counters(name)
    assert c["extensions"] >= 1 and c["reruns"] >= c["extensions"]


@pytest.mark.parametrize("name", rr.REPEAT_CASES)
def test_repeated_ids_give_the_same_bits_twice(name):
    """One plain repeat in one process.  (That the order is defined by lane number, not by the memory, is the code's to show.)"""
    X, Y, C, M, R, kw = CASES[name]
    a, err_a = rr.run_library(rr.OURS, X, Y, C, M, R, **kw)
    b, err_b = rr.run_library(rr.OURS, X, Y, C, M, R, **kw)
    assert err_a is None and err_b is None
    assert rr.same_coo(a, b) and rr.same_coo(a, truth(name))
    Wa, _ = resident(X, Y, C, M, R, kw)
    Wb, _ = resident(X, Y, C, M, R, kw)
    assert np.array_equal(Wa.indptr, Wb.indptr) and np.array_equal(Wa.indices, Wb.indices) and np.array_equal(Wa.data.view(np.uint32), Wb.data.view(np.uint32))
