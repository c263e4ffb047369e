"""CPU half of the tf-idf weighting tests (cases: tests/tfidf_weight_cases.py; GPU half: tests/test_gpu_tfidf_weight.py).

* the numpy mirror (pecos_amd.features.tfidf_weight) and the restatement (oracle/tfidf_oracle.py) against the compiled reference's own
  c_tfidf_predict (oracle/_ref), bit for bit, sublinear_tf INCLUDED: counts 1 .. 512 and larger ones with the transform laid bare
  (count_sweep), rows of 0 .. 1025 entries that a tree or per-step reduction gets wrong (row_lengths), ensembles of 1, 2 and 3 bases;
* the logf form this project computed before differs from the reference on count_sweep, asserted, so the case keeps its teeth;
* the raw-count cases (epsilon_edges, value_edges), which no text reaches, against a scalar restatement of tfidf.hpp:798-822 in C, compiled
  here with the flags of oracle/Makefile's liboracle.so rule (-ffp-contract=off).
The library's own host weighting (calls of <= 4 documents) answers only where a GPU is present: it is held to the same bar in the GPU half.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import tfidf_weight_cases as wc


@pytest.fixture(scope="module")
def ref(oracle_mod, tmp_path_factory):
    """{case name: (folder, the reference's X)} of every text case, computed once (oracle_mod builds oracle/_ref where the reference's sources are)."""
    if not wc.reference_available():
        pytest.skip("oracle/_ref not built")
    return wc.reference_predict(wc.all_text_cases(), tmp_path_factory.mktemp("tfidf_weight_ref"))


def _cases(group):
    return {"count_sweep": lambda: wc.count_sweep()[0], "row_lengths": lambda: [c for _, c in wc.row_lengths()], "ensembles": wc.ensembles}[group]()


GROUPS = ("count_sweep", "row_lengths", "ensembles")


def _same_matrix(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), f"{what}: pattern differs"
    wc.same_values(got.data, want.data, what)


@pytest.mark.parametrize("group", GROUPS)
def test_host_tokenizer_counts_are_the_chosen_counts(group, tmp_path):
    # the premise of every text case: the documents give exactly the counts they were built from (host half of this library, no GPU)
    from pecos_amd import clib
    for case in _cases(group)[:: 4 if group == "row_lengths" else 1]:
        h = clib.tfidf_load(case.write(str(tmp_path / case.name)))
        try:
            C = clib.tfidf_counts(h, case.docs, threads=2)
        finally:
            clib.tfidf_destruct(h)
        _same_matrix(C, case.counts, case.name)


@pytest.mark.parametrize("group", GROUPS)
def test_reference_pattern_is_the_chosen_pattern(group, ref):
    for case in _cases(group):
        X = ref[case.name][1]
        assert X.shape == case.counts.shape and np.array_equal(X.indptr, case.counts.indptr) and np.array_equal(X.indices, case.counts.indices), case.name


def test_count_sweep_shows_the_transform_itself(ref):
    # the precondition at work: the reference's X is (float)(log((double)c) + 1.0) x 2^-40 exactly, under both norms -- and the logf form
    # differs from it in fp32 bits at every count the generator named
    cases, counts, telling = wc.count_sweep()
    want = wc.sweep_expected(counts)
    old = (wc.tf_float_log(counts) * np.float32(wc.TINY_IDF)).astype(np.float32)
    at = np.isin(counts, telling)
    assert at.sum() == len(telling) >= 34 and {28, 35, 42, 49, 52} <= set(telling.tolist())
    for case in cases:
        X = ref[case.name][1]
        wc.same_values(X.data, want, case.name)
        assert np.all(wc.bits(old)[at] != wc.bits(X.data)[at]), case.name
        assert np.array_equal(wc.bits(old)[~at], wc.bits(X.data)[~at]), case.name


@pytest.mark.parametrize("group", GROUPS)
def test_mirror_vs_reference(group, ref):
    from pecos_amd.features import tfidf_weight
    for case in _cases(group):
        _same_matrix(case.weigh(tfidf_weight), ref[case.name][1], f"tfidf_weight, {case.name}")


@pytest.mark.parametrize("group", GROUPS)
def test_oracle_vs_reference(group, ref):
    from oracle.tfidf_oracle import TfidfOracle
    for case in _cases(group):
        folder, X = ref[case.name]
        indptr, idx, val = TfidfOracle(folder).predict(case.docs)
        assert np.array_equal(indptr, X.indptr.astype(np.uint64)) and np.array_equal(idx, X.indices.astype(np.uint32)), case.name
        wc.same_values(val, X.data, f"tfidf_oracle, {case.name}")


def test_row_lengths_are_order_sensitive(ref):
    # the generator's claim seen on the reference's own output: with the denominator summed pairwise (numpy) or in fp64, the rows of 65
    # entries and more come out with other bits than the reference's
    (cfg, case), = [(g, c) for g, c in wc.row_lengths() if g == dict(norm="l2", binary=False, sublinear_tf=False, use_idf=True)]
    X = ref[case.name][1]
    idf = case.bases[0].idf
    for r, L in enumerate(wc.LENGTHS):
        a, b = X.indptr[r], X.indptr[r + 1]
        assert b - a == L
        if L < 65:
            continue
        v = (case.counts.data[a:b] * idf[X.indices[a:b]]).astype(np.float32)
        for d in (np.float32(np.sum(v * v, dtype=np.float32)), np.float32(np.sum((v * v).astype(np.float64)))):
            assert np.any(wc.bits(v / np.float32(np.sqrt(d))) != wc.bits(X.data[a:b])), L


# ------------------------------------------------------------------------------------------------------------------ raw cases vs a scalar restatement
_RESTATEMENT = r"""
#include <float.h>
#include <math.h>
/* one row of term counts -> tf -> x idf -> norm, every step in float, in stored order (behaviour of tfidf.hpp:798-822) */
void weigh_row(const unsigned* col, const float* count, unsigned n, const float* idf, int binary, int sublinear_tf, int norm_p, float* out) {
    float denom = 0.0f;
    for (unsigned i = 0; i < n; ++i) {
        float v = binary ? 1.0f : count[i];
        if (sublinear_tf) v = (float)(log((double)v) + 1.0);
        if (idf) v = v * idf[col[i]];
        out[i] = v;
        float term = norm_p == 1 ? fabsf(v) : v * v;
        denom = denom + term;
    }
    if (fabsf(denom) < FLT_EPSILON) denom = 1.0f;
    else if (norm_p == 2) denom = sqrtf(denom);
    for (unsigned i = 0; i < n; ++i) out[i] = out[i] / denom;
}
"""


@pytest.fixture(scope="module")
def weigh_row(tmp_path_factory):
    d = tmp_path_factory.mktemp("tfidf_restatement")
    src, lib = str(d / "weigh_row.c"), str(d / "weigh_row.so")
    with open(src, "w") as f:
        f.write(_RESTATEMENT)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-o", lib, src, "-lm"])
    fn = ctypes.CDLL(lib).weigh_row
    fn.restype = None
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]

    def run(case):
        C = case.counts
        col = np.ascontiguousarray(C.indices, dtype=np.uint32)
        cnt = np.ascontiguousarray(C.data, dtype=np.float32)
        idf = np.ascontiguousarray(case.idf, dtype=np.float32) if case.idf is not None else None
        out = np.zeros(C.nnz + 1, dtype=np.float32)
        for r in range(C.shape[0]):
            a, b = int(C.indptr[r]), int(C.indptr[r + 1])
            fn(col.ctypes.data + 4 * a, cnt.ctypes.data + 4 * a, b - a, idf.ctypes.data if idf is not None else None, int(case.binary), int(case.sublinear_tf),
               1 if case.norm == "l1" else 2, out.ctypes.data + 4 * a)
        return out[:C.nnz]
    return run


def _raw_cases():
    return wc.epsilon_edges()[0] + wc.value_edges()


@pytest.mark.parametrize("name", [c.name for c in _raw_cases()])
def test_mirror_vs_scalar_restatement(name, weigh_row):
    case, = [c for c in _raw_cases() if c.name == name]
    got = wc.mirror(case)
    assert np.array_equal(got.indptr, case.counts.indptr) and np.array_equal(got.indices, case.counts.indices), name
    wc.same_values(got.data, weigh_row(case), name)


def test_restatement_vs_reference_on_text_rows(weigh_row, ref):
    # the restatement itself is the reference's arithmetic: on single-base text cases it gives the reference's bits
    for case in wc.count_sweep()[0] + [c for _, c in wc.row_lengths()]:
        wc.same_values(weigh_row(wc.raw_of_text(case)), ref[case.name][1].data, case.name)


def test_epsilon_edges_do_what_their_labels_say(weigh_row):
    # kept: the row is divided by the denominator (l1: the values sum to 1 in magnitude; l2: by sqrt(FLT_EPSILON)); replaced: divided by 1
    cases, labels = wc.epsilon_edges()
    for case in cases:
        out = weigh_row(case)
        C = case.counts
        v = (C.data * case.idf[C.indices]).astype(np.float32)
        for r, label in enumerate(labels[case.norm]):
            a, b = C.indptr[r], C.indptr[r + 1]
            d = np.float32(1) if label == "replaced" else wc.EPS if case.norm == "l1" else np.float32(np.sqrt(wc.EPS))
            wc.same_values(out[a:b], (v[a:b] / d).astype(np.float32), f"{case.name} row {r} ({label})")
            assert label == "kept" or np.array_equal(wc.bits(out[a:b]), wc.bits(v[a:b]))
