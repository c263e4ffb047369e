"""No GPU: the numpy statement of the top-k order (tests/topk_order.py) against the reference, its case table against the library's own dispatch.

- topk() equals the C restatement, and the compiled reference when it is built, on every NaN-free row of the table, at the model shapes
  tests/test_gpu_topk_forms.py runs (flat, 20 482 labels, two layers), sparse and dense X: where the reference defines an order, this is it.
- The restatement's unsorted scoring route carries a NaN weight's sign and payload through `0 + 1 * w`: the GPU tests may compare NaN scores bit for bit.
- The (k, cand_stride) pairs of the table, run through xrl_debug_k2_form -- the function launch_k2_topk dispatches on -- name every NS bucket of the
  wave form, reg, lds and big, and both sides of every hand-over.
- Every row's precondition holds."""
import numpy as np
import pytest
import scipy.sparse as smat

import topk_models as M
import topk_order as T
from conftest import assert_same_topk


def _nan_free(rows):
    return [s for s in rows if s.nan_free]


def _references(oracle_mod, folder):
    refs = [("restatement", oracle_mod.OracleModel.load(folder))]
    if oracle_mod.ref_available():
        refs += [("compiled reference", oracle_mod.RefModel(folder)), ("compiled reference CSC", oracle_mod.RefModel(folder, "CSC"))]
    return refs


def _hold(case, ks, refs, dense):
    for k in ks:
        want = M.expected_csr(case, k)
        for name, ref in refs:
            for Xq in (case.X, np.ascontiguousarray(case.X.toarray())) if dense else (case.X,):
                got = ref.predict(Xq, beam_size=case.beam, only_topk=k, post_processor="noop")
                assert_same_topk(got, want, exact_scores=True, what=f"{name} k={k} dense={not smat.issparse(Xq)}")


def test_score_key_orders_like_the_floats():
    rng = np.random.default_rng(3)
    bits = np.concatenate([rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32),
                           np.array([0, T.NEG_ZERO, 1, 0x80000001, T.POS_INF, T.NEG_INF, T.POS_MAX, T.NEG_MAX], np.uint32)])
    bits = bits[~T.is_nan(bits)]
    key, val = T.score_key(bits).astype(np.int64), bits.view(np.float32).astype(np.float64)
    i, j = rng.integers(0, len(bits), 20000), rng.integers(0, len(bits), 20000)
    assert np.array_equal(np.sign(key[i] - key[j]), np.sign(val[i] - val[j]))
    k = T.score_key(np.array([T.POS_NAN, T.POS_INF, T.POS_MAX, 0, T.NEG_ZERO, T.NEG_MAX, T.NEG_INF, T.NEG_NAN], np.uint32)).astype(np.int64)
    assert k[0] > k[1] > k[2] > k[3] == k[4] > k[5] > k[6] > k[7] > 0
    pos, b = T.topk(np.array([T.NEG_NAN, 0x3F800000, T.POS_NAN, T.NEG_ZERO, 0, T.POS_NAN], np.uint32), 5)
    assert pos.tolist() == [2, 5, 1, 3, 4] and b.tolist() == [T.POS_NAN, T.POS_NAN, 0x3F800000, T.NEG_ZERO, 0]


@pytest.mark.parametrize("L", T.FLAT_L)
def test_every_row_of_the_table_is_what_it_is_named_for(L):
    rows = T.scenario_rows(L)
    for s in rows:
        assert len(s.bits) == L and len(s.stored) == L
        T.check_precondition(s)
    names = {s.name for s in rows}
    assert {"descending", "ascending", "all_equal", "zeros", "subnormals", "inf_fltmax"} <= names
    for k in T.K_VALUES:          # n < k, n = k, n = k + 1: no room for a tie at rank k before n = k + 1, for the NaN rows before n = k + 2
        assert (f"tie_run_k{k}" in names) == (L >= k + 1)
        assert (f"nan_last_k{k}" in names) == (2 <= k <= L - 2) == (f"nan_before_fill_k{k}" in names) == (f"nan_after_fill_k{k}" in names)
    if L >= 65:
        assert any(not s.stored.all() for s in rows), "no unstored cell"


def test_flat_lengths_lie_on_either_side_of_every_k():
    for k in T.K_VALUES:
        assert k == 1 or any(L < k for L in T.FLAT_L)
        assert any(L > k + 1 for L in T.FLAT_L)
    pairs = [(L, k) for L in T.FLAT_L for k in T.K_VALUES]
    for d in (-1, 0, 1, 2):      # n = k - 1, k, k + 1, k + 2
        assert sum(L - k == d for L, k in pairs) >= 2, f"n = k {d:+d} is reached by fewer than two (L, k) pairs"


@pytest.mark.parametrize("L", T.FLAT_L)
def test_topk_is_the_reference_order_flat(L, tmp_path, oracle_mod):
    case = M.flat_case(str(tmp_path / "m"), L, _nan_free(T.scenario_rows(L)))
    _hold(case, T.K_VALUES, _references(oracle_mod, case.folder), dense=False)
    fin = M.flat_case(str(tmp_path / "f"), L, M.finite_rows(T.scenario_rows(L)))
    _hold(fin, (1, 64, 65, 193), _references(oracle_mod, fin.folder), dense=True)


def test_topk_is_the_reference_order_beyond_the_lds_limit(tmp_path, oracle_mod):
    rows = M.big_rows()
    for s in rows:
        T.check_precondition(s)
    case = M.flat_case(str(tmp_path / "m"), T.BIG_L, _nan_free(rows))
    _hold(case, T.BIG_K, _references(oracle_mod, case.folder), dense=False)


def test_topk_is_the_reference_order_two_layers(tmp_path, oracle_mod):
    for finite_only in (False, True):
        cases = M.two_layer_cases(str(tmp_path / f"m{int(finite_only)}"), finite_only=finite_only)
        refs = None
        for beam, case in cases.items():
            assert {len(c) for c in case.cand} - {0} and max(len(c) for c in case.cand) <= case.cand_stride
            for s in case.rows:
                if s is not None:
                    T.check_precondition(s)
            keep = [r for r, s in enumerate(case.rows) if s is None or s.nan_free]
            sub = case._replace(X=case.X[keep], cand=[case.cand[r] for r in keep], label=[case.label[r] for r in keep], rows=[case.rows[r] for r in keep])
            refs = refs or _references(oracle_mod, case.folder)
            _hold(sub, M.TWO_LAYER_K, refs, dense=finite_only)
        assert any(len(c) == 0 for c in cases[1].cand), "no query without candidates"
        assert len({len(c) for c in cases[3].cand}) >= 4, "ncand does not differ within one launch"
        assert all(len(c) < cases[3].cand_stride for c in cases[3].cand), "n < cand_stride is not reached"


def test_topk_of_unsorted_scores_is_the_reference_order_under_a_combiner(tmp_path, oracle_mod):
    # the bound-pruned model of the GPU tests: its expected rows come from the unsorted scoring route; the sorted one must agree
    cases = M.pruned_cases(str(tmp_path / "m"), oracle_mod)
    refs = _references(oracle_mod, cases[2].folder)
    for beam, case in cases.items():
        M.check_pruned_precondition(case)
        assert max(M.PRUNED_CHUNKS) <= 128 and 2 <= beam <= 32 and case.cand_stride <= 2048
        for k in M.PRUNED_K:
            want = M.expected_csr(case, k)
            for name, ref in refs:
                assert_same_topk(ref.predict(case.X, beam_size=beam, only_topk=k, post_processor=M.PRUNED_PP), want, exact_scores=True, what=f"{name} beam={beam} k={k}")
    assert {len(c) for cs in cases.values() for c in cs.cand} >= {64, 65, 127, 129, 192, 193, 832, 833}


def test_nan_weights_keep_sign_and_payload_through_the_scoring(tmp_path, oracle_mod):
    # the unsorted route (predict_on_selected_outputs: no std::sort on NaN keys) on every label of the NaN rows
    L = 129
    rows = [s for s in T.scenario_rows(L) if not s.nan_free]
    assert len(rows) == 3 * 5                       # k = 2, 63, 64, 65, 127
    case = M.flat_case(str(tmp_path / "m"), L, rows)
    om = oracle_mod.OracleModel.load(case.folder)
    S = smat.csr_matrix(np.ones((len(rows), L), np.float32))
    got = om.predict_on_selected_outputs(case.X, S, "noop")
    for r, s in enumerate(rows):
        lo, hi = got.indptr[r], got.indptr[r + 1]
        bits = np.zeros(L, np.uint32)
        bits[got.indices[lo:hi]] = got.data[lo:hi].astype(np.float32).view(np.uint32)
        assert np.array_equal(bits, case.cand[r]), s.name
        assert (bits == T.POS_NAN).sum() == 2 and (bits == T.NEG_NAN).sum() == 2


# ------------------------------------------------------------------------------------------------------------------ the dispatch
def table_shapes():
    """(k, cand_stride) of every stand-alone K2 case of tests/test_gpu_topk_forms.py (a launch keeps the k it was asked for on shorter rows too)."""
    shapes = {(k, L) for L in T.FLAT_L for k in T.K_VALUES}
    shapes |= {(k, T.BIG_L) for k in T.BIG_K}
    shapes |= {(k, T.cand_bound(M.CHUNKS, beam)) for beam in M.PARENT_SETS for k in M.TWO_LAYER_K}
    return sorted(shapes)


def test_case_table_names_every_form_and_every_handover():
    from pecos_amd import clib
    seen = {}
    for k, cs in table_shapes():
        got = clib.debug_k2_form(k, cs)
        assert got == T.expected_form(k, cs), f"k={k} cand_stride={cs}: the library dispatches to {got}"
        seen[(k, cs)] = got
        assert clib.debug_k2_form(k, cs, k2_big_min_k=1) == ("big", 0)
        assert clib.debug_k2_form(k, cs, k2_big_min_k=k + 1) == got and clib.debug_k2_form(k, cs, k2_big_min_k=k) == ("big", 0)
    forms = set(seen.values())
    assert {("wave", ns) for ns in T.WAVE_NS} <= forms, f"NS buckets named: {sorted(f for f in forms if f[0] == 'wave')}"
    assert {("reg", 0), ("lds", 0), ("big", 0)} <= forms
    # both sides of every NS bucket edge, at one k
    for ns in T.WAVE_NS[:-1]:
        nxt = T.WAVE_NS[T.WAVE_NS.index(ns) + 1]
        assert seen[(64, 64 * ns)] == ("wave", ns) and seen[(64, 64 * ns + 1)] == ("wave", nxt)
    # wave -> reg at cand_stride 2048 / 2049, on k = 64; k = 64 / 65 on both sides of it; lds -> big at 20 480 / 20 481
    assert seen[(64, 2048)] == ("wave", 32) and seen[(64, 2049)] == ("reg", 0)
    assert seen[(65, 2048)] == ("lds", 0) and seen[(65, 2049)] == ("lds", 0)
    assert seen[(1, 2305)] == ("reg", 0) and seen[(193, 2305)] == ("lds", 0)
    assert seen[(20480, T.BIG_L)] == ("lds", 0) and seen[(20481, T.BIG_L)] == ("big", 0)


def test_dispatch_of_the_pruning_stages():
    from pecos_amd import clib
    for cs in (1, 64, 65, 832, 833, 1024, 1025, 2048):
        whole = clib.debug_k2_form(20, cs)
        assert clib.debug_k2_form(20, cs, stage=1) == whole
        assert clib.debug_k2_form(20, cs, k2_big_min_k=1, stage=1) == whole and clib.debug_k2_form(20, cs, k2_big_min_k=1, stage=2)[0] != "big"
        # the list form walks every bucket but NS = 16, which keeps the batch-sized grid
        assert clib.debug_k2_form(20, cs, stage=2) == (("wave" if whole[1] == 16 else "list"), whole[1])
        # a rank-limited stage holds registers for the candidates it looks at
        assert clib.debug_k2_form(20, cs, stage=1, limited_cands=64) == ("wave", 1)
        assert clib.debug_k2_form(20, cs, stage=1, limited_cands=4096) == whole
    for k, cs in ((65, 100), (20, 2049)):
        with pytest.raises(RuntimeError, match="register top-k"):
            clib.debug_k2_form(k, cs, stage=1)
    with pytest.raises(RuntimeError, match="resolved to 0"):
        clib.debug_k2_form(0, 100)
