"""GPU (-m gpu): the first stage of a bound-pruned tile-format layer in ONE launch (library option leaf_fuse, csrc/xrl_k1t.hip SEL): K1T's
epilogue ranks the candidates it has just computed, sets the done flags and stores the candidate rows of the unfinished queries only.
For every case: leaf_fuse=1 == leaf_fuse=0 == reference (label ids, order, fp32 score bits -- the sigmoid family at the suite's
tolerance against the reference, bit-exact between the two paths -- and counts), and the profile shows that the fused launch really ran
(no k2_topk slot on the layer) or really fell back (slot present) where the case says so."""
import os

import numpy as np
import pytest
import scipy.sparse as smat

from conftest import assert_same_topk

pytestmark = pytest.mark.gpu

EXACT_PP = lambda pp: pp is None or "sigmoid" not in pp   # noqa: E731


@pytest.fixture(scope="module")
def clib():
    from pecos_amd import clib
    assert clib.device_count() > 0, "no GPU visible"
    return clib


@pytest.fixture(scope="module")
def XLM():
    from pecos_amd import XLinearModel
    return XLinearModel


def _reference(oracle_mod, folder, wmt="BINARY_SEARCH_CHUNKED"):
    return oracle_mod.RefModel(folder, wmt) if oracle_mod.ref_available() else oracle_mod.OracleModel.load(folder, wmt)


def _tile_pipeline(clib, h):
    clib.set_option(h, "dense_layers", 0)    # every layer on the tile pipeline (tile rows are built for every layer)
    clib.set_option(h, "adaptive", 0)        # always staged: the pruning feedback does not switch a layer to one unstaged pass


def _restore(clib, h):
    for k, v in (("dense_layers", 1), ("adaptive", 1), ("leaf_fuse", 1), ("tile_rows", 1), ("prune", 1)):
        clib.set_option(h, k, v)


def _predict_profiled(m, clib, X, kw):
    h = m.model.model_chain
    clib.profile_reset(h); clib.profile_enable(h, True)
    out = m.predict(X, **kw)
    prof = clib.profile_get(h)
    clib.profile_enable(h, False)
    return out, {(r["name"], int(r["layer"])) for r in prof}


def check_case(m, clib, X, kw, want, layer, fused, what):
    """leaf_fuse = 1 and 2 == leaf_fuse = 0 (always bit for bit) == want; on `layer` the fused launch ran (fused=True) or the old launches did."""
    h = m.model.model_chain
    clib.set_option(h, "leaf_fuse", 0)
    a0, p0 = _predict_profiled(m, clib, X, kw)
    assert {("k0_prolongate", layer), ("k2_topk", layer)} <= p0, f"{what}: leaf_fuse=0 must run K0 and K2 on layer {layer}: {sorted(p0)}"
    a1 = None
    for lf in (2, 1):
        clib.set_option(h, "leaf_fuse", lf)
        a1, p1 = _predict_profiled(m, clib, X, kw)
        if fused:
            first = ("k1_sparse", layer) in p1 and ("k2_topk", layer) not in p1
            assert first, f"{what}: leaf_fuse={lf}: the fused launch did not run on layer {layer}: {sorted(p1)}"
            # 1 (default): the launch derives its items too (beams of up to 32 parents); 2: K0 is still launched
            assert (("k0_prolongate", layer) in p1) == (lf == 2), f"{what}: leaf_fuse={lf}: {sorted(p1)}"
            assert {("k0b_remaining", layer), ("k1_sparse_rest", layer), ("k2_topk_rest", layer)} <= p1, f"{what}: later stages missing: {sorted(p1)}"
        else:
            assert {("k0_prolongate", layer), ("k2_topk", layer)} <= p1, f"{what}: leaf_fuse={lf}: expected the fallback on layer {layer}: {sorted(p1)}"
        assert_same_topk(a1, a0, exact_scores=True, what=f"{what}: leaf_fuse {lf} vs 0")
        if want is not None:
            assert_same_topk(a1, want, exact_scores=EXACT_PP(kw.get("post_processor")), what=f"{what}: leaf_fuse={lf} vs reference")
    if want is not None:
        assert_same_topk(a0, want, exact_scores=EXACT_PP(kw.get("post_processor")), what=f"{what}: leaf_fuse=0 vs reference")
    return a1


@pytest.mark.parametrize("width", [24, 50, 80, 120])          # children per leaf parent: NR = 1, 2, 3, 4 columns per lane
@pytest.mark.parametrize("permute_leaf", [False, True])       # without / with perm_inv
def test_widths_layouts_postprocessors(width, permute_leaf, XLM, clib, oracle_mod, tmp_path):
    import xrl_synth
    folder = str(tmp_path / "m")
    D, P = 300, 12
    xrl_synth.make_model(folder, D, P * width, [80, 60, 20], seed=61 + width, shape=[4, P, P * width], permute_leaf=permute_leaf)
    X = xrl_synth.make_queries(150, D, 20, seed=62, relabel_seed=61 + width)
    for wmt in ("BINARY_SEARCH_CHUNKED", "HASH_CHUNKED"):   # HASH_CHUNKED: sparse X adds the bias first
        m = XLM.load(folder, weight_matrix_type=wmt) if wmt != "BINARY_SEARCH_CHUNKED" else XLM.load(folder)
        h = m.model.model_chain
        ref = _reference(oracle_mod, folder, wmt)
        _tile_pipeline(clib, h)
        for kw in (dict(beam_size=6, only_topk=10), dict(beam_size=6, only_topk=10, post_processor="sigmoid"),
                   dict(beam_size=4, only_topk=7, post_processor="log-l2-hinge"), dict(beam_size=2, only_topk=1), dict(beam_size=10, only_topk=20)):
            check_case(m, clib, X, kw, ref.predict(X, **kw), 2, True, f"width {width} permute={permute_leaf} {wmt} {kw}")
        _restore(clib, h)


@pytest.mark.parametrize("variant", ["all_saturated", "bias_only", "descending"])
def test_massive_ties(variant, XLM, clib, oracle_mod, tmp_path):
    # the models of test_gpu_parity.test_bound_pruning_with_massive_ties: candidate POSITION decides (almost) everything
    import xrl_synth
    folder = str(tmp_path / "m")
    D = 120
    xrl_synth.make_model(folder, D, 700, [60, 40, 12], seed=41, shape=[5, 40, 700], permute_leaf=True)
    for d in range(3):
        f = os.path.join(folder, "ranker", f"{d}.model", "W.npz")
        W = smat.load_npz(f).tocsc().astype(np.float32)
        if variant == "descending":
            col = np.repeat(np.arange(W.shape[1]), np.diff(W.indptr))
            W.data[:] = (1.5 / (1.0 + 0.01 * col)).astype(np.float32)
        else:
            W.data[:] = 2.0
        smat.save_npz(f, W, compressed=False)
    X = xrl_synth.make_queries(50, D, 12, seed=43, relabel_seed=41)
    if variant == "bias_only":
        X = smat.csr_matrix(X.shape, dtype=np.float32)
    m = XLM.load(folder)
    h = m.model.model_chain
    om = oracle_mod.OracleModel.load(folder)
    _tile_pipeline(clib, h)
    for k in (1, 10, 20):
        for kw in (dict(beam_size=10, only_topk=k), dict(beam_size=3, only_topk=k), dict(beam_size=7, only_topk=k, post_processor="log-l2-hinge"),
                   dict(beam_size=7, only_topk=k, post_processor="sigmoid")):
            check_case(m, clib, X, kw, om.predict(X, **kw), 2, True, f"{variant} {kw}")
    _restore(clib, h)


def test_small_parents_single_parent_beams_empty_rows(XLM, clib, oracle_mod, tmp_path):
    import xrl_synth
    folder = str(tmp_path / "m")
    D = 200
    # 20 children per leaf parent (17..32 columns: 32 lanes per item), fewer than k = 30: the first stage can never be final
    xrl_synth.make_model(folder, D, 400, [60, 40, 15], seed=71, shape=[4, 20, 400], permute_leaf=True)
    X = xrl_synth.make_queries(130, D, 16, seed=72, relabel_seed=71).tolil()
    for r in (0, 5, 64, 65, 129):            # empty query rows (both halves of a wavefront, the last query of an odd batch)
        X.rows[r] = []; X.data[r] = []
    X = X.tocsr().astype(np.float32); X.sort_indices()
    m = XLM.load(folder)
    h = m.model.model_chain
    ref = _reference(oracle_mod, folder)
    _tile_pipeline(clib, h)
    for kw in (dict(beam_size=5, only_topk=20), dict(beam_size=3, only_topk=10), dict(beam_size=2, only_topk=3, post_processor="log-l3-hinge")):
        check_case(m, clib, X, kw, ref.predict(X, **kw), 2, True, f"small parents {kw}")
    # k = 30 > 20 children: k <= 20 is what the extraction serves, so this is the fallback; k = 20 == 20 children is fused and final only on ties
    check_case(m, clib, X, dict(beam_size=5, only_topk=30), ref.predict(X, beam_size=5, only_topk=30), 2, False, "k=30 > children, k > 20")
    # odd row counts: the last wavefront's second half has no query
    for n in (1, 2, 3, 127):
        kw = dict(beam_size=5, only_topk=10)
        check_case(m, clib, X[:n], kw, ref.predict(X[:n], **kw), 2, True, f"{n} rows")
    _restore(clib, h)


def test_beams_of_one_parent_and_empty_beams(XLM, clib, oracle_mod, tmp_path):
    # prune=0.6 on the leaf layer removes most children: parents with few children -> short candidate rows, fewer than k
    import xrl_synth
    folder = str(tmp_path / "m")
    D = 200
    xrl_synth.make_model(folder, D, 1000, [60, 40, 15], seed=81, shape=[4, 20, 1000], permute_leaf=True, prune=0.6)
    X = xrl_synth.make_queries(90, D, 16, seed=82, relabel_seed=81)
    m = XLM.load(folder)
    h = m.model.model_chain
    ref = _reference(oracle_mod, folder)
    _tile_pipeline(clib, h)
    for kw in (dict(beam_size=6, only_topk=10), dict(beam_size=2, only_topk=20), dict(beam_size=6, only_topk=5, post_processor="log-l2-hinge")):
        check_case(m, clib, X, kw, ref.predict(X, **kw), 2, True, f"pruned leaf {kw}")
    _restore(clib, h)
    # short and EMPTY beams: layer 1's C keeps children {0, 1} of parent 0, child {4} of parent 2 and none of parents 1 and 3 -- with beam_size 2 a
    # query enters the leaf with two, one (limited == false: done whatever the scores) or no parents (no item: count 0, done) of beam_in = 2
    folder2 = str(tmp_path / "m2")
    xrl_synth.make_model(folder2, D, 240, [60, 40, 15], seed=83, shape=[4, 8, 240], permute_leaf=True)
    f = os.path.join(folder2, "ranker", "1.model", "C.npz")
    C = smat.load_npz(f).tocsc()
    Cn = smat.csc_matrix((np.ones(3, np.float32), np.array([0, 1, 4], np.int32), np.array([0, 2, 2, 3, 3])), shape=C.shape)
    smat.save_npz(f, Cn, compressed=False)
    X2 = xrl_synth.make_queries(200, D, 16, seed=84, relabel_seed=83)
    m2 = XLM.load(folder2)
    h2 = m2.model.model_chain
    ref2 = _reference(oracle_mod, folder2)
    _tile_pipeline(clib, h2)
    for kw in (dict(beam_size=2, only_topk=10), dict(beam_size=2, only_topk=5, post_processor="log-l2-hinge"), dict(beam_size=3, only_topk=20)):
        want = ref2.predict(X2, **kw)
        if kw["beam_size"] == 2:
            per_row = np.diff(want.indptr)
            assert (per_row == 0).any() and (per_row == min(kw["only_topk"], 30)).any(), "the case must hold empty and full beams"
        check_case(m2, clib, X2, kw, want, 2, True, f"short and empty beams {kw}")
    _restore(clib, h2)


@pytest.mark.parametrize("variant", ["x_nonfinite", "x_huge", "w_inf", "w_nan"])
def test_guard_nonfinite(variant, XLM, clib, oracle_mod, tmp_path):
    # the models of test_gpu_parity.test_bound_pruning_guard_nonfinite: a query the guard does not clear is never done after the first stage
    import xrl_synth
    folder = str(tmp_path / "m")
    D = 120
    xrl_synth.make_model(folder, D, 700, [60, 40, 12], seed=51, shape=[5, 40, 700], permute_leaf=True)
    rng = np.random.default_rng(11)
    positive = variant in ("x_huge", "w_inf")
    for d in range(3):
        f = os.path.join(folder, "ranker", f"{d}.model", "W.npz")
        W = smat.load_npz(f).tocsc().astype(np.float32)
        if positive:
            W.data[:] = np.abs(W.data) + 0.01
        if variant == "w_inf" and d >= 1:
            W.data[rng.integers(0, len(W.data), 6)] = np.inf
        if variant == "w_nan" and d >= 1:
            W.data[rng.integers(0, len(W.data), 6)] = np.nan
            W.data[rng.integers(0, len(W.data), 6)] = -np.inf
        smat.save_npz(f, W, compressed=False)
    X = xrl_synth.make_queries(64, D, 14, seed=53, relabel_seed=51).tocsr()
    X.data = np.abs(X.data)
    if variant == "x_nonfinite":
        for r in range(0, 64, 2):
            lo, hi = X.indptr[r], X.indptr[r + 1]
            if hi - lo >= 3:
                X.data[lo + int(rng.integers(0, hi - lo))] = [np.nan, np.inf, -np.inf, 0.0][(r // 2) % 4]
    if variant == "x_huge":
        for r in range(0, 64, 3):
            lo, hi = X.indptr[r], X.indptr[r + 1]
            if hi > lo:
                X.data[lo + int(rng.integers(0, hi - lo))] = [3.0e38, np.inf, 1.0e30][(r // 3) % 3]
    m = XLM.load(folder)
    h = m.model.model_chain
    om = _reference(oracle_mod, folder)
    _tile_pipeline(clib, h)
    for kw in (dict(beam_size=10, only_topk=10), dict(beam_size=3, only_topk=20), dict(beam_size=25, only_topk=5, post_processor="log-l2-hinge"),
               dict(beam_size=7, only_topk=12, post_processor="sigmoid")):
        clib.set_option(h, "prune", 0)
        base = m.predict(X, **kw)
        clib.set_option(h, "prune", 1)
        got = check_case(m, clib, X, kw, om.predict(X, **kw) if positive else None, 2, True, f"{variant} {kw}")
        # pruning (fused or not) must not change a bit, NaN scores included
        assert np.array_equal(got.indptr, base.indptr) and np.array_equal(got.indices, base.indices), (variant, kw)
        assert np.array_equal(got.data.view(np.uint32), base.data.view(np.uint32)), (variant, kw)
    _restore(clib, h)


def test_fallbacks(XLM, clib, oracle_mod, tmp_path):
    import xrl_synth
    folder = str(tmp_path / "m")
    D = 300
    xrl_synth.make_model(folder, D, 12 * 50, [80, 60, 20], seed=91, shape=[4, 12, 600], permute_leaf=True)
    X = xrl_synth.make_queries(100, D, 20, seed=92, relabel_seed=91)
    m = XLM.load(folder)
    h = m.model.model_chain
    ref = _reference(oracle_mod, folder)
    _tile_pipeline(clib, h)
    # k = 21: beyond the extraction (kTopkExtractMaxK = 20)
    kw = dict(beam_size=6, only_topk=21)
    check_case(m, clib, X, kw, ref.predict(X, **kw), 2, False, "k=21")
    # tile_rows=0: the entry-list kernel K1 serves the layer
    clib.set_option(h, "tile_rows", 0)
    kw = dict(beam_size=6, only_topk=10)
    check_case(m, clib, X, kw, ref.predict(X, **kw), 2, False, "tile_rows=0")
    clib.set_option(h, "tile_rows", 1)
    check_case(m, clib, X, kw, ref.predict(X, **kw), 2, True, "tile_rows=1 again")
    # dense X
    Xd = np.ascontiguousarray(X.toarray())
    check_case(m, clib, Xd, kw, ref.predict(Xd, **kw), 2, False, "dense X")
    # noop: no combiner, the layer is not bound-pruned at all (one pass, with or without the option)
    kwn = dict(beam_size=6, only_topk=10, post_processor="noop")
    want = ref.predict(X, **kwn)
    for lf in (0, 1, 2):
        clib.set_option(h, "leaf_fuse", lf)
        got, prof = _predict_profiled(m, clib, X, kwn)
        assert ("k2_topk", 2) in prof and ("k2_topk_rest", 2) not in prof, sorted(prof)
        assert_same_topk(got, want, exact_scores=True, what=f"noop leaf_fuse={lf}")
    _restore(clib, h)
    # two tiles per parent: chunks wider than 128 columns
    folder2 = str(tmp_path / "m2")
    xrl_synth.make_model(folder2, D, 8 * 150, [80, 60, 20], seed=93, shape=[4, 8, 1200], permute_leaf=True)
    X2 = xrl_synth.make_queries(100, D, 20, seed=94, relabel_seed=93)
    m2 = XLM.load(folder2)
    h2 = m2.model.model_chain
    _tile_pipeline(clib, h2)
    ref2 = _reference(oracle_mod, folder2)
    check_case(m2, clib, X2, kw, ref2.predict(X2, **kw), 2, False, "two tiles per parent")
    _restore(clib, h2)


def test_wiki10_shape_three_stages_repeated_predicts(XLM, clib, oracle_mod, tmp_path):
    # beam 20, k 20: first, MIDDLE and last stage on the leaf; the default options (pruning feedback on): predicts #1 to #7 identical
    import xrl_synth
    folder = str(tmp_path / "m")
    ks, X, cfg = xrl_synth.make_config("wiki10-31k", folder, scale=0.1)
    X = X[:600]
    m = XLM.load(folder)
    h = m.model.model_chain
    ref = _reference(oracle_mod, folder)
    leaf = len(ks) - 1
    kw = dict(beam_size=cfg["beam"], only_topk=20)
    want = ref.predict(X, **kw)
    outs = {}
    for lf in (0, 1, 2):
        clib.set_option(h, "leaf_fuse", lf)
        clib.set_option(h, "adaptive", 0); clib.set_option(h, "adaptive", 1)      # (resets the feedback's state)
        for i in range(7):
            got = m.predict(X, **kw)
            assert_same_topk(got, want, exact_scores=True, what=f"wiki10 shape leaf_fuse={lf} predict #{i + 1}")
        outs[lf] = got
    assert_same_topk(outs[1], outs[0], exact_scores=True, what="wiki10 shape leaf_fuse 1 vs 0")
    assert_same_topk(outs[2], outs[0], exact_scores=True, what="wiki10 shape leaf_fuse 2 vs 0")
    # always staged: the profile names the three stages, the first one fused
    clib.set_option(h, "adaptive", 0)
    clib.set_option(h, "leaf_fuse", 1)
    got, prof = _predict_profiled(m, clib, X, kw)
    assert_same_topk(got, want, exact_scores=True, what="wiki10 shape staged")
    assert ("k1_sparse", leaf) in prof and ("k2_topk", leaf) not in prof, sorted(prof)
    assert {("k0b_remaining_mid", leaf), ("k1_sparse_mid", leaf), ("k2_topk_mid", leaf), ("k0b_remaining", leaf), ("k1_sparse_rest", leaf), ("k2_topk_rest", leaf)} <= prof, sorted(prof)
    clib.set_option(h, "leaf_fuse", 0)
    got0, prof0 = _predict_profiled(m, clib, X, kw)
    assert ("k2_topk", leaf) in prof0, sorted(prof0)
    assert_same_topk(got0, want, exact_scores=True, what="wiki10 shape staged, leaf_fuse=0")
    for pp in ("sigmoid", "log-l1-hinge"):
        kw2 = dict(beam_size=cfg["beam"], only_topk=20, post_processor=pp)
        check_case(m, clib, X, kw2, ref.predict(X, **kw2), leaf, True, f"wiki10 shape {pp}")
    _restore(clib, h)
