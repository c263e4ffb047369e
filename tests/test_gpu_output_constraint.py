"""Output constraint on the device (xrl_set_output_constraint, the constrained route: offsets -> K1P -> K2 over a kept-children view) on the
GPU, through the C ABI: a constrained handle against the oracle on the pruned layers, the compiled reference on the rewritten folder and
this library's fast kernels loaded from that folder; the view against tests/constraint_view.py; the pair kernel's boundaries; shapes,
life cycle, refusals and the device ensemble.

(No entry point hands an initial beam (csr_codes) to a handle that can carry a constraint -- the single-layer API runs on handles of its
own -- so "codes naming a dropped parent" has no test here; a dropped parent's range in the view is empty, which the view tests assert.)"""
import os

import numpy as np
import pytest
import scipy.sparse as smat

import constraint_view as cv
import edge_inputs as ei
import xrl_synth
from conftest import GOLDEN, assert_same_topk, load_X

pytestmark = pytest.mark.gpu

SYNTH = ("s_eurlex", "s_pruned", "s_deep", "s_flat", "s_wide", "s_nobias", "s_contig")
LAYOUTS = ("BINARY_SEARCH_CHUNKED", "HASH_CHUNKED", "CSC")
PPS = ("noop", "l3-hinge", "sigmoid", "log-sigmoid")
KW = dict(beam_size=10, only_topk=10)
CONSTRAINED_NAMES = {"k0_constrained", "k1p_constrained", "k2_constrained"}


@pytest.fixture(scope="module")
def clib():
    from pecos_amd import clib
    assert clib.device_count() > 0, "no GPU visible"
    return clib


@pytest.fixture(scope="module")
def XLM():
    from pecos_amd import XLinearModel
    return XLinearModel


@pytest.fixture(autouse=True)
def _no_warm_up(monkeypatch):
    monkeypatch.setenv("XRL_WARM", "0")      # many tiny models are loaded here: skip the load-time warm-up of the serving path


@pytest.fixture(scope="module")
def goldens(oracle_mod):
    out = {}
    for name in SYNTH:
        folder = os.path.join(GOLDEN, "synth", name)
        layers = oracle_mod.load_model_folder(folder)
        X = load_X(os.path.join(GOLDEN, "synth", name + "__X.npz"))
        out[name] = dict(folder=folder, layers=layers, X=X, Xd=np.ascontiguousarray(X.toarray()), sets=cv.kept_sets(layers[-1]["C"].shape[0], in_tree=layers[-1]["C"].indices))
    return out


def handle(m):
    return m.model.model_chain


def test_the_compiled_reference_takes_part(oracle_mod):
    """Every comparison below has three sides: the oracle, this library's fast kernels, and the compiled reference on the rewritten folder.
    The last one is made only where oracle/_ref is built; where it is not, this test says so instead of letting that side vanish unnoticed."""
    if not oracle_mod.ref_available():
        pytest.skip("oracle/_ref is not built: the comparisons with the compiled reference were NOT made in this run")


def check(a, want, exact, what):
    assert_same_topk(a, smat.csr_matrix(want), exact_scores=exact, what=what)


def references(oracle_mod, layers, folder, layout):
    """(oracle on the pruned layers or None, compiled reference on the rewritten folder or None) for one layout."""
    orc = oracle_mod.OracleModel(layers, layout) if layout != "CSC" else None      # (the restatement has no whole-model CSC arithmetic)
    ref = oracle_mod.RefModel(folder, layout) if oracle_mod.ref_available() else None
    return orc, ref


def check_all(a, orc, ref, fast, Xq, kw, layout, what):
    """A constrained answer against every reference there is.  noop / hinge: bit for bit.  Sigmoid family: the suite's bar against the CPU
    references (same labels, order and counts, scores within 1e-5 relative).  HASH_CHUNKED x dense X: the reference sums in its hash map's
    order; this library gives the BINARY_SEARCH_CHUNKED arithmetic there, which is what the oracle states."""
    exact = "sigmoid" not in (kw.get("post_processor") or "")
    dense = not smat.issparse(Xq)
    if orc is not None:
        check(a, orc.predict(Xq, **kw), exact, "oracle " + what)
    if ref is not None and not (layout == "HASH_CHUNKED" and dense):
        check(a, ref.predict(Xq, **kw), exact, "reference " + what)
    if fast is not None:
        check(a, fast.predict(Xq, **kw), True, "fast kernels " + what)


# ------------------------------------------------------------------------------------------------------------------ 1. main matrix
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SYNTH)
def test_constrained_predict_equals_the_pruned_model(name, layout, goldens, oracle_mod, XLM, clib, tmp_path):
    g = goldens[name]
    m = XLM.load(g["folder"], weight_matrix_type=layout)
    plain = m.predict(g["X"], **KW)
    for sname, labels in g["sets"].items():
        folder = cv.prune_folder(g["folder"], str(tmp_path / sname), labels)
        pruned, _ = cv.prune_layers(g["layers"], labels)
        orc, ref = references(oracle_mod, pruned, folder, layout)
        fast = XLM.load(folder, weight_matrix_type=layout)
        m.set_output_constraint(labels)
        assert clib.output_constraint_info(handle(m))[0]
        for pp in PPS:
            for kind, Xq in (("sparse", g["X"]), ("dense", g["Xd"])):
                kw = dict(KW, post_processor=pp)
                check_all(m.predict(Xq, **kw), orc, ref, fast, Xq, kw, layout, f"{name} {layout} {sname} {pp} {kind}")
    m.set_output_constraint(None)
    check(m.predict(g["X"], **KW), plain, True, f"{name} {layout} after the clear")


def test_labels_the_tree_does_not_hold(goldens, oracle_mod, XLM, clib, tmp_path):
    """s_pruned's tree holds 391 of its 500 labels.  A kept label outside the tree is simply absent; a kept set WITHOUT any label of the tree
    empties every layer: every row comes back empty, as from the reference.  (The fast kernels are not asked about the emptied folder: a
    model without a single child is not something they launch on.)"""
    g = goldens["s_pruned"]
    held = np.unique(g["layers"][-1]["C"].indices)
    absent = np.setdiff1d(np.arange(g["layers"][-1]["C"].shape[0]), held)
    assert len(absent) >= 2
    m = XLM.load(g["folder"])
    for sname, labels, with_fast in (("absent_only", absent[:2], False), ("absent_and_held", np.concatenate([absent[:2], held[::40]]), True)):
        folder = cv.prune_folder(g["folder"], str(tmp_path / sname), labels)
        pruned, _ = cv.prune_layers(g["layers"], labels)
        orc, ref = references(oracle_mod, pruned, folder, "BINARY_SEARCH_CHUNKED")
        fast = XLM.load(folder) if with_fast else None
        m.set_output_constraint(labels)
        for Xq in (g["X"], g["Xd"]):
            a = m.predict(Xq, **KW)
            check_all(a, orc, ref, fast, Xq, KW, "BINARY_SEARCH_CHUNKED", f"s_pruned {sname}")
            assert not (set(a.indices.tolist()) & set(absent.tolist()))
            if not with_fast:
                assert a.nnz == 0 and clib.output_constraint_info(handle(m)) == (True, [0, 0, 0])


# ------------------------------------------------------------------------------------------------------------------ 2. the view
def _odd_tree(folder):
    """Two layers; the four parents of the leaf layer have 63, 64, 65 and 130 children (leaf ids permuted)."""
    xrl_synth.make_model(folder, 80, 322, [20, 8], seed=5, shape=[4, 322], permute_leaf=True)
    f = os.path.join(folder, "ranker", "1.model", "C.npz")
    C = smat.load_npz(f).tocsc()
    C = smat.csc_matrix((C.data, C.indices, np.array([0, 63, 127, 192, 322], dtype=C.indptr.dtype)), shape=C.shape)
    smat.save_npz(f, C, compressed=False)
    return folder


def _view_sets(layers):
    """Kept sets that keep the first child of a range, the last child of a range, no child of a parent, exactly one parent of a layer."""
    C = cv._stored_csc(layers[-1]["C"])
    P = C.shape[1]
    ranges = [C.indices[C.indptr[p]: C.indptr[p + 1]] for p in range(P)]
    full = [r for r in ranges if len(r)]
    sets = {
        "first_of_each": np.array([r[0] for r in full]),
        "last_of_each": np.array([r[-1] for r in full]),
        "first_and_last": np.concatenate([np.array([r[0], r[-1]]) for r in full]),
        "one_parent_whole": full[-1].copy(),
        "all_but_one_parent": np.concatenate(full[1:]) if len(full) > 1 else full[0][1:],
        "every_third": np.arange(0, C.shape[0], 3),
        "position_63_64": np.concatenate([r[63:65] for r in full if len(r) > 64] or [full[0][:1]]),
    }
    return {k: v for k, v in sets.items() if 0 < len(set(v.tolist())) < C.shape[0]}


@pytest.mark.parametrize("tree", ("odd", "flat200", "s_contig", "s_pruned", "s_deep"))
def test_view_equals_the_numpy_rule(tree, oracle_mod, XLM, clib, tmp_path):
    if tree == "odd":
        folder = _odd_tree(str(tmp_path / "odd"))
    elif tree == "flat200":
        folder = str(tmp_path / "flat")
        xrl_synth.make_model(folder, 60, 200, [10], seed=6, shape=[200])
    else:
        folder = os.path.join(GOLDEN, "synth", tree)
    layers = oracle_mod.load_model_folder(folder)
    m = XLM.load(folder)
    h = handle(m)
    bytes_plain = clib.clib_float32.xrl_model_device_bytes(h)
    for sname, labels in _view_sets(layers).items():
        m.set_output_constraint(labels)
        views, kept = cv.view_arrays(layers, labels)
        active, got_kept = clib.output_constraint_info(h)
        assert active and got_kept == kept, f"{tree} {sname}: kept per layer {got_kept} != {kept}"
        for l, want in enumerate(views):
            got = clib.debug_output_constraint_view(h, l, layers[l]["C"].shape[1], kept[l])
            if want is None:
                assert got is None, f"{tree} {sname} layer {l}: a view above the rule's stop"
                continue
            assert got is not None, f"{tree} {sname} layer {l}: no view"
            assert np.array_equal(got[0], want[0]), f"{tree} {sname} layer {l}: chunk_col'"
            assert np.array_equal(got[1], want[1]), f"{tree} {sname} layer {l}: perm_inv'"
        assert clib.clib_float32.xrl_model_device_bytes(h) > bytes_plain, "the view is counted in the handle's bytes"
    m.set_output_constraint(None)
    assert clib.output_constraint_info(h) == (False, [int(L["C"].nnz) for L in layers])
    # (the CSC copy of W the route scores against stays after the clear; the views are gone)
    assert all(clib.debug_output_constraint_view(h, l, layers[l]["C"].shape[1], 0) is None for l in range(len(layers)))


# ------------------------------------------------------------------------------------------------------------------ 3. pair kernel
LENGTHS = (0, 1, 15, 16, 17, 33)


def _boundary_model(folder, bias):
    """[2, 24]: leaf column c holds LENGTHS[c % 6] feature entries (features 0 .. n-1), every second one a bias entry as well (bias > 0)."""
    xrl_synth.make_model(folder, 40, 24, [12, 8], seed=9, shape=[2, 24], bias=bias, post_processor="noop", permute_leaf=True)
    f = os.path.join(folder, "ranker", "1.model", "W.npz")
    rows = 41 if bias > 0 else 40
    rng = np.random.default_rng(3)
    cols_i, cols_v, ptr = [], [], [0]
    for c in range(24):
        n = LENGTHS[c % 6]
        idx = list(range(n))
        if bias > 0 and (c // 6) % 2 == 0:
            idx.append(40)
        cols_i += idx
        cols_v += rng.standard_normal(len(idx)).astype(np.float32).tolist()
        ptr.append(len(cols_i))
    W = smat.csc_matrix((np.array(cols_v, np.float32), np.array(cols_i, np.int32), np.array(ptr, np.int64)), shape=(rows, 24))
    smat.save_npz(f, W, compressed=False)
    return folder


def _boundary_queries():
    rng = np.random.default_rng(4)
    rows = []
    for n in LENGTHS:
        for lo in (0, 5):                                     # rows that start at feature 0 and rows that start past the short columns
            x = np.zeros(40, np.float32)
            x[lo: lo + n] = rng.standard_normal(min(n, 40 - lo)).astype(np.float32)
            rows.append(x)
    X = smat.csr_matrix(np.stack(rows))
    X.sort_indices()
    return X


@pytest.mark.parametrize("bias", (1.0, 0.0))
def test_pair_kernel_boundaries(bias, oracle_mod, XLM, tmp_path):
    folder = _boundary_model(str(tmp_path / "m"), bias)
    layers = oracle_mod.load_model_folder(folder)
    X = _boundary_queries()
    Xd = np.ascontiguousarray(X.toarray())
    assert sorted(set(np.diff(X.indptr).tolist())) == sorted(LENGTHS)
    labels = np.arange(0, 24, 1)[np.arange(24) % 4 != 3]      # 18 of 24 labels: every column length, with and without a bias entry
    pruned, _ = cv.prune_layers(layers, labels)
    pfolder = cv.prune_folder(folder, str(tmp_path / "p"), labels)
    for layout in LAYOUTS:
        m = XLM.load(folder, weight_matrix_type=layout)
        m.set_output_constraint(labels)
        orc, ref = references(oracle_mod, pruned, pfolder, layout)
        fast = XLM.load(pfolder, weight_matrix_type=layout)
        for pp in ("noop", "l3-hinge"):
            for Xq in (X, Xd):
                kw = dict(beam_size=2, only_topk=24, post_processor=pp)
                check_all(m.predict(Xq, **kw), orc, ref, fast, Xq, kw, layout, f"bias={bias} {layout} {pp} {'sparse' if Xq is X else 'dense'}")


@pytest.mark.parametrize("case", [c for c in ei.CASES if c.name in ("cross_flt_min", "neg_zero_weights-half", "neg_zero_weights-all")], ids=lambda c: c.name)
def test_numeric_edges_through_the_constrained_route(case, oracle_mod, XLM, tmp_path):
    folder = ei.build_model(case.model, str(tmp_path / "m"))
    layers = oracle_mod.load_model_folder(folder)
    X = case.queries()
    labels = cv.kept_sets(layers[-1]["C"].shape[0])["every_second"]
    pruned, _ = cv.prune_layers(layers, labels)
    pfolder = cv.prune_folder(folder, str(tmp_path / "p"), labels)
    kw = ei.case_kw(case)
    for layout in LAYOUTS:
        orc, ref = references(oracle_mod, pruned, pfolder, layout)
        if layout == "BINARY_SEARCH_CHUNKED":
            ei.check_precondition(case, orc.predict(X, **kw), "on the pruned model")
        m = XLM.load(folder, weight_matrix_type=layout)
        m.set_output_constraint(labels)
        fast = XLM.load(pfolder, weight_matrix_type=layout)
        for Xq in (X, ei.dense_of(X)):
            check_all(m.predict(Xq, **kw), orc, ref, fast, Xq, kw, layout, f"{case.name} {layout} {'sparse' if Xq is X else 'dense'}")


def test_non_finite_x_touches_matching_entries_only(goldens, oracle_mod, XLM):
    """One NaN and one inf in x at features a kept column holds: every score equals the oracle's (a NaN is a NaN, everything else bit for
    bit), sparse X.  The kept set is smaller than k and the beam wider than every layer, so no ordering of NaN scores enters the answer."""
    g = goldens["s_wide"]
    labels = g["sets"]["six_labels"]
    pruned, _ = cv.prune_layers(g["layers"], labels)
    W = g["layers"][-1]["W"].tocsc()
    feats = W.indices[W.indptr[labels[0]]: W.indptr[labels[0] + 1]]
    feats = feats[feats < g["X"].shape[1]]
    X = g["X"].tolil(copy=True)
    X[0, int(feats[0])] = np.nan
    X[1, int(feats[-1])] = np.inf
    X = X.tocsr().astype(np.float32)
    X.sort_indices()
    kw = dict(beam_size=10, only_topk=10, post_processor="noop")
    m = XLM.load(g["folder"])
    m.set_output_constraint(labels)
    a, b = m.predict(X, **kw), oracle_mod.OracleModel(pruned).predict(X, **kw)
    assert np.array_equal(a.indptr, b.indptr) and (np.diff(a.indptr) < 10).all()
    seen_nan = seen_inf = 0
    for r in range(a.shape[0]):
        da = dict(zip(a.indices[a.indptr[r]: a.indptr[r + 1]].tolist(), a.data[a.indptr[r]: a.indptr[r + 1]].tolist()))
        db = dict(zip(b.indices[b.indptr[r]: b.indptr[r + 1]].tolist(), b.data[b.indptr[r]: b.indptr[r + 1]].tolist()))
        assert set(da) == set(db), f"row {r}"
        for lab, v in da.items():
            w = db[lab]
            if np.isnan(w):
                assert np.isnan(v), f"row {r} label {lab}"
                seen_nan += 1
            else:
                assert np.float32(v).view(np.uint32) == np.float32(w).view(np.uint32), f"row {r} label {lab}: {v} vs {w}"
                seen_inf += int(np.isinf(w))
    assert seen_nan >= 1 and seen_inf >= 1, "the planted NaN / inf did not reach a kept column"
    assert all(np.isfinite(a.data[a.indptr[r]: a.indptr[r + 1]]).all() for r in range(2, a.shape[0])), "a row without a planted value turned non-finite"


# ------------------------------------------------------------------------------------------------------------------ 4. shapes
def test_shapes(goldens, oracle_mod, XLM, clib):
    g = goldens["s_eurlex"]
    labels = g["sets"]["every_second"]
    pruned, _ = cv.prune_layers(g["layers"], labels)
    orc = oracle_mod.OracleModel(pruned)
    m = XLM.load(g["folder"])
    h = handle(m)
    m.set_output_constraint(labels)
    X, Xd = g["X"], g["Xd"]
    for Xq in (X, Xd):
        for n in (0, 1):
            a = m.predict(Xq[:n], **KW)
            assert a.shape[0] == n
            if n:
                check(a, orc.predict(Xq[:n], **KW), True, f"{n} rows")
        X48 = Xq[np.arange(48) % Xq.shape[0]]
        clib.set_option(h, "max_batch_rows", 7)
        check(m.predict(X48, **KW), orc.predict(X48, **KW), True, "max_batch_rows = 7 on 48 rows")
        clib.set_option(h, "overlap_min_rows", 8)
        check(m.predict(X48, **KW), orc.predict(X48, **KW), True, "two lanes, 7-row batches")
        clib.set_option(h, "max_batch_rows", 0)
        check(m.predict(X48, **KW), orc.predict(X48, **KW), True, "two lanes")
        clib.set_option(h, "overlap_min_rows", 0)
        for kw in (dict(beam_size=10, only_topk=1), dict(beam_size=1, only_topk=10), dict(beam_size=64, only_topk=10),
                   dict(beam_size=10, only_topk=70), dict(beam_size=70, only_topk=70)):
            check(m.predict(Xq, **kw), orc.predict(Xq, **kw), True, f"{kw}")
    clib.set_option(h, "k2_big_min_k", 5)                     # the segmented-sort K2 maps positions through the view as well
    check(m.predict(X, **KW), orc.predict(X, **KW), True, "k2_big")
    clib.set_option(h, "k2_big_min_k", 0)


def test_device_entry_points_and_row_ranges(goldens, oracle_mod, XLM, clib):
    import torch
    from pecos_amd.features import predict_from_torch
    g = goldens["s_deep"]
    labels = g["sets"]["ten_percent"]
    pruned, _ = cv.prune_layers(g["layers"], labels)
    X = g["X"]
    want = oracle_mod.OracleModel(pruned).predict(X, **KW)
    m = XLM.load(g["folder"])
    m.set_output_constraint(labels)
    crow, col, val = (torch.from_numpy(X.indptr.astype(np.int64)).cuda(), torch.from_numpy(X.indices.astype(np.int32)).cuda(),
                      torch.from_numpy(X.data.astype(np.float32)).cuda())
    idx, sc, cnt = predict_from_torch(m, crow, col, val, X.shape[1], **KW)
    from pecos_amd.distributed import rows_to_csr
    check(rows_to_csr(idx.cpu().numpy().view(np.uint32), sc.cpu().numpy(), cnt.cpu().numpy(), m.nr_pred_cols), want, True, "xrl_predict_device")
    # xrl_predict_device_rows: rows [5, 5 + 20) only
    h = handle(m)
    q = clib.queries_upload(h, X)
    with clib.freeing(q):
        o_idx = torch.full((X.shape[0], 10), -1, dtype=torch.int32, device="cuda")
        o_sc = torch.zeros((X.shape[0], 10), dtype=torch.float32, device="cuda")
        o_cnt = torch.full((X.shape[0],), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        clib.predict_device_rows(h, q, 10, None, 10, o_idx.data_ptr(), o_sc.data_ptr(), o_cnt.data_ptr(), 10, 5, 20)
        c = o_cnt.cpu().numpy()
        assert (c[:5] == -1).all() and (c[25:] == -1).all()
        part = rows_to_csr(o_idx.cpu().numpy().view(np.uint32)[5:25], o_sc.cpu().numpy()[5:25], c[5:25], m.nr_pred_cols)
        check(part, want[5:25], True, "xrl_predict_device_rows")


# ------------------------------------------------------------------------------------------------------------------ 5. life cycle
def _profile_names(clib, h, fn):
    clib.profile_reset(h)
    clib.profile_enable(h, True)
    fn()
    names = {r["name"] for r in clib.profile_get(h)}
    clib.profile_enable(h, False)
    clib.profile_reset(h)
    return names


def test_life_cycle(goldens, oracle_mod, XLM, clib, monkeypatch):
    import torch
    g = goldens["s_eurlex"]
    X = g["X"]
    m = XLM.load(g["folder"])
    h = handle(m)
    other = XLM.load(g["folder"])                             # never constrained
    plain = other.predict(X, **KW)
    names_plain = _profile_names(clib, other.model.model_chain, lambda: other.predict(X, **KW))
    assert names_plain and not (names_plain & CONSTRAINED_NAMES)

    def oracle(labels):
        return oracle_mod.OracleModel(cv.prune_layers(g["layers"], labels)[0]).predict(X, **KW)

    a, b = g["sets"]["ten_percent"], g["sets"]["every_second"]
    m.set_output_constraint(a)
    check(m.predict(X, **KW), oracle(a), True, "first set")
    names = _profile_names(clib, h, lambda: m.predict(X, **KW))
    assert names == CONSTRAINED_NAMES, names
    m.set_output_constraint(b)
    check(m.predict(X, **KW), oracle(b), True, "second set")
    m.set_output_constraint(None)
    check(m.predict(X, **KW), plain, True, "after the clear")
    assert _profile_names(clib, h, lambda: m.predict(X, **KW)) == names_plain
    # a full set behaves as a clear
    m.set_output_constraint(a)
    m.set_output_constraint(range(m.nr_pred_cols))
    assert clib.output_constraint_info(h)[0] is False
    check(m.predict(X, **KW), plain, True, "after a full set")
    # the device-list form, a torch tensor produced on a side stream, equals the host-list form (int64 and int32 tensors)
    m.set_output_constraint(b)
    want_info, want = clib.output_constraint_info(h), m.predict(X, **KW)
    m.set_output_constraint(None)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t32 = torch.arange(0, m.nr_pred_cols, 2, device="cuda", dtype=torch.int32) + 0
    clib.set_output_constraint_device(h, t32.data_ptr(), t32.numel(), stream=s.cuda_stream)     # the entry point itself, on the side stream
    assert clib.output_constraint_info(h) == want_info
    check(m.predict(X, **KW), want, True, "xrl_set_output_constraint_device")
    m.set_output_constraint(None)
    # ... and through the model's method, which must take that entry point for a tensor on the model's device (never the host list)
    calls = []
    real_dev, real_host = clib.set_output_constraint_device, clib.set_output_constraint
    monkeypatch.setattr(clib, "set_output_constraint_device", lambda *a, **k: (calls.append("device"), real_dev(*a, **k))[1])
    monkeypatch.setattr(clib, "set_output_constraint", lambda *a, **k: (calls.append("host"), real_host(*a, **k))[1])
    for dtype in (torch.int64, torch.int32):
        with torch.cuda.stream(s):
            t = (torch.arange(0, m.nr_pred_cols, 2, device="cuda", dtype=dtype) + 0)
            m.set_output_constraint(t)
        assert clib.output_constraint_info(h) == want_info
        check(m.predict(X, **KW), want, True, f"device list {dtype}")
        m.set_output_constraint(None)
    assert calls == ["device", "device"], calls
    monkeypatch.undo()
    # selected outputs answer as they do without the constraint
    S = smat.csr_matrix((plain.data, plain.indices, plain.indptr), shape=(plain.shape[0], m.nr_pred_cols))
    before = m.predict(X, selected_outputs_csr=S)
    m.set_output_constraint(a)
    check(m.predict(X, selected_outputs_csr=S), before, True, "selected outputs on a constrained handle")


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(goldens, XLM, clib, tmp_path):
    g = goldens["s_eurlex"]
    X = g["X"]
    m = XLM.load(g["folder"])
    h = handle(m)
    a = g["sets"]["ten_percent"]
    m.set_output_constraint(a)
    info, want = clib.output_constraint_info(h), m.predict(X, **KW)
    bad = np.concatenate([a[:3], [m.nr_pred_cols + 5, m.nr_pred_cols], a[3:]]).astype(np.uint32)
    with pytest.raises(RuntimeError, match=r"labels\[3\] = %d is out of range" % (m.nr_pred_cols + 5)):
        clib.set_output_constraint(h, bad)
    with pytest.raises(RuntimeError, match="empty label list"):
        clib.set_output_constraint(h, np.zeros(0, np.uint32))
    with pytest.raises(RuntimeError, match="empty label list"):
        m.set_output_constraint([])
    # the device form refuses the same way: a raw list, and a tensor whose id does not fit 31 bits (it travels as the 32-bit word it is)
    import torch
    d_bad = torch.from_numpy(bad.view(np.int32)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=r"xrl_set_output_constraint_device: labels\[3\] = %d is out of range" % (m.nr_pred_cols + 5)):
        clib.set_output_constraint_device(h, d_bad.data_ptr(), d_bad.numel())
    with pytest.raises(RuntimeError, match=r"labels\[1\] = %d is out of range" % (2**31 + 5)):
        m.set_output_constraint(torch.tensor([int(a[0]), 2**31 + 5, int(a[1])], dtype=torch.int64, device="cuda"))
    assert clib.output_constraint_info(h) == info, "a refused call changed the constraint in force"
    check(m.predict(X, **KW), want, True, "after refused calls")
    q = clib.queries_upload(h, X)
    with clib.freeing(q):
        with pytest.raises(RuntimeError, match="xrl_predict_stats: not available while an output constraint is set"):
            clib.predict_stats(h, q, 10, None, 10)
    with pytest.raises(RuntimeError, match="devices: the handle carries an output constraint"):
        clib.set_option(h, "devices", 2)
    m.set_output_constraint(None)
    clib.set_option(h, "devices", 2)
    with pytest.raises(RuntimeError, match="several devices"):
        m.set_output_constraint(a)
    clib.set_option(h, "devices", 1)
    # mmap handles carry no CSC weights
    mm = str(tmp_path / "mmap")
    XLM.compile_mmap_model(g["folder"], mm)
    m2 = XLM.load(mm)
    with pytest.raises(RuntimeError, match="no CSC weights"):
        m2.set_output_constraint(a)
    check(m2.predict(X, **KW), m.predict(X, **KW), True, "the refused mmap handle still predicts")


# ------------------------------------------------------------------------------------------------------------------ 7. ensemble
def test_two_constrained_models_through_the_device_ensemble(goldens, oracle_mod, XLM):
    import torch
    from pecos_amd.distributed import rows_to_csr
    from pecos_amd.features import ensemble_average, ensemble_device, predict_from_torch
    ga, gb = goldens["s_nobias"], goldens["s_contig"]           # same feature and label counts
    X = ga["X"]
    assert gb["X"].shape[1] == X.shape[1] and ga["layers"][-1]["C"].shape[0] == gb["layers"][-1]["C"].shape[0]
    labels = ga["sets"]["ten_percent"]
    crow, col, val = (torch.from_numpy(X.indptr.astype(np.int64)).cuda(), torch.from_numpy(X.indices.astype(np.int32)).cuda(),
                      torch.from_numpy(X.data.astype(np.float32)).cuda())
    res, want = [], []
    for g in (ga, gb):
        m = XLM.load(g["folder"])
        m.set_output_constraint(labels)
        res.append(predict_from_torch(m, crow, col, val, X.shape[1], **KW))
        want.append(oracle_mod.OracleModel(cv.prune_layers(g["layers"], labels)[0]).predict(X, **KW))
    o = ensemble_device(res, mode="average")
    got = rows_to_csr(o[0].cpu().numpy().view(np.uint32), o[1].cpu().numpy(), o[2].cpu().numpy(), want[0].shape[1])
    check(got, ensemble_average([smat.csr_matrix(w) for w in want]), True, "ensemble of two constrained models")


def test_text2text_under_a_constraint(oracle_mod, XLM, tmp_path):
    """Text2Text.set_output_constraint(items): strings -> ids, unknown strings ignored, every model of the ensemble constrained; the
    predict (tokenise, tf-idf on the device, both beam searches, the device ensemble, threshold and cut) equals Text2Text.finish of the
    oracle's answers on the pruned layers."""
    from pecos_amd.features import Text2Text, Tfidf
    from test_tfidf import _case
    folder, corpus, X = _case("word_bigram_trunc")
    items = [f"item {i}" for i in range(600)]
    models, layers = [], []
    for i, seed in enumerate((81, 82)):
        f = str(tmp_path / f"p{i}")
        xrl_synth.make_model(f, X.shape[1], 600, [120, 60, 20], seed=seed, shape=[6, 48, 600])
        models.append(XLM.load(f)); layers.append(oracle_mod.load_model_folder(f))
    vec = Tfidf.load(folder)
    t2t = Text2Text(vec, [(m, {}) for m in models], items)
    keep = np.arange(0, 600, 7)
    t2t.set_output_constraint([items[i] for i in keep] + ["no such item"])
    Xh = vec.predict(corpus)
    Xh.sort_indices()
    for thr, k in ((None, 6), (0.2, 4)):
        got = t2t.predict(corpus, threshold=thr, beam_size=8, only_topk=k)
        singles = [oracle_mod.OracleModel(cv.prune_layers(L, keep)[0]).predict(Xh, beam_size=8, only_topk=k) for L in layers]
        want = Text2Text.finish([smat.csr_matrix(s) for s in singles], threshold=thr, only_topk=k)
        assert set(got.indices.tolist()) <= set(keep.tolist())
        check(got, want, True, f"Text2Text threshold {thr} only_topk {k}")
    t2t.set_output_constraint(None)
    assert not (set(t2t.predict(corpus, beam_size=8, only_topk=6).indices.tolist()) <= set(keep.tolist())), "the clear did not reach the models"
