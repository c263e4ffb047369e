"""GPU (-m gpu): the device-resident entry points on buffers the CALLER owns (xrl_queries_from_device_csr / _drm, xrl_queries_tfidf_device,
xrl_queries_concat_device_ex, xrl_predict_device[_rows]).  The rest of the suite hands over freshly allocated tensors only: 512-byte aligned,
followed by allocator slack, result stride == k.  Here every input is a view at an odd element offset inside a larger tensor of the test's whose
other elements are poison (tests/device_views.py: quiet NaNs, valid feature ids that carry weights, row pointer 0), the arrays END where the
entry point was told they end, and every output sits between bands of a sentinel with a row stride larger than k.  A kernel that reads a
neighbour's data computes something else than the oracle (tests/test_caller_buffers_cpu.py shows that for every cut point); one that writes a
neighbour's data breaks a band, a column >= k or a row outside the range.  Nothing here can fault unless the library has an addressing bug: the
test allocates everything a documented over-read may touch, and the one null-pointer case (all rows empty, nnz == 0) was added after reading
that no kernel dereferences col / val of an empty row (K1Q: no chunk; K1 / K1T: load_features runs only while some item has features left;
K1C: the shorter list is streamed; xguard: no element).

Kernel families and layouts come from FAMILIES of test_gpu_numeric_edges.py; element offsets rotate over the families like the fuzz rotates its
lookups."""
import os

import numpy as np
import pytest
import scipy.sparse as smat

import device_views as V
from conftest import GOLDEN, assert_same_topk, load_raw_csr
from test_caller_buffers_cpu import model_case
from test_gpu_numeric_edges import BSC, FAMILIES, Family, _Applied, _rescore_csc

pytestmark = pytest.mark.gpu

KW = dict(beam_size=10, only_topk=10)                     # the goldens' first case
SPARSE_FAMS = [f for f in FAMILIES if f.xkind == "sparse"]
DENSE_FAMS = [f for f in FAMILIES if f.xkind == "dense"]
SPARSE_MODELS = ("s_eurlex", "s_deep", "s_wide", "s_flat", "odd_d")
DENSE_MODELS = ("s_eurlex", "s_deep", "odd_d")


@pytest.fixture(scope="module")
def clib():
    from pecos_amd import clib
    assert clib.device_count() > 0, "no GPU visible"
    return clib


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    """A device fault is a finding, not a reason to go on launching kernels: the session ends with the test that met it."""
    import torch
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"device fault: {err}", returncode=3)


@pytest.fixture(scope="module")
def loaded(tmp_path_factory, clib):
    """(model name, layout) -> (folder, golden / seeded X, XLinearModel); only the current model's handles stay alive (each reserves pinned staging)."""
    from pecos_amd import XLinearModel
    root = tmp_path_factory.mktemp("caller")
    state = {"model": None, "h": {}}

    def get(model, layout=BSC):
        if state["model"] != model:
            state["h"].clear()
            state["model"] = model
        folder, X = fuse_case(root) if model == "fuse" else model_case(model, root)
        if layout not in state["h"]:
            state["h"][layout] = XLinearModel.load(folder, weight_matrix_type=layout)
        return folder, X, state["h"][layout]
    return get


def fuse_case(root):
    """One tile of 24 columns per leaf parent: the model shape of test_leaf_fuse.py on which the fused leaf (K1T with the selecting epilogue) runs."""
    import xrl_synth
    folder = os.path.join(str(root), "fuse")
    if not os.path.isdir(folder):
        xrl_synth.make_model(folder, 300, 12 * 24, [80, 60, 20], seed=85, shape=[4, 12, 12 * 24], permute_leaf=True)
    X = xrl_synth.make_queries(60, 300, 20, seed=62, relabel_seed=85).astype(np.float32)
    X.sort_indices()
    return folder, X


def _golden(model, xkind):
    import json
    for c in json.load(open(os.path.join(GOLDEN, "manifest.json")))["synth"]:
        if c["model"] == model and c["x"] == xkind and c["kwargs"] == KW:
            return load_raw_csr(os.path.join(GOLDEN, "preds", c["pred"]))
    return None


class _Expect:
    """What rows [b, e) of the queries must come out as, for one layout: the C restatement (oracle_mod.OracleModel).  It has no whole-model CSC
    arithmetic: for that layout the compiled reference answers when it is built; else the scores are re-scored through the restatement's CSC
    route on the returned pattern and labels / order / bits are those of the library's own host-ABI predict, which uploads the rows itself."""

    def __init__(self, oracle_mod, folder, layout, m, X, kw):
        self.orc = oracle_mod.OracleModel.load(folder, layout if layout != "CSC" else BSC)
        self.X, self.kw = X, kw
        if layout != "CSC":
            self.want = self.orc.predict(X, **kw)
        else:
            self.want = oracle_mod.RefModel(folder, "CSC").predict(X, **kw) if oracle_mod.ref_available() else None
        self.clean = m.predict(X, **kw) if self.want is None else None

    def check(self, got, b, e, what):
        if self.want is not None:
            assert_same_topk(got, self.want[b:e], exact_scores=True, what=what)
            return
        assert_same_topk(got, self.clean[b:e], exact_scores=True, what=what + " vs the host-ABI predict")
        if got.nnz:
            a, r = _rescore_csc(self.orc, self.X[b:e], got, self.kw.get("post_processor"))
            assert np.array_equal(a.view(np.uint32), r.view(np.uint32)), f"{what}: scores differ from the restated CSC route"


def _predict(clib, h, q, n, k, kw, b=0, e=None, out=None, stride=None):
    """Rows [b, e) of query handle q into banded sentinel buffers of n rows: predict_device for the whole range, predict_device_rows otherwise."""
    import torch
    e = n if e is None else e
    out = out or V.sentinel_out(n, stride or k)
    (wi, pi), (wv, pv), (wc, pc) = out
    torch.cuda.synchronize()
    args = (h, q, kw["beam_size"], kw.get("post_processor"), kw["only_topk"], V.addr(pi), V.addr(pv), V.addr(pc), pi.shape[1])
    if (b, e) == (0, n):
        clib.predict_device(*args, sync=True)
    else:
        clib.predict_device_rows(*args, b, e - b, sync=True)
    return out


def _rows(out, b, e, k, n_cols):
    from pecos_amd.distributed import rows_to_csr
    (_, pi), (_, pv), (_, pc) = out
    cnt = pc[b:e].cpu().numpy()
    assert ((cnt >= 0) & (cnt <= k)).all(), f"row counts outside [0, {k}]: {cnt[(cnt < 0) | (cnt > k)][:4]}"
    return rows_to_csr(pi[b:e, :k].cpu().numpy().view(np.uint32), pv[b:e, :k].cpu().numpy(), cnt, n_cols)


def _assert_untouched(out, b, e, k, what):
    """Columns >= k of every row, the rows outside [b, e) and both bands of the three buffers still hold the sentinel."""
    (wi, pi), (wv, pv), (wc, pc) = out
    idx, val, cnt = pi.cpu().numpy(), pv.cpu().numpy(), pc.cpu().numpy()
    outside = np.ones(idx.shape[0], bool); outside[b:e] = False
    assert (idx[:, k:] == V.SENT_IDX).all() and (val[:, k:] == V.SENT_VAL).all(), f"{what}: a column >= k = {k} was written"
    assert (idx[outside] == V.SENT_IDX).all() and (val[outside] == V.SENT_VAL).all() and (cnt[outside] == V.SENT_IDX).all(), f"{what}: a row outside [{b}, {e}) was written"
    V.assert_bands_intact(wi, pi, np.int32(V.SENT_IDX), what + " labels")
    V.assert_bands_intact(wv, pv, np.float32(V.SENT_VAL), what + " scores")
    V.assert_bands_intact(wc, pc, np.int32(V.SENT_IDX), what + " counts")


class _SparseViews:
    """Banded device copies of X[:R] for (col offset, val offset, crow offset, R), made once: everything behind indptr[R] is poison."""

    def __init__(self, X):
        self.X, self.made = X, {}

    def get(self, offs, crow_off, R):
        key = (offs, crow_off, R)
        if key not in self.made:
            X, D = self.X, self.X.shape[1]
            nnz = int(X.indptr[R])
            self.made[key] = (V.banded(X.indptr[: R + 1].astype(np.int64), crow_off, 16, V.poison_like("rowptr"), "cuda"),
                              V.banded(X.indices[:nnz].astype(np.int32), offs[0], V.BAND, V.poison_like("index", D), "cuda"),
                              V.banded(X.data[:nnz].astype(np.float32), offs[1], V.BAND, V.poison_like("value"), "cuda"), nnz)
        return self.made[key]

    def assert_intact(self):
        D = self.X.shape[1]
        for key, (crow, col, val, _) in self.made.items():
            V.assert_bands_intact(*crow, V.poison_like("rowptr"), f"crow {key}")
            V.assert_bands_intact(*col, V.poison_like("index", D), f"col {key}")
            V.assert_bands_intact(*val, V.poison_like("value"), f"val {key}")


# ------------------------------------------------------------------------------------------------------------------ 1: sparse X
@pytest.mark.parametrize("model", SPARSE_MODELS)
def test_sparse_x_cut_and_windowed_between_poison(model, loaded, clib, oracle_mod):
    mi = SPARSE_MODELS.index(model)
    X0 = loaded(model)[1]
    X, cuts = V.with_tails(X0)
    n0, D = X0.shape[0], X0.shape[1]
    views = _SparseViews(X)
    golden = _golden(model, "sparse")
    assert golden is not None or model == "odd_d"
    # every family on s_eurlex; on the other models a rotating quarter of them plus the CSC and HASH_CHUNKED layouts
    fams = [(i, f) for i, f in enumerate(SPARSE_FAMS) if model == "s_eurlex" or f.layout != BSC or i % 4 == mi % 4]
    expect, ran = {}, []
    for i, fam in fams:
        folder, _, m = loaded(model, fam.layout)
        h = m.model.model_chain
        k = clib.effective_topk(h, KW["only_topk"])
        if fam.layout not in expect:
            expect[fam.layout] = _Expect(oracle_mod, folder, fam.layout, m, X, KW)
        ex = expect[fam.layout]
        offs, crow_off = V.SPARSE_OFFSETS[i % 4], (i // 4) % 2
        with _Applied(clib, h, fam):
            for R in cuts:
                (_, crow), (_, col), (_, val), nnz = views.get(offs, crow_off, R)
                what = f"{model} [{fam.name}] col+{offs[0]} val+{offs[1]} crow+{crow_off} rows {R} nnz {nnz}"
                q = clib.queries_from_device_csr(h, R, D, V.addr(crow), V.addr(col), V.addr(val), nnz)
                out = _predict(clib, h, q, R, k, KW)
                clib.queries_free(q)
                got = _rows(out, 0, R, k, m.nr_pred_cols)
                ex.check(got, 0, R, what)
                if golden is not None and fam.layout == BSC:
                    assert_same_topk(got[:n0], golden, exact_scores=True, what=what + " vs the recorded reference predictions")
                _assert_untouched(out, 0, R, k, what)
            # the no-copy row window: row_ptr advanced to row r0, col / val bases unchanged, nnz the total
            for r0, R in ((3, cuts[i % 8]), (n0 + 2 + i % 5, cuts[-1])):
                (_, crow), (_, col), (_, val), nnz = views.get(offs, crow_off, R)
                what = f"{model} [{fam.name}] col+{offs[0]} val+{offs[1]} crow+{crow_off} window [{r0}, {R})"
                q = clib.queries_from_device_csr(h, R - r0, D, V.addr(crow) + 8 * r0, V.addr(col), V.addr(val), nnz)
                out = _predict(clib, h, q, R - r0, k, KW)
                clib.queries_free(q)
                ex.check(_rows(out, 0, R - r0, k, m.nr_pred_cols), r0, R, what)
                _assert_untouched(out, 0, R - r0, k, what)
        ran.append(fam.name)
    views.assert_intact()
    print(f"\nCALLER-BUFFERS sparse {model}: {len(ran)} families x {len(cuts)} cuts + 2 windows: {', '.join(ran)}")


NULL_FAMS = [Family("defaults", {}, None, "sparse", BSC), Family("tile format leaf_fuse=1", dict(dense_layers=0, adaptive=0, leaf_fuse=1), None, "sparse", BSC),
             Family("tile format leaf_fuse=0", dict(dense_layers=0, adaptive=0, leaf_fuse=0), None, "sparse", BSC),
             Family("CSC (K1C)", {}, None, "sparse", "CSC"), Family("HASH_CHUNKED", {}, None, "sparse", "HASH_CHUNKED")]


def test_all_rows_empty_with_null_col_and_val(loaded, clib, oracle_mod):
    # nnz == 0: xrl_queries_from_device_csr accepts null col / val; no kernel may form an address from them (see the module docstring)
    n = 5
    for model in ("s_eurlex", "s_flat"):
        D = loaded(model)[1].shape[1]
        X = smat.csr_matrix((n, D), dtype=np.float32)
        for fam in NULL_FAMS:
            folder, _, m = loaded(model, fam.layout)
            h = m.model.model_chain
            k = clib.effective_topk(h, KW["only_topk"])
            ex = _Expect(oracle_mod, folder, fam.layout, m, X, KW)
            wc, crow = V.banded(np.zeros(n + 1, np.int64), 1, 16, V.poison_like("rowptr"), "cuda")
            with _Applied(clib, h, fam):
                q = clib.queries_from_device_csr(h, n, D, V.addr(crow), 0, 0, 0)
                out = _predict(clib, h, q, n, k, KW, stride=k + 3)
                clib.queries_free(q)
            what = f"{model} [{fam.name}] all rows empty, null col / val"
            ex.check(_rows(out, 0, n, k, m.nr_pred_cols), 0, n, what)
            _assert_untouched(out, 0, n, k, what)


# ------------------------------------------------------------------------------------------------------------------ 2: dense X
def _profiled(clib, h, fn):
    clib.profile_reset(h); clib.profile_enable(h, True)
    try:
        r = fn()
        return r, {(p["name"], int(p["layer"])) for p in clib.profile_get(h) if p["launches"] > 0}
    finally:
        clib.profile_enable(h, False)


@pytest.mark.parametrize("model", DENSE_MODELS)
def test_dense_x_at_element_offsets_inside_nan(model, loaded, clib, oracle_mod):
    X0 = loaded(model)[1]
    X, _ = V.with_tails(X0)
    Xd = np.ascontiguousarray(X.toarray())
    n, D = Xd.shape
    golden = _golden(model, "dense")
    bufs = {eo: V.banded(Xd[: n - eo], eo, 2 * D, V.poison_like("value"), "cuda") for eo in range(4)}     # (the buffer ends behind row n - eo - 1)
    expect, ran = {}, []
    for fam in DENSE_FAMS:
        folder, _, m = loaded(model, fam.layout)
        h = m.model.model_chain
        k = clib.effective_topk(h, KW["only_topk"])
        if fam.layout not in expect:
            expect[fam.layout] = _Expect(oracle_mod, folder, fam.layout, m, Xd, KW)
        is_k1g = fam.opts.get("k1g_min_items") == 1
        with _Applied(clib, h, fam):
            for eo, (whole, view) in bufs.items():
                R = n - eo
                what = f"{model} [{fam.name}] dense X + {eo} elements, rows {R}"
                q = clib.queries_from_device_drm(h, R, D, V.addr(view))
                out, prof = _profiled(clib, h, lambda: _predict(clib, h, q, R, k, KW))
                clib.queries_free(q)
                if is_k1g:       # otherwise a silent fall-back would hide the kernel
                    assert any(name == "k1g_dense_x" for name, _ in prof), f"{what}: k1g_dense_x did not run: {sorted(prof)}"
                got = _rows(out, 0, R, k, m.nr_pred_cols)
                expect[fam.layout].check(got, 0, R, what)
                if golden is not None and fam.layout == BSC:
                    assert_same_topk(got[: X0.shape[0]], golden, exact_scores=True, what=what + " vs the recorded reference predictions")
                _assert_untouched(out, 0, R, k, what)
        ran.append(fam.name)
    for eo, (whole, view) in bufs.items():
        V.assert_bands_intact(whole, view, V.poison_like("value"), f"dense X + {eo}")
    print(f"\nCALLER-BUFFERS dense {model}: offsets 0..3 x {len(ran)} families: {', '.join(ran)}")


# ------------------------------------------------------------------------------------------------------------------ 3: results
_TILE = dict(dense_layers=0, adaptive=0)
# (name, model, layout, dense X, options, launches the profile must show on the LAST layer (name prefixes), launches it must not show there)
ROUTES = [("K1Q last layer", "s_eurlex", BSC, False, dict(dense_layers=2), ("k1q",), ("k2_topk",)),
          ("K2", "s_eurlex", BSC, False, dict(_TILE, leaf_fuse=0), ("k2_topk",), ()),
          ("k2_big_min_k=1", "s_eurlex", BSC, False, dict(_TILE, leaf_fuse=0, k2_big_min_k=1), ("k2_topk",), ()),
          ("leaf_fuse", "fuse", BSC, False, dict(_TILE, leaf_fuse=1), ("k1_sparse",), ("k2_topk",)),
          ("K1G + K2", "s_eurlex", BSC, True, dict(k1g_min_items=1), ("k1g_dense_x", "k2_topk"), ()),
          ("CSC", "s_eurlex", "CSC", False, {}, ("k1c_csc", "k2_topk"), ()),
          ("s_flat", "s_flat", BSC, False, {}, (), ())]


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_result_rows_between_sentinels(route, loaded, clib, oracle_mod):
    import torch
    from pecos_amd.distributed import PackedTopk
    name, model, layout, dense, opts, must, must_not = route
    folder, X0, m = loaded(model, layout)
    h = m.model.model_chain
    Xs, _ = V.with_tails(X0)
    Xq = np.ascontiguousarray(Xs.toarray()) if dense else Xs
    n = Xq.shape[0]
    last = clib.xlinear_get_int_attr(h, "depth") - 1
    fam = Family(name, opts, None, "dense" if dense else "sparse", layout)
    q = clib.queries_upload(h, Xq)
    try:
        for topk in (9, 10):                                     # odd k: PackedTopk's score pointer base + 4k is only 4-byte aligned
            kw = dict(beam_size=6, only_topk=topk)
            k = clib.effective_topk(h, topk)
            assert k == topk
            ex = _Expect(oracle_mod, folder, layout, m, Xq, kw)
            with _Applied(clib, h, fam):
                # (a) separate buffers at odd element offsets, row stride k + 3: the whole range, and a range with row_begin > 0
                for j, (b, e) in enumerate(((0, n), (7, n - 5))):
                    what = f"{name}: k {k} stride {k + 3} rows [{b}, {e})"
                    bufs = V.sentinel_out(n, k + 3, elem_offsets=((1, 3, 2), (3, 2, 1))[j])
                    out, prof = _profiled(clib, h, lambda: _predict(clib, h, q, n, k, kw, b, e, out=bufs))
                    on_last = {nm for nm, l in prof if l == last} | {nm for nm, l in prof if nm.startswith("k1q_fused") and nm.endswith(f"_{last}")}
                    for want in must:
                        assert any(nm.startswith(want) for nm in on_last), f"{what}: no {want}* launch on the last layer: {sorted(prof)}"
                    for bad in must_not:
                        assert bad not in on_last, f"{what}: a {bad} launch wrote the last layer: {sorted(prof)}"
                    ex.check(_rows(out, b, e, k, m.nr_pred_cols), b, e, what)
                    _assert_untouched(out, b, e, k, what)
                # (b) the layout of PackedTopk.pointers(): labels and scores interleaved in ONE buffer of row stride 2k + 1, the score pointer
                #     base + 4k; column 2k is the slot gather() folds the count into -- a label store one column too far lands in the scores
                for parts in (1, 2):
                    pk = PackedTopk(np.array([0, n]), 0, k, torch.device("cuda", 0), parts=parts)
                    held = []
                    for p in range(parts):
                        shape = tuple(pk.buf[p].shape)
                        held.append(V.banded(np.full(shape, V.SENT_IDX, np.int32), (1, 3)[p], V.BAND, np.int32(V.SENT_IDX), "cuda"))
                        pk.buf[p] = held[p][1]
                    wc, pc = V.banded(np.full(tuple(pk.cnt.shape), V.SENT_IDX, np.int32), 1, V.BAND, np.int32(V.SENT_IDX), "cuda")
                    pk.cnt = pc
                    torch.cuda.synchronize()
                    for p in range(parts):
                        b, e = pk.rows(p)
                        pi, pv, pcn, ps = pk.pointers(p)
                        assert ps == 2 * k + 1 and pv == pi + 4 * k
                        if parts == 1:
                            clib.predict_device(h, q, 6, None, topk, pi, pv, pcn, ps, sync=True)
                        else:
                            clib.predict_device_rows(h, q, 6, None, topk, pi, pv, pcn, ps, b, e - b, sync=True)
                    cnt = pc.cpu().numpy()
                    assert ((cnt >= 0) & (cnt <= k)).all()
                    for p in range(parts):
                        b, e = pk.rows(p)
                        what = f"{name}: k {k} packed, part {p} of {parts}, rows [{b}, {e})"
                        buf = pk.buf[p].cpu().numpy()
                        assert (buf[:, 2 * k] == V.SENT_IDX).all(), f"{what}: the count column was written"
                        assert (buf[e - b:] == V.SENT_IDX).all(), f"{what}: rows behind the part were written"
                        from pecos_amd.distributed import rows_to_csr
                        got = rows_to_csr(buf[: e - b, :k].view(np.uint32), np.ascontiguousarray(buf[: e - b, k: 2 * k]).view(np.float32), cnt[b:e], m.nr_pred_cols)
                        ex.check(got, b, e, what)
                        V.assert_bands_intact(*held[p], np.int32(V.SENT_IDX), what)
                    V.assert_bands_intact(wc, pc, np.int32(V.SENT_IDX), f"{name}: k {k} packed counts")
    finally:
        clib.queries_free(q)
    print(f"\nCALLER-BUFFERS results {name}: k 9 and 10, strided + packed (1 and 2 parts), predict_device and predict_device_rows")


# ------------------------------------------------------------------------------------------------------------------ 4: tf-idf weighting
def test_tfidf_device_banded_three_destinations(manifest, loaded, clib):
    import torch
    from test_abi_and_host import _tfidf_case
    h = loaded("s_flat")[2].model.model_chain            # (the producer takes the device and the stream from the handle; nothing is predicted)
    names = [c["name"] for c in manifest["tfidf"]]
    assert "addone_trigram" in names and "sublinear" in names
    for ci, c in enumerate(manifest["tfidf"]):
        counts, want, kw = _tfidf_case(c)
        rows, D = counts.shape
        nnz = int(counts.nnz)
        if c["name"] == "addone_trigram":
            lens = np.diff(counts.indptr)
            assert (lens == 0).any() and (lens == 64).any() and (lens > 64).any()
        offs, crow_off = V.SPARSE_OFFSETS[ci % 4], ci % 2
        wr, crow = V.banded(counts.indptr.astype(np.int64), crow_off, 16, V.poison_like("rowptr"), "cuda")
        wc, col = V.banded(counts.indices.astype(np.int32), offs[0], V.BAND, V.poison_like("index", D), "cuda")
        idf = V.banded(kw["idf"].astype(np.float32), (ci + 1) % 4, V.BAND, V.poison_like("value"), "cuda") if kw["idf"] is not None else None
        for dest in ("handle", "caller", "in place"):
            wv, cnt = V.banded(counts.data.astype(np.float32), offs[1], V.BAND, V.poison_like("value"), "cuda")
            wo = po = None
            if dest == "caller":
                wo, po = V.banded(np.full(nnz, V.SENT_VAL, np.float32), (offs[1] + 1) % 4 or 1, V.BAND, np.float32(V.SENT_VAL), "cuda")
            out_addr = None if dest == "handle" else V.addr(po) if dest == "caller" else V.addr(cnt)
            torch.cuda.synchronize()
            q = clib.queries_tfidf_device(h, rows, D, V.addr(crow), V.addr(col), V.addr(cnt), nnz, V.addr(idf[1]) if idf else None,
                                          kw["binary"], kw["sublinear_tf"], 1 if kw["norm"] == "l1" else 2, out_addr=out_addr)
            got = clib.queries_download(q)
            clib.queries_free(q)
            what = f"tf-idf {c['name']} -> {dest}"
            assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), what
            views = [got.data] + ([po.cpu().numpy()] if dest == "caller" else []) + ([cnt.cpu().numpy()] if dest == "in place" else [])
            for data in views:
                assert np.array_equal(data.view(np.uint32), want.data.view(np.uint32)), what          # (sublinear_tf included)
            if dest != "in place":
                assert np.array_equal(cnt.cpu().numpy().view(np.uint32), counts.data.astype(np.float32).view(np.uint32)), f"{what}: the counts were changed"
            V.assert_bands_intact(wv, cnt, V.poison_like("value"), what + " counts")       # (in place: the elements past nnz)
            if wo is not None:
                V.assert_bands_intact(wo, po, np.float32(V.SENT_VAL), what + " d_out")
        V.assert_bands_intact(wr, crow, V.poison_like("rowptr"), c["name"] + " crow")
        V.assert_bands_intact(wc, col, V.poison_like("index", D), c["name"] + " col")
        if idf:
            V.assert_bands_intact(*idf, V.poison_like("value"), c["name"] + " idf")


# ------------------------------------------------------------------------------------------------------------------ 5: [X_feat | X_emb]
@pytest.mark.parametrize("dense_cols", [1, 63, 64, 65])
def test_concat_device_banded(dense_cols, loaded, clib):
    import torch
    from pecos_amd.features import concat_features
    _, X0, m = loaded("s_eurlex")
    h = m.model.model_chain
    X, _ = V.with_tails(X0)
    n, D = X.shape
    emb = (np.random.default_rng(300 + dense_cols).standard_normal((n, dense_cols)) + 0.01).astype(np.float32)
    i = (1, 63, 64, 65).index(dense_cols)
    offs = V.SPARSE_OFFSETS[i]
    wr, crow = V.banded(X.indptr.astype(np.int64), 1 - i % 2, 16, V.poison_like("rowptr"), "cuda")
    wc, col = V.banded(X.indices.astype(np.int32), offs[0], V.BAND, V.poison_like("index", D), "cuda")
    wv, val = V.banded(X.data.astype(np.float32), offs[1], V.BAND, V.poison_like("value"), "cuda")
    we, temb = V.banded(emb, (1, 3, 1, 2)[i], V.BAND, V.poison_like("value"), "cuda")
    torch.cuda.synchronize()
    for norm in (False, True):
        z = concat_features(X, emb, normalize_emb=norm)
        q = clib.queries_concat_device(h, n, D, V.addr(crow), V.addr(col), V.addr(val), int(X.nnz), dense_cols, V.addr(temb), normalize_emb=norm)
        got = clib.queries_download(q)
        clib.queries_free(q)
        what = f"concat dense_cols {dense_cols} normalize_emb={norm}"
        assert got.shape == z.shape and np.array_equal(got.indptr, z.indptr) and np.array_equal(got.indices, z.indices), what
        is_emb = got.indices >= D
        assert np.array_equal(got.data[~is_emb].view(np.uint32), z.data[~is_emb].view(np.uint32)), what
        if norm:                                  # the bound of test_device_concat_vs_reference_concat_features
            assert np.all(np.abs(got.data[is_emb] - z.data[is_emb]) <= 1e-6 * np.abs(z.data[is_emb]) + 1e-30), what
        else:
            assert np.array_equal(got.data[is_emb].view(np.uint32), z.data[is_emb].view(np.uint32)), what
    for whole, view, fill, nm in ((wr, crow, V.poison_like("rowptr"), "crow"), (wc, col, V.poison_like("index", D), "col"),
                                  (wv, val, V.poison_like("value"), "val"), (we, temb, V.poison_like("value"), "emb")):
        V.assert_bands_intact(whole, view, fill, f"concat dense_cols {dense_cols} {nm}")
