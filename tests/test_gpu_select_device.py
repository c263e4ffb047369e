"""Selected outputs on the device (xrl_predict_selected_device: K7 plans the reference's tree walk, K4 scores it, nothing visits the host) on the
GPU: parity with the oracle, the reference where built, and the host route; the row shapes at which the plan kernel can go wrong; composition
with xrl_predict_device; flagged rows; a caller's stream and the profile; argument checks with a live handle."""
import os

import numpy as np
import pytest
import scipy.sparse as smat

import select_plan as sp
from conftest import GOLDEN, assert_same_topk, load_X
from device_views import SENT_IDX, SENT_VAL, assert_bands_intact, sentinel_out

pytestmark = pytest.mark.gpu

SYNTH = ("s_eurlex", "s_contig", "s_deep", "s_nobias", "s_flat", "s_wide")
EXACT_PP = lambda pp: pp is None or "sigmoid" not in pp          # noqa: E731
PREFIX = "xrl_predict_selected_device: "


@pytest.fixture(scope="module")
def clib():
    from pecos_amd import clib
    assert clib.device_count() > 0, "no GPU visible"
    return clib


class Loaded:
    """A golden model on the device and beside it: handle, oracle, tree arrays, queries (host, and uploaded sparse / dense)."""

    def __init__(self, clib, oracle_mod, name):
        from pecos_amd import XLinearModel
        folder = os.path.join(GOLDEN, "synth", name)
        self.name, self.clib = name, clib
        self.m = XLinearModel.load(folder)
        self.h = self.m.model.model_chain
        self.layers = oracle_mod.load_model_folder(folder)
        self.om = oracle_mod.OracleModel(self.layers)
        self.rm = oracle_mod.RefModel(folder, "CSC") if oracle_mod.ref_available() else None
        self.tree = sp.tree_arrays(self.layers)
        self.depth = len(self.layers)
        self.nr = self.m.nr_pred_cols
        self.X = load_X(os.path.join(GOLDEN, "synth", name + "__X.npz"))
        self.Xd = np.ascontiguousarray(self.X.toarray())
        self.q = {"sparse": clib.queries_upload(self.h, self.X), "dense": clib.queries_upload(self.h, self.Xd)}
        self.default_exact = all("sigmoid" not in L["post_processor"] for L in self.layers)

    def close(self):
        for q in self.q.values():
            self.clib.queries_free(q)

    def rows_of_X(self, n):
        """(sparse, dense, handles) of the first n query rows, cycling when the golden has fewer."""
        pick = np.arange(n) % self.X.shape[0]
        Xs = self.X[pick].tocsr()
        Xs.sort_indices()
        Xn = np.ascontiguousarray(Xs.toarray())
        return Xs, Xn


@pytest.fixture(scope="module")
def loaded(clib, oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Loaded(clib, oracle_mod, name)
        return cache[name]
    yield get
    for v in cache.values():
        v.close()


def run(clib, h, q, idx, cnt, pp=None, out_stride=None, stream=None, sync=True, out=None, status=None):
    """One call on host arrays idx int32 [n, stride] / cnt int32 [n] or None; returns (rc, message, (o_idx, o_val, o_cnt) tensors)."""
    import torch
    n, stride = idx.shape
    out_stride = out_stride or stride
    d_idx = torch.from_numpy(np.ascontiguousarray(idx)).cuda()
    d_cnt = torch.from_numpy(np.ascontiguousarray(cnt)).cuda() if cnt is not None else None
    if out is None:
        out = (torch.full((n, out_stride), SENT_IDX, dtype=torch.int32, device="cuda"),
               torch.full((n, out_stride), SENT_VAL, dtype=torch.float32, device="cuda"),
               torch.full((n,), -1, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    lib = clib.clib_float32
    import ctypes
    vp = ctypes.c_void_p
    rc = lib.xrl_predict_selected_device(vp(h), vp(q), pp.encode() if pp else None, vp(d_idx.data_ptr()), vp(d_cnt.data_ptr() if d_cnt is not None else 0),
                                         stride, vp(out[0].data_ptr()), vp(out[1].data_ptr()), vp(out[2].data_ptr()), out_stride,
                                         vp(status.data_ptr() if status is not None else 0), vp(stream or 0), 1 if sync else 0)
    err = lib.xrl_last_error()
    lib.xrl_clear_error()
    run.keep = (d_idx, d_cnt)                             # alive until the caller has synchronised an asynchronous call
    return rc, (err or b"").decode(), out


def to_csr(out, n_cols):
    """The fixed-stride device result as CSR in the STORED order; entries beyond a row's count are not looked at."""
    idx, val, cnt = out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy(), out[2].cpu().numpy().astype(np.int64)
    assert (cnt >= 0).all() and (cnt <= idx.shape[1]).all(), cnt
    mask = np.arange(idx.shape[1])[None, :] < cnt[:, None]
    S = smat.csr_matrix((idx.shape[0], n_cols), dtype=np.float32)
    S.indptr, S.indices, S.data = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), idx[mask].astype(np.int64), val[mask]
    return S


def untouched_beyond_counts(out):
    idx, val, cnt = out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy()
    tail = np.arange(idx.shape[1])[None, :] >= cnt[:, None]
    return (idx[tail] == SENT_IDX).all() and (val[tail] == np.float32(SENT_VAL)).all()


# ------------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", SYNTH)
def test_parity_with_oracle_reference_and_host_route(name, loaded, clib):
    import torch
    from pecos_amd.features import predict_selected_from_torch
    L = loaded(name)
    T = L.om.predict(L.X, beam_size=6, only_topk=8)      # the pattern of test_predict_on_selected_outputs: the oracle's top-8
    S = smat.csr_matrix((T.data, T.indices, T.indptr), shape=(T.shape[0], L.nr))
    rows = [S.indices[S.indptr[r]: S.indptr[r + 1]].astype(np.uint32)[::-1] for r in range(S.shape[0])]     # (score order reversed: any order will do)
    idx, cnt = sp.fixed_stride(rows, 8, fill=0)
    crow = torch.from_numpy(L.X.indptr.astype(np.int64)).cuda()
    col = torch.from_numpy(L.X.indices.astype(np.int32)).cuda()
    val = torch.from_numpy(L.X.data.astype(np.float32)).cuda()
    for pp in (None, "sigmoid", "log-l2-hinge", "noop"):
        exact = EXACT_PP(pp) and (pp is not None or L.default_exact)
        kw = {"post_processor": pp} if pp else {}
        for kind, Xq in (("sparse", L.X), ("dense", L.Xd)):
            what = f"{name} {pp} {kind}"
            rc, err, out = run(clib, L.h, L.q[kind], idx, cnt, pp)
            assert rc == 0, err
            a = to_csr(out, L.nr)
            assert_same_topk(a, L.om.predict_on_selected_outputs(Xq, S, pp), exact_scores=exact, what="oracle " + what)
            if L.rm is not None:
                assert_same_topk(a, L.rm.predict_on_selected_outputs(Xq, S, pp), exact_scores=exact, what="ref " + what)
            assert_same_topk(a, L.m.predict(Xq, selected_outputs_csr=S, **kw), exact_scores=True, what="host route " + what)
        t = predict_selected_from_torch(L.m, crow, col, val, L.X.shape[1], torch.from_numpy(idx).cuda(), torch.from_numpy(cnt).cuda(), post_processor=pp)
        assert t[0].shape == (len(rows), 8) and t[0].dtype == torch.int32 and t[1].dtype == torch.float32
        assert_same_topk(to_csr(t, L.nr), L.m.predict(L.X, selected_outputs_csr=S, **kw), exact_scores=True, what=f"from_torch {name} {pp}")
    if name == "s_eurlex":
        _from_torch_with_embedding_block(L, clib)


def _from_torch_with_embedding_block(L, clib):
    """predict_selected_from_torch(emb=...): [X_feat | X_emb] assembled on the device, then K7 + K4.  The last H feature columns play the
    embedding block (+ 0.25: no cell is zero), the labels are the model's own top 7; labels, order and score bits must be the host route's on
    the same matrix -- concat_features' for normalize_emb=False, and for True the matrix the device assembled (read back), because the device
    normalisation is only within 1e-6 of sklearn's."""
    import torch
    from pecos_amd.features import concat_features, predict_selected_from_torch
    H, D = 24, L.X.shape[1]
    X_feat = L.X[:, : D - H].tocsr(); X_feat.sort_indices()
    emb = np.ascontiguousarray(L.X[:, D - H:].toarray()) + np.float32(0.25)
    host_cat = concat_features(X_feat, emb, normalize_emb=False)
    T = L.m.predict(host_cat, only_topk=7)
    S = smat.csr_matrix((T.data, T.indices, T.indptr), shape=(T.shape[0], L.nr))
    idx, cnt = sp.fixed_stride([S.indices[S.indptr[r]: S.indptr[r + 1]].astype(np.uint32) for r in range(S.shape[0])], 7, fill=0)
    crow = torch.from_numpy(X_feat.indptr.astype(np.int64)).cuda()
    col = torch.from_numpy(X_feat.indices.astype(np.int32)).cuda()
    val = torch.from_numpy(X_feat.data.astype(np.float32)).cuda()
    temb = torch.from_numpy(emb).cuda()
    q = clib.queries_concat_device(L.h, X_feat.shape[0], D - H, crow.data_ptr(), col.data_ptr(), val.data_ptr(), int(X_feat.nnz), H, temb.data_ptr(),
                                   normalize_emb=True)
    try:
        device_cat = clib.queries_download(q)
    finally:
        clib.queries_free(q)
    assert device_cat.shape == host_cat.shape and np.array_equal(device_cat.indices, host_cat.indices)
    for normalize, X_cat in ((False, host_cat), (True, device_cat)):
        t = predict_selected_from_torch(L.m, crow, col, val, D - H, torch.from_numpy(idx).cuda(), torch.from_numpy(cnt).cuda(), emb=temb,
                                        normalize_emb=normalize)
        assert t[0].shape == (S.shape[0], 7)
        assert_same_topk(to_csr(t, L.nr), L.m.predict(X_cat, selected_outputs_csr=S), exact_scores=True, what=f"from_torch emb normalize_emb={normalize}")


# ------------------------------------------------------------------------------------------------------------------ 2. row shapes
def _special_rows(L, cap):
    """Rows of at most `cap` labels: all under one leaf parent; under pairwise different top-level ancestors."""
    parent = L.tree[-1][0]
    kids = np.flatnonzero(parent == np.bincount(parent[parent != sp.NONE]).argmax()).astype(np.uint32)
    top = np.arange(len(parent), dtype=np.int64)
    for l in range(len(L.tree) - 1, 0, -1):
        top = L.tree[l][0][top].astype(np.int64)
    _, first = np.unique(top, return_index=True)
    return kids[:cap], first.astype(np.uint32)[:cap]


STRIDES = (64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024)      # 64 NS and 64 NS + 1 (the next instantiation); 64 NS - 1 is a row length below


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("name", ("s_deep", "s_wide"))
def test_row_shapes(name, stride, loaded, clib):
    L = loaded(name)
    rng = np.random.default_rng(stride)
    full = min(stride, L.nr)
    lengths = sorted({0, 1, 63, 64, min(65, full), full - 1, full})
    rows = [rng.permutation(rng.choice(L.nr, n, replace=False)).astype(np.uint32) for n in lengths]
    rows.append(np.sort(rng.choice(L.nr, full, replace=False)).astype(np.uint32)[::-1])         # given descending
    rows.extend(_special_rows(L, full))
    Xs, Xn = L.rows_of_X(len(rows))
    S = sp.rows_to_csr(rows, L.nr)
    want = L.m.predict(Xs, selected_outputs_csr=S)
    assert_same_topk(want, L.om.predict_on_selected_outputs(Xs, S), exact_scores=L.default_exact, what=f"{name}: host route vs oracle")
    for r, lab in enumerate(rows):                                                               # the order is the numpy plan's, too
        assert np.array_equal(want.indices[want.indptr[r]: want.indptr[r + 1]].astype(np.uint32), sp.plan_order(L.tree, lab, L.nr))
    q = clib.queries_upload(L.h, Xs)
    try:
        idx, cnt = sp.fixed_stride(rows, stride, fill=0x7FFFFFFF)                               # the filler behind a row is no label: never read
        # out_stride > sel_stride, sentinel-filled banded outputs at odd offsets: slots beyond each count and the bands stay untouched
        (wi, oi), (wv, ov), (wc, oc) = sentinel_out(len(rows), stride + 3, elem_offsets=(1, 2, 3))
        rc, err, out = run(clib, L.h, q, idx, cnt, out_stride=stride + 3, out=(oi, ov, oc))
        assert rc == 0, err
        assert_same_topk(to_csr(out, L.nr), want, exact_scores=True, what=f"{name} stride {stride}")
        assert untouched_beyond_counts(out)
        assert_bands_intact(wi, oi, np.int32(SENT_IDX), "labels"); assert_bands_intact(wv, ov, np.float32(SENT_VAL), "scores")
        assert_bands_intact(wc, oc, np.int32(SENT_IDX), "counts")
        # a count above the stride is the stride; no counts at all = the stride in every row
        fulls = [r for r in rows if len(r) == full]
        if full == stride:
            qf = clib.queries_upload(L.h, Xs[: len(fulls)])
            try:
                fi, fc = sp.fixed_stride(fulls, stride)
                wantf = L.m.predict(Xs[: len(fulls)], selected_outputs_csr=sp.rows_to_csr(fulls, L.nr))
                for c in (fc + 5, None):
                    rc, err, out = run(clib, L.h, qf, fi, c)
                    assert rc == 0, err
                    assert_same_topk(to_csr(out, L.nr), wantf, exact_scores=True, what=f"{name} stride {stride} counts {'above' if c is not None else 'null'}")
            finally:
                clib.queries_free(qf)
    finally:
        clib.queries_free(q)


def test_rows_in_batches(loaded, clib):
    # max_batch_rows (the option the beam search's batching observes): 3 rows per batch, the scratch rows restart at every batch
    L = loaded("s_deep")
    rows = sp.random_rows(np.arange(L.nr, dtype=np.uint32), lengths=(5, 0, 40, 33, 1, 40, 17, 2), seed=3)
    Xs, _ = L.rows_of_X(len(rows))
    want = L.m.predict(Xs, selected_outputs_csr=sp.rows_to_csr(rows, L.nr))
    q = clib.queries_upload(L.h, Xs)
    try:
        idx, cnt = sp.fixed_stride(rows, 40)
        clib.set_option(L.h, "max_batch_rows", 3)
        rc, err, out = run(clib, L.h, q, idx, cnt)
        assert rc == 0, err
        assert_same_topk(to_csr(out, L.nr), want, exact_scores=True, what="batches of 3 rows")
    finally:
        clib.set_option(L.h, "max_batch_rows", 0)
        clib.queries_free(q)


# ------------------------------------------------------------------------------------------------------------------ 3. composition
@pytest.mark.parametrize("name", ("s_eurlex", "s_deep"))
def test_rescoring_the_models_own_topk(name, loaded, clib):
    import torch
    L = loaded(name)
    n = L.X.shape[0]
    idx = torch.zeros((n, 8), dtype=torch.int32, device="cuda"); val = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    cnt = torch.zeros((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    clib.predict_device(L.h, L.q["sparse"], 6, None, 8, idx.data_ptr(), val.data_ptr(), cnt.data_ptr(), 8)
    o = (torch.zeros_like(idx), torch.zeros_like(val), torch.zeros_like(cnt))
    torch.cuda.synchronize()
    clib.predict_selected_device(L.h, L.q["sparse"], None, idx.data_ptr(), cnt.data_ptr(), 8, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), 8)
    top, sel = to_csr((idx, val, cnt), L.nr), to_csr(o, L.nr)
    assert np.array_equal(top.indptr, sel.indptr)
    for r in range(n):
        a, b = slice(top.indptr[r], top.indptr[r + 1]), slice(sel.indptr[r], sel.indptr[r + 1])
        assert set(top.indices[a].tolist()) == set(sel.indices[b].tolist()), f"row {r}: label sets"
    assert np.allclose(sel.toarray(), top.toarray(), atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------ 4. bad rows
def _bad_case(L, kind, n_rows=9, stride=8):
    rng = np.random.default_rng(11)
    pool = sp.rooted_labels(L.tree)
    rows = [rng.choice(pool, rng.integers(1, stride + 1), replace=False).astype(np.uint32) for _ in range(n_rows)]

    def spoil(r):
        lab = rows[r][: stride - 1].copy()
        if kind == "twice":
            return np.concatenate([lab, lab[:1]])
        if kind == "range":
            return np.concatenate([lab, [L.nr]]).astype(np.uint32)
        orphans = np.setdiff1d(np.arange(L.nr, dtype=np.uint32), pool)
        return np.concatenate([lab, orphans[:1]])
    return rows, spoil


@pytest.mark.parametrize("kind, model, code, words", [("twice", "s_deep", sp.TWICE, "holds a label twice"),
                                                     ("range", "s_deep", sp.OUT_OF_RANGE, "label id out of range"),
                                                     ("orphan", "s_pruned", sp.NO_PARENT, "has no parent in layer")])
def test_bad_rows(kind, model, code, words, loaded, clib):
    # flagged inputs: the kernel bounds-checks before it indexes
    import torch
    from pecos_amd.core import ScipyCompressedSparseAllocator
    L = loaded(model)
    rows, spoil = _bad_case(L, kind)
    Xs, _ = L.rows_of_X(len(rows))
    q = clib.queries_upload(L.h, Xs)
    try:
        for bad in ([0], [len(rows) // 2], [len(rows) - 1], [6, 2]):
            given = [spoil(r) if r in bad else rows[r] for r in range(len(rows))]
            idx, cnt = sp.fixed_stride(given, 8)
            first = min(bad)
            # the host route refuses the same input in the same words
            with pytest.raises(RuntimeError, match=words) as host:
                S = smat.csr_matrix((len(rows), L.nr), dtype=np.float32)
                S.indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
                S.indices = np.concatenate([g for g in given]).astype(np.int64); S.data = np.ones(len(S.indices), np.float32)
                L.clib.xlinear_predict_on_selected_outputs(L.h, Xs, S, None, -1, ScipyCompressedSparseAllocator())
            rc, err, _ = run(clib, L.h, q, idx, cnt, sync=True)
            assert rc == -1 and words in err, (rc, err)
            if len(bad) == 1:
                assert err == str(host.value), (err, str(host.value))
            status = torch.full((2,), 77, dtype=torch.int32, device="cuda")
            rc, err, out = run(clib, L.h, q, idx, cnt, sync=False, status=status)
            torch.cuda.synchronize()
            assert rc == 0 and err == "", (rc, err)
            assert status.cpu().numpy().view(np.uint32).tolist() == [code, first]
            got = to_csr(out, L.nr)
            good = [r for r in range(len(rows)) if r not in bad]
            want = L.om.predict_on_selected_outputs(Xs[good], sp.rows_to_csr([rows[r] for r in good], L.nr))
            for r in bad:
                assert got.indptr[r + 1] == got.indptr[r], f"bad row {r} has a count"
            assert_same_topk(_take_rows(got, good), want, exact_scores=L.default_exact, what=f"{kind} in rows {bad}: the other rows")
            assert untouched_beyond_counts(out)
        # no bad row: {0, 0xFFFFFFFF}
        status = torch.full((2,), 77, dtype=torch.int32, device="cuda")
        idx, cnt = sp.fixed_stride(rows, 8)
        rc, err, out = run(clib, L.h, q, idx, cnt, sync=False, status=status)
        torch.cuda.synchronize()
        assert rc == 0 and status.cpu().numpy().view(np.uint32).tolist() == [0, 0xFFFFFFFF]
    finally:
        clib.queries_free(q)


def _take_rows(M, keep):
    """Rows `keep` of a CSR in stored order."""
    parts = [(M.indices[M.indptr[r]: M.indptr[r + 1]], M.data[M.indptr[r]: M.indptr[r + 1]]) for r in keep]
    S = smat.csr_matrix((len(keep), M.shape[1]), dtype=np.float32)
    S.indptr = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int64)
    S.indices = np.concatenate([p[0] for p in parts]).astype(np.int64) if parts else np.zeros(0, np.int64)
    S.data = np.concatenate([p[1] for p in parts]).astype(np.float32) if parts else np.zeros(0, np.float32)
    return S


# ------------------------------------------------------------------------------------------------------------------ 5. stream, profile
def test_side_stream_without_sync_and_profile(loaded, clib):
    import torch
    L = loaded("s_deep")
    rows = sp.random_rows(np.arange(L.nr, dtype=np.uint32), lengths=(7, 0, 30, 12, 30), seed=5)
    Xs, _ = L.rows_of_X(len(rows))
    want = L.m.predict(Xs, selected_outputs_csr=sp.rows_to_csr(rows, L.nr))
    q = clib.queries_upload(L.h, Xs)
    s = torch.cuda.Stream()
    try:
        idx, cnt = sp.fixed_stride(rows, 30)
        clib.profile_enable(L.h, True); clib.profile_reset(L.h)
        rc, err, out = run(clib, L.h, q, idx, cnt, stream=s.cuda_stream, sync=False)
        assert rc == 0, err
        s.synchronize()
        assert_same_topk(to_csr(out, L.nr), want, exact_scores=True, what="side stream")
        prof = clib.profile_get(L.h)
        plan = [p for p in prof if p["name"] == "k7_select_plan"]
        score = [p for p in prof if p["name"] == "k4_selected_dev"]
        assert len(plan) == 1 and plan[0]["launches"] == 1, prof
        assert sorted(p["layer"] for p in score) == list(range(L.depth)) and all(p["launches"] == 1 for p in score), prof
        assert {p["name"] for p in prof} == {"k7_select_plan", "k4_selected_dev"}, prof        # nothing of the host route, nothing else
    finally:
        clib.profile_reset(L.h); clib.profile_enable(L.h, False)
        clib.queries_free(q)


# ------------------------------------------------------------------------------------------------------------------ 6. argument checks
def test_argument_checks_with_a_live_handle(loaded, clib, manifest):
    L = loaded("s_eurlex")
    idx = np.zeros((L.X.shape[0], 8), np.int32)
    clib.profile_enable(L.h, True); clib.profile_reset(L.h)
    try:
        import ctypes
        vp, lib = ctypes.c_void_p, clib.clib_float32
        for stride, out_stride, words in ((0, 8, "sel_stride must be 1..1024, got 0"), (1025, 1025, "sel_stride must be 1..1024, got 1025"),
                                          (8, 7, "out_stride 7 smaller than sel_stride 8")):
            # (made-up array addresses: the call is refused before it looks at them)
            rc = lib.xrl_predict_selected_device(vp(L.h), vp(L.q["sparse"]), None, vp(0x1000), None, stride, vp(0x1000), vp(0x1000), vp(0x1000), out_stride,
                                                 None, None, 1)
            err = (lib.xrl_last_error() or b"").decode(); lib.xrl_clear_error()
            assert rc == -1 and err.startswith(PREFIX) and words in err, (rc, err)
        # the feature dimension, as the host route checks it
        Xbad = smat.csr_matrix((L.X.shape[0], L.X.shape[1] + 3), dtype=np.float32)
        qb = clib.queries_upload(L.h, Xbad)
        try:
            rc, err, _ = run(clib, L.h, qb, idx, None)
            assert rc == -1 and err == PREFIX + "Feature dimension of query matrix does not match weight matrix", (rc, err)
        finally:
            clib.queries_free(qb)
        assert clib.profile_get(L.h) == []                    # refused before any launch
    finally:
        clib.profile_reset(L.h); clib.profile_enable(L.h, False)
    # mmap handles carry no CSC weights: refused like the host entry point refuses them
    mm = [c for c in manifest["mmap"] if c["kind"] == "synth"]
    if mm:
        from pecos_amd import XLinearModel
        m = XLinearModel.load(os.path.join(GOLDEN, "mmap", mm[0]["model"]))
        X = load_X(os.path.join(GOLDEN, "synth", mm[0]["model"] + "__X.npz"))
        q = clib.queries_upload(m.model.model_chain, X)
        try:
            rc, err, _ = run(clib, m.model.model_chain, q, np.zeros((X.shape[0], 4), np.int32), None)
            assert rc == -1 and err == PREFIX + "predict_on_selected_outputs: the layer's CSC weights are not available", (rc, err)
        finally:
            clib.queries_free(q)
