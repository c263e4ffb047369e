"""PairwiseANN (K18) without a GPU: the numpy statement of the rule against the compiled reference, the folder reader's refusals, the Python
surface.  The statement and the case makers here are the ones tests/test_gpu_pairwise.py runs the device against."""
import ctypes
import json
import os

import numpy as np
import pytest
import scipy.sparse as smat

import hnsw_rule as hr
from clustering_rule import REF, CsrView, load

F32 = np.float32
KINDS = ("csr", "drm")
CAP, KEEP = 1024, 512          # (test_gpu_pairwise.py checks them against xrl_debug_pairwise_caps)


def statement(X, Yc, Q, keys, k, same=False):
    """predict_single per pair: emplace every entry of the column in stored order, pop to k, sort_heap.
    -> (Imat, Mmat, Dmat, Vmat) [batch, k] with zeros beyond each pair's entries, and (sorted, stream, replay, second_pass) the device must count."""
    out = [np.zeros((len(keys), k), dtype=t) for t in (np.uint32, np.uint32, F32, F32)]
    forms = [0, 0, 0, 0]
    row = (lambda M, r: (M.indices[M.indptr[r]:M.indptr[r + 1]], M.data[M.indptr[r]:M.indptr[r + 1]])) if smat.issparse(X) else (lambda M, r: M[r])
    for b, l in enumerate(keys):
        q, span = row(Q, 0 if same else b), slice(Yc.indptr[l], Yc.indptr[l + 1])
        rows, vals = Yc.indices[span], Yc.data[span]
        with np.errstate(over="ignore", invalid="ignore"):
            d = np.array([hr.sparse_dist(*q, *row(X, r), False) for r in rows], dtype=F32) if smat.issparse(X) else hr.dense_dist(q, X[rows], False)
        h = []
        for p in range(len(rows)):
            h.append((d[p], p))
            hr.push_heap(h, "max")
        while k < len(rows) and len(h) > k:
            hr.pop_heap(h, len(h), "max")
            h.pop()
        hr.sort_heap(h)
        for t, (dd, p) in enumerate(h):
            out[0][b, t], out[1][b, t], out[2][b, t], out[3][b, t] = rows[p], 1, dd, vals[p]
        n, first = len(rows), np.sort(d)[:min(len(rows), k + 1)]
        ordered = not np.isnan(d).any() and len(np.unique(first)) == len(first)
        parallel = n <= CAP or k + 1 <= KEEP
        forms[(0 if n <= CAP else 1) if parallel and ordered else 2] += 1
        forms[3] += int(n > CAP and k + 1 <= KEEP and not ordered)
    return out, tuple(forms)


def items(kind, n, dim, seed):
    """n rows of distinct random values; a sparse row always stores id 0, so no two distances to a query that stores id 0 tie by sharing nothing."""
    rs = np.random.RandomState(seed)
    A = rs.randn(n, dim).astype(F32)
    if kind == "drm":
        return A
    A *= rs.rand(n, dim) < 0.25
    A[:, 0] = rs.randn(n).astype(F32) + F32(3)
    return smat.csr_matrix(A)


def columns(n_rows, lengths, seed, value=None):
    """Y_csc [n_rows, len(lengths)]: column l holds lengths[l] different rows in a random order."""
    rs = np.random.RandomState(seed)
    ind = np.concatenate([rs.permutation(n_rows)[:n] for n in lengths] + [np.zeros(0, int)]).astype(np.int32)
    data = rs.rand(len(ind)).astype(F32) if value is None else np.full(len(ind), value, dtype=F32)
    return smat.csc_matrix((data, ind, np.cumsum([0] + list(lengths))), shape=(n_rows, len(lengths)))


def same_outputs(got, want):
    return all(np.array_equal(np.asarray(g).view(np.uint32), np.asarray(w).view(np.uint32)) for g, w in zip(got, want))


def _view(M):
    keep = (M.indptr.astype(np.uint64), M.indices.astype(np.uint32), M.data.astype(F32)) if smat.issparse(M) else (np.ascontiguousarray(M, dtype=F32),)
    return (CsrView if smat.issparse(M) else hr.DrmView)(M.shape[0], M.shape[1], *(a.ctypes.data for a in keep)), keep


def can_witness(kind):
    return hr.have_reference() and (kind == "csr" or hr.host_has_avx512f())


class Reference(object):
    """c_pairwise_ann_{train,load,save,predict,...}_{csr,drm}_ip_f32 of the compiled reference."""

    def __init__(self, kind, X=None, Yc=None, folder=None):
        lib, vp = load(REF), ctypes.c_void_p
        self.fn = {n: getattr(lib, "c_pairwise_ann_%s_%s_ip_f32" % (n, kind)) for n in ("train", "load", "save", "destruct", "searchers_create", "searchers_destruct", "predict")}
        for n, (res, args) in dict(train=(vp, [vp, vp]), load=(vp, [ctypes.c_char_p, ctypes.c_bool]), save=(None, [vp, ctypes.c_char_p]), destruct=(None, [vp]),
                                   searchers_create=(vp, [vp, ctypes.c_uint32]), searchers_destruct=(None, [vp]),
                                   predict=(None, [vp, ctypes.c_uint32, ctypes.c_uint32] + [vp] * 6 + [ctypes.c_bool])).items():
            self.fn[n].restype, self.fn[n].argtypes = res, args
        if folder is None:
            (vx, kx), (vy, ky) = _view(X), _view(Yc)
            self.h = self.fn["train"](ctypes.byref(vx), ctypes.byref(vy))
        else:
            self.h = self.fn["load"](os.path.join(folder, "c_model").encode(), False)

    def predict(self, Q, keys, k, same=False, searchers=1):
        out = [np.zeros((len(keys), k), dtype=t) for t in (np.uint32, np.uint32, F32, F32)]
        s, (vq, kq), keys = self.fn["searchers_create"](self.h, searchers), _view(Q), np.ascontiguousarray(keys, dtype=np.uint32)
        self.fn["predict"](s, len(keys), k, ctypes.byref(vq), keys.ctypes.data, *(o.ctypes.data for o in out), same)
        self.fn["searchers_destruct"](s)
        return out

    def save(self, folder):
        os.makedirs(folder, exist_ok=True)
        self.fn["save"](self.h, os.path.join(folder, "c_model").encode())


def tie_case(kind, where, n, k=10, dim=19, seed=5):
    """One column of n rows under query row 0, with X rows repeated so that two distances tie inside the kept set, across rank k / k + 1, only
    beyond rank k + 1, or everywhere (all rows equal).  -> X, Yc, Q."""
    X, Q, Yc = items(kind, n, dim, seed), items(kind, 1, dim, seed + 1), columns(n, [n], seed + 2)
    A = X.toarray() if kind == "csr" else X
    if where == "everywhere":
        A[:] = A[0]
    else:
        order = np.argsort(hr.dense_dist(Q.toarray()[0] if kind == "csr" else Q[0], A, False), kind="stable")   # (any ranking of distinct rows serves)
        r = {"inside": 3, "across": k - 1, "beyond": k + 1}[where]
        A[order[r + 1]] = A[order[r]]
    return (smat.csr_matrix(A) if kind == "csr" else A), Yc, Q


NAN_ROWS = ["nan", "0.5", "lo", "nan2", "hi", "0.25", "0.5", "-1.0"]


def nan_case(kind):
    """A column whose distances under the query (2, 2, 0, 1) hold inf + -inf (the host's default NaN), both infinities and a tie."""
    X = hr._rows(hr.kind_rows(NAN_ROWS), 4, kind)
    return X, columns(len(NAN_ROWS), [len(NAN_ROWS), 3], 2), hr._rows(hr.KIND_QUERIES[:2], 4, kind)


# ------------------------------------------------------------------------------------------------ the statement against the compiled reference
@pytest.mark.parametrize("kind", KINDS)
def test_statement_is_the_reference(kind):
    if not can_witness(kind):
        pytest.skip("the compiled reference (and avx512f for dense rows) is not here")
    lengths = [0, 1, 2, 9, 10, 11, 63, 64, 65, 300]
    X, Yc, Q = items(kind, 300, 19, 1), columns(300, lengths, 2), items(kind, len(lengths), 19, 3)
    keys = np.arange(len(lengths), dtype=np.uint32)
    for k in (1, 10):
        assert same_outputs(Reference(kind, X, Yc).predict(Q, keys, k), statement(X, Yc, Q, keys, k)[0])
    for where in ("inside", "across", "beyond", "everywhere"):
        X, Yc, Q = tie_case(kind, where, 40)
        assert same_outputs(Reference(kind, X, Yc).predict(Q, np.zeros(1, np.uint32), 10), statement(X, Yc, Q, [0], 10)[0]), where
    X, Yc, Q = nan_case(kind)
    keys = np.array([0, 1], dtype=np.uint32)
    for k in (3, 8):
        assert same_outputs(Reference(kind, X, Yc).predict(Q, keys, k), statement(X, Yc, Q, keys, k)[0])


def test_statement_expects_the_forms():
    X, Yc, Q = tie_case("drm", "beyond", 40)
    assert statement(X, Yc, Q, [0], 10)[1] == (1, 0, 0, 0)
    X, Yc, Q = tie_case("drm", "across", CAP + 40)
    assert statement(X, Yc, Q, [0], 10)[1] == (0, 0, 1, 1)
    assert statement(X, Yc, Q, [0], KEEP)[1] == (0, 0, 1, 0)
    assert statement(*nan_case("csr"), [0, 1], 8)[1][2] >= 1


# ------------------------------------------------------------------------------------------------ the folder reader, no GPU
def write_folder(folder, kind, X, Yc, pairwise_ann_t=None, version="v1.0", patch=None):
    """c_model/{config.json, index.mmap_store} as PairwiseANN::save writes them; patch(dict of parts) may damage the parts."""
    from pecos_amd.pairwise import PairwiseANN  # noqa: F401  (the module exists)
    os.makedirs(os.path.join(folder, "c_model"), exist_ok=True)
    t = {"csr": "pecos::ann::PairwiseANN<pecos::ann::FeatVecSparseIPSimd<uint32_t, float>, pecos::csr_t>",
         "drm": "pecos::ann::PairwiseANN<pecos::ann::FeatVecDenseIPSimd<float>, pecos::drm_t>"}[kind]
    parts = dict(y_ptr=Yc.indptr.astype(np.uint64), y_idx=Yc.indices.astype(np.uint32), y_val=Yc.data.astype(F32), x_val=(X.data if kind == "csr" else X.ravel()).astype(F32))
    if kind == "csr":
        parts.update(x_ptr=X.indptr.astype(np.uint64), x_idx=X.indices.astype(np.uint32))
    if patch:
        patch(parts)
    s = hr._Store()
    for v in (X.shape[0], Yc.shape[1], X.shape[1], Yc.shape[0], Yc.shape[1]):
        s.u32(v)
    s.put(np.uint64(len(parts["y_idx"])).tobytes())
    for name in ("y_ptr", "y_idx", "y_val"):
        s.put(parts[name].tobytes())
    s.u32(X.shape[0]), s.u32(X.shape[1])
    s.put(np.uint64(len(parts["x_val"])).tobytes())
    for name in (("x_ptr", "x_idx", "x_val") if kind == "csr" else ("x_val",)):
        s.put(parts[name].tobytes())
    open(os.path.join(folder, "c_model", "index.mmap_store"), "wb").write(s.tobytes())
    cfg = {"pairwise_ann_t": pairwise_ann_t or t, "train_params": {}}
    if version is not None:
        cfg["version"] = version
    json.dump(cfg, open(os.path.join(folder, "c_model", "config.json"), "w"), indent=4)
    return os.path.join(folder, "c_model")


def _set(name, at, value):
    def patch(parts):
        parts[name] = parts[name].copy()
        parts[name][at] = value
    return patch


@pytest.mark.parametrize("kind", KINDS)
def test_check_folder_reads_and_refuses(tmp_path, kind):
    from pecos_amd import clib
    X, Yc = items(kind, 30, 7, 1), columns(30, [0, 4, 30], 2)
    info = clib.pairwise_check_folder(write_folder(str(tmp_path / "ok"), kind, X, Yc))
    assert (info["num_input_keys"], info["num_label_keys"], info["feat_dim"], info["data_type"], info["nnz_of_Y"], info["max_col"]) == (30, 3, 7, kind, 34, 30)
    refusals = [(dict(pairwise_ann_t="pecos::ann::PairwiseANN<other>"), "Inconsistent PairwiseANN_T: .* inp = pecos::ann::PairwiseANN<other>"),
                (dict(version="v0.9"), "Unable to load memory-mapped file with version = v0.9"),
                (dict(version=None), "Unable to load memory-mapped file with version = not found"),
                (dict(patch=_set("y_idx", 5, 30)), "Y has a row id at or above X_trn.rows = 30"),
                (dict(patch=_set("x_val", 3, np.inf)), "a value of X_trn is not finite")]
    if kind == "csr":
        r = int(np.argmax(np.diff(X.indptr) >= 2))       # a row of two ids or more
        refusals += [(dict(patch=_set("x_idx", X.indptr[r] + 1, X.indices[X.indptr[r]])), "unsorted or repeated column ids"),
                     (dict(patch=_set("x_idx", X.indptr[r + 1] - 1, 7)), "at or above feat_dim = 7")]
    for n, (kw, message) in enumerate(refusals):
        with pytest.raises(RuntimeError, match=message):
            clib.pairwise_check_folder(write_folder(str(tmp_path / str(n)), kind, X, Yc, **kw))


# ------------------------------------------------------------------------------------------------ the Python surface, no GPU
def test_python_surface_messages_and_defaults(tmp_path):
    from pecos_amd.pairwise import PairwiseANN
    assert PairwiseANN.TrainParams().to_dict() == {"metric_type": "ip"}
    assert PairwiseANN.PredParams().to_dict() == {"batch_size": 1024, "only_topk": 10}
    X, Y = items("drm", 4, 3, 1), columns(4, [2], 2)
    with pytest.raises(ValueError, match="type\\(Y\\) should be either a csr_matrix or csc_matrix"):
        PairwiseANN.train(X, Y.toarray())
    with pytest.raises(ValueError, match="is NOT supported"):
        PairwiseANN.train([[1.0]], Y)
    with pytest.raises(NotImplementedError, match="data_type=drm and metric_type=l2 not implemented"):
        PairwiseANN.train(X, Y, train_params={"metric_type": "l2"})
    json.dump({"model": "HNSW"}, open(tmp_path / "param.json", "w"))
    with pytest.raises(ValueError, match="param\\[model\\] != cls.__name__"):
        PairwiseANN.load(str(tmp_path))
    json.dump({"model": "PairwiseANN", "data_type": "drm", "metric_type": "ip"}, open(tmp_path / "param.json", "w"))
    with pytest.raises(ValueError, match="c_model_dir did not exist"):
        PairwiseANN.load(str(tmp_path))
    model = PairwiseANN(None, 4, 1, 3, "drm")
    searchers = type("S", (), {"pred_params": PairwiseANN.PredParams(batch_size=2)})()
    for args, err, message in (((X.astype(np.float32), np.zeros(4, np.uint32), searchers), ValueError, "cur_batch_size > searchers.batch_size"),
                               ((smat.csr_matrix(X), np.zeros(4, np.uint32), searchers), ValueError, "data_type=csr is NOT consistent"),
                               ((X[:, :2].copy(), np.zeros(4, np.uint32), searchers), ValueError, "input_feat_py.cols=2 is NOT consistent"),
                               ((X, [0, 0, 0, 0], searchers), TypeError, "type\\(label_keys\\) != np.array"),
                               ((X, np.zeros(3, np.uint32), searchers), ValueError, "input_feat_py.rows != label_keys.shape\\[0\\]")):
        with pytest.raises(err, match=message):
            model.predict(*args)
    with pytest.raises(ValueError, match="self.model_ptr must exist"):
        model.searchers_create()
