"""Matcher-aware negatives (K14, the resident single-layer predict, train_chain_device): the statement of the union rule in numpy, the
reference's layer loop (pecos/xmc/base.py:1512-1572) in scipy with the layer predict and the layer trainer passed in as functions -- so it
runs over the reference's library, this library's host entry points, or anything else --, and the case generators of the tests."""
import os
import sys

import numpy as np
import scipy.sparse as smat

import ranker_training_rule as rr

F32 = np.float32
REFPY = os.path.join(rr.REPO, "oracle", "_ref", "refpy")
CAP = 1024
SCHEMES = {"tfn+man": "tfn+man", "man": "man", "usn+tfn+man": "usn+tfn+man", "perlayer": ["tfn", "tfn", "tfn+man"]}
POST = ("l3-hinge", "noop")
TRAIN_KW = dict(threshold=rr.E2E_KW["threshold"], max_iter=rr.E2E_KW["max_iter"], solver_type=rr.E2E_KW["solver_type"])


# ------------------------------------------------------------------------------------------------ the union
def raw_csr(shape, rows):
    """A CSR from per-row (column ids, values) kept exactly as given: unsorted ids, duplicates and explicit zeros stay."""
    ptr, ind, val = [0], [], []
    for ids, vs in rows:
        ind.extend(ids); val.extend(vs); ptr.append(len(ind))
    m = smat.csr_matrix(shape, dtype=F32)
    m.indptr, m.indices, m.data = np.array(ptr, np.int64), np.array(ind, np.int64), np.array(val, F32)
    return m


def union(mats):
    """The rule, from its definition: a CSR that stores 1.0 at (r, c) wherever at least one operand (CSR, read as stored) stores an entry
    at (r, c); every row strictly ascending.  Values are never read."""
    shape = mats[0].shape
    ptr, ind = [0], []
    for r in range(shape[0]):
        ids = np.concatenate([np.asarray(A.indices[A.indptr[r]:A.indptr[r + 1]], dtype=np.int64) for A in mats] + [np.zeros(0, np.int64)])
        ind.append(np.unique(ids))
        ptr.append(ptr[-1] + len(ind[-1]))
    out = smat.csr_matrix(shape, dtype=F32)
    out.indptr, out.indices = np.array(ptr, np.int64), np.concatenate(ind + [np.zeros(0, np.int64)])
    out.data = np.ones(ptr[-1], F32)
    return out


def same_pattern(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a.indptr, np.int64), np.asarray(b.indptr, np.int64)) and \
        np.array_equal(np.asarray(a.indices, np.int64), np.asarray(b.indices, np.int64))


def row_of(total, n_ops, cols, rs, relation="random"):
    """Per operand the column ids of one row that holds ``total`` entries over the ``n_ops`` operands."""
    share = [total // n_ops + (1 if k < total % n_ops else 0) for k in range(n_ops)]
    if relation == "disjoint":
        ids = rs.choice(cols, total, replace=False)
        return [ids[sum(share[:k]):sum(share[:k + 1])] for k in range(n_ops)]
    if relation == "identical":
        ids = rs.choice(cols, max(share), replace=False)
        return [ids[:n] for n in share]
    return [rs.choice(cols, n, replace=n > cols) for n in share]


TOTALS = (0, 1, 63, 64, 65, 127, 128, 129, CAP - 1, CAP, CAP + 1, 5000)


def totals_case(n_ops, relation="random", totals=TOTALS, cols=20000, seed=0):
    """n_ops operands whose row r holds totals[r] entries over all of them (shuffled order, random values)."""
    rs = np.random.RandomState(seed + 31 * n_ops)
    per_row = [row_of(t, n_ops, cols, rs, relation) for t in totals]
    return [raw_csr((len(totals), cols), [(row[k], rs.standard_normal(len(row[k]))) for row in per_row]) for k in range(n_ops)]


def interleaved_case(cols=4000):
    """Two operands whose sorted union puts equal ids on both sides of 64-entry step boundaries: A = 0, 1, 2, ...; B = 63, 64, 127, 128, ..."""
    a = np.arange(200)
    b = np.array([63, 64, 127, 128, 191, 192, 63, 199, 3000])
    return [raw_csr((1, cols), [(a[::-1], np.ones(len(a)))]), raw_csr((1, cols), [(b, np.zeros(len(b)))])]


def duplicates_case(cols=500):
    """A column stored 2 and 65 times inside one operand's row; rows in descending and in shuffled order; ids 0 and cols - 1."""
    rs = np.random.RandomState(5)
    r0 = np.concatenate([[7, 7], np.arange(20, 40)])
    r1 = np.concatenate([np.full(65, 11), [0, cols - 1, 11, 3]])
    r2 = np.arange(cols - 1, cols - 130, -1)
    r3 = rs.permutation(300)
    vals = [np.nan, 0.0, -1.5]
    A = raw_csr((4, cols), [(r, np.resize(vals, len(r))) for r in (r0, r1, r2, r3)])
    B = raw_csr((4, cols), [([7], [0.0]), ([], []), ([cols - 1, 0], [np.nan, -0.0]), (rs.permutation(300)[:50], np.zeros(50))])
    return [A, B]


def union_cases():
    out = {f"totals_{n}ops": totals_case(n) for n in (1, 2, 3, 8)}
    out["identical_3ops"] = totals_case(3, "identical")
    out["disjoint_3ops"] = totals_case(3, "disjoint")
    out["interleaved"] = interleaved_case()
    out["duplicates"] = duplicates_case()
    out["empty_operand"] = [totals_case(1, totals=(5, 70))[0], smat.csr_matrix((2, 20000), dtype=F32)]
    out["no_rows"] = [smat.csr_matrix((0, 9), dtype=F32), smat.csr_matrix((0, 9), dtype=F32)]
    out["one_row"] = totals_case(2, totals=(130,))
    out["all_empty"] = [smat.csr_matrix((3, 9), dtype=F32)]
    return out


# ------------------------------------------------------------------------------------------------ the chain loop
def binarized(A):
    A = smat.csc_matrix(A, dtype=F32, copy=True)
    A.data[:] = 1
    return A


def chain_loop(X, Y, chain, schemes, predict_layer, train_layer, pred_params, matching_chain=None, bias=1.0):
    """The reference's loop in scipy.  chain: the C matrices (CSC), root first; schemes: one per layer; pred_params: per layer
    (post_processor, only_topk); predict_layer(X, csr_codes or None, W, C, post_processor, only_topk, bias) -> csr;
    train_layer(X, Y, C, M) -> W (csc, (features + 1) x labels).  Returns dict(W, M, M_pred): per layer, M None under a single-cluster
    root, M_pred None where no prediction was run."""
    depth = len(chain)
    Ys = [smat.csc_matrix(Y, dtype=F32)]
    for C in reversed(chain[1:]):
        Ys.append(smat.csc_matrix(Ys[-1].tocsr() * C.tocsr(), dtype=F32))
    Ys.reverse()
    matching_chain = matching_chain or [None] * depth
    out = dict(W=[], M=[], M_pred=[])
    M_pred = None
    for t, (Yt, C) in enumerate(zip(Ys, chain)):
        shape = (X.shape[0], C.shape[1])
        pred_t = None
        if t == 0 and C.shape[1] == 1:
            M = None
        else:
            M = smat.csc_matrix(shape, dtype=F32)
            if "usn" in schemes[t] and matching_chain[t] is not None:
                M += binarized(matching_chain[t])
            if "tfn" in schemes[t]:
                M += binarized(Ys[t - 1] if t else smat.csc_matrix(Yt.tocsr() * C.tocsr()))
            if t and any("man" in s for s in schemes[t:]):
                pp, k = pred_params[t - 1]
                M_pred = predict_layer(X, M_pred, out["W"][-1], chain[t - 1], pp, k, bias)
                pred_t = M_pred
            if t and "man" in schemes[t]:
                M += binarized(M_pred)
            M = smat.csc_matrix(M, dtype=F32)
            M.sort_indices()
        W = smat.csc_matrix(train_layer(X, Yt, C, M), dtype=F32)
        W.sort_indices()
        out["W"].append(W); out["M"].append(M); out["M_pred"].append(pred_t)
    return out


def ours_host_backend(train_kw=None):
    """(predict_layer, train_layer) over this library's host entry points; train_kw: the solver's keywords (default TRAIN_KW)."""
    train_kw = TRAIN_KW if train_kw is None else train_kw
    from pecos_amd import clib
    from pecos_amd.core import ScipyCompressedSparseAllocator, ScipyCscF32, ScipyCsrF32
    ones = lambda n: smat.csc_matrix((np.ones(n, F32), np.arange(n), np.array([0, n])), shape=(n, 1))      # noqa: E731

    def predict_layer(X, codes, W, C, pp, k, bias):
        alloc = ScipyCompressedSparseAllocator()
        clib.xlinear_single_layer_predict(X, codes, W, C, pp, k, 1, bias, alloc)
        return alloc.get()

    def train_layer(X, Y, C, M):
        M = ones(X.shape[0]) if M is None else M
        return clib.xlinear_single_layer_train(ScipyCsrF32(X), ScipyCscF32(smat.csc_matrix(Y, dtype=F32)), ScipyCscF32(smat.csc_matrix(C, dtype=F32)),
                                               ScipyCscF32(smat.csc_matrix(M, dtype=F32)), None, **train_kw)
    return predict_layer, train_layer


def refpy_available():
    return os.path.isdir(os.path.join(REFPY, "pecos")) and os.path.exists(rr.REF)


def import_refpy():
    if REFPY not in sys.path:
        sys.path.insert(0, REFPY)
    import pecos.xmc  # noqa: F401
    import pecos.xmc.xlinear.model  # noqa: F401
    return sys.modules["pecos"]


def reference_backend(threads=1, train_kw=None):
    """(predict_layer, train_layer) over the compiled reference through its own python package."""
    train_kw = TRAIN_KW if train_kw is None else train_kw
    import_refpy()
    from pecos.xmc import MLModel, MLProblem

    def predict_layer(X, codes, W, C, pp, k, bias):
        return MLModel(W=W, C=C, bias=bias, pred_params=MLModel.PredParams(only_topk=k, post_processor=pp)).predict(X, csr_codes=codes, threads=threads)

    def train_layer(X, Y, C, M):
        prob = MLProblem(X, Y, C=C, M=M, threads=threads)
        return MLModel.train(prob, train_params=MLModel.TrainParams(threads=threads, **train_kw)).W
    return predict_layer, train_layer


# ------------------------------------------------------------------------------------------------ the recorded fixture
def layer_pred_params(post_processor):
    """E2E_KW's prediction parameters per layer of the three-layer chain: the beam above the leaves, only_topk at them."""
    return [(post_processor, rr.E2E_KW["beam_size"]), (post_processor, rr.E2E_KW["beam_size"]), (post_processor, rr.E2E_KW["only_topk"])]


def usn_chain(seed=77):
    """A small random matching_chain for the e2e chain 1 <- 2 <- 8 <- 64 (500 instances): 3 random clusters per instance and layer."""
    rs = np.random.RandomState(seed)
    out = []
    for K in (1, 2, 8):
        n = min(3, K)
        cols = np.concatenate([rs.choice(K, n, replace=False) for _ in range(500)])
        out.append(smat.csr_matrix((np.ones(len(cols), F32), (np.repeat(np.arange(500), n), cols)), shape=(500, K)))
    return out


def config_key(scheme, post_processor):
    return f"{scheme}__{post_processor}"


def put_sparse(out, key, A, stored=None):
    """A's arrays under ``key``; with ``stored`` (a dict the caller keeps) a matrix that equals an earlier one bit for bit is recorded as
    that one's name (``key__same``): the same matrix under several schemes is kept once."""
    parts = (np.array(A.shape, np.int64), np.asarray(A.indptr, np.int64), np.asarray(A.indices, np.int32), np.asarray(A.data, F32).view(np.uint32))
    if stored is not None:
        mark = b"|".join(p.tobytes() for p in parts)
        if mark in stored:
            out[f"{key}__same"] = np.array(stored[mark])
            return
        stored[mark] = key
    out[f"{key}__shape"], out[f"{key}__indptr"], out[f"{key}__indices"], out[f"{key}__bits"] = parts


def get_sparse(rec, key, kind):
    if f"{key}__same" in rec:
        key = str(rec[f"{key}__same"])
    if f"{key}__shape" not in rec:
        return None
    m = kind(tuple(int(v) for v in rec[f"{key}__shape"]), dtype=F32)
    m.indptr, m.indices, m.data = rec[f"{key}__indptr"].astype(np.int64), rec[f"{key}__indices"].astype(np.int64), rec[f"{key}__bits"].view(F32)
    return m


def recorded_chain(rec):
    return [get_sparse(rec, f"chain__{t}", smat.csc_matrix) for t in range(int(rec["depth"][0]))]


def recorded_config(rec, scheme, post_processor):
    """dict(W, M, M_pred) per layer as recorded from the reference (W and M sorted CSC, M_pred CSR as returned)."""
    k, depth = config_key(scheme, post_processor), int(rec["depth"][0])
    return dict(W=[get_sparse(rec, f"{k}__W{t}", smat.csc_matrix) for t in range(depth)], M=[get_sparse(rec, f"{k}__M{t}", smat.csc_matrix) for t in range(depth)],
                M_pred=[get_sparse(rec, f"{k}__P{t}", smat.csr_matrix) for t in range(depth)])


def same_bits(a, b):
    return same_pattern(a, b) and np.array_equal(np.asarray(a.data, F32).view(np.uint32), np.asarray(b.data, F32).view(np.uint32))


def wt_to_w(Wt):
    """W^T (CSR, labels x rows of W) as W in CSC."""
    return smat.csc_matrix((Wt.data, Wt.indices, Wt.indptr), shape=(Wt.shape[1], Wt.shape[0]), dtype=F32)


def result_to_csr(result, n_cols):
    """A result triple of torch tensors as a scipy CSR, rows in stored (best-first) order."""
    idx, val, cnt = (t.cpu().numpy() for t in result)
    cnt = np.minimum(cnt, idx.shape[1])
    keep = np.arange(idx.shape[1])[None, :] < cnt[:, None]
    m = smat.csr_matrix((idx.shape[0], n_cols), dtype=F32)
    m.indptr, m.indices, m.data = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), idx[keep].astype(np.int64), val[keep].astype(F32)
    return m


def csr_to_codes(csr, stride=None, pad=0):
    """A scipy CSR as the fixed-stride arrays (idx int32 [rows, stride], val float32, cnt int32 [rows]); cells beyond a row's count hold pad."""
    lens = np.diff(csr.indptr)
    stride = int(max(1, lens.max() if stride is None and len(lens) else (stride or 1)))
    idx, val = np.full((csr.shape[0], stride), pad, np.int32), np.zeros((csr.shape[0], stride), F32)
    for r in range(csr.shape[0]):
        n = min(int(lens[r]), stride)
        idx[r, :n], val[r, :n] = csr.indices[csr.indptr[r]:csr.indptr[r] + n], csr.data[csr.indptr[r]:csr.indptr[r] + n]
    return idx, val, lens.astype(np.int32)
