"""The rule of the ranker training (K13), stated in numpy with explicit float32 / float64 roundings, and what the training tests share:
the ctypes caller of the host training entry points of any library (``c_xlinear_single_layer_train_*`` in the reference,
``xrl_single_layer_train_*`` with the same argument list here), the case generators, and two deliberately wrong variants.

The statement follows the reference at threads = 1 (pecos/core/xmc/linear_solver.hpp:420-528, 667-779, 797-860; utils/matrix.hpp:837-877,
971-976).  Its shuffle restates the C++ standard library the reference is compiled with here (libstdc++: shuffle's two positions per draw
up to 65 535 elements, uniform_int_distribution's multiply-and-reject downscaling of a 32-bit generator); every job reads std::mt19937(0)."""
import ctypes
import os

import numpy as np
import scipy.sparse as smat

from clustering_rule import CsrView, DrmView, Mt19937, last_error, load, shuffle

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OURS = os.environ.get("PECOS_XRL_AMD_SO") or os.path.join(REPO, "pecos_amd", "lib", "libxrl_amd.so")
REF = os.path.join(REPO, "oracle", "_ref", "libpecos_float32.so")
L2_DUAL, L1_DUAL, LR_DUAL, L2_PRIMAL = 1, 3, 7, 2
F32, F64 = np.float32, np.float64
INF = float("inf")
COUNTERS = ("jobs", "batches", "slots", "stride", "iters", "shrinks", "reactivations", "max_iter_stops", "clipped", "lane_rows", "wave_rows",
            "extensions", "reruns")


# ------------------------------------------------------------------------------------------------ the statement
def _chain(terms):
    """+0 + t0 + t1 + ... in fp32, one rounded addition after the other."""
    return np.cumsum(np.concatenate([np.zeros(1, F32), np.asarray(terms, F32)]), dtype=F32)[-1]


def _pairwise(terms):
    """The same terms summed as a balanced tree (the wrong variant "pairwise")."""
    t = [F32(v) for v in terms]
    if not t:
        return F32(0)
    while len(t) > 1:
        t = [F32(t[k] + t[k + 1]) if k + 1 < len(t) else t[k] for k in range(0, len(t), 2)]
    return t[0]


def jobs_of(Y, C, M):
    """[(code, label)] in the reference's order: code-major over C's stored entries; pure multi-label without C or M."""
    if C is None or M is None:
        return [(None, l) for l in range(Y.shape[1])]
    return [(k, int(l)) for k in range(C.shape[1]) for l in C.indices[C.indptr[k]:C.indptr[k + 1]]]


def statement(X, Y, C=None, M=None, R=None, threshold=0.0, max_nonzeros=0, solver=L1_DUAL, Cp=1.0, Cn=1.0, max_iter=1000, eps=0.1, bias=1.0,
              variant=None):
    """The rule.  X: CSR (sorted rows) or ndarray; Y, C, M, R: CSC as stored (never canonicalised).  Returns dict(rows, cols, vals: the COO
    in job order with a label's entries ascending; counters: iters, shrinks, reactivations, max_iter_stops, clipped; per_job: [(label,
    iterations, instances)]).  variant: None, "pairwise" (the dot as a balanced tree) or "alpha64" (alpha kept in fp64)."""
    assert variant in (None, "pairwise", "alpha64") and solver in (L1_DUAL, L2_DUAL)
    if not smat.issparse(X):
        from clustering_rule import as_full_csr
        X = as_full_csr(X)
    N, d = X.shape
    xp, xi, xv = X.indptr, X.indices, X.data.astype(F32)
    rows_of = [(xi[xp[i]:xp[i + 1]], xv[xp[i]:xp[i + 1]]) for i in range(N)]
    dot_sum = _pairwise if variant == "pairwise" else _chain
    l2 = solver == L2_DUAL
    bias = float(bias)
    out_r, out_c, out_v, per_job = [], [], [], []
    ctr = dict(iters=0, shrinks=0, reactivations=0, max_iter_stops=0, clipped=0)
    for code, label in jobs_of(Y, C, M):
        # -- init_worker
        cost, y = {}, {}
        if code is None:
            index = list(range(N))
        else:
            index = [int(i) for i in M.indices[M.indptr[code]:M.indptr[code + 1]]]
        for i in index:
            y[i], cost[i] = -1, F32(1)
        for p in range(Y.indptr[label], Y.indptr[label + 1]):
            i = int(Y.indices[p])
            y[i] = 1
            if cost.get(i, F32(0)) == 0:
                index.append(i)
            cost[i] = F32(R.data[p]) if R is not None else F32(1)
        n = len(index)
        # -- set-up
        w = np.zeros(d, F32)
        b = F32(0)
        alpha, QD = {}, {}

        def class_cost(i):
            return (Cp if y[i] > 0 else Cn) * F64(cost[i])

        for i in index:
            f, v = rows_of[i]
            q = F32(0.5 / class_cost(i)) if l2 else F32(0)
            xx = _chain(v * v)
            QD[i] = F32(F64(q) + (F64(xx) + (bias * bias if bias > 0 else 0.0)))
            alpha[i] = F32(0) if variant != "alpha64" else F64(0)
        # -- the sweeps
        g = Mt19937(0)
        pgmax_old, pgmin_old = INF, -INF
        active, it, converged = n, 0, False
        while it < max_iter:
            pgmax_new, pgmin_new = -INF, INF
            head = index[:active]
            shuffle(g, head)
            index[:active] = head
            s = 0
            while s < active:
                i = index[s]
                f, v = rows_of[i]
                yi = y[i]
                dot = dot_sum(w[f] * v)
                G = F64(yi) * (F64(dot) + (F64(b) * bias if bias > 0 else 0.0)) - 1.0
                Cub = INF if l2 else class_cost(i)
                diag = 0.5 / class_cost(i) if l2 else 0.0
                G = G + F64(alpha[i]) * diag
                PG, shrink = 0.0, False
                if alpha[i] == 0:
                    if G > pgmax_old:
                        shrink = True
                    elif G < 0:
                        PG = G
                elif F64(alpha[i]) == Cub:
                    if G < pgmin_old:
                        shrink = True
                    elif G > 0:
                        PG = G
                else:
                    PG = G
                if shrink:
                    active -= 1
                    index[s], index[active] = index[active], index[s]
                    ctr["shrinks"] += 1
                    continue
                pgmax_new, pgmin_new = max(pgmax_new, PG), min(pgmin_new, PG)
                if abs(PG) > 1.0e-12:
                    old = F64(alpha[i])
                    t = old - G / F64(QD[i])
                    t = 0.0 if t < 0.0 else t
                    if Cub < t:
                        t = Cub
                        ctr["clipped"] += 1
                    alpha[i] = F32(t) if variant != "alpha64" else F64(t)
                    dd = (F64(alpha[i]) - old) * F64(yi)
                    w[f] = (w[f].astype(F64) + dd * v.astype(F64)).astype(F32)
                    if bias > 0:
                        b = F32(F64(b) + dd * bias)
                s += 1
            it += 1
            if pgmax_new - pgmin_new <= eps:
                if active == n:
                    converged = True
                    break
                active, pgmax_old, pgmin_old = n, INF, -INF
                ctr["reactivations"] += 1
                continue
            pgmax_old, pgmin_old = pgmax_new, pgmin_new
            if pgmax_old <= 0:
                pgmax_old = INF
            if pgmin_old >= 0:
                pgmin_old = -INF
        ctr["iters"] += it
        ctr["max_iter_stops"] += 0 if converged else 1
        per_job.append((label, it, n))
        # -- emission
        passes = np.flatnonzero(np.abs(w).astype(F64) >= threshold)
        push_bias = bias > 0 and F64(abs(b)) >= threshold
        if max_nonzeros and len(passes) >= max_nonzeros:
            order = sorted(passes, key=lambda k: (-abs(w[k]), k))[:max_nonzeros]
            if bias > 0:
                if abs(b) > abs(w[order[-1]]):
                    order.pop()
                else:
                    push_bias = False
            passes = np.sort(np.array(order, dtype=np.int64))
        for k in passes:
            out_r.append(int(k)); out_c.append(label); out_v.append(w[k])
        if push_bias:
            out_r.append(d); out_c.append(label); out_v.append(b)
    return dict(rows=np.array(out_r, np.uint64), cols=np.array(out_c, np.uint64), vals=np.array(out_v, F32), counters=ctr, per_job=per_job)


def canonical(rows, cols, vals):
    """A COO as (cols, rows, value bits) sorted by (label, feature): what the 8-thread runs and the max_nonzeros cases are compared by."""
    o = np.lexsort((rows, cols))
    return np.asarray(cols)[o].astype(np.uint64), np.asarray(rows)[o].astype(np.uint64), np.asarray(vals, F32)[o].view(np.uint32)


def same_coo(a, b, canon=False):
    """a, b: (rows, cols, vals) or dicts with those keys; bit equality, in order or after canonical()."""
    a = (a["rows"], a["cols"], a["vals"]) if isinstance(a, dict) else a
    b = (b["rows"], b["cols"], b["vals"]) if isinstance(b, dict) else b
    if canon:
        a, b = canonical(*a), canonical(*b)
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(np.asarray(a[2], F32).view(np.uint32), np.asarray(b[2], F32).view(np.uint32)))


# ------------------------------------------------------------------------------------------------ the ctypes caller
class CscView(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_uint32), ("cols", ctypes.c_uint32), ("col_ptr", ctypes.c_void_p), ("row_idx", ctypes.c_void_p), ("val", ctypes.c_void_p)]


_COO_ALLOC = ctypes.CFUNCTYPE(None, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)


def _csc_view(m, keep):
    ptr, idx, val = m.indptr.astype(np.uint64), m.indices.astype(np.uint32), m.data.astype(F32)
    keep.extend((ptr, idx, val))
    return CscView(m.shape[0], m.shape[1], ptr.ctypes.data, idx.ctypes.data, val.ctypes.data)


def entry_stem(lib):
    """The reference exports its trainer as c_xlinear_single_layer_train_*; this library keeps that name free (a binding that takes this
    library first and the reference otherwise keeps the reference's trainer) and exports xrl_single_layer_train_*."""
    return "xrl_single_layer_train" if hasattr(lib, "xrl_single_layer_train_csr_f32") else "c_xlinear_single_layer_train"


def run_library(path, X, Y, C=None, M=None, R=None, threshold=0.0, max_nonzeros=0, solver=L1_DUAL, Cp=1.0, Cn=1.0, max_iter=1000, eps=0.1, bias=1.0,
                threads=1):
    """The host training entry point for a scipy CSR (``*_csr_f32``) or an ndarray (``*_drm_f32``) of the library at ``path`` -> (dict(rows,
    cols, vals, shape) or None, error or None).  Y, C, M, R are CSC and are passed as stored."""
    lib = load(path)
    stem = entry_stem(lib)
    keep = []
    if smat.issparse(X):
        ptr, idx, val = X.indptr.astype(np.uint64), X.indices.astype(np.uint32), X.data.astype(F32)
        xview = CsrView(X.shape[0], X.shape[1], ptr.ctypes.data, idx.ctypes.data, val.ctypes.data)
        fn = getattr(lib, stem + "_csr_f32")
    else:
        val = np.ascontiguousarray(X, dtype=F32)
        xview = DrmView(X.shape[0], X.shape[1], val.ctypes.data)
        fn = getattr(lib, stem + "_drm_f32")
    views = [_csc_view(m, keep) if m is not None else None for m in (Y, C, M, R)]
    got = {}

    def alloc(rows, cols, nnz, row_pp, col_pp, val_pp):
        got["shape"] = (rows, cols)
        got["rows"], got["cols"], got["vals"] = np.zeros(nnz, np.uint64), np.zeros(nnz, np.uint64), np.zeros(nnz, F32)
        for pp, arr in ((row_pp, got["rows"]), (col_pp, got["cols"]), (val_pp, got["vals"])):
            ctypes.cast(pp, ctypes.POINTER(ctypes.c_uint64))[0] = arr.ctypes.data

    fn.restype = None
    fn.argtypes = [ctypes.c_void_p] * 5 + [_COO_ALLOC, ctypes.c_double, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_size_t,
                   ctypes.c_double, ctypes.c_double, ctypes.c_int]
    fn(ctypes.byref(xview), *[ctypes.byref(v) if v is not None else None for v in views], _COO_ALLOC(alloc), threshold, max_nonzeros, solver, Cp, Cn, max_iter,
       eps, bias, threads)
    err = last_error(lib) if hasattr(lib, "xrl_last_error") else None
    return (got if "rows" in got else None), err


def reference(X, Y, C=None, M=None, R=None, threads=1, **kw):
    return run_library(REF, X, Y, C, M, R, threads=threads, **kw)[0]


def counters(path=OURS):
    """xrl_debug_train_counters of the library's last training, by name."""
    lib = load(path)
    out = (ctypes.c_uint64 * len(COUNTERS))()
    lib.xrl_debug_train_counters.restype, lib.xrl_debug_train_counters.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]
    assert lib.xrl_debug_train_counters(out, len(COUNTERS)) == 0
    return dict(zip(COUNTERS, (int(v) for v in out)))


# ------------------------------------------------------------------------------------------------ cases
def raw_csc(shape, cols):
    """A CSC from per-column (row ids, values) kept exactly as given: unsorted ids and explicit zeros stay."""
    ptr, ind, val = [0], [], []
    for ids, vs in cols:
        ind.extend(ids); val.extend(vs); ptr.append(len(ind))
    m = smat.csc_matrix(shape, dtype=F32)
    m.indptr, m.indices, m.data = np.array(ptr, np.int64), np.array(ind, np.int64), np.array(val, F32)
    return m


def rows_csr(cols, lengths, seed, scale=1.0):
    """A CSR whose row r stores lengths[r] entries: sorted distinct columns, N(0, 1) * scale values."""
    rs = np.random.RandomState(seed)
    ptr, ind, val = [0], [], []
    for n in lengths:
        ind.extend(np.sort(rs.choice(cols, n, replace=False))); val.extend(rs.standard_normal(n) * scale); ptr.append(len(ind))
    m = smat.csr_matrix((len(lengths), cols), dtype=F32)
    m.indptr, m.indices, m.data = np.array(ptr, np.int64), np.array(ind, np.int64), np.array(val, F32)
    return m


def problem(N, d, L, K, per_row, per_label, seed, scale=1.0):
    """A clustered problem: X (CSR), Y (CSC, ones), C (CSC: label l under code l % K ... in ascending label order), M = pattern of Y * C."""
    rs = np.random.RandomState(seed)
    X = rows_csr(d, np.minimum(d, np.maximum(1, rs.poisson(per_row, N))), seed + 1, scale)
    Y = raw_csc((N, L), [(np.sort(rs.choice(N, min(N, max(1, int(rs.poisson(per_label)))), replace=False)),) * 2 for _ in range(L)])
    Y.data[:] = 1
    code = rs.randint(0, K, L)
    C = raw_csc((L, K), [(np.flatnonzero(code == k), np.ones(int((code == k).sum()))) for k in range(K)])
    M = smat.csc_matrix((Y.tocsr() * C.tocsr()).tocsc(), dtype=F32)
    M.sort_indices()
    return X, Y, C, M


def layouts():
    """The label and matrix layouts of the issue on one small X: see the comments."""
    N, d = 40, 30
    X = rows_csr(d, [5] * N, 31)
    cols = [
        (list(range(0, 6)), [1] * 6),                 # 0: ordinary, positives inside its M column
        ([], []),                                      # 1: no positives
        (list(range(0, 12)), [1] * 12),                # 2: only positives: its M column is exactly them
        ([30, 33, 31], [1, 1, 1]),                     # 3: positives all outside its M column, stored unsorted
        ([2, 20, 5], [5.0, 0.0, 5.0]),                 # 4: values 5.0 and an explicit zero (which counts as a positive)
        ([7, 8], [1, 1]),                              # 5: in no column of C
        ([1, 3], [1, 1]),                              # 6
    ]
    Y = raw_csc((N, 7), cols)
    C = raw_csc((7, 3), [([1, 0], [1, 1]), ([2], [1]), ([6, 4, 3], [1, 1, 1])])        # columns 0 and 2 list labels in descending order
    M = raw_csc((N, 3), [(list(range(0, 10)), [1] * 9 + [0.0]), (list(range(0, 12)), [1] * 12), ([20, 2, 5, 1, 3, 9, 12], [1, 0.0, 1, 1, 1, 1, 1])])
    return X, Y, C, M


def relevance(Y, seed):
    """R on Y's pattern with costs 0.25 .. 4."""
    R = Y.copy()
    R.data = np.random.RandomState(seed).choice(np.array([0.25, 0.5, 1, 2, 4], F32), len(Y.data)).astype(F32)
    return R


def one_entry_rows(n, d=7, seed=3):
    """n rows of one entry each, and one label over every third row: jobs of exactly n instances in the pure multi-label form."""
    rs = np.random.RandomState(seed)
    X = smat.csr_matrix((n, d), dtype=F32)
    X.indptr, X.indices, X.data = np.arange(n + 1, dtype=np.int64), rs.randint(0, d, n).astype(np.int64), rs.standard_normal(n).astype(F32)
    Y = raw_csc((n, 1), [(np.arange(0, n, 3), np.ones(len(range(0, n, 3))))])
    return X, Y


def job_sizes_problem(sizes=(0, 1, 2, 3, 4, 5, 63, 64, 65, 1000), d=50, seed=9):
    """One code per size: M's column k lists sizes[k] rows, and its one label's positives are every second of them."""
    N = max(sizes) + 5
    X = rows_csr(d, [6] * N, seed)
    rs = np.random.RandomState(seed)
    mcols, ycols = [], []
    for n in sizes:
        ids = np.sort(rs.choice(N, n, replace=False))
        mcols.append((ids, np.ones(n)))
        ycols.append((ids[::2], np.ones(len(ids[::2]))))
    K = len(sizes)
    return X, raw_csc((N, K), ycols), raw_csc((K, K), [([k], [1]) for k in range(K)]), raw_csc((N, K), mcols)


def row_lengths_problem(lengths=(0, 1, 63, 64, 65, 127, 128, 129, 1000), d=1200, seed=4):
    """Feature rows of the given lengths (twice each), pure multi-label with three labels."""
    X = rows_csr(d, list(lengths) * 2, seed, scale=0.3)
    N = X.shape[0]
    Y = raw_csc((N, 3), [(np.arange(0, N, 2), np.ones((N + 1) // 2)), (np.arange(1, N, 3), np.ones(len(range(1, N, 3)))), ([N - 1], [1])])
    return X, Y


def ties_problem():
    """Duplicated feature columns (|w| ties) and a bias that displaces the least kept feature."""
    N, d = 60, 12
    rs = np.random.RandomState(12)
    base = rs.standard_normal((N, 4)).astype(F32)
    D = np.concatenate([base, base, -base], axis=1)            # features f, f + 4 and f + 8 carry the same |w|
    X = smat.csr_matrix(D)
    X.sort_indices()
    Y = raw_csc((N, 2), [(np.flatnonzero(base[:, 0] + base[:, 1] > 0),) * 2, (np.flatnonzero(base[:, 2] > 0.5),) * 2])
    Y.data[:] = 1
    return X, Y


def cases():
    """{name: (X, Y, C, M, R, keywords of statement() / run_library())}: what the CPU half checks against the compiled reference and the GPU
    half against all three.  Small enough for the plain-Python statement."""
    c = {}
    X, Y, C, M = problem(300, 120, 24, 4, 9, 12, 1)
    for solver, tag in ((L1_DUAL, "l1"), (L2_DUAL, "l2")):
        c[f"coded_{tag}"] = (X, Y, C, M, None, dict(solver=solver, threshold=0.1, max_iter=100))
        c[f"coded_{tag}_costs"] = (X, Y, C, M, relevance(Y, 5), dict(solver=solver, Cp=2.0, Cn=0.5, threshold=0.1, max_iter=100))
        c[f"pure_{tag}"] = (X[:80], smat.csc_matrix(Y[:80, :6]), None, None, None, dict(solver=solver, threshold=0.1, max_iter=100))
        for b in (1.0, 0.5, 0.0, -1.0):
            c[f"bias{b}_{tag}"] = (X, Y, C, M, None, dict(solver=solver, bias=b, threshold=0.05, max_iter=30))
        for it in (0, 1, 2):
            c[f"iter{it}_{tag}"] = (X, Y, C, M, None, dict(solver=solver, max_iter=it, threshold=0.0))
        c[f"eps_small_{tag}"] = (X, Y, C, M, None, dict(solver=solver, eps=1e-6, max_iter=100, threshold=0.1))
        c[f"layouts_{tag}"] = layouts() + (None, dict(solver=solver, threshold=0.01, max_iter=50))
        c[f"layouts_{tag}_R"] = layouts() + (relevance(layouts()[1], 6), dict(solver=solver, threshold=0.01, max_iter=50))
        Xs, Ys, Cs, Ms = job_sizes_problem()
        c[f"job_sizes_{tag}"] = (Xs, Ys, Cs, Ms, None, dict(solver=solver, threshold=0.01, max_iter=20))
        Xr, Yr = row_lengths_problem()
        c[f"row_lengths_{tag}"] = (Xr, Yr, None, None, None, dict(solver=solver, threshold=0.001, max_iter=30))
        Xt, Yt = ties_problem()
        for k in (1, 5, 100):
            c[f"maxnz{k}_{tag}"] = (X, Y, C, M, None, dict(solver=solver, max_nonzeros=k, threshold=0.01, max_iter=30))
            c[f"ties_maxnz{k}_{tag}"] = (Xt, Yt, None, None, None, dict(solver=solver, max_nonzeros=k, threshold=0.0, max_iter=30))
        rare = raw_csc((Xt.shape[0], 2), [([3, 17, 40], [1, 1, 1]), ([3], [1])])               # few positives: |b| is near 1, above every |w|
        c[f"ties_bias_{tag}"] = (Xt, rare, None, None, None, dict(solver=solver, max_nonzeros=2, threshold=0.0, max_iter=30))
        c[f"thr_all_{tag}"] = (X, Y, C, M, None, dict(solver=solver, threshold=0.0, max_iter=30))
        c[f"thr_none_{tag}"] = (X, Y, C, M, None, dict(solver=solver, threshold=1e6, max_iter=30))
    # shrinking, re-activation, clipping at C (L1 loss), a stop by max_iter: separable-ish data with a small C and a tight eps
    Xh, Yh, Ch, Mh = problem(400, 40, 6, 2, 6, 60, 7, scale=2.0)
    c["shrink_l1"] = (Xh, Yh, Ch, Mh, None, dict(solver=L1_DUAL, Cp=0.5, Cn=0.5, eps=0.01, max_iter=100, threshold=0.0))
    c["shrink_l2"] = (Xh, Yh, Ch, Mh, None, dict(solver=L2_DUAL, eps=0.01, max_iter=100, threshold=0.0))
    c["stop_l1"] = (Xh, Yh, Ch, Mh, None, dict(solver=L1_DUAL, Cp=8.0, Cn=8.0, eps=1e-6, max_iter=2, threshold=0.0))
    # the wrong variants must show: long rows whose products cancel (order of the additions), many updates of one alpha (its width)
    Xo = rows_csr(400, [200] * 120, 21, scale=3.0)
    Yo = raw_csc((120, 2), [(np.arange(0, 120, 2), np.ones(60)), (np.arange(0, 120, 5), np.ones(24))])
    c["order_l2"] = (Xo, Yo, None, None, None, dict(solver=L2_DUAL, eps=1e-4, max_iter=40, threshold=0.0))
    c["order_l1"] = (Xo, Yo, None, None, None, dict(solver=L1_DUAL, eps=1e-4, max_iter=40, threshold=0.0))
    return c


def scale_problem():
    """20 000 rows x 2 000 labels under 64 clusters (too large for the plain-Python statement: checked against the reference only)."""
    X, Y, C, M = problem(20000, 5000, 2000, 64, 20, 30, 41)
    return X, Y, C, M, dict(solver=L2_DUAL, threshold=0.1, max_iter=20)


BIG_JOBS = (65535, 65536, 65537)       # the sizes around libstdc++'s switch from two positions per draw to one


def big_job(n):
    X, Y = one_entry_rows(n)
    return X, Y, dict(solver=L1_DUAL, threshold=0.0, max_iter=2)


E2E_KW = dict(nr_splits=4, min_codes=4, threshold=0.05, max_iter=50, solver_type="L2R_L2LOSS_SVC_DUAL", beam_size=4, only_topk=5, post_processor="l3-hinge")


def e2e_problem():
    """500 instances x 200 features x 64 labels under 8 bottom clusters: with E2E_KW the chain is 1 <- 2 <- 8 <- 64 (three layers)."""
    X, Y, _, _ = problem(500, 200, 64, 8, 12, 25, 51)
    C = raw_csc((64, 8), [(np.arange(8 * k, 8 * k + 8), np.ones(8)) for k in range(8)])
    return X, Y, C


def digest(coo):
    """sha256 over the canonical (label, feature, value bits) of a COO: what the golden file keeps of results too large to store."""
    import hashlib
    h = hashlib.sha256()
    for a in canonical(coo["rows"], coo["cols"], coo["vals"]):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# the cases on which each wrong variant must differ from the reference
VARIANT_CASES = {"pairwise": ("order_l2", "order_l1"), "alpha64": ("order_l2", "order_l1")}


def dense_ok(X):
    """Cases small enough to run through the dense entry point as well."""
    return smat.issparse(X) and X.shape[0] * X.shape[1] <= 40000
