"""The rule of the primal L2-loss SVC training (K16), stated in numpy with explicit float32 / float64 roundings, and what its tests share.

The statement follows the reference at threads = 1: SVMWorker::solve_l2r_l2_svc_primal (pecos/core/xmc/linear_solver.hpp:407-417) over
l2r_erm_fun / l2r_l2_svc_fun (:62-323), NEWTON::newton / pcg / norm (utils/newton.hpp:98-273) and the vector helpers
(utils/matrix.hpp:862-976), between the job set-up and the emission that the dual solvers share (init_worker, SVMJob::solve; restated in
ranker_training_rule.py).  value_type is float: the vectors w, g, M, s, r, d, Hd, z, wx, tmp, the bias parts and get_c() are fp32, the
scalars f, alpha, beta, zTr, dHd, Q, gnorm, wTw, sTs, wTs, gTs, xTs are fp64.  Every do_dot_product is an fp32 chain from +0 in index order;
norm() is an fp64 chain.  An axpy with a double factor is y = fl32((double)y + a * (double)x); one with a float factor is fp32 throughout.

THE COMPRESSED FORM.  A feature that no instance of a job stores stays (+-)0 in every vector and 1 in M, adds (+-)0 to chains that start at
+0, and its emitted weight is +0 -- as long as every scalar multiplied into a vector (pcg's alpha and beta - 1) is finite.  The statement
therefore walks only the job's touched features, in ascending order; a job that meets a non-finite alpha or beta is flagged and what the
statement returns for it is not the reference's (the device refuses the call).  tests/test_primal_training_cpu.py proves the form against
the dense reference."""
import ctypes

import numpy as np
import scipy.sparse as smat

from clustering_rule import CsrView, DrmView, last_error, load
from ranker_training_rule import (F32, F64, INF, L1_DUAL, L2_DUAL, L2_PRIMAL, LR_DUAL, OURS, REF, CscView, _COO_ALLOC, _csc_view,  # noqa: F401
                                  as_stored_transpose, canonical, jobs_of, problem, raw_csc, relevance, rows_csr, run_library, same_coo, wt_as_coo)

COUNTERS = ("jobs", "batches", "slots", "stride", "newton_iters", "cg_iters", "hv_calls", "halvings", "end_before_first", "end_gradient",
            "end_linesearch", "end_actred", "end_cap", "cg_dhd", "cg_q", "cg_positive", "cg_cap", "lane_rows", "wave_rows", "nonfinite_jobs")
VARIANTS = (None, "no_alias", "dot64", "cg_touched")
MAX_NEWTON, MAX_HALVINGS, EPS_CG, ALPHA_PCG = 1000, 20, 0.5, 0.01


def _chain32(terms):
    return np.cumsum(np.concatenate([np.zeros(1, F32), np.asarray(terms, F32)]), dtype=F32)[-1]


def _chain64(terms):
    return np.cumsum(np.concatenate([np.zeros(1, F64), np.asarray(terms, F64)]), dtype=F64)[-1]


def _axpy64(a, x, y):
    """y + a * x with a double factor: the product and the sum are fp64, the store rounds to fp32."""
    return (y.astype(F64) + F64(a) * x.astype(F64)).astype(F32)


def statement(*a, **kw):
    """The rule.  X: CSR (sorted rows) or ndarray; Y, C, M, R: CSC as stored.  Returns dict(rows, cols, vals: the COO in job order with a
    label's entries ascending; counters: COUNTERS[4:] summed over the jobs; trace: one dict per job -- label, instances, touched,
    max_cg_iter, newton_exit ("before_first" / "gradient" / "linesearch" / "f_low" / "actred" / "cap"), newton_iters, cg_exits (one of
    "dhd" / "q" / "positive" / "cap" per pcg run), cg_iters (per run), halvings (per line search), alias_overwrites (a compacted slot of
    tmp overwritten by a later instance's raw value while grad ran), nonfinite (False, or "alpha" / "beta": the first scalar of pcg that was not finite)).  variant: None or a
    deliberately wrong one: "no_alias" (grad compacts into an array of its own), "dot64" (dot products accumulated in fp64), "cg_touched"
    (max_cg_iter from the job's touched features, not from d).  Overflows and divisions by zero are IEEE results, hence the errstate."""
    with np.errstate(all="ignore"):
        return _statement(*a, **kw)


def _statement(X, Y, C=None, M=None, R=None, threshold=0.0, max_nonzeros=0, solver=L2_PRIMAL, Cp=1.0, Cn=1.0, max_iter=1000, eps=0.1, bias=1.0,
               variant=None):
    assert variant in VARIANTS and solver == L2_PRIMAL
    if not smat.issparse(X):
        from clustering_rule import as_full_csr
        X = as_full_csr(X)
    N, d = X.shape
    xp, xi, xv = X.indptr, X.indices, X.data.astype(F32)
    rows_of = [(xi[xp[i]:xp[i + 1]], xv[xp[i]:xp[i + 1]]) for i in range(N)]
    bias = float(bias)
    has_b = bias > 0
    chain = (lambda t: F32(_chain64(np.asarray(t, F32).astype(F64)))) if variant == "dot64" else _chain32
    out_r, out_c, out_v, traces = [], [], [], []
    ctr = dict.fromkeys(COUNTERS[4:], 0)
    for code, label in jobs_of(Y, C, M):
        # -- init_worker (as ranker_training_rule states it)
        cost, y = {}, {}
        index = list(range(N)) if code is None else [int(i) for i in M.indices[M.indptr[code]:M.indptr[code + 1]]]
        for i in index:
            y[i], cost[i] = -1, F32(1)
        for p in range(int(Y.indptr[label]), int(Y.indptr[label + 1])):
            i = int(Y.indices[p])
            y[i] = 1
            if cost.get(i, F32(0)) == 0:
                index.append(i)
            cost[i] = F32(R.data[p]) if R is not None else F32(1)
        n = len(index)
        for i in index:
            ctr["wave_rows" if len(rows_of[i][0]) >= 64 else "lane_rows"] += 1
        T = np.unique(np.concatenate([rows_of[i][0] for i in index] + [np.zeros(0, xi.dtype)])).astype(np.int64)     # the touched features, ascending
        tr = dict(label=label, instances=n, touched=len(T), newton_exit=None, newton_iters=0, cg_exits=[], cg_iters=[], halvings=[], alias_overwrites=0,
                  nonfinite=False)
        yf = {i: F32(y[i]) for i in y}
        c32 = {i: F32(F64(cost[i]) * (Cp if y[i] > 0 else Cn)) for i in y}                       # get_c
        w = np.zeros(d, F32)
        b = F32(0)
        wx = np.zeros(N, F32)
        tmp = np.zeros(N + n + 1, F32)
        I = []

        def dot(u, v):
            return chain(u[T] * v[T])

        def row_dot(u, i):
            f, v = rows_of[i]
            return chain(u[f] * v)

        def xv_into(u, bu, out):                                       # Xv
            for i in index:
                r = row_dot(u, i)
                out[i] = F32(F64(r) + bias * F64(bu)) if has_b else r

        def c_times_loss(i, wxi):
            dd = 1.0 - F64(yf[i]) * F64(wxi)
            return F64(c32[i]) * dd * dd if dd > 0 else F64(0)

        def fun():
            nonlocal wTw
            xv_into(w, b, wx)
            wTw = F64(dot(w, w))
            if has_b:
                wTw = wTw + F64(b) * F64(b)
            f = F64(0)
            for i in index:
                f = f + c_times_loss(i, wx[i])
            return f + 0.5 * wTw

        def grad():
            nonlocal I
            I = []
            vals = []                                                  # "no_alias": the compacted values in an array of their own
            for i in index:
                if variant != "no_alias" and i < len(I):
                    tr["alias_overwrites"] += 1
                tmp[i] = F32(wx[i] * yf[i])
                if tmp[i] < 1:
                    v = F32(F32(c32[i] * yf[i]) * F32(tmp[i] - F32(1)))
                    if variant == "no_alias":
                        vals.append(v)
                    else:
                        tmp[len(I)] = v
                    I.append(i)
            g = np.zeros(d, F32)
            bg = F32(0)
            for p, i in enumerate(I):                                  # subXTv: a float factor, fp32 throughout
                v = vals[p] if variant == "no_alias" else tmp[p]
                f, xval = rows_of[i]
                g[f] = g[f] + v * xval
                if has_b:
                    bg = F32(F64(bg) + bias * F64(v))
            g[T] = w[T] + F32(2) * g[T]                                # do_xp2y
            if has_b:
                bg = F32(b + F32(2) * bg)
            return g, bg

        def norm(g, bg):
            return np.sqrt(_chain64(g[T].astype(F64) * g[T].astype(F64)) + F64(bg) * F64(bg))

        def hv(s, bs):
            ctr["hv_calls"] += 1
            Hs = np.zeros(d, F32)
            bHs = F32(0)
            for i in I:
                xTs = F64(row_dot(s, i))
                if has_b:
                    xTs = xTs + bias * F64(bs)
                xTs = F64(c32[i]) * xTs
                f, xval = rows_of[i]
                Hs[f] = _axpy64(xTs, xval, Hs[f])
                if has_b:
                    bHs = F32(F64(bHs) + xTs * bias)
            Hs[T] = s[T] + F32(2) * Hs[T]
            bHs = F32(bs + F32(2) * bHs)
            return Hs, bHs

        max_cg_iter = max((len(T) if variant == "cg_touched" else d) + int(has_b), 5)
        tr["max_cg_iter"] = max_cg_iter

        def pcg(g, Mv, bg, bM):
            s = np.zeros(d, F32)
            r = np.zeros(d, F32)
            z = np.zeros(d, F32)
            r[T] = -g[T]
            z[T] = r[T] / Mv[T]
            dv = z.copy()
            bs = bd = bz = br = F32(0)
            if has_b:
                br = F32(-bg)
                bz = F32(br / bM)
                bd = bz
            zTr = F64(dot(z, r))
            if has_b:
                zTr = zTr + F64(bz) * F64(br)
            rt = np.sqrt(np.sqrt(zTr))
            cgtol = EPS_CG if EPS_CG < rt else rt
            Q = F64(0)
            it, how = 0, "cap"
            while it < max_cg_iter:
                it += 1
                Hd, bHd = hv(dv, bd)
                dHd = F64(dot(dv, Hd))
                if has_b:
                    dHd = dHd + F64(bd) * F64(bHd)
                if dHd <= 1.0e-16:
                    how = "dhd"
                    break
                alpha = zTr / dHd
                if not np.isfinite(alpha):
                    tr["nonfinite"] = tr["nonfinite"] or "alpha"
                s[T] = _axpy64(alpha, dv[T], s[T])
                if has_b:
                    bs = F32(F64(bs) + alpha * F64(bd))
                alpha = -alpha
                r[T] = _axpy64(alpha, Hd[T], r[T])
                if has_b:
                    br = F32(F64(br) + alpha * F64(bHd))
                newQ = -0.5 * F64(F32(dot(s, r) - dot(s, g)))
                if has_b:
                    newQ = newQ - 0.5 * F64(F32(F32(bs * br) - F32(bs * bg)))
                Qdiff = newQ - Q
                if newQ <= 0 and Qdiff <= 0:
                    if it * Qdiff >= cgtol * newQ:
                        how = "q"
                        break
                else:
                    how = "positive"
                    break
                Q = newQ
                z[T] = r[T] / Mv[T]
                if has_b:
                    bz = F32(br / bM)
                znew = F64(dot(z, r))
                if has_b:
                    znew = znew + F64(bz) * F64(br)
                beta = znew / zTr
                if not np.isfinite(beta):
                    tr["nonfinite"] = tr["nonfinite"] or "beta"
                dv[T] = _axpy64(beta - 1.0, dv[T], dv[T])
                dv[T] = _axpy64(1.0, z[T], dv[T])
                if has_b:
                    bd = F32(F64(bd) * beta)
                    bd = F32(F64(bd) + 1.0 * F64(bz))
                zTr = znew
            tr["cg_exits"].append(how)
            tr["cg_iters"].append(it)
            ctr["cg_iters"] += it
            ctr["cg_" + {"dhd": "dhd", "q": "q", "positive": "positive", "cap": "cap"}[how]] += 1
            return s, bs

        def linesearch(f, s, g, bs, bg):
            nonlocal w, b, wTw
            fold = f
            xv_into(s, bs, tmp)
            sTs, wTs, gTs = F64(dot(s, s)), F64(dot(s, w)), F64(dot(s, g))
            if has_b:
                sTs, wTs, gTs = sTs + F64(bs) * F64(bs), wTs + F64(bs) * F64(b), gTs + F64(bs) * F64(bg)
            alpha = F64(1)
            k = 0
            while k < MAX_HALVINGS:
                loss = F64(0)
                for i in index:
                    loss = loss + c_times_loss(i, F64(tmp[i]) * alpha + F64(wx[i]))
                f = loss + (alpha * alpha * sTs + wTw) / 2.0 + alpha * wTs
                if f - fold <= 0.01 * alpha * gTs:
                    for i in index:
                        wx[i] = F32(F64(wx[i]) + alpha * F64(tmp[i]))
                    break
                alpha = alpha * 0.5
                k += 1
            tr["halvings"].append(k)
            ctr["halvings"] += k
            if k >= MAX_HALVINGS:
                return fold, 0.0
            w[T] = _axpy64(alpha, s[T], w[T])
            b = F32(F64(b) + alpha * F64(bs))
            wTw = wTw + (alpha * alpha * sTs + 2 * alpha * wTs)
            return f, alpha

        # -- newton (w0 == w == 0: the two evaluations at the start are one)
        wTw = F64(0)
        f = fun()
        g, bg = grad()
        gnorm0 = gnorm = norm(g, bg)
        it = 1
        if gnorm <= eps * gnorm0:
            tr["newton_exit"] = "before_first"
        while tr["newton_exit"] is None and it <= MAX_NEWTON:
            Mv = np.ones(d, F32)
            bM = F32(1)
            for i in I:                                                # get_diag_preconditioner: do_ax2py with the fp32 factor 2 * get_c
                fz, xval = rows_of[i]
                a2 = F32(F32(2) * c32[i])
                Mv[fz] = Mv[fz] + F32(xval * xval) * a2
                if has_b:
                    bM = F32(F64(bM) + bias * bias * 2 * F64(c32[i]))
            Mv[T] = ((1 - ALPHA_PCG) + ALPHA_PCG * Mv[T].astype(F64)).astype(F32)
            bM = F32((1 - ALPHA_PCG) + ALPHA_PCG * F64(bM))
            s, bs = pcg(g, Mv, bg, bM)
            fold = f
            f, step = linesearch(f, s, g, bs, bg)
            tr["newton_iters"] = it
            if step == 0:
                tr["newton_exit"] = "linesearch"
                break
            g, bg = grad()
            gnorm = norm(g, bg)
            if gnorm <= eps * gnorm0:
                tr["newton_exit"] = "gradient"
                break
            if f < -1.0e32:
                tr["newton_exit"] = "f_low"
                break
            if abs(fold - f) <= 1.0e-12 * abs(f):
                tr["newton_exit"] = "actred"
                break
            it += 1
        if tr["newton_exit"] is None:
            tr["newton_exit"] = "cap"
        ctr["newton_iters"] += tr["newton_iters"]
        ctr[{"before_first": "end_before_first", "gradient": "end_gradient", "linesearch": "end_linesearch", "actred": "end_actred", "cap": "end_cap",
             "f_low": "end_actred"}[tr["newton_exit"]]] += 1
        ctr["nonfinite_jobs"] += bool(tr["nonfinite"])
        traces.append(tr)
        # -- emission (SVMJob::solve)
        passes = np.flatnonzero(np.abs(w).astype(F64) >= threshold)
        push_bias = has_b and F64(abs(b)) >= threshold
        if max_nonzeros and len(passes) >= max_nonzeros:
            order = sorted(passes, key=lambda k: (-abs(w[k]), k))[:max_nonzeros]
            if has_b:
                if abs(b) > abs(w[order[-1]]):
                    order.pop()
                else:
                    push_bias = False
            passes = np.sort(np.array(order, dtype=np.int64))
        for k in passes:
            out_r.append(int(k)); out_c.append(label); out_v.append(w[k])
        if push_bias:
            out_r.append(d); out_c.append(label); out_v.append(b)
    return dict(rows=np.array(out_r, np.uint64), cols=np.array(out_c, np.uint64), vals=np.array(out_v, F32), counters=ctr, trace=traces)


# ------------------------------------------------------------------------------------------------ the ctypes callers
def run_newton(path, X, Y, C=None, M=None, R=None, threshold=0.0, max_nonzeros=0, solver=L2_PRIMAL, Cp=1.0, Cn=1.0, max_iter=1000, eps=0.1, bias=1.0,
               threads=1):
    """xrl_single_layer_train_newton_{csr,drm}_f32 of the library at ``path`` -> (dict(rows, cols, vals, shape) or None, error or None)."""
    lib = load(path)
    keep = []
    if smat.issparse(X):
        ptr, idx, val = X.indptr.astype(np.uint64), X.indices.astype(np.uint32), X.data.astype(F32)
        xview = CsrView(X.shape[0], X.shape[1], ptr.ctypes.data, idx.ctypes.data, val.ctypes.data)
        fn = getattr(lib, "xrl_single_layer_train_newton_csr_f32")
    else:
        val = np.ascontiguousarray(X, dtype=F32)
        xview = DrmView(X.shape[0], X.shape[1], val.ctypes.data)
        fn = getattr(lib, "xrl_single_layer_train_newton_drm_f32")
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
    return (got if "rows" in got else None), last_error(lib)


def reference(X, Y, C=None, M=None, R=None, threads=1, **kw):
    """The compiled reference's c_xlinear_single_layer_train_* with the primal solver."""
    kw.setdefault("solver", L2_PRIMAL)
    lib = load(REF)
    assert not hasattr(lib, "xrl_single_layer_train_csr_f32")
    return run_library(REF, X, Y, C, M, R, threads=threads, **kw)[0]


def counters(path=OURS):
    """xrl_debug_newton_counters of the library's last primal training, by name."""
    lib = load(path)
    out = (ctypes.c_uint64 * len(COUNTERS))()
    lib.xrl_debug_newton_counters.restype, lib.xrl_debug_newton_counters.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]
    assert lib.xrl_debug_newton_counters(out, len(COUNTERS)) == 0
    return dict(zip(COUNTERS, (int(v) for v in out)))


def resident(X, Y, C, M, R, kw, stream=None):
    """xrl_train_layer_newton_device over uploaded handles (the Python surface picks it by the solver number) -> (W^T, counters)."""
    from pecos_amd import DeviceMatrix, clib
    hs = [DeviceMatrix.upload(X)] + [None if A is None else DeviceMatrix.upload(as_stored_transpose(A)) for A in (Y, C, M, R)]
    out = DeviceMatrix(clib.train_layer_device(*(h and h.handle for h in hs), threshold=kw.get("threshold", 0.0), max_nonzeros_per_label=kw.get("max_nonzeros", 0),
                                               solver_type=L2_PRIMAL, Cp=kw.get("Cp", 1.0), Cn=kw.get("Cn", 1.0), max_iter=kw.get("max_iter", 1000),
                                               eps=kw.get("eps", 0.1), bias=kw.get("bias", 1.0), stream=stream))
    return out.download(), clib.newton_counters()


def same_counters(got, want):
    """The device's counters (COUNTERS[4:]) against the statement's."""
    return {k: got[k] for k in COUNTERS[4:]} == {k: want[k] for k in COUNTERS[4:]}


# ------------------------------------------------------------------------------------------------ cases
def renumbered(X, mult=37, add=5, width=None):
    """X with feature f moved to mult * f + add inside a matrix `width` wide (at least 10 times wider)."""
    d = X.shape[1]
    width = width or max(10 * d, mult * d + add + 1)
    Z = smat.csr_matrix((X.shape[0], width), dtype=F32)
    Z.indptr, Z.indices, Z.data = X.indptr.copy(), (X.indices.astype(np.int64) * mult + add), X.data.astype(F32)
    return Z


def alias_problem(positive_row=1):
    """40 rows x 12 features, one code whose M column lists rows 10, 20, 30 and one label whose only positive is `positive_row`, which M
    does not list: it is appended to index.  At row 1 its id is below the number of active instances when grad reaches it (three, as all of
    10, 20, 30 are active at w = 0), so its raw wx * y overwrites the compacted slot 1; at row 39 (the same data moved there) nothing is
    overwritten."""
    X = rows_csr(12, [5] * 40, 101).tolil()
    if positive_row != 1:
        X[positive_row] = X[1]
    X = smat.csr_matrix(X.tocsr(), dtype=F32)
    X.sort_indices()
    Y = raw_csc((40, 1), [([positive_row], [1])])
    C = raw_csc((1, 1), [([0], [1])])
    M = raw_csc((40, 1), [([10, 20, 30], [1, 1, 1])])
    return X, Y, C, M


def small_d_problem(d, seed=0):
    """30 rows over d features (every row stores at least one), two labels, pure multi-label."""
    rs = np.random.RandomState(200 + seed + d)
    X = rows_csr(d, [max(1, min(d, int(k))) for k in rs.randint(1, d + 1, 30)], 300 + seed + d)
    Y = raw_csc((30, 2), [(np.arange(0, 30, 3), np.ones(10)), (np.arange(1, 30, 4), np.ones(8))])
    return X, Y


def touched_problem(counts=(1, 63, 64, 65, 129, 1000), seed=17):
    """One code per count: its M column lists 12 rows that together store exactly `count` distinct features of d = 1100."""
    d, rows = 1100, []
    rs = np.random.RandomState(seed)
    ptr, ind, val, mcols, ycols = [0], [], [], [], []
    for k, cnt in enumerate(counts):
        feats = np.sort(rs.choice(d, cnt, replace=False))
        ids = list(range(12 * k, 12 * k + 12))
        for j, r in enumerate(ids):
            mine = feats if j == 0 else np.sort(rs.choice(feats, max(1, min(cnt, 1 + (j * cnt) // 12)), replace=False))
            ind.extend(mine); val.extend(rs.standard_normal(len(mine)) * 0.5); ptr.append(len(ind))
        mcols.append((ids, np.ones(12)))
        ycols.append((ids[::3], np.ones(4)))
    N, K = 12 * len(counts), len(counts)
    X = smat.csr_matrix((N, d), dtype=F32)
    X.indptr, X.indices, X.data = np.array(ptr, np.int64), np.array(ind, np.int64), np.array(val, F32)
    return X, raw_csc((N, K), ycols), raw_csc((K, K), [([k], [1]) for k in range(K)]), raw_csc((N, K), mcols)


def cases():
    """{name: (X, Y, C, M, R, keywords)}: what the CPU half checks against the compiled reference and the GPU half against all three."""
    import ranker_training_rule as rr
    c = {}
    X, Y, C, M = problem(300, 120, 24, 4, 9, 12, 1)
    c["coded"] = (X, Y, C, M, None, dict(threshold=0.1))
    c["coded_costs"] = (X, Y, C, M, relevance(Y, 5), dict(Cp=2.0, Cn=0.5, threshold=0.1))
    c["pure"] = (X[:80], smat.csc_matrix(Y[:80, :6]), None, None, None, dict(threshold=0.1))
    for b in (1.0, 0.5, 0.0, -1.0):
        c[f"bias{b}"] = (X, Y, C, M, None, dict(bias=b, threshold=0.05))
    for e in (1e-4, 0.0):
        c[f"eps{e:g}"] = (X[:120], smat.csc_matrix(Y[:120, :6]), None, None, None, dict(eps=e, threshold=0.0))
    c["layouts"] = rr.layouts() + (None, dict(threshold=0.01))
    c["layouts_R"] = rr.layouts() + (relevance(rr.layouts()[1], 6), dict(threshold=0.01))
    Xs, Ys, Cs, Ms = rr.job_sizes_problem(sizes=(0, 1, 2, 5, 63, 64, 65, 1000))
    c["job_sizes"] = (Xs, Ys, Cs, Ms, None, dict(threshold=0.01))
    Xr, Yr = rr.row_lengths_problem()
    c["row_lengths"] = (Xr, Yr, None, None, None, dict(threshold=0.001))
    c["touched"] = touched_problem() + (None, dict(threshold=0.0))
    for d in (1, 3, 4, 5):
        for b in (1.0, 0.0):
            c[f"d{d}_bias{b}"] = small_d_problem(d) + (None, None, None, dict(bias=b, threshold=0.0, eps=1e-6))
    c["wide_nobias"] = (X, Y, C, M, None, dict(bias=-1.0, threshold=0.0))
    c["alias"] = alias_problem(1) + (None, dict(threshold=0.0, eps=0.01))
    c["alias_twin"] = alias_problem(39) + (None, dict(threshold=0.0, eps=0.01))
    Xt, Yt = rr.ties_problem()
    for k in (1, 5, 100):
        c[f"maxnz{k}"] = (X, Y, C, M, None, dict(max_nonzeros=k, threshold=0.01))
        c[f"ties_maxnz{k}"] = (Xt, Yt, None, None, None, dict(max_nonzeros=k, threshold=0.0))
    rare = raw_csc((Xt.shape[0], 2), [([3, 17, 40], [1, 1, 1]), ([3], [1])])
    c["ties_bias"] = (Xt, rare, None, None, None, dict(max_nonzeros=2, threshold=0.0))
    c["thr_all"] = (X, Y, C, M, None, dict(threshold=0.0))
    c["thr_none"] = (X, Y, C, M, None, dict(threshold=1e6))
    Xd, Yd, Cd, Md, where = rr.repeats_problem()
    c["dups"] = (Xd, Yd, Cd, Md, None, dict(threshold=0.0))
    c["dups_R"] = (Xd, Yd, Cd, Md, rr.repeats_relevance(Yd, where, False), dict(threshold=0.0))
    c["dups_R0"] = (Xd, Yd, Cd, Md, rr.repeats_relevance(Yd, where, True), dict(threshold=0.0))
    # long rows whose products cancel: the order and the width of the additions show
    Xo = rows_csr(400, [200] * 120, 21, scale=3.0)
    Yo = raw_csc((120, 2), [(np.arange(0, 120, 2), np.ones(60)), (np.arange(0, 120, 5), np.ones(24))])
    c["order"] = (Xo, Yo, None, None, None, dict(eps=1e-4, threshold=0.0))
    for name, (Xe, Ye, kw) in empties().items():
        c[name] = (Xe, Ye, None, None, None, kw)
    return c


def empties():
    """No rows / no labels / no features."""
    X, Y, _, _ = problem(20, 10, 3, 1, 4, 5, 2)
    return {"no_rows": (smat.csr_matrix((0, 10), dtype=F32), raw_csc((0, 3), [([], [])] * 3), dict(threshold=0.0)),
            "no_labels": (X, raw_csc((20, 0), []), dict(threshold=0.0)),
            "no_features": (smat.csr_matrix((20, 0), dtype=F32), Y, dict(threshold=0.0))}


def search_problem(seed):
    """Problem `seed` of the search: 4 .. 13 rows over 1 .. 6 features, one label, values and costs over several magnitudes."""
    rs = np.random.RandomState(5000 + seed)
    N, d = int(rs.randint(4, 14)), int(rs.randint(1, 7))
    scale = float(rs.choice([0.1, 1.0, 30.0, 1e3]))
    X = rows_csr(d, [int(k) for k in rs.randint(1, d + 1, N)], 7000 + seed, scale=scale)
    Y = raw_csc((N, 1), [(np.sort(rs.choice(N, int(rs.randint(1, N)), replace=False)),) * 2])
    Y.data[:] = 1
    kw = dict(eps=float(rs.choice([0.0, 1e-6, 1e-3])), bias=float(rs.choice([1.0, 0.0])), Cp=float(rs.choice([1.0, 100.0, 1e4])), Cn=1.0, threshold=0.0)
    return X, Y, kw


def cg_cap_wide_problem():
    """Problem 8 of the search (13 rows x 4 features, Cp = 1e4: ill-conditioned, its CG runs take all five steps of max(4 + 1, 5)) inside
    60 features: there the cap is 61 and a run goes on to a sixth step, which a cap taken from the touched features would cut."""
    X, Y, kw = search_problem(8)
    return renumbered(X, mult=7, add=3, width=60), Y, None, None, None, kw


def search_cases(limit=3000, want=("halving", "dhd", "positive", "cg_cap", "linesearch", "actred")):
    """A seeded search over small problems for traces that show a line-search halving and the rarer CG / Newton exits.  -> {what: (X, Y,
    None, None, None, kw)} for what it found; deterministic."""
    found = {}
    for seed in range(limit):
        X, Y, kw = search_problem(seed)
        t = statement(X, Y, **kw)["trace"][0]
        if t["nonfinite"]:
            continue
        met = set()
        if any(t["halvings"]) and t["newton_exit"] != "linesearch":
            met.add("halving")
        met.update("cg_cap" if e == "cap" else e for e in t["cg_exits"] if e != "q")
        met.add("newton_cap" if t["newton_exit"] == "cap" else t["newton_exit"])
        for m in met:
            if m in want and m not in found:
                found[m] = (X, Y, None, None, None, kw)
        if len(found) == len(want):
            break
    return found


def nonfinite_problem(limit=200):
    """A seeded search over small problems with huge values for one whose trace shows a NON-FINITE alpha in pcg (zTr / dHd with both
    infinite) while X itself is finite and leaves a feature untouched: the device refuses it, naming the label.  -> (X, Y, None, None,
    None, kw); deterministic."""
    for seed in range(limit):
        rs = np.random.RandomState(9000 + seed)
        N, d = int(rs.randint(4, 10)), int(rs.randint(2, 6))
        scale = float(rs.choice([1e15, 1e19, 1e22, 1e30, 1e37]))
        X = rows_csr(d + 3, [int(k) for k in rs.randint(1, d + 1, N)], 9500 + seed, scale=scale)
        Y = raw_csc((N, 1), [(np.sort(rs.choice(N, int(rs.randint(1, N)), replace=False)),) * 2])
        Y.data[:] = 1
        kw = dict(eps=1e-3, bias=float(rs.choice([1.0, 0.0])), threshold=0.0, Cp=float(rs.choice([1.0, 1e-30, 1e30])))
        t = statement(X, Y, **kw)["trace"][0]
        if t["nonfinite"] == "alpha" and t["touched"] < X.shape[1]:
            return X, Y, None, None, None, kw
    raise AssertionError("no case with a non-finite alpha")


# ------------------------------------------------------------------------------------------------ the recorded reference
import os  # noqa: E402

from ranker_training_rule import REPO  # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "primal_training_ref.npz")
PRIMAL = "L2R_L2LOSS_SVC_PRIMAL"
E2E_BASE = dict(nr_splits=4, min_codes=4, threshold=0.05, max_iter=30)
# XLinearModel.train on relevance_rule.fixture_problem() (200 x 64 features x 48 labels, the chain 1 <- 4 <- 16 <- 48): name -> (keywords, with R)
E2E_CONFIGS = {
    "man": (dict(solver_type=PRIMAL, negative_sampling_scheme="tfn+man", post_processor="l3-hinge", beam_size=3, only_topk=4), False),
    "induce": (dict(solver_type=PRIMAL, rel_mode="induce", rel_norm="l1"), True),
    "mixed": (dict(layer_solvers=("L2R_L2LOSS_SVC_DUAL", "L2R_L1LOSS_SVC_DUAL", PRIMAL)), False),
}
E2E_PREDICTED, E2E_QUERIES, E2E_PREDICT_KW = "man", 70, dict(beam_size=3, only_topk=4, post_processor="l3-hinge")


def e2e_kwargs(name, ours=False):
    """X, Y (CSC), C, R and the keywords of XLinearModel.train for a configuration.  "mixed" gives one solver per layer through
    train_params: the reference's own parameter objects, or (ours) the same as plain dicts."""
    import relevance_rule as rl
    kw, with_R = E2E_CONFIGS[name]
    X, Y, C, R = rl.fixture_problem()
    full = dict(E2E_BASE, **kw)
    solvers = full.pop("layer_solvers", None)
    if solvers:
        layer = [dict(threshold=E2E_BASE["threshold"], max_iter=E2E_BASE["max_iter"], solver_type=s) for s in solvers]
        if ours:
            full = dict(train_params=dict(nr_splits=4, min_codes=4, hlm_args=dict(neg_mining_chain="tfn", model_chain=layer)))
        else:
            from pecos.xmc import HierarchicalMLModel, MLModel
            from pecos.xmc.xlinear.model import XLinearModel
            full = dict(train_params=XLinearModel.TrainParams(nr_splits=4, min_codes=4, hlm_args=HierarchicalMLModel.TrainParams(
                neg_mining_chain="tfn", model_chain=[MLModel.TrainParams(**p) for p in layer])))
    return X, smat.csc_matrix(Y), C, (R if with_R else None), full


def recorded():
    return np.load(FIXTURE)


def recorded_case(rec, name):
    """(rows, cols, vals) of a case as the reference gave them (canonical order for the max_nonzeros cases)."""
    return rec[f"case__{name}__rows"].astype(np.uint64), rec[f"case__{name}__cols"].astype(np.uint64), rec[f"case__{name}__bits"].view(F32)
