"""The rule of the label clustering (K11), stated in numpy, and what the clustering tests share: the ctypes caller of
``c_run_clustering_*`` for any library, the case generators, the wrong variants used as preconditions (two orders, and the centre kept
unscaled under an infinite norm), and an opt-in trace of what left fp32's range at which node and iteration.

The statement follows the reference at threads = 1 (pecos/core/utils/clustering.hpp:189-503, matrix.hpp:79-152, 808-1047) in fp32 steps:
every product rounded, every addition rounded.  Its draws restate the C++ standard library the reference is compiled with here
(libstdc++: mt19937, uniform_int_distribution's multiply-and-reject downscaling of a 32-bit generator, shuffle's two-positions-per-draw)."""
import ctypes
import os

import numpy as np
import scipy.sparse as smat

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OURS = os.environ.get("PECOS_XRL_AMD_SO") or os.path.join(REPO, "pecos_amd", "lib", "libxrl_amd.so")
REF = os.path.join(REPO, "oracle", "_ref", "libpecos_float32.so")
KMEANS, SKMEANS = 0, 5
F32 = np.float32


# ------------------------------------------------------------------------------------------------ the draws
class Mt19937:
    """std::mt19937(seed): the raw 32-bit outputs."""

    def __init__(self, seed):
        self.bg = np.random.MT19937()
        self.bg._legacy_seeding(int(seed) & 0xFFFFFFFF)
        self.buf, self.at = [], 0

    def __call__(self):
        if self.at == len(self.buf):
            self.buf, self.at = [int(v) for v in self.bg.random_raw(256)], 0
        self.at += 1
        return self.buf[self.at - 1]


def uniform_int(g, a, b):
    """std::uniform_int_distribution<T>(a, b)(g) over a 32-bit generator: a raw draw when the range is all 32 bits, else the
    multiply-and-reject downscaling (bits/uniform_int_dist.h)."""
    urange = b - a
    assert 0 <= urange <= 0xFFFFFFFF
    if urange == 0xFFFFFFFF:
        return a + g()
    rng = urange + 1
    product = g() * rng
    low = product & 0xFFFFFFFF
    if low < rng:
        threshold = ((1 << 32) - rng) % rng
        while low < threshold:
            product = g() * rng
            low = product & 0xFFFFFFFF
    return a + (product >> 32)


def shuffle(g, a):
    """std::shuffle(a.begin(), a.end(), g) in place (bits/stl_algo.h): two swap positions per draw while the range allows it."""
    n = len(a)
    if n == 0:
        return
    if 0xFFFFFFFF // n >= n:
        i = 1
        if n % 2 == 0:
            j = uniform_int(g, 0, 1)
            a[i], a[j] = a[j], a[i]
            i += 1
        while i < n:
            swap_range = i + 1
            x = uniform_int(g, 0, swap_range * (swap_range + 1) - 1)
            p0, p1 = x // (swap_range + 1), x % (swap_range + 1)
            a[i], a[p0] = a[p0], a[i]
            i += 1
            a[i], a[p1] = a[p1], a[i]
            i += 1
        return
    for i in range(1, n):
        j = uniform_int(g, 0, i)
        a[i], a[j] = a[j], a[i]


def sample_rate(d, depth, max_rate, min_rate, warmup):
    """clustering.hpp:156-167 in float arithmetic."""
    warm = int(F32(depth) * F32(warmup))
    if d < warm:
        return F32(min_rate), warm
    return F32(min_rate) + (F32(max_rate) - F32(min_rate)) * F32(d + 1 - warm) / F32(depth - warm), warm


# ------------------------------------------------------------------------------------------------ the statement
def _chain(terms):
    """+0 + t0 + t1 + ... in fp32, one rounded addition after the other."""
    return np.cumsum(np.concatenate([np.zeros(1, F32), np.asarray(terms, F32)]), dtype=F32)[-1]


def as_full_csr(X):
    """A dense matrix as the CSR that stores every entry, zeros included (how the dense entry point computes)."""
    X = np.ascontiguousarray(X, dtype=F32)
    r, c = X.shape
    m = smat.csr_matrix((r, c), dtype=F32)
    m.indptr, m.indices, m.data = np.arange(r + 1, dtype=np.int64) * c, np.tile(np.arange(c, dtype=np.int64), r), X.reshape(-1).copy()
    return m


def _first_inf(terms):
    """The position in the chain +0 + t0 + t1 + ... at which it first becomes infinite (None: it never does)."""
    run = np.cumsum(np.asarray(terms, F32), dtype=F32)
    at = np.flatnonzero(np.isinf(run))
    return int(at[0]) if len(at) else None


def statement(X, depth, algo=SKMEANS, seed=0, max_iter=20, max_rate=1.0, min_rate=1.0, warmup=1.0, variant=None, nnz=None, trace=False):
    """The rule on a CSR with sorted rows.  Returns dict(codes, scores [depth, L], node_seed, work {node id: (start, working end, r pos,
    l pos)}, perm [depth, L], first_touch [depth], iters {node id: iterations run}).  variant: None, "reverse_walk" (the centre walks
    each half's elements in descending order), "ascending_norm" (the SKMEANS norm past the switch in ascending feature order) or
    "unscaled_on_inf" (a half whose norm is infinite keeps its summed centre, where the rule multiplies it by 1 / sqrt(inf) = 0).
    ``nnz``: the entry count the norm-order switch sees, when it is not X's own.
    trace=True adds ``trace``, {(node id, iteration, or "whole" for a sampled level's last assignment): dict} with
      norms       the two ||c||^2 (right, left) of a SKMEANS iteration past the first, else None
      inf_sides   "R", "L", "RL" or "": the sides whose norm is +inf;  inf_norms = how many
      zeroed      the sides whose centre an infinite norm turned into zeros (inf_norms, unless the variant leaves them)
      zero_norm_sides   (present when not empty) the sides whose summed centre holds a nonzero entry while every square underflows:
                  the norm is 0 and the centre is not scaled
      inf_at      per side, the position in the norm's chain at which it first becomes infinite (None: never); the chain walks the
                  node's features in ascending order while dense, in the side's order of first touch after the switch
      runs        the features stored by at least one element of the node's whole range (the device's runs of the node)
      pos_inf, neg_inf, inf_scores   the +inf, -inf and all infinite scores of the range the iteration scored
      id_decides  the sort's two scores on either side of the midpoint are equal and infinite: the id splits the tie
      nans        NaNs in the centre and in the scores of the scored range"""
    assert variant in (None, "reverse_walk", "ascending_norm", "unscaled_on_inf")
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return _statement(X, depth, algo, seed, max_iter, max_rate, min_rate, warmup, variant, nnz, trace)


def _statement(X, depth, algo, seed, max_iter, max_rate, min_rate, warmup, variant, nnz, want_trace):
    L, cols = X.shape
    indptr, indices, data = X.indptr, X.indices, X.data.astype(F32)
    nnz = int(indptr[-1]) if nnz is None else nnz
    rows = [(indices[indptr[e]:indptr[e + 1]], data[indptr[e]:indptr[e + 1]]) for e in range(L)]
    elements = list(range(L))
    g = Mt19937(seed)
    node_seed = [uniform_int(g, 0, 0xFFFFFFFF) for _ in range(2 << depth)]
    rng_of = {1: (0, L)}
    scores = np.zeros(L, F32)
    out_scores = np.zeros((depth, L), F32)
    work, iters, perms, first_touch_levels = {}, {}, np.zeros((depth, L), np.uint32), []
    first_touch = False
    trace = {}

    def score_and_split(c, s, e, note=None):
        for p in range(s, e):
            idx, val = rows[elements[p]]
            scores[elements[p]] = _chain(c[idx] * val)
        ids = np.array(elements[s:e], dtype=np.int64)
        order = np.lexsort((ids, scores[ids]))                 # (score, id); -0 == +0
        mid = (s + e) >> 1
        before = elements[s:mid]
        ids = ids[order]
        if note is not None:
            sc = scores[ids]
            note.update(pos_inf=int(np.isposinf(sc).sum()), neg_inf=int(np.isneginf(sc).sum()), inf_scores=int(np.isinf(sc).sum()),
                        id_decides=bool(np.isinf(sc[mid - s - 1]) and sc[mid - s - 1] == sc[mid - s]),
                        nans=int(np.isnan(c).sum()) + int(np.isnan(sc).sum()))
        elements[s:mid] = sorted(int(v) for v in ids[:mid - s])
        elements[mid:e] = sorted(int(v) for v in ids[mid - s:])
        return elements[s:mid] != before

    def accumulate(c, touched, half, alpha):
        for p in (reversed(half) if variant == "reverse_walk" else half):
            idx, val = rows[elements[p]]
            c[idx] = c[idx] + val * alpha
            if first_touch and algo == SKMEANS:
                for f in idx:
                    if f not in touched:
                        touched[int(f)] = len(touched)

    def norm_sq(c, touched, runs=None):
        """-> (||c||^2, where its chain over the node's runs first becomes infinite)"""
        if first_touch and variant != "ascending_norm":
            order = np.array(list(touched), dtype=np.int64)    # dicts keep the order of insertion
            return _chain(c[order] * c[order]), (_first_inf(c[order] * c[order]) if want_trace else None)
        return _chain(c * c), (_first_inf(c[runs] * c[runs]) if want_trace else None)

    def scaled(c, a, side, note):
        if not a > 0:
            if a == 0 and np.any(c != 0):
                note["zero_norm_sides"] = note.get("zero_norm_sides", "") + side
            return c
        if np.isinf(a):
            note["inf_sides"] += side
            if variant == "unscaled_on_inf":
                return c
            note["zeroed"] += 1
        return (c.astype(np.float64) * (1.0 / np.sqrt(np.float64(a)))).astype(F32)

    for d in range(depth):
        nodes = 1 << d
        rate, _ = sample_rate(d, depth, max_rate, min_rate, warmup)
        sampled = float(rate) < 1.0
        if float(nnz) / (float(nodes) * float(cols)) < 1:
            first_touch = True
        first_touch_levels.append(first_touch)
        perm = np.arange(L, dtype=np.uint32)
        for nid in range(nodes, 2 * nodes):
            s, e = rng_of[nid]
            g = Mt19937(node_seed[nid])
            we = e
            if sampled:
                pos = list(range(s, e))
                shuffle(g, pos)
                perm[s:e] = pos
                elements[s:e] = [elements[p] for p in pos]
                we = s + int(F32(rate) * F32(e - s))
            n, mid = we - s, (s + we) >> 1
            c = np.zeros(cols, F32)
            r_pos = l_pos = 0
            iters[nid] = 0
            node_runs = np.unique(np.concatenate([rows[elements[p]][0] for p in range(s, e)] + [np.zeros(0, np.int64)])).astype(np.int64) if want_trace else None
            for k in range(max_iter):
                iters[nid] += 1
                c = np.zeros(cols, F32)
                note = dict(norms=None, inf_sides="", zeroed=0, inf_at=(None, None), runs=len(node_runs)) if want_trace else None
                if k == 0:
                    r = uniform_int(g, 0, n - 1)
                    l = (r + uniform_int(g, 1, n - 1)) % n
                    r_pos, l_pos = s + r, s + l
                    idx, val = rows[elements[r_pos]]
                    c[idx] = c[idx] + val
                    idx, val = rows[elements[l_pos]]
                    c[idx] = c[idx] + (-val)
                elif algo == KMEANS:
                    accumulate(c, {}, range(mid, we), F32(1.0 / (we - mid)))
                    accumulate(c, {}, range(s, mid), F32(-1.0 / (mid - s)))
                else:
                    c2, t1, t2 = np.zeros(cols, F32), {}, {}
                    side = note if want_trace else dict(inf_sides="", zeroed=0)
                    accumulate(c, t1, range(mid, we), F32(1.0))
                    a1, at1 = norm_sq(c, t1, node_runs)
                    c = scaled(c, a1, "R", side)
                    accumulate(c2, t2, range(s, mid), F32(1.0))
                    a2, at2 = norm_sq(c2, t2, node_runs)
                    c2 = scaled(c2, a2, "L", side)
                    c = c + (-c2)
                    if want_trace:
                        note.update(norms=(a1, a2), inf_at=(at1, at2))
                changed = score_and_split(c, s, we, note)
                if want_trace:
                    note["inf_norms"] = len(note["inf_sides"])
                    note["nans"] += sum(int(np.isnan(a)) for a in note["norms"] or ())
                    trace[(nid, k)] = note
                if not changed:
                    break
            work[nid] = (s, we, r_pos, l_pos)
            m = (s + e) >> 1
            rng_of[2 * nid], rng_of[2 * nid + 1] = (s, m), (m, e)
            if sampled:
                note = dict(norms=None, inf_sides="", inf_norms=0, zeroed=0, inf_at=(None, None), runs=len(node_runs)) if want_trace else None
                score_and_split(c, s, e, note)
                if want_trace:
                    trace[(nid, "whole")] = note
        perms[d] = perm
        out_scores[d] = scores
    codes = np.zeros(L, np.uint32)
    for leaf in range(1 << depth):
        s, e = rng_of[(1 << depth) + leaf]
        codes[elements[s:e]] = leaf
    out = dict(codes=codes, scores=out_scores, node_seed=np.array(node_seed, np.uint32), work=work, perm=perms,
               first_touch=first_touch_levels, iters=iters)
    if want_trace:
        out["trace"] = trace
    return out


# ------------------------------------------------------------------------------------------------ calling a library
class CsrView(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_uint32), ("cols", ctypes.c_uint32), ("row_ptr", ctypes.c_void_p), ("col_idx", ctypes.c_void_p), ("val", ctypes.c_void_p)]


class DrmView(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_uint32), ("cols", ctypes.c_uint32), ("val", ctypes.c_void_p)]


class Param(ctypes.Structure):
    _fields_ = [("partition_algo", ctypes.c_uint64), ("seed", ctypes.c_int), ("kmeans_max_iter", ctypes.c_uint64), ("threads", ctypes.c_int),
                ("max_sample_rate", ctypes.c_float), ("min_sample_rate", ctypes.c_float), ("warmup_ratio", ctypes.c_float)]


def make_param(algo=SKMEANS, seed=0, max_iter=20, max_rate=1.0, min_rate=1.0, warmup=1.0, threads=1):
    return Param(algo, seed, max_iter, threads, max_rate, min_rate, warmup)


_libs = {}


def load(path):
    if path not in _libs:
        _libs[path] = ctypes.CDLL(path)
    return _libs[path]


def last_error(lib):
    lib.xrl_last_error.restype = ctypes.c_char_p
    e = lib.xrl_last_error()
    if e:
        lib.xrl_clear_error()
    return e.decode() if e else None


def run_library(path, X, depth, threads=1, **kw):
    """c_run_clustering_csr_f32 (scipy CSR) or c_run_clustering_drm_f32 (ndarray) of the library at ``path`` -> (codes, error or None)."""
    lib = load(path)
    param = make_param(threads=threads, **kw)
    codes = np.full(X.shape[0], 0xFFFFFFFF, dtype=np.uint32)
    if smat.issparse(X):
        ptr, idx, val = X.indptr.astype(np.uint64), X.indices.astype(np.uint32), X.data.astype(F32)
        view = CsrView(X.shape[0], X.shape[1], ptr.ctypes.data, idx.ctypes.data, val.ctypes.data)
        fn = lib.c_run_clustering_csr_f32
    else:
        val = np.ascontiguousarray(X, dtype=F32)
        view = DrmView(X.shape[0], X.shape[1], val.ctypes.data)
        fn = lib.c_run_clustering_drm_f32
    fn.restype, fn.argtypes = None, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    fn(ctypes.byref(view), depth, ctypes.byref(param), codes.ctypes.data)
    return codes, (last_error(lib) if hasattr(lib, "xrl_last_error") else None)


def reference(X, depth, threads=1, **kw):
    return run_library(REF, X, depth, threads=threads, **kw)[0]


# ------------------------------------------------------------------------------------------------ cases
def random_csr(rows, cols, per_row, seed, empty_rows=()):
    """Sparse rows of about ``per_row`` entries, N(0, 1) values, sorted indices; ``empty_rows`` are emptied."""
    rs = np.random.RandomState(seed)
    ind, ptr, val = [], [0], []
    for r in range(rows):
        k = 0 if r in empty_rows else min(cols, max(1, int(rs.poisson(per_row))))
        ind.extend(np.sort(rs.choice(cols, k, replace=False)))
        ptr.append(len(ind))
    val = rs.standard_normal(len(ind)).astype(F32)
    m = smat.csr_matrix((rows, cols), dtype=F32)
    m.indptr, m.indices, m.data = np.array(ptr, np.int64), np.array(ind, np.int64), val
    return m


def near_duplicate(rows=600, cols=4000, pattern=30, keep=0.9, seed=0):
    """Rows that are near copies of one another: one pattern of ``pattern`` columns, each row keeps each with probability ``keep``, values
    u_j * (1 + 2^-21 * N(0, 1)).  Scores then tie to within rounding, so the order of the additions decides codes."""
    rs = np.random.RandomState(seed)
    cols_of = np.sort(rs.choice(cols, pattern, replace=False))
    u = rs.standard_normal(pattern)
    ind, ptr, val = [], [0], []
    for r in range(rows):
        k = rs.rand(pattern) < keep
        ind.extend(cols_of[k])
        val.extend(u[k] * (1 + 2.0 ** -21 * rs.standard_normal(int(k.sum()))))
        ptr.append(len(ind))
    m = smat.csr_matrix((rows, cols), dtype=F32)
    m.indptr, m.indices, m.data = np.array(ptr, np.int64), np.array(ind, np.int64), np.array(val, F32)
    return m


def first_centre_rows(rows, seed):
    """The two rows (r, l) whose difference is the root's first centre when nothing is sampled."""
    g = Mt19937(seed)
    node_seed = [uniform_int(g, 0, 0xFFFFFFFF) for _ in range(2)]
    g = Mt19937(node_seed[1])
    r = uniform_int(g, 0, rows - 1)
    return r, (r + uniform_int(g, 1, rows - 1)) % rows


def run_lengths_matrix(rows=1000, lengths=(1000, 129, 65, 64, 63, 1, 1, 1), seed=5):
    """Column j is stored in ``lengths[j]`` rows: at depth 1 the one node's run of feature j has that many entries."""
    rs = np.random.RandomState(seed)
    D = np.zeros((rows, len(lengths)), dtype=F32)
    for j, n in enumerate(lengths):
        pick = np.arange(rows) if n == rows else rs.choice(rows, n, replace=False)
        D[pick, j] = rs.standard_normal(n).astype(F32) + (3 if j == 0 else 0)
    m = smat.csr_matrix(D)
    m.sort_indices()
    return m


# seeds of near_duplicate() found by tests/golden/make_golden_clustering.py's search: the order preconditions hold on them
NEAR_DUPLICATE_SEEDS = {SKMEANS: 8, KMEANS: 1}

SAMPLING = {"warm": dict(min_rate=0.1, max_rate=1.0, warmup=0.4), "half": dict(min_rate=0.5, max_rate=0.5, warmup=0.0),
            "full": dict(min_rate=1.0, max_rate=1.0, warmup=0.0)}


def cases():
    """{name: (X as a sorted scipy CSR, depth, keywords of statement() / run_library())}: the cases of the CPU and the GPU half."""
    c = {}
    for algo, tag in ((SKMEANS, "sk"), (KMEANS, "km")):
        for seed in (0, 1, 2):
            c[f"rand300_{tag}_s{seed}"] = (random_csr(300, 2000, 8, 2), 5, dict(algo=algo, seed=seed))
        c[f"pow2_{tag}"] = (random_csr(32, 40, 5, 11), 5, dict(algo=algo))
        c[f"pow2p1_{tag}"] = (random_csr(33, 40, 5, 12), 5, dict(algo=algo))
        c[f"odd127_{tag}"] = (random_csr(127, 60, 6, 13), 6, dict(algo=algo))
        c[f"n1025_{tag}"] = (random_csr(1025, 300, 6, 14), 4, dict(algo=algo))
        c[f"n259_{tag}"] = (random_csr(259, 100, 6, 15), 3, dict(algo=algo))
        c[f"n255_{tag}"] = (random_csr(255, 100, 6, 16), 2, dict(algo=algo))
        c[f"depth1_{tag}"] = (random_csr(130, 20, 5, 1), 1, dict(algo=algo))
        c[f"depth10_{tag}"] = (random_csr(1100, 500, 6, 17), 10, dict(algo=algo))
        c[f"onecol_{tag}"] = (random_csr(70, 1, 1, 18, empty_rows=(3, 4, 40)), 3, dict(algo=algo))
        r, l = first_centre_rows(90, 4)
        c[f"empty_{tag}"] = (random_csr(90, 50, 4, 19, empty_rows=(0, r, 57, 89)), 4, dict(algo=algo, seed=4))
        one = random_csr(1, 30, 9, 20)
        c[f"equal_{tag}"] = (smat.vstack([one] * 100).tocsr(), 4, dict(algo=algo))
        fifty = random_csr(50, 80, 6, 21)
        c[f"dup_{tag}"] = (smat.vstack([fifty] * 3).tocsr(), 4, dict(algo=algo))
        c[f"runs_{tag}"] = (run_lengths_matrix(), 1, dict(algo=algo))
        c[f"dense_norm_{tag}"] = (random_csr(200, 10, 5, 22), 5, dict(algo=algo))            # never switches
        c[f"first_touch_{tag}"] = (random_csr(100, 5000, 8, 23), 4, dict(algo=algo))         # first-touch from the root on
        for it in (0, 1, 2):
            c[f"iter{it}_{tag}"] = (random_csr(300, 2000, 8, 2), 5, dict(algo=algo, max_iter=it))
            c[f"iter{it}_sampled_{tag}"] = (random_csr(500, 300, 8, 3), 5, dict(algo=algo, max_iter=it, **SAMPLING["warm"]))
        for name, kw in SAMPLING.items():
            c[f"sample_{name}_{tag}"] = (random_csr(500, 300, 8, 3), 5, dict(algo=algo, **kw))
        s = NEAR_DUPLICATE_SEEDS[algo]
        c[f"near_duplicate_{tag}"] = (near_duplicate(seed=s), 6, dict(algo=algo, seed=s))
        sub = random_csr(200, 300, 8, 24)
        sub.data = (sub.data.astype(np.float64) * 1e-20).astype(F32)                         # products and sums of squares are subnormal
        c[f"subnormal_{tag}"] = (sub, 4, dict(algo=algo))
    for X, _, _ in c.values():
        X.sort_indices()
    return c


def scaled_csr(X, factor, rows=None):
    """X with the values of ``rows`` (all rows when None) multiplied by ``factor`` in fp64 and rounded to fp32."""
    X = X.copy()
    per_row = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    pick = np.ones(X.nnz, bool) if rows is None else np.isin(per_row, np.asarray(rows))
    X.data[pick] = (X.data[pick].astype(np.float64) * factor).astype(F32)
    return X


def with_column_zero(X, values):
    """X with column 0 stored in every row, holding ``values``."""
    D = X.toarray()
    D[:, 0] = 0
    m = smat.csr_matrix(D)
    first = smat.csr_matrix((np.asarray(values, F32), (np.arange(X.shape[0]), np.zeros(X.shape[0], np.int64))), shape=X.shape)
    m = (m + first).tocsr().astype(F32)
    m.sort_indices()
    return m


def two_blocks(rows=64, cols=30, block_cols=6, factor=3e18, rest_factor=1.0, seed=0, rng_seed=30, shared=True):
    """Half of the rows ("the block") store every one of the first ``block_cols`` columns with a positive value times ``factor``; the
    others are sparse rows of N(0, 1) times ``rest_factor`` on the remaining columns, and with ``shared`` a few of them store column 0 as
    well.  The block holds
    the root's first right row and not its first left row, so the root's first split is the block against the rest: from then on one
    half sums only block rows and the other none."""
    rs = np.random.RandomState(rng_seed)
    r, l = first_centre_rows(rows, seed)
    block = [r] + [int(v) for v in rs.permutation([i for i in range(rows) if i not in (r, l)])[:rows // 2 - 1]]
    D = np.zeros((rows, cols), np.float64)
    for i in range(rows):
        if i in block:
            D[i, :block_cols] = (0.5 + np.abs(rs.standard_normal(block_cols))) * factor
        else:
            k = max(1, int(rs.poisson(5)))
            D[i, block_cols + rs.choice(cols - block_cols, min(k, cols - block_cols), replace=False)] = rs.standard_normal(min(k, cols - block_cols)) * rest_factor
            if shared and rs.rand() < 0.25:
                D[i, 0] = rs.standard_normal() * rest_factor
    m = smat.csr_matrix(D.astype(F32))
    m.sort_indices()
    return m


def late_overflow(rows=48, plain_cols=200, huge_rows=24, huge=6e18, seed=33):
    """Ordinary sparse rows of about nine entries on the first ``plain_cols`` columns; the last ``huge_rows`` rows also store one column of
    their own past those, holding about ``huge``: each such square is about 4e37, so a half's norm overflows only at the tenth of them.
    In ascending feature order they come after every ordinary feature, and in first-touch order after the features of nine rows: past
    the 64th term of the chain either way."""
    rs = np.random.RandomState(seed)
    D = np.zeros((rows, plain_cols + huge_rows), np.float64)
    for i in range(rows):
        D[i, rs.choice(plain_cols, max(4, int(rs.poisson(9))), replace=False)] = 1.0
    D[:, :plain_cols] *= rs.standard_normal((rows, plain_cols))
    for j in range(huge_rows):
        D[rows - huge_rows + j, plain_cols + j] = huge * rs.uniform(0.9, 1.1) * rs.choice([-1.0, 1.0])
    m = smat.csr_matrix(D.astype(F32))
    m.sort_indices()
    return m


def spread_columns(X, cols, top=False):
    """X's column ids under the strictly increasing map j -> j * ((cols - 1) // (X's cols - 1)); with ``top`` the last column goes to
    cols - 1.  The order of the ids, and so the rule's walk, is unchanged; only the first-touch switch sees the width."""
    old = X.shape[1]
    step = (cols - 1) // (old - 1)
    new = np.arange(old, dtype=np.int64) * step
    if top:
        new[-1] = cols - 1
    assert np.all(np.diff(new) > 0) and new[-1] < cols
    m = smat.csr_matrix((X.shape[0], cols), dtype=F32)
    m.indptr, m.indices, m.data = X.indptr.astype(np.int64), new[X.indices], X.data.astype(F32)
    return m


WIDE_IDS_DEPTH, WIDE_IDS_KW = 6, dict(algo=SKMEANS, seed=NEAR_DUPLICATE_SEEDS[SKMEANS])


def wide_ids(cols=None):
    """The compact matrix of the widest-ids case (cols=None): the SKMEANS near-duplicate case, on which the norm's order decides codes,
    with its 30 columns renumbered 0 .. 29; or those columns spread over ``cols`` with the last one at cols - 1.  The rule sees column
    ids only through their order and through the first-touch switch, so every spread wide enough to be in first-touch order from the
    root has the codes and scores of statement(compact, nnz=0)."""
    X = near_duplicate(seed=NEAR_DUPLICATE_SEEDS[SKMEANS])
    used = np.unique(X.indices)
    m = smat.csr_matrix((X.shape[0], len(used)), dtype=F32)
    m.indptr, m.indices, m.data = X.indptr, np.searchsorted(used, X.indices).astype(np.int64), X.data
    return m if cols is None else spread_columns(m, cols, top=True)


def range_edge_cases():
    """{name: (X, depth, keywords)}: finite inputs whose norms, centres or scores leave fp32's range, up or down, while no centre entry
    and no score of any iteration is a NaN (tests/test_clustering_cpu.py checks that on the statement's trace, and what each name
    claims).  Small: at most 128 rows, depth at most 4."""
    c = {}
    base, wide = random_csr(64, 30, 5, 7), random_csr(64, 5000, 5, 8)
    signs = np.random.RandomState(75)
    col0 = signs.choice([-1.0, 1.0], 64) * signs.uniform(1.0, 2.0, 64)
    for algo, tag in ((SKMEANS, "sk"), (KMEANS, "km")):
        kw = dict(algo=algo)
        c[f"collapse_dense_{tag}"] = (scaled_csr(base, 3e18), 3, kw)                          # both norms overflow, no score does
        c[f"collapse_first_touch_{tag}"] = (scaled_csr(wide, 3e18), 3, kw)
        c[f"inf_scores_dense_{tag}"] = (scaled_csr(base, 1e19), 3, kw)                        # some score chains overflow as well
        c[f"inf_scores_first_touch_{tag}"] = (scaled_csr(wide, 1e19), 3, kw)
        c[f"one_half_{tag}"] = (two_blocks(), 3, kw)                                          # also: some nodes of level 1 and 2 overflow, some do not
        c[f"one_half_first_touch_{tag}"] = (spread_columns(two_blocks(), 5000), 3, kw)
        c[f"late_dense_{tag}"] = (late_overflow(), 1, kw)
        c[f"late_first_touch_{tag}"] = (spread_columns(late_overflow(), 5000), 1, kw)
        c[f"inf_ties_{tag}"] = (with_column_zero(base, col0 * 1e30), 3, kw)                   # scores +inf and -inf, the id splits
        c[f"subnormal_norm_{tag}"] = (scaled_csr(base, 3e-23), 3, kw)
        c[f"zero_norm_{tag}"] = (two_blocks(factor=1.0, rest_factor=1e-26, shared=False), 3, kw)
        c[f"sampled_{tag}"] = (scaled_csr(base, 3e18 if algo == SKMEANS else 1e19), 3, dict(algo=algo, **SAMPLING["half"]))
    r, l = first_centre_rows(64, 0)
    c["all_but_first_centre_sk"] = (scaled_csr(base, 1e20, rows=[i for i in range(64) if i not in (r, l)]), 1, dict(algo=SKMEANS))
    for X, _, _ in c.values():
        X.sort_indices()
    return c


def dense_ok(X):
    """Cases small enough to run through the dense entry point as well."""
    return X.shape[0] * X.shape[1] <= 3_000_000
