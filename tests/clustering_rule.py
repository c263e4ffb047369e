"""The rule of the label clustering (K11), stated in numpy, and what the clustering tests share: the ctypes caller of
``c_run_clustering_*`` for any library, the case generators, and the two wrong-order variants used as preconditions.

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


def statement(X, depth, algo=SKMEANS, seed=0, max_iter=20, max_rate=1.0, min_rate=1.0, warmup=1.0, variant=None, nnz=None):
    """The rule on a CSR with sorted rows.  Returns dict(codes, scores [depth, L], node_seed, work {node id: (start, working end, r pos,
    l pos)}, perm [depth, L], first_touch [depth], iters {node id: iterations run}).  variant: None, "reverse_walk" (the centre walks
    each half's elements in descending order) or "ascending_norm" (the SKMEANS norm past the switch in ascending feature order)."""
    assert variant in (None, "reverse_walk", "ascending_norm")
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

    def score_and_split(c, s, e):
        for p in range(s, e):
            idx, val = rows[elements[p]]
            scores[elements[p]] = _chain(c[idx] * val)
        ids = np.array(elements[s:e], dtype=np.int64)
        order = np.lexsort((ids, scores[ids]))                 # (score, id); -0 == +0
        mid = (s + e) >> 1
        before = elements[s:mid]
        ids = ids[order]
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

    def norm_sq(c, touched):
        if first_touch and variant != "ascending_norm":
            order = np.array(list(touched), dtype=np.int64)    # dicts keep the order of insertion
            return _chain(c[order] * c[order])
        return _chain(c * c)

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
            for k in range(max_iter):
                iters[nid] += 1
                c = np.zeros(cols, F32)
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
                    accumulate(c, t1, range(mid, we), F32(1.0))
                    a = norm_sq(c, t1)
                    if a > 0:
                        c = (c.astype(np.float64) * (1.0 / np.sqrt(np.float64(a)))).astype(F32)
                    accumulate(c2, t2, range(s, mid), F32(1.0))
                    a = norm_sq(c2, t2)
                    if a > 0:
                        c2 = (c2.astype(np.float64) * (1.0 / np.sqrt(np.float64(a)))).astype(F32)
                    c = c + (-c2)
                if not score_and_split(c, s, we):
                    break
            work[nid] = (s, we, r_pos, l_pos)
            m = (s + e) >> 1
            rng_of[2 * nid], rng_of[2 * nid + 1] = (s, m), (m, e)
            if sampled:
                score_and_split(c, s, e)
        perms[d] = perm
        out_scores[d] = scores
    codes = np.zeros(L, np.uint32)
    for leaf in range(1 << depth):
        s, e = rng_of[(1 << depth) + leaf]
        codes[elements[s:e]] = leaf
    return dict(codes=codes, scores=out_scores, node_seed=np.array(node_seed, np.uint32), work=work, perm=perms,
                first_touch=first_touch_levels, iters=iters)


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


def dense_ok(X):
    """Cases small enough to run through the dense entry point as well."""
    return X.shape[0] * X.shape[1] <= 3_000_000
