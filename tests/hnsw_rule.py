"""HNSW search (K17): the numpy statement of the rule, a reader and a writer of the reference's index folder, the ctypes callers of this
library and of the compiled reference, case generators, and the wrong variants the tests show to differ.

The statement:
  sparse   dot = 0.0f + the rounded fp32 products of the matching ids in ascending id order, one addition after the other, no FMA;
           ip = (float)(1.0 - (double)dot); l2 = (float)((double)(0.0f + 0.0f) - 2.0 * (double)dot)
  dense    the reference's avx512f clone: 16 fused accumulators, the 4-wide fold, unfused groups of 4, a fused scalar tail
  search   the reference's predict_single / search_level, over libstdc++'s push_heap / pop_heap / sort_heap with a comparator that reads
           the distance only
  NaN      finite inputs only, so every NaN distance is the x86 host's default NaN 0xFFC00000 (numpy on x86 leaves the same bits); the
           traversal's comparisons are the reference's as written, all false under a NaN
"""
import ctypes
import json
import os
import struct

import numpy as np
import scipy.sparse as smat

from clustering_rule import OURS, REF, CsrView, DrmView, last_error, load

F32 = np.float32
TYPES = {("csr", "ip"): "pecos::ann::HNSW<float, pecos::ann::FeatVecSparseIPSimd<uint32_t, float>>",
         ("csr", "l2"): "pecos::ann::HNSW<float, pecos::ann::FeatVecSparseL2Simd<uint32_t, float>>",
         ("drm", "ip"): "pecos::ann::HNSW<float, pecos::ann::FeatVecDenseIPSimd<float>>",
         ("drm", "l2"): "pecos::ann::HNSW<float, pecos::ann::FeatVecDenseL2Simd<float>>"}
COUNTERS = ("dist", "pops", "admissions", "passes", "max_cand", "rerun", "lds_queries", "hbm_queries")


def host_has_avx512f():
    try:
        return "avx512f" in open("/proc/cpuinfo").read()
    except OSError:
        return False


def have_reference():
    return os.path.exists(REF)


# ------------------------------------------------------------------------------------------------ arithmetic
def fma32(a, b, c):
    """round_fp32(a * b + c) with ONE rounding, elementwise over fp32 arrays.  a * b is exact in fp64; the fp64 sum is corrected to
    round-to-odd with the exact error of TwoSum, after which the rounding to fp32 is the rounding of the exact value."""
    p = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (np.atleast_1d(s).view(np.int64) & 1) == 0
    fix = (np.atleast_1d(e) != 0) & even & np.isfinite(np.atleast_1d(s))
    s1 = np.atleast_1d(s).copy()
    s1[fix] = np.nextafter(s1[fix], np.where(np.atleast_1d(e)[fix] > 0, np.inf, -np.inf))
    return s1.astype(F32).reshape(np.shape(s))


def _mul(a, b):
    return (a.astype(F32) * b.astype(F32)).astype(F32)


def dense_dist(q, V, l2, mode="rule"):
    """distance(q, V[i]) for every row of V [n, len] -> fp32 [n].  mode: "rule" (the avx512f clone), or a WRONG variant:
    "unfused_main" (the 16-lane loop with a rounded product), "sequential" (one chain over the elements in order)."""
    q = np.asarray(q, dtype=F32)
    V = np.asarray(V, dtype=F32)
    V = V.reshape(-1, q.shape[0]) if q.shape[0] else V.reshape(V.shape[0], 0)
    n, ln = V.shape
    if l2:
        A = (q[None, :] - V).astype(F32)
        B = A
    else:
        A = np.broadcast_to(q[None, :], V.shape)
        B = V
    if mode == "sequential":
        s = np.zeros(n, dtype=F32)
        for k in range(ln):
            s = (s + _mul(A[:, k], B[:, k])).astype(F32)
    else:
        acc = np.zeros((n, 16), dtype=F32)
        for i in range(ln // 16):
            a, b = A[:, 16 * i:16 * i + 16], B[:, 16 * i:16 * i + 16]
            acc = (acc + _mul(a, b)).astype(F32) if mode == "unfused_main" else fma32(a, b, acc)
        qq = ((acc[:, 0:4] + acc[:, 4:8]).astype(F32) + (acc[:, 8:12] + acc[:, 12:16]).astype(F32)).astype(F32)
        k = 16 * (ln // 16)
        while k + 4 <= ln:
            qq = (qq + _mul(A[:, k:k + 4], B[:, k:k + 4])).astype(F32)
            k += 4
        s = (((qq[:, 0] + qq[:, 1]).astype(F32) + qq[:, 2]).astype(F32) + qq[:, 3]).astype(F32)
        while k < ln:
            s = fma32(A[:, k], B[:, k], s)
            k += 1
    return s if l2 else (1.0 - s.astype(np.float64)).astype(F32)


def sparse_dist(qi, qv, ii, iv, l2):
    """One sparse distance: ids ascending on both sides."""
    _, pa, pb = np.intersect1d(qi, ii, assume_unique=True, return_indices=True)
    dot = F32(0.0)
    for x, y in zip(qv[pa].astype(F32), iv[pb].astype(F32)):
        dot = F32(dot + F32(x * y))
    if l2:
        return F32(np.float64(F32(0.0) + F32(0.0)) - 2.0 * np.float64(dot))
    return F32(1.0 - np.float64(dot))


# ------------------------------------------------------------------------------------------------ libstdc++'s heaps
def _comp(kind, a, b, ties):
    """kind "max": std::less, "min": std::greater, on the distance only; ties="id" is the WRONG variant that also reads the node id."""
    if ties == "id" and a[0] == b[0]:
        return a[1] < b[1] if kind == "max" else a[1] > b[1]
    return a[0] < b[0] if kind == "max" else a[0] > b[0]


def _push_heap_at(h, hole, top, value, kind, ties):
    parent = (hole - 1) // 2 if hole > 0 else 0
    while hole > top and _comp(kind, h[parent], value, ties):
        h[hole] = h[parent]
        hole = parent
        parent = (hole - 1) // 2 if hole > 0 else 0
    h[hole] = value


def push_heap(h, kind, ties="dist"):
    """std::push_heap over the whole list (the new value is its last entry)."""
    _push_heap_at(h, len(h) - 1, 0, h[-1], kind, ties)


def _adjust_heap(h, hole, ln, value, kind, ties):
    top, child = hole, hole
    while child < (ln - 1) // 2:
        child = 2 * (child + 1)
        if _comp(kind, h[child], h[child - 1], ties):
            child -= 1
        h[hole] = h[child]
        hole = child
    if ln % 2 == 0 and child == (ln - 2) // 2:
        child = 2 * (child + 1)
        h[hole] = h[child - 1]
        hole = child - 1
    _push_heap_at(h, hole, top, value, kind, ties)


def pop_heap(h, n, kind, ties="dist"):
    """std::pop_heap over h[0:n): the top goes to h[n - 1]."""
    if n > 1:
        value = h[n - 1]
        h[n - 1] = h[0]
        _adjust_heap(h, 0, n - 1, value, kind, ties)


def sort_heap(h, kind="max", ties="dist"):
    for n in range(len(h), 1, -1):
        pop_heap(h, n, kind, ties)


def heap_pop_order(dists, kind):
    """Push (dists[i], i) one by one, then pop all: the ids in the order they leave (what the reference's heap_t does)."""
    h = []
    for i, d in enumerate(dists):
        h.append((F32(d), i))
        push_heap(h, kind)
    out = []
    while h:
        pop_heap(h, len(h), kind)
        out.append(h.pop()[1])
    return out


# ------------------------------------------------------------------------------------------------ the index
class Index(object):
    """num_node, feat_dim, maxM, maxM0, efC, max_level, init_node, l1_levels; data_type "csr" / "drm", metric "ip" / "l2";
    l0: list of id arrays; l1: {(node, level): id array} (missing = empty); items: ndarray [N, dim] or csr_matrix."""

    def __init__(self, items, l0, l1=None, maxM=None, maxM0=None, max_level=0, init_node=0, metric="ip", efC=100, l1_levels=None):
        self.data_type = "csr" if smat.issparse(items) else "drm"
        if self.data_type == "csr":
            items = items.tocsr().astype(F32)
            items.sort_indices()
        else:
            items = np.ascontiguousarray(items, dtype=F32)
        self.items, self.metric = items, metric
        self.num_node, self.feat_dim = items.shape
        self.l0 = [np.asarray(x, dtype=np.uint32) for x in l0]
        self.l1 = {k: np.asarray(v, dtype=np.uint32) for k, v in (l1 or {}).items()}
        self.maxM0 = maxM0 if maxM0 is not None else max([len(x) for x in self.l0] + [2])
        self.maxM = maxM if maxM is not None else max([len(x) for x in self.l1.values()] + [self.maxM0 // 2, 1])
        self.max_level, self.init_node, self.efC = max_level, init_node, efC
        self.l1_levels = max_level if l1_levels is None else l1_levels

    @property
    def l2(self):
        return self.metric == "l2"

    def neighbours(self, node, level):
        return self.l0[node] if level == 0 else self.l1.get((node, level), np.zeros(0, dtype=np.uint32))

    def row(self, X, r):
        if smat.issparse(X):
            return X.indices[X.indptr[r]:X.indptr[r + 1]], X.data[X.indptr[r]:X.indptr[r + 1]]
        return X[r]

    def dist(self, q, nodes, dense_mode="rule"):
        nodes = np.asarray(nodes, dtype=np.int64)
        if self.data_type == "drm":
            return dense_dist(q, self.items[nodes], self.l2, dense_mode)
        return np.array([sparse_dist(q[0], q[1], *self.row(self.items, n), self.l2) for n in nodes], dtype=F32)


HOST_NAN, POSITIVE_NAN = np.uint32(0xFFC00000).view(F32), np.uint32(0x7FC00000).view(F32)
NAN_VARIANTS = ("upper_not_ge", "break_not_le", "admit_not_ge", "positive_nan")
# where the statement met a NaN (beside COUNTERS in a trace; the device does not count these): an upper level entered with a NaN curr_dist, an
# upper-level neighbour at a NaN distance, the break test with a NaN on either side, the admission test decided by `d < ub` (the heap full) with a
# NaN on either side, pops of the pop-down to topk over a heap that holds a NaN
NAN_COUNTERS = ("nan_entry", "nan_upper", "nan_break", "nan_admit", "nan_popdown")


def search_one(ix, q, efS, topk, trace=None, dense_mode="rule", ties="dist", upper="pass", nan="rule"):
    """predict_single for one query -> [(dist, id)] ascending.  trace: a dict of counters to add to.  dense_mode / ties / upper / nan select
    a WRONG variant (upper="step": move to a better neighbour at once and fetch ITS list, instead of finishing the pass; nan: one of
    NAN_VARIANTS -- a comparison written as the negation of its opposite, which differs exactly under a NaN, or every NaN distance given
    the positive default NaN 0x7FC00000 instead of the host's 0xFFC00000)."""
    t = trace if trace is not None else {}
    for k in COUNTERS + NAN_COUNTERS:
        t.setdefault(k, 0)

    def dist(nodes):
        ds = np.asarray(ix.dist(q, nodes, dense_mode), dtype=F32)
        return np.where(np.isnan(ds), POSITIVE_NAN, ds) if nan == "positive_nan" else ds

    lt_upper = (lambda d, c: not (d >= c)) if nan == "upper_not_ge" else (lambda d, c: d < c)
    gt_break = (lambda c, u: not (c <= u)) if nan == "break_not_le" else (lambda c, u: c > u)
    lt_admit = (lambda d, u: not (d >= u)) if nan == "admit_not_ge" else (lambda d, u: d < u)
    curr = ix.init_node
    curr_dist = dist([curr])[0]
    t["dist"] += 1
    for level in range(ix.max_level, 0, -1):
        t["nan_entry"] += int(np.isnan(curr_dist))
        changed, left = True, ix.num_node + 1          # (the rule's passes end by themselves: curr_dist falls strictly; a wrong variant's need not)
        while changed and left:
            changed, left = False, left - 1
            t["passes"] += 1
            nb = ix.neighbours(curr, level)
            ds = dist(nb) if len(nb) else []
            t["dist"] += len(nb)
            for j in range(len(nb)):
                t["nan_upper"] += int(np.isnan(ds[j]))
                if lt_upper(ds[j], curr_dist):
                    curr_dist, curr, changed = ds[j], int(nb[j]), True
                    if upper == "step":
                        break
    ef = max(efS, topk)
    visited = {curr}
    ub = dist([curr])[0]
    t["dist"] += 1
    top, cand = [(ub, curr)], [(ub, curr)]
    max_cand = 1
    while cand:
        c = cand[0]
        t["nan_break"] += int(np.isnan(c[0]) or np.isnan(ub))
        if gt_break(c[0], ub):
            break
        pop_heap(cand, len(cand), "min", ties)
        cand.pop()
        t["pops"] += 1
        fresh = []
        for nb in ix.neighbours(c[1], 0):
            if int(nb) not in visited:
                visited.add(int(nb))
                fresh.append(int(nb))
        ds = dist(fresh) if fresh else []
        t["dist"] += len(fresh)
        for d, nb in zip(ds, fresh):
            t["nan_admit"] += int(len(top) >= ef and (np.isnan(d) or np.isnan(ub)))
            if len(top) < ef or lt_admit(d, ub):
                cand.append((d, nb))
                push_heap(cand, "min", ties)
                max_cand = max(max_cand, len(cand))
                top.append((d, nb))
                push_heap(top, "max", ties)
                if len(top) > ef:
                    pop_heap(top, len(top), "max", ties)
                    top.pop()
                ub = top[0][0]
                t["admissions"] += 1
    if topk < efS:
        while len(top) > topk:
            t["nan_popdown"] += int(any(np.isnan(d) for d, _ in top))
            pop_heap(top, len(top), "max", ties)
            top.pop()
    sort_heap(top, "max", ties)
    t["max_cand"] = max(t["max_cand"], max_cand)
    return top


def statement(ix, X, efS, topk, fill_idx=0, fill_val=0.0, **variant):
    """-> (idx [rows, topk] u32, dist [rows, topk] f32, count [rows], trace).  Entries past a row's count keep the fill."""
    rows = X.shape[0]
    idx = np.full((rows, topk), fill_idx, dtype=np.uint32)
    dist = np.full((rows, topk), fill_val, dtype=F32)
    count = np.zeros(rows, dtype=np.uint32)
    trace = {k: 0 for k in COUNTERS + NAN_COUNTERS}
    if smat.issparse(X):
        X = X.tocsr().astype(F32)
        X.sort_indices()
    for r in range(rows):
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):     # overflowing and NaN distances are part of the rule
            got = search_one(ix, ix.row(X, r), efS, topk, trace, **variant)
        count[r] = len(got)
        for k, (d, i) in enumerate(got):
            idx[r, k], dist[r, k] = i, d
    return idx, dist, count, trace


# ------------------------------------------------------------------------------------------------ the folder: writer and reader
class _Store(object):
    """The reference's mmap container: blocks at 16-byte-aligned offsets, the metadata, the 16-byte signature."""

    def __init__(self):
        self.body, self.blocks = bytearray(), []

    def put(self, data):
        data = bytes(data)
        end = self.blocks[-1][0] + self.blocks[-1][1] if self.blocks else 0
        pad = (16 - end % 16) % 16
        self.body += b"\0" * pad
        self.blocks.append((end + pad, len(data)))
        self.body += data

    def u32(self, v):
        self.put(struct.pack("<I", v))

    def vec(self, arr):
        arr = np.ascontiguousarray(arr)
        self.put(struct.pack("<Q", arr.size))
        self.put(arr.tobytes())

    def tobytes(self):
        meta = len(self.body)
        out = bytes(self.body) + struct.pack("<Q", len(self.blocks)) + b"".join(struct.pack("<QQ", o, s) for o, s in self.blocks)
        return out + b"\x93PECOS" + b"<" + b"\x01" + struct.pack("<Q", meta)


def node_records(ix):
    """(mem_start_of_node u64 [N + 1], buffer bytes, node_mem_size) of graph_l0: degree, maxM0 ids, len, values (, ids)."""
    parts, start = [], [0]
    for i in range(ix.num_node):
        nb = ix.l0[i]
        rec = np.zeros(1 + ix.maxM0, dtype=np.uint32)
        rec[0] = len(nb)
        rec[1:1 + len(nb)] = nb
        if ix.data_type == "drm":
            body = struct.pack("<I", ix.feat_dim) + ix.items[i].astype(F32).tobytes()
        else:
            ids, vals = ix.row(ix.items, i)
            body = struct.pack("<I", len(ids)) + vals.astype(F32).tobytes() + ids.astype(np.uint32).tobytes()
        parts.append(rec.tobytes() + body)
        start.append(start[-1] + len(parts[-1]))
    size = (start[-1] // ix.num_node) if ix.data_type == "drm" and ix.num_node else 0
    return np.array(start, dtype=np.uint64), b"".join(parts), size


def write_folder(ix, folder, pred_kwargs=None, hnsw_t=None, version="v2.0", patch=None):
    """param.json + c_model/{config.json, index.mmap_store} as HNSW.save writes them.  patch(dict of raw parts) may damage the parts
    (the refusal tests); hnsw_t / version override config.json."""
    cdir = os.path.join(folder, "c_model")
    os.makedirs(cdir, exist_ok=True)
    start, buf, node_mem = node_records(ix)
    L = ix.l1_levels
    l1 = np.zeros((ix.num_node, L, 1 + ix.maxM), dtype=np.uint32)
    for (node, level), nb in ix.l1.items():
        l1[node, level - 1, 0] = len(nb)
        l1[node, level - 1, 1:1 + len(nb)] = nb
    parts = dict(num_node=ix.num_node, maxM=ix.maxM, maxM0=ix.maxM0, efC=ix.efC, max_level=ix.max_level, init_node=ix.init_node, start=start,
                 buf=bytearray(buf), node_mem=node_mem, l1=l1, feat_dim=ix.feat_dim)
    if patch:
        patch(parts)
    s = _Store()
    for k in ("num_node", "maxM", "maxM0", "efC", "max_level", "init_node"):
        s.u32(parts[k])
    for v in (parts["num_node"], parts["feat_dim"], parts["maxM0"], parts["node_mem"]):
        s.u32(v)
    s.vec(parts["start"])
    s.vec(np.frombuffer(bytes(parts["buf"]), dtype=np.uint8))
    for v in (parts["num_node"], L, parts["maxM"], L * (1 + parts["maxM"]), 1 + parts["maxM"]):
        s.u32(v)
    s.vec(parts["l1"].reshape(-1))
    open(os.path.join(cdir, "index.mmap_store"), "wb").write(s.tobytes())
    config = {"hnsw_t": hnsw_t or TYPES[(ix.data_type, ix.metric)], "train_params": {k: int(parts[k]) for k in ("efC", "init_node", "maxM", "maxM0", "max_level", "num_node")}}
    if version is not None:
        config["version"] = version
    json.dump(config, open(os.path.join(cdir, "config.json"), "w"), indent=4)
    param = {"__meta__": {"class_fullname": "pecos.ann.hnsw.model###HNSW"}, "model": "HNSW", "data_type": ix.data_type, "metric_type": ix.metric,
             "num_item": ix.num_node, "feat_dim": ix.feat_dim,
             "pred_kwargs": dict({"__meta__": {"class_fullname": "pecos.ann.hnsw.model###HNSW.PredParams"}, "efS": 100, "topk": 10, "threads": 1}, **(pred_kwargs or {}))}
    json.dump(param, open(os.path.join(folder, "param.json"), "w"), indent=1)
    return folder


def read_folder(folder):
    """The folder back as an Index (the reader of the tests; the library has its own in C++)."""
    param = json.load(open(os.path.join(folder, "param.json")))
    raw = open(os.path.join(folder, "c_model", "index.mmap_store"), "rb").read()
    assert raw[-16:-10] == b"\x93PECOS" and raw[-10:-9] == b"<" and raw[-9] == 1
    meta = struct.unpack("<Q", raw[-8:])[0]
    nb = struct.unpack("<Q", raw[meta:meta + 8])[0]
    blocks = [struct.unpack("<QQ", raw[meta + 8 + 16 * i:meta + 24 + 16 * i]) for i in range(nb)]
    it = iter(blocks)

    def u32():
        o, s = next(it)
        assert s == 4
        return struct.unpack("<I", raw[o:o + 4])[0]

    def vec(dtype):
        o, s = next(it)
        n = struct.unpack("<Q", raw[o:o + 8])[0]
        o, s = next(it)
        assert s == n * np.dtype(dtype).itemsize
        return np.frombuffer(raw[o:o + s], dtype=dtype)

    num_node, maxM, maxM0, efC, max_level, init_node = (u32() for _ in range(6))
    n0, feat_dim, deg0, node_mem = (u32() for _ in range(4))
    start, buf = vec(np.uint64), vec(np.uint8).tobytes()
    n1, L, deg1, node_mem1, level_mem1 = (u32() for _ in range(5))
    b1 = vec(np.uint32)
    dense = param["data_type"] == "drm"
    l0, rows = [], []
    for i in range(num_node):
        at = i * node_mem if dense else int(start[i])
        rec = np.frombuffer(buf, dtype=np.uint32, count=2 + maxM0, offset=at)
        l0.append(rec[1:1 + rec[0]].copy())
        ln, at = int(rec[1 + maxM0]), at + 4 * (2 + maxM0)
        vals = np.frombuffer(buf, dtype=F32, count=ln, offset=at)
        rows.append((vals, None) if dense else (vals, np.frombuffer(buf, dtype=np.uint32, count=ln, offset=at + 4 * ln)))
    if dense:
        items = np.array([r[0] for r in rows], dtype=F32).reshape(num_node, feat_dim)
    else:
        ptr = np.cumsum([0] + [len(r[0]) for r in rows])
        items = smat.csr_matrix((np.concatenate([r[0] for r in rows] + [np.zeros(0, F32)]), np.concatenate([r[1] for r in rows] + [np.zeros(0, np.uint32)]), ptr),
                                shape=(num_node, feat_dim))
    l1 = {}
    b1 = b1.reshape(num_node, L, 1 + maxM) if L else b1
    for i in range(num_node):
        for lv in range(1, L + 1):
            if b1[i, lv - 1, 0]:
                l1[(i, lv)] = b1[i, lv - 1, 1:1 + b1[i, lv - 1, 0]].copy()
    return Index(items, l0, l1, maxM=maxM, maxM0=maxM0, max_level=max_level, init_node=init_node, metric=param["metric_type"], efC=efC, l1_levels=L)


# ------------------------------------------------------------------------------------------------ the libraries
def _view(X):
    if smat.issparse(X):
        X = X.tocsr()
        keep = (X.indptr.astype(np.uint64), X.indices.astype(np.uint32), X.data.astype(F32))
        return CsrView(X.shape[0], X.shape[1], keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data), keep, "csr"
    keep = (np.ascontiguousarray(X, dtype=F32),)
    return DrmView(X.shape[0], X.shape[1], keep[0].ctypes.data), keep, "drm"


def _outputs(rows, topk, fill_idx, fill_val):
    return np.full((rows, topk), fill_idx, dtype=np.uint32), np.full((rows, topk), fill_val, dtype=F32)


class Reference(object):
    """A folder loaded by the compiled reference: c_ann_hnsw_{load,predict,destruct}_{csr,drm}_{ip,l2}_f32 on folder/c_model."""

    def __init__(self, folder):
        lib = load(REF)
        param = json.load(open(os.path.join(folder, "param.json")))
        sfx = "_%s_%s_f32" % (param["data_type"], param["metric_type"])
        ld, self.pr, self.de = getattr(lib, "c_ann_hnsw_load" + sfx), getattr(lib, "c_ann_hnsw_predict" + sfx), getattr(lib, "c_ann_hnsw_destruct" + sfx)
        ld.restype, ld.argtypes = ctypes.c_void_p, [ctypes.c_char_p, ctypes.c_bool]
        self.pr.restype, self.pr.argtypes = None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p]
        self.de.restype, self.de.argtypes = None, [ctypes.c_void_p]
        self.h = ld(os.path.join(folder, "c_model").encode(), False)

    def predict(self, X, efS, topk, threads=1, fill_idx=0, fill_val=0.0):
        view, keep, _ = _view(X)
        idx, dist = _outputs(X.shape[0], topk, fill_idx, fill_val)
        self.pr(self.h, ctypes.byref(view), idx.ctypes.data, dist.ctypes.data, efS, topk, threads, None)
        return idx, dist

    def close(self):
        if self.h:
            self.de(self.h)
            self.h = None


def run_reference(folder, X, efS, topk, threads=1, fill_idx=0, fill_val=0.0):
    """Load, predict, destruct through the compiled reference -> (idx, dist)."""
    r = Reference(folder)
    try:
        return r.predict(X, efS, topk, threads, fill_idx, fill_val)
    finally:
        r.close()


def train_reference(X, folder, metric="ip", M=8, efC=100, threads=1, max_level_upper_bound=-1):
    """HNSW.train + save through the compiled reference (deterministic with threads=1) -> folder."""
    lib = load(REF)
    view, keep, kind = _view(X)
    sfx = "_%s_%s_f32" % (kind, metric)
    tr, sv, de = getattr(lib, "c_ann_hnsw_train" + sfx), getattr(lib, "c_ann_hnsw_save" + sfx), getattr(lib, "c_ann_hnsw_destruct" + sfx)
    tr.restype, tr.argtypes = ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int]
    sv.restype, sv.argtypes = None, [ctypes.c_void_p, ctypes.c_char_p]
    de.restype, de.argtypes = None, [ctypes.c_void_p]
    h = tr(ctypes.byref(view), M, efC, threads, max_level_upper_bound)
    os.makedirs(folder, exist_ok=True)
    sv(h, os.path.join(folder, "c_model").encode())
    de(h)
    param = {"model": "HNSW", "data_type": kind, "metric_type": metric, "num_item": X.shape[0], "feat_dim": X.shape[1], "pred_kwargs": {"efS": 100, "topk": 10, "threads": 1}}
    json.dump(param, open(os.path.join(folder, "param.json"), "w"), indent=1)
    return folder


def ours():
    lib = load(OURS)
    lib.xrl_hnsw_load.restype, lib.xrl_hnsw_load.argtypes = ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.xrl_hnsw_check_folder.restype, lib.xrl_hnsw_check_folder.argtypes = ctypes.c_int, [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32]
    lib.xrl_hnsw_destruct.restype, lib.xrl_hnsw_destruct.argtypes = None, [ctypes.c_void_p]
    lib.xrl_hnsw_info.restype, lib.xrl_hnsw_info.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    lib.xrl_hnsw_searchers_create.restype, lib.xrl_hnsw_searchers_create.argtypes = ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_uint32]
    lib.xrl_hnsw_searchers_destruct.restype, lib.xrl_hnsw_searchers_destruct.argtypes = None, [ctypes.c_void_p]
    for n in ("xrl_hnsw_predict_csr_f32", "xrl_hnsw_predict_drm_f32"):
        fn = getattr(lib, n)
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p]
    lib.xrl_debug_hnsw_counters.restype, lib.xrl_debug_hnsw_counters.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int]
    lib.xrl_debug_hnsw_caps.restype, lib.xrl_debug_hnsw_caps.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]
    return lib


def check_folder(folder):
    """xrl_hnsw_check_folder (the loader's reading and refusals, no GPU) -> (info of 10 values, error or None)."""
    lib = ours()
    out = np.zeros(10, dtype=np.uint64)
    rc = lib.xrl_hnsw_check_folder(os.path.join(folder, "c_model").encode(), out.ctypes.data, 10)
    return out, (last_error(lib) if rc else None)


def caps():
    lib = ours()
    out = np.zeros(4, dtype=np.uint64)
    lib.xrl_debug_hnsw_caps(out.ctypes.data, 4)
    return dict(zip(("CAP", "cand_cap", "lds_degree", "max_slots"), (int(v) for v in out)))


def counters(reset=False):
    lib = ours()
    out = np.zeros(8, dtype=np.uint64)
    lib.xrl_debug_hnsw_counters(out.ctypes.data, 8, 1 if reset else 0)
    return dict(zip(COUNTERS, (int(v) for v in out)))


class Ours(object):
    """A folder loaded by this library on device 0 (GPU tests)."""

    def __init__(self, folder, device=0):
        self.lib = ours()
        h = ctypes.c_void_p()
        rc = self.lib.xrl_hnsw_load(os.path.join(folder, "c_model").encode(), device, ctypes.byref(h))
        self.error = last_error(self.lib) if rc else None
        self.h = h if not rc else None

    def info(self):
        out = np.zeros(10, dtype=np.uint64)
        self.lib.xrl_hnsw_info(self.h, out.ctypes.data, 10)
        return out

    def predict(self, X, efS, topk, searchers=None, fill_idx=0, fill_val=0.0, threads=1):
        """-> (idx, dist, error or None); the outputs start as the fill."""
        view, keep, kind = _view(X)
        idx, dist = _outputs(X.shape[0], topk, fill_idx, fill_val)
        fn = getattr(self.lib, "xrl_hnsw_predict_%s_f32" % kind)
        rc = fn(self.h, ctypes.byref(view), idx.ctypes.data, dist.ctypes.data, efS, topk, threads, searchers)
        return idx, dist, (last_error(self.lib) if rc else None)

    def searchers(self, n):
        return self.lib.xrl_hnsw_searchers_create(self.h, n)

    def free_searchers(self, s):
        self.lib.xrl_hnsw_searchers_destruct(s)

    def close(self):
        if self.h:
            self.lib.xrl_hnsw_destruct(self.h)
            self.h = None


# ------------------------------------------------------------------------------------------------ cases
def dense_items(n, dim, seed, scale=1.0):
    return (np.random.RandomState(seed).randn(n, dim) * scale).astype(F32)


def sparse_items(n, dim, per_row, seed, lengths=None):
    """Rows of `per_row` (or lengths[i]) distinct ascending ids, N(0, 1) values that are never 0."""
    rs = np.random.RandomState(seed)
    ind, ptr, val = [], [0], []
    for r in range(n):
        k = min(dim, lengths[r] if lengths is not None else per_row)
        ids = np.sort(rs.choice(dim, size=k, replace=False))
        v = rs.randn(k).astype(F32)
        v[v == 0] = 1.0
        ind.extend(ids)
        val.extend(v)
        ptr.append(len(ind))
    return smat.csr_matrix((np.array(val, dtype=F32), np.array(ind, dtype=np.int32), np.array(ptr, dtype=np.int64)), shape=(n, dim))


def random_graph(n, deg, seed, maxM0=None, levels=0, maxM=None):
    """A connected level-0 graph (a ring plus random distinct neighbours, `deg` per node) and `levels` sparse upper levels over every 2nd,
    4th, ... node; -> (l0, l1, max_level, init_node)."""
    rs = np.random.RandomState(seed)
    l0 = []
    for i in range(n):
        others = [j for j in rs.permutation(n) if j != i and j != (i + 1) % n][:max(0, min(deg, n - 1) - 1)]
        nb = ([(i + 1) % n] if n > 1 and deg > 0 else []) + others
        l0.append(np.array(nb[:deg], dtype=np.uint32))
    l1, init = {}, 0
    for lv in range(1, levels + 1):
        members = list(range(0, n, 2 ** lv))
        for a in members:
            nb = [b for b in rs.permutation(members) if b != a][:(maxM or max(1, deg // 2))]
            l1[(a, lv)] = np.array(nb, dtype=np.uint32)
    return l0, l1, levels, init


def full_graph(n):
    """Every node lists every other node: topk = num_node returns every item, so the answer reads the distance statement."""
    return [np.array([j for j in range(n) if j != i], dtype=np.uint32) for i in range(n)]


def star_index(values):
    """Node 0 is the entry point and lists every other node in order; item i is {0: values[i]}, so a query {0: 1} is at distance 1 - values[i]."""
    n = len(values)
    items = smat.csr_matrix((np.asarray(values, dtype=np.float32), (np.arange(n), np.zeros(n, int))), shape=(n, 1))
    l0 = [np.arange(1, n)] + [[] for _ in range(n - 1)]
    return Index(items, l0, maxM0=max(n - 1, 2), metric="ip"), smat.csr_matrix(np.ones((1, 1), dtype=np.float32))


def heap_lists():
    rs = np.random.RandomState(9)
    for n in range(1, 71):
        yield "equal", n, np.full(n, 0.5, dtype=np.float32)
        yield "two", n, rs.choice(np.array([0.25, 0.5], dtype=np.float32), size=n)


# ------------------------------------------------------------------------------------------------ cases: distances that leave fp32's range
# Finite inputs only: the loader and the check kernels refuse the rest.  BIG * 2 and BIG + BIG overflow, BIG - BIG is 0, and inf + -inf is the
# host's default NaN 0xFFC00000.  Vectors are written as {position: value}; every other position is +0 (dense) or not stored (sparse).
BIG = F32(3e38)
FLT_MAX = np.finfo(F32).max


def _dense(rows, dim):
    A = np.zeros((len(rows), dim), dtype=F32)
    for r, row in enumerate(rows):
        for k, v in row.items():
            A[r, k] = v
    return A


def _csr(rows, dim):
    """Every listed entry is STORED, a zero or a -0.0 too."""
    ptr = np.cumsum([0] + [len(row) for row in rows])
    ids = np.array([k for row in rows for k in sorted(row)], dtype=np.int32)
    vals = np.array([row[k] for row in rows for k in sorted(row)], dtype=F32)
    return smat.csr_matrix((vals, ids, ptr), shape=(len(rows), dim))


def _rows(rows, dim, kind):
    return _dense(rows, dim) if kind == "drm" else _csr([{k: v for k, v in row.items() if v != 0} for row in rows], dim)


def seed_rows():
    """The nine items and three queries of 20 dimensions every type is run on: under a query of twos item 0 is inf + -inf, items 1 and 2 the
    two infinities, items 7 and 8 the same in the dense rule's unfused group of 4."""
    B = BIG
    items = [{0: B, 1: -B, 4: 1.0}, {0: B, 1: B}, {0: -B, 1: -B}, {k: (1.0, 2.0)[k] if k < 2 else 0.5 for k in range(20)}, {0: -1.0, 1: 0.25},
             {0: -B, 1: 1.0, 2: B}, {0: 1e-30, 1: 1e-30}, {16: B, 17: -B}, {16: B, 17: B, 18: B, 19: -B}]
    queries = [{k: 2.0 for k in (0, 1, 2, 16, 17, 18, 19)}, {0: 1e-30, 1: -1e-30}, {k: 1.0 if k else B for k in range(20)}]
    return items, queries


STAGE_POSITIONS = {3: (0, 1, 2),                     # the fused tail alone
                   4: (0, 1, 3),                     # one unfused group
                   16: (0, 1, 4, 8, 12),             # one fused block: lanes that meet in the fold's first, second and last addition
                   23: (0, 4, 16, 17, 20, 22),       # 16 + 4 + 3: a fused lane, its fold partner, two lanes of the unfused group, two tail elements
                   39: (0, 16, 32, 36)}              # 32 + 4 + 3: positions 0 and 16 share accumulator lane 0


def stage_rows(ln):
    """Dense vectors of length ln with BIG and -BIG (and BIG and BIG) at every pair of STAGE_POSITIONS, in both orders: the overflow and the
    inf + -inf land in one accumulator lane, across lanes in the fold, in an unfused group, in the tail.  Then sums that reach FLT_MAX
    exactly, pass it by a quarter and by half an ulp (the tie rounds to even: the overflow), zeros, -0.0 and values whose squares are
    subnormal.  At 39 also 36 powers of two whose squares are the 24 bits of FLT_MAX, every partial sum exact in any order, then with
    2^51 and 2^52 in the fused tail (a quarter ulp more, and the overflow).  Queries: twos, ones, +-BIG at the positions, 1e-20 at both
    ends (dense l2 distances of 1e-40 .. 4e-40), zeros."""
    P = STAGE_POSITIONS[ln]
    a, b = 0, ln - 1
    items = []
    for i in P:
        for j in P:
            if i != j:
                items.append({i: BIG, j: -BIG})
            if i < j:
                items.append({i: BIG, j: BIG})
    items += [{a: 2.0 ** 127, b: 2.0 ** 127 - 2.0 ** 104}, {a: FLT_MAX, b: 2.0 ** 102}, {a: FLT_MAX, b: 2.0 ** 103},
              {}, {a: -0.0, b: 1e-20}, {a: 1e-20, b: -1e-20}, {a: 1.0, b: -0.0}]
    if ln == 39:
        bits = [2.0 ** (e // 2) for e in range(127, 103, -1) for _ in range(1 + e % 2)]         # an odd exponent is two equal squares
        assert len(bits) == 36 and sum(x * x for x in bits) == float(FLT_MAX)
        items += [dict(enumerate(bits)), dict(enumerate(bits + [2.0 ** 51])), dict(enumerate(bits + [0.0, 2.0 ** 52]))]
    queries = [{k: 2.0 for k in range(ln)}, {k: 1.0 for k in range(ln)}, {p: (BIG if n % 2 == 0 else -BIG) for n, p in enumerate(P)},
               {a: 1e-20, b: 1e-20}, {}]
    return items, queries


def sparse_dot_rows():
    """Sparse rows of 40 columns: the chain 0 + inf + -inf, both infinities from products and from the addition, FLT_MAX reached exactly (l2:
    -2 * FLT_MAX overflows in the final rounding from fp64), the tie at FLT_MAX + half an ulp, products and sums that are subnormal
    (l2 shows -2e-40; ip hides them behind 1 -), stored zeros and stored -0.0 that match an id on either side, and an empty row."""
    B = BIG
    items = [{0: B, 1: -B}, {0: -B, 1: B, 2: 1.0}, {0: B, 1: B}, {0: -B, 1: -B}, {0: 2.0 ** 127, 5: 2.0 ** 127 - 2.0 ** 104}, {0: FLT_MAX, 5: 2.0 ** 103},
             {0: FLT_MAX, 5: 2.0 ** 102}, {3: 1e-20}, {3: 1e-20, 7: 1e-20}, {3: 1e-25}, {3: -1e-20, 7: 1e-20}, {0: 0.0, 1: 2.0, 2: -0.0}, {0: -0.0}, {2: 0.0, 3: 0.0},
             {1: 0.5, 39: B}, {}, {0: 1.0, 1: 1.0, 2: 1.0, 3: 1.0, 5: 1.0, 7: 1.0, 39: 1.0}]
    queries = [{0: 2.0, 1: 2.0, 2: 2.0}, {0: 1.0, 1: 1.0, 5: 1.0}, {3: 1e-20, 7: 1e-20}, {0: 0.0, 1: 1.0, 2: B, 3: -0.0}, {0: 2.0, 1: -2.0, 39: 2.0}, {},
               {0: -0.0, 2: -0.0}, {3: -1e-20, 7: -1e-25}]
    return items, queries


# A distance by name, as items of 4 dimensions (one unfused group of the dense rule, a chain of the sparse one).  Under the query (2, 2, 0, 1):
# ip: "nan" NaN, "lo" -inf, "hi" +inf, a number x the distance 1 - x;  sparse l2 is -2 * dot, so "lo" and "hi" change places;  dense l2 has no
# NaN (its terms are squares): every named kind is +inf there.  The other queries turn the kinds into each other.
KIND_ROWS = {"nan": {0: BIG, 1: -BIG}, "nan2": {0: -BIG, 1: BIG}, "lo": {0: BIG, 1: BIG}, "hi": {0: -BIG, 1: -BIG}}
KIND_QUERIES = [{0: 2.0, 1: 2.0, 3: 1.0}, {0: 2.0, 1: -2.0, 3: 1.0}, {0: 1.0, 1: 1.0, 3: 1.0}, {3: 1.0}]


def kind_rows(kinds):
    return [dict(KIND_ROWS[k]) if k in KIND_ROWS else {3: float(k)} for k in kinds]


def range_edge_cases():
    """{name: (Index, queries, [(efS, topk), ...])}: at most 64 nodes, 8 queries and 40 dimensions each; all four types."""
    cases = {}
    types = [(k, m) for k in ("csr", "drm") for m in ("ip", "l2")]
    items, queries = seed_rows()
    for kind, metric in types:
        for init in (0, 3):
            ix = Index(_rows(items, 20, kind), full_graph(9), init_node=init, metric=metric)
            cases["seed_%s_%s_init%d" % (kind, metric, init)] = (ix, _rows(queries, 20, kind), [(9, 9)])
    for ln in sorted(STAGE_POSITIONS):
        items, queries = stage_rows(ln)
        for metric in ("ip", "l2"):
            ix = Index(_dense(items, ln), full_graph(len(items)), metric=metric)
            cases["stages_%s_len%d" % (metric, ln)] = (ix, _dense(queries, ln), [(len(items), len(items))])
    items, queries = sparse_dot_rows()
    for metric in ("ip", "l2"):
        ix = Index(_csr(items, 40), full_graph(len(items)), metric=metric)
        cases["sparse_dot_%s" % metric] = (ix, _csr(queries, 40), [(len(items), len(items))])
    # NaN in the traversal: two upper levels, the entry point a NaN (init 0) or finite among NaN neighbours (init 4); efS below, at and above the
    # node count, topk below efS (the pop-down runs over a heap that holds NaNs) and above it
    rs = np.random.RandomState(17)
    kinds = [str(k) for k in rs.choice(["nan", "nan2", "nan", "lo", "hi", "0.25", "0.5", "-1.0", "3.0"], size=24)]
    kinds[0], kinds[4], kinds[8], kinds[2] = "nan", "0.75", "nan2", "-2.0"
    l0, l1, levels, _ = random_graph(24, 4, 18, levels=2, maxM=3)
    for kind, metric in (("csr", "ip"), ("drm", "ip"), ("csr", "l2")):
        for init in (0, 4):
            ix = Index(_rows(kind_rows(kinds), 4, kind), l0, l1, maxM=3, max_level=levels, init_node=init, metric=metric)
            cases["nan_walk_%s_%s_init%d" % (kind, metric, init)] = (ix, _rows(KIND_QUERIES, 4, kind), [(4, 4), (24, 24), (12, 5), (3, 8), (30, 24), (1, 1)])
    # ties: twelve nodes at each infinity, efS below the size of a tie
    kinds = [str(k) for k in np.random.RandomState(19).permutation(["lo"] * 12 + ["hi"] * 12 + ["0.5", "0.5", "-1.0", "2.0", "0.0", "7.0"])]
    l0, l1, levels, init = random_graph(30, 5, 20, levels=1)
    for kind, metric in types:
        ix = Index(_rows(kind_rows(kinds), 4, kind), l0, l1, max_level=levels, init_node=init, metric=metric)
        cases["inf_ties_%s_%s" % (kind, metric)] = (ix, _rows(KIND_QUERIES, 4, kind), [(5, 5), (5, 3), (30, 30), (8, 20)])
    return cases


def range_edge_blocks(cases):
    """The layout of the recording tests/golden/hnsw/range_edges.npz: one block of rows * topk entries per (case by name, setting in order)."""
    at = 0
    for name in sorted(cases):
        ix, Q, settings = cases[name]
        for efS, topk in settings:
            yield name, efS, topk, slice(at, at + Q.shape[0] * topk)
            at += Q.shape[0] * topk


def range_edge_recording(path, cases):
    """{(name, efS, topk): (idx u32 [rows, topk], distance bits u32 [rows, topk])} as the compiled reference returned them on an avx512f host."""
    rec = np.load(path)
    blocks = list(range_edge_blocks(cases))
    assert rec["layout"].tolist() == ["%s:%d:%d:%d" % (n, e, t, s.stop) for n, e, t, s in blocks], "the cases changed: record range_edges.npz again"
    return {(n, e, t): (rec["idx"][s].astype(np.uint32).reshape(-1, t), rec["bits"][s].reshape(-1, t)) for n, e, t, s in blocks}
