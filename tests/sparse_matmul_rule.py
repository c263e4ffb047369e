"""Sparse matrix products (K10): the rule of ``xrl_sparse_matmul_device`` restated in numpy, a ctypes caller of the two
``c_sparse_matmul_*`` entry points (of the compiled reference or of this library), and the cases both test halves run.

Matrices are RAW CSR here -- ``Csr(indptr u64, indices u32, data f32, shape)`` -- because the stored order, duplicates, explicit zeros
and column ids up to 2^32 - 2 are the point, and a scipy constructor may change or refuse any of them."""
import collections
import ctypes as C
import os

import numpy as np

Csr = collections.namedtuple("Csr", ["indptr", "indices", "data", "shape"])
FLT_MIN = np.float32(1.17549435e-38)
SENT_IDX = 0xA5A5A5A5
SENT_BITS = 0x7FC5A5A5          # a NaN no product of the cases carries


def csr(indptr, indices, data, shape):
    return Csr(np.ascontiguousarray(indptr, dtype=np.uint64), np.ascontiguousarray(indices, dtype=np.uint32),
               np.ascontiguousarray(data, dtype=np.float32), (int(shape[0]), int(shape[1])))


def from_rows(rows, cols):
    """rows: per row a list of (column, value) in the order to store."""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]) if rows else np.zeros(1)
    flat = [e for r in rows for e in r]
    return csr(indptr, [e[0] for e in flat], [e[1] for e in flat], (len(rows), cols))


def from_scipy(M):
    M = M.tocsr()
    return csr(M.indptr, M.indices, M.data, M.shape)


def transpose_view(M):
    """The same arrays read as the other format: CSR arrays of M are the CSC arrays of M^T."""
    return Csr(M.indptr, M.indices, M.data, (M.shape[1], M.shape[0]))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rule(A, B, eliminate_zeros=False, sorted_indices=True):
    """(indptr, indices, data) of A * B by the rule; indices / data are the WHOLE buffers the allocator is asked for (the count before
    elimination): with eliminate_zeros the entries past indptr[-1] hold what the un-compacted product held there."""
    assert A.shape[1] == B.shape[0]
    zero = np.float32(0.0)
    out_i, out_v, ptr = [], [], [0]
    with np.errstate(all="ignore"):
        for i in range(A.shape[0]):
            acc = {}                                                     # insertion order = first touch
            for s in range(int(A.indptr[i]), int(A.indptr[i + 1])):
                k, a = int(A.indices[s]), A.data[s]
                for t in range(int(B.indptr[k]), int(B.indptr[k + 1])):
                    j = int(B.indices[t])
                    acc[j] = np.float32(acc.get(j, zero) + np.float32(a * B.data[t]))
            cols = sorted(acc) if sorted_indices else list(acc)
            out_i += cols
            out_v += [acc[j] for j in cols]
            ptr.append(len(out_i))
    indptr = np.asarray(ptr, dtype=np.uint64)
    indices, data = np.asarray(out_i, dtype=np.uint32), np.asarray(out_v, dtype=np.float32)
    if eliminate_zeros:
        keep = data != 0                                                 # (NaN != 0)
        n = int(keep.sum())
        row_of = np.repeat(np.arange(A.shape[0]), np.diff(indptr).astype(np.int64))
        indptr = np.concatenate([[0], np.cumsum(np.bincount(row_of[keep], minlength=A.shape[0]))]).astype(np.uint64)
        indices, data = indices.copy(), data.copy()
        indices[:n], data[:n] = indices[keep].copy(), data[keep].copy()
    return indptr, indices, data


def same(got, want):
    """row pointer, indices and value BITS of two (indptr, indices, data) triples"""
    return (np.array_equal(np.asarray(got[0], dtype=np.uint64), np.asarray(want[0], dtype=np.uint64))
            and np.array_equal(np.asarray(got[1], dtype=np.uint32), np.asarray(want[1], dtype=np.uint32))
            and np.array_equal(bits(got[2]), bits(want[2])))


def logical(res):
    """the stored entries of a whole-buffer triple: up to indptr[-1]"""
    n = int(res[0][-1]) if len(res[0]) else 0
    return res[0], res[1][:n], res[2][:n]


# ---------------------------------------------------------------------------------------------------------------- native entry points
class _Mat(C.Structure):       # ScipyCsrF32 and ScipyCscF32 share the layout (matrix.hpp:49-62)
    _fields_ = [("rows", C.c_uint32), ("cols", C.c_uint32), ("ptr", C.POINTER(C.c_uint64)), ("idx", C.POINTER(C.c_uint32)), ("val", C.POINTER(C.c_float))]


_ALLOC = C.CFUNCTYPE(None, C.c_bool, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p)


class Allocator:
    """Allocates arrays PRE-FILLED with sentinels and records what it was asked for."""

    def __init__(self):
        self.calls = []
        self.indptr = self.indices = self.data = None

    def __call__(self, is_col_major, rows, cols, nnz, p_indices, p_indptr, p_data):
        self.calls.append((bool(is_col_major), int(rows), int(cols), int(nnz)))
        self.indptr = np.full((cols if is_col_major else rows) + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        self.indices = np.full(nnz, SENT_IDX, dtype=np.uint32)
        self.data = np.full(nnz, SENT_BITS, dtype=np.uint32).view(np.float32)
        for dst, arr in ((p_indices, self.indices), (p_indptr, self.indptr), (p_data, self.data)):
            C.cast(dst, C.POINTER(C.c_uint64)).contents.value = arr.ctypes.data


def _view(M, fmt):
    m = _Mat()
    m.rows, m.cols = M.shape
    ptr = M.indptr if len(M.indptr) else np.zeros(1, dtype=np.uint64)
    idx = M.indices if len(M.indices) else np.zeros(1, dtype=np.uint32)
    val = M.data if len(M.data) else np.zeros(1, dtype=np.float32)
    m.ptr, m.idx, m.val = ptr.ctypes.data_as(C.POINTER(C.c_uint64)), idx.ctypes.data_as(C.POINTER(C.c_uint32)), val.ctypes.data_as(C.POINTER(C.c_float))
    m._keep = (ptr, idx, val)
    return m


def native_matmul(lib, X, Y, fmt="csr", eliminate_zeros=False, sorted_indices=True, threads=1):
    """``c_sparse_matmul_<fmt>_f32`` of ``lib`` (a ctypes.CDLL: the compiled reference or this library).  X, Y: Csr whose arrays are the
    CSR arrays (fmt "csr") or the CSC arrays (fmt "csc": indptr = col_ptr, shape = the matrix's own (rows, cols)).  Returns
    ((indptr, indices, data) as the allocator's whole buffers, the allocator's calls)."""
    fn = getattr(lib, f"c_sparse_matmul_{fmt}_f32")
    fn.restype, fn.argtypes = None, [C.POINTER(_Mat), C.POINTER(_Mat), _ALLOC, C.c_bool, C.c_bool, C.c_int]
    alloc = Allocator()
    px, py = _view(X, fmt), _view(Y, fmt)
    fn(C.byref(px), C.byref(py), _ALLOC(alloc), bool(eliminate_zeros), bool(sorted_indices), int(threads))
    return (alloc.indptr, alloc.indices, alloc.data), alloc.calls


def ref_lib():
    from oracle.xrl_oracle import REF_SO
    return C.CDLL(REF_SO)


# ---------------------------------------------------------------------------------------------------------------------------- cases
def rand_csr(rng, rows, cols, per_row, dup=False, sort=False):
    out = []
    for _ in range(rows):
        n = int(rng.integers(0, per_row + 1))
        c = rng.integers(0, cols, n) if dup else rng.choice(cols, min(n, cols), replace=False)
        if sort:
            c = np.sort(c)
        out.append(list(zip(c.tolist(), rng.standard_normal(len(c)).astype(np.float32).tolist())))
    return from_rows(out, cols)


def shuffled_pair(seed=5):
    """50 x 40 by 40 x 300, the left rows in shuffled stored order: the case whose values depend on the order of the additions"""
    rng = np.random.default_rng(seed)
    return rand_csr(rng, 50, 40, 30), rand_csr(rng, 40, 300, 60, sort=True)


def sort_left_rows(A):
    idx, val = A.indices.copy(), A.data.copy()
    for i in range(A.shape[0]):
        b, e = int(A.indptr[i]), int(A.indptr[i + 1])
        o = np.argsort(idx[b:e], kind="stable")
        idx[b:e], val[b:e] = idx[b:e][o], val[b:e][o]
    return Csr(A.indptr, idx, val, A.shape)


def product_counts(cap=1024):
    return [0, 1, 63, 64, 65, 127, 128, 129, cap - 1, cap, cap + 1, 20000]


def counted_rows(counts, seed=11, cols=300):
    """One left row per count F: its entries name right rows of at most 70 stored entries (duplicate columns allowed, one of them empty) whose
    lengths sum to F, in shuffled order.  Returns (A, B, the counts)."""
    rng = np.random.default_rng(seed)
    b_rows, a_rows = [[]], []                                             # right row 0 is empty
    for F in counts:
        entries, left = [(0, 2.0)] if F else [], F
        while left:
            n = int(min(left, rng.integers(1, 71)))
            c = rng.integers(0, cols, n)
            b_rows.append(list(zip(c.tolist(), rng.standard_normal(n).astype(np.float32).tolist())))
            entries.append((len(b_rows) - 1, float(np.float32(rng.standard_normal()))))
            left -= n
        rng.shuffle(entries)
        a_rows.append([tuple(e) for e in entries])
    return from_rows(a_rows, len(b_rows)), from_rows(b_rows, cols), list(counts)


def one_column(F):
    """all F products in one column, valued so that any reordered or tree-shaped sum differs: 1e8, 1, -1e8, 3, ..."""
    cyc = [1e8, 1.0, -1e8, 3.0, 0.5, -1e8, 1e8, 7.0]
    return from_rows([[(0, cyc[s % len(cyc)] * (1 + s // len(cyc))) for s in range(F)]], 1), from_rows([[(7, 1.0)]], 9)


def all_distinct(F, seed=3):
    """one left entry, a right row of F distinct columns in shuffled stored order"""
    rng = np.random.default_rng(seed)
    c = rng.permutation(3 * F)[:F]
    return from_rows([[(0, 1.5)]], 1), from_rows([list(zip(c.tolist(), rng.standard_normal(F).astype(np.float32).tolist()))], 3 * F)


def run_boundaries(seed=9):
    """runs of the column-ordered products that start and end one before, at and one after every 64-product step, the products themselves
    in shuffled order: right row c is the single entry (c, v_c), the left row names column c once per product"""
    rng = np.random.default_rng(seed)
    mult = [63, 1, 1, 63, 2, 62, 64, 65, 1, 62, 3, 61, 128, 1, 63]
    prods = [c for c, m in enumerate(mult) for _ in range(m)]
    rng.shuffle(prods)
    A = from_rows([[(int(c), float(np.float32(rng.standard_normal() * 10.0 ** int(rng.integers(-3, 4))))) for c in prods]], len(mult))
    B = from_rows([[(5 * c + 1, float(np.float32(rng.standard_normal())))] for c in range(len(mult))], 5 * len(mult) + 2)
    return A, B


def duplicates(seed=13):
    rng = np.random.default_rng(seed)
    return rand_csr(rng, 12, 20, 25, dup=True), rand_csr(rng, 20, 16, 20, dup=True)


def numeric_edges():
    """One left row over right rows of one or two entries; per output column a named edge.  Stored (unsorted) order on both sides."""
    inf, nan, tiny = np.float32(np.inf), np.float32(np.nan), np.float32(1e-20)
    sub = np.float32(3e-42)
    b_rows = [
        [(40, 1.0)],                     # 0: explicit zero product (a = 0)
        [(41, 0.0), (30, 1.0)],          # 1: zero by b; and 1 ...
        [(30, -1.0)],                    # 2: ... - 1: a cancelling sum
        [(31, 0.0)],                     # 3: a = -1: the product is -0, and 0 + (-0) = +0
        [(32, 2.0)],                     # 4: a = NaN
        [(33, 1.0), (34, 1.0)],          # 5: a = inf: +inf, and inf ...
        [(34, 1.0)],                     # 6: a = -inf: ... - inf = NaN
        [(35, tiny)],                    # 7: a = 1e-20: a subnormal product
        [(36, 1.0), (36, 1.0)],          # 8: a = 3e-42: a subnormal sum (duplicate column in one right row)
        [(37, 0.75)],                    # 9: a = FLT_MIN: below FLT_MIN ...
        [(37, 0.75)],                    # 10: a = FLT_MIN: ... the sum crosses it
        [(38, 0.0)],                     # 11: a = inf: 0 * inf = NaN
        [(39, -0.0), (39, 0.0)],         # 12: a = 1: -0 + 0
        [(2, 1.0)],                      # 13: a = 1 then a = -1 from the same right row: zero at a low column
    ]
    a_row = [(0, 0.0), (1, 1.0), (2, 1.0), (3, -1.0), (4, nan), (5, inf), (6, -inf), (7, tiny), (8, sub), (9, FLT_MIN), (10, FLT_MIN), (11, inf),
             (12, 1.0), (13, 1.0), (13, -1.0)]
    return from_rows([a_row, [], a_row[::-1]], len(b_rows)), from_rows(b_rows, 48)


def shapes():
    """name -> (A, B): the widest column ids, empty rows, empty operands, no rows, one row"""
    wide = 2 ** 32 - 1
    B_wide = from_rows([[(wide - 1, 2.0), (0, 3.0)], [], [(0, 1.0), (wide - 1, -1.0)]], wide)
    A3 = from_rows([[(2, 1.0), (0, 0.5)], [], [(1, 4.0)], [(0, 1.0)]], 3)
    return {
        "widest_columns": (A3, B_wide),
        "empty_left": (from_rows([[], [], []], 3), B_wide),
        "empty_right": (A3, from_rows([[], [], []], 7)),
        "no_rows": (csr([0], [], [], (0, 3)), B_wide),
        "one_row": (from_rows([[(1, 2.0), (1, 3.0)]], 2), from_rows([[(1, 1.0)], [(4, 1.0), (0, 2.0)]], 6)),
        "no_inner": (csr([0, 0, 0], [], [], (2, 0)), csr([0], [], [], (0, 5))),
    }


def cpu_cases(cap=1024):
    """name -> (A, B): everything both halves compare; small enough for the numpy restatement"""
    out = {"shuffled": shuffled_pair(), "duplicates": duplicates(), "numeric_edges": numeric_edges(), "run_boundaries": run_boundaries(),
           "one_column_65": one_column(65), "one_column_cap": one_column(cap), "one_column_cap1": one_column(cap + 1),
           "all_distinct_64": all_distinct(64), "all_distinct_cap": all_distinct(cap), "all_distinct_cap1": all_distinct(cap + 1)}
    A, B, _ = counted_rows(product_counts(cap))
    out["counted_rows"] = (A, B)
    for k, v in shapes().items():
        out["shape_" + k] = v
    return out


def reference_can_run(A, B):
    """The reference keeps a dense accumulator as long as the product is wide per thread: 2^32 - 1 columns are 48 GiB each."""
    return B.shape[1] <= 1 << 24


SETTINGS = [(False, True), (True, True), (False, False), (True, False)]      # (eliminate_zeros, sorted_indices)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_matmul")
WRAPPER_COMBOS = [("csr", "csr"), ("csc", "csc"), ("csc", "csr"), ("csr", "csc")]      # (format of X, format of Y) the python wrapper takes
