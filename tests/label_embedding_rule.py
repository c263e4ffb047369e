"""Label embeddings (K12): the rules R1 - R5 of ``xrl_label_embedding_device`` restated in numpy, a deliberately wrong variant of each
that the cases are built to catch, and the cases both test halves run.

Matrices are the raw ``Csr(indptr u64, indices u32, data f32, shape)`` of tests/sparse_matmul_rule.py: stored order, duplicates and
explicit zeros are the point.  R3's product is that file's ``rule``."""
import numpy as np
import scipy.sparse as smat

import sparse_matmul_rule as smr
from sparse_matmul_rule import Csr, bits, csr, from_rows, from_scipy, same  # noqa: F401

CAP = 1024
T27 = np.float32(2.0 ** -27)
ORDER_V_BITS = (0x3F961097, 0x3FBD4672, 0x3FC41EF5, 0x3FDBB3CA)
ORDER_SKLEARN_BITS = (0x3F42C56F, 0x3F540F96, 0x3F56617A)          # what sklearn stores for v's entry of the first three rows
METHODS = ("pifa", "pifa_lf_concat", "pii")


def triple(M):
    return M.indptr, M.indices, M.data


def to_scipy(M):
    """scipy CSR over the same arrays, order and explicit zeros kept (small column counts only)"""
    S = smat.csr_matrix(M.shape, dtype=np.float32)
    S.indptr, S.indices, S.data = M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.copy()
    return S


# ------------------------------------------------------------------------------------------------------------------------ the rules
def normalize(M, variant=None):
    """R1.  variant "reversed": the row is walked last entry first; "double_square": the square is taken in double."""
    data = M.data.astype(np.float32)
    out = data.copy()
    with np.errstate(all="ignore"):
        sq = (data.astype(np.float64) * data.astype(np.float64)) if variant == "double_square" else (data * data).astype(np.float64)
        for r in range(M.shape[0]):
            b, e = int(M.indptr[r]), int(M.indptr[r + 1])
            if e == b:
                continue
            q = sq[b:e][::-1] if variant == "reversed" else sq[b:e]
            s = np.cumsum(np.concatenate([[0.0], q]))[-1]               # one chain from +0.0, in the order of q
            if s == 0.0:
                continue
            out[b:e] = (data[b:e].astype(np.float64) / np.sqrt(s)).astype(np.float32)
    return Csr(M.indptr, M.indices, out, M.shape)


def transpose(M, variant=None):
    """R2.  variant "row_reversed": every output row in the opposite of the stable order."""
    rows, cols = M.shape
    idx = M.indices.astype(np.int64)
    order = np.argsort(idx, kind="stable")
    cnt = np.bincount(idx, minlength=cols) if len(idx) else np.zeros(cols, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    if variant == "row_reversed":
        order = np.concatenate([order[int(indptr[j]):int(indptr[j + 1])][::-1] for j in range(cols)]) if cols and len(order) else order
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(M.indptr.astype(np.int64)))
    return csr(indptr, row_of[order], M.data[order], (cols, rows))


def transpose_column(M, j):
    """(source rows, values) of output row j of R2, for matrices too wide to transpose on the host"""
    row_of = np.repeat(np.arange(M.shape[0], dtype=np.int64), np.diff(M.indptr.astype(np.int64)))
    keep = M.indices == np.uint32(j)
    return row_of[keep].astype(np.uint32), M.data[keep]


def hstack(mats):
    """R5's concatenation: per row every part's entries as stored, later parts' ids shifted by the widths before them."""
    rows = mats[0].shape[0]
    width = sum(m.shape[1] for m in mats)
    assert all(m.shape[0] == rows for m in mats) and width < 2 ** 32
    idx, val, ptr, off = [], [], [0], np.concatenate([[0], np.cumsum([m.shape[1] for m in mats])])
    for r in range(rows):
        for k, m in enumerate(mats):
            b, e = int(m.indptr[r]), int(m.indptr[r + 1])
            idx.append(m.indices[b:e].astype(np.uint64) + np.uint64(off[k]))
            val.append(m.data[b:e])
        ptr.append(ptr[-1] + sum(int(m.indptr[r + 1]) - int(m.indptr[r]) for m in mats))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)  # noqa: E731
    return csr(ptr, cat(idx, np.uint32), cat(val, np.float32), (rows, width))


def product(A, B):
    p = smr.logical(smr.rule(A, B, False, True))
    return csr(p[0], p[1], p[2], (A.shape[0], B.shape[1]))


def embedding(Y, X=None, Z=None, method="pifa", normalized_Y=True, variant=None):
    """R3 / R4 / R5.  variant: a wrong variant of R1 or R2, applied wherever that rule is."""
    nv = variant if variant in ("reversed", "double_square") else None
    tv = variant if variant == "row_reversed" else None
    if method == "pii":
        return normalize(transpose(Y, tv), nv)
    E = normalize(product(transpose(normalize(Y, nv) if normalized_Y else Y, tv), X), nv)
    return hstack([E, Z]) if method == "pifa_lf_concat" else E


# ------------------------------------------------------------------------------------------------------------------------ the cases
def order_rows(reverse=False):
    """The four rows [1.0, v, t x 4096], t = 2^-27, on which an fp32 result sees the order of the fp64 sum; v's entry is entry 1 (or, reversed, the
    one before the last)."""
    rows = []
    for vb in ORDER_V_BITS:
        v = np.array([vb], dtype=np.uint32).view(np.float32)[0]
        r = [(0, np.float32(1.0)), (1, v)] + [(2 + i, T27) for i in range(4096)]
        rows.append(r[::-1] if reverse else r)
    return from_rows(rows, 4098)


NORMALIZE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1025, 4098, 0, 5)


def random_rows(lengths=NORMALIZE_LENGTHS, scale=1.0, seed=1, cols=5000):
    rng = np.random.default_rng(seed)
    rows = [list(zip(rng.choice(cols, n, replace=False).tolist(), (rng.standard_normal(n) * scale).astype(np.float32))) for n in lengths]
    return from_rows(rows, cols)


def special_rows():
    f = np.float32
    nan2 = np.array([0x7F812345], dtype=np.uint32).view(np.float32)[0]       # a signalling NaN with a payload
    nneg = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]
    rows = [
        [(0, f(0.0)), (3, f(-0.0)), (5, f(0.0))],                              # all zero, explicit: untouched
        [(1, f(-0.0)), (2, f(3.0)), (4, f(0.0)), (2, f(-4.0))],               # signed zeros, a duplicate id
        [(0, f(np.inf)), (1, f(2.0)), (2, f(-np.inf)), (3, f(-0.0))],         # inf -> NaN, the rest signed zeros
        [(0, f(1.0)), (1, nan2), (2, f(2.0)), (3, nneg)],                      # NaN poisons the row
        [(9, f(1e-30)), (1, f(-2e-30))],                                       # squares far below the fp32 range: zero squares, untouched
        [(i, f(1e30)) for i in range(70)],                                     # squares overflow, wavefront form
        [(i, nan2 if i == 66 else f(i)) for i in range(130)],                  # NaN in the second step of the wavefront form
        [(i, f(np.inf) if i == 3 else f(-1.5)) for i in range(64)],
    ]
    return from_rows(rows, 200)


TRANSPOSE_COUNTS = (0, 1, 63, 64, 65, CAP - 1, CAP, CAP + 1, 20000, 0, 130)


def counted_columns(counts=TRANSPOSE_COUNTS, rows=20011, seed=2, unsorted=True):
    """Column j holds counts[j] entries.  Source rows hold their entries in shuffled column order (unsorted rows), some source rows are
    empty, and row 7 stores a column id twice."""
    rng = np.random.default_rng(seed)
    per_row = [[] for _ in range(rows)]
    for j, c in enumerate(counts):
        for r in np.sort(rng.choice(rows - 11, c, replace=False)) + 11:         # (rows 0 .. 10 stay empty but for row 7)
            per_row[int(r)].append(j)
    big, last = int(np.argmax(counts)), max(j for j, c in enumerate(counts) if c)
    per_row[7] = [big, last, big]                                             # (the counts of these two columns grow by 2 and 1)
    out = []
    for r in per_row:
        if unsorted and len(r) > 1:
            r = [r[i] for i in rng.permutation(len(r))]
        out.append([(j, np.float32(rng.standard_normal())) for j in r])
    return from_rows(out, len(counts))


def golden_inputs():
    """Y 400 x 260, X 400 x 150 (the matrices of the chained clustering test) and a Z 260 x 40."""
    import clustering_rule as cr
    rs = np.random.RandomState(3)
    X = cr.random_csr(400, 150, 6, 41)
    Y = smat.random(400, 260, density=0.02, format="csr", random_state=rs, dtype=np.float32)
    Y.data[:] = 1.0
    Y.data[::7] = 2.0                                                          # (so that normalising Y changes more than a scale per row)
    Z = cr.random_csr(260, 40, 3, 43)
    return Y.astype(np.float32), X, Z


def golden_key(method, normalized_Y):
    return f"{method}__{'norm' if normalized_Y else 'raw'}"


GOLDEN_CHAIN = dict(max_leaf_size=10, threads=1, seed=2)


def order_case(flip=False, xs=None):
    """One label carried by three samples whose X rows share feature 0 with values 1e8, 1, -1e8: its embedding's entry is +0 or 1 * y by
    the order of the additions.  flip: the samples in the other order."""
    f = np.float32
    xs = xs or ([f(1e8), f(-1e8), f(1.0)] if flip else [f(1e8), f(1.0), f(-1e8)])
    Y = from_rows([[(0, f(1.0)), (1, f(1.0))], [(0, f(1.0))], [(0, f(1.0)), (1, f(3.0))], [(1, f(2.0))]], 2)
    X = from_rows([[(0, xs[0]), (2, f(1.0))], [(0, xs[1])], [(0, xs[2]), (1, f(0.5))], [(1, f(1.0))]], 3)
    return Y, X


def transpose_order_case():
    """A pair on which the order inside the transpose's rows reaches the bits of the PIFA product: label 0's samples carry 1, 1e8, -1e8
    -- (1 + 1e8) - 1e8 = 0 in source order, (-1e8 + 1e8) + 1 = 1 with the row reversed."""
    return order_case(xs=[np.float32(1.0), np.float32(1e8), np.float32(-1e8)])


def sparse_edges():
    """Y with an empty column (label 2: an empty embedding row), an empty row (sample 1) and duplicate entries (sample 3 names label 0 twice)."""
    f = np.float32
    Y = from_rows([[(0, f(1.0)), (3, f(2.0))], [], [(1, f(1.0))], [(0, f(0.5)), (3, f(1.0)), (0, f(0.25))], [(3, f(1.0)), (1, f(4.0))]], 4)
    X = from_rows([[(0, f(1.0)), (4, f(2.0))], [(1, f(1.0))], [(4, f(-3.0)), (2, f(1.0))], [(0, f(7.0)), (3, f(0.1))], []], 5)
    Z = from_rows([[(0, f(1.0))], [], [(1, f(2.0)), (0, f(3.0))], [(1, f(-1.0))]], 2)
    return Y, X, Z
