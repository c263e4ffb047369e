"""K12D: the rule R3D of ``xrl_label_embedding_dense_device`` in numpy, one wrong variant (the fused chain), the case both test halves run."""
import numpy as np

import label_embedding_rule as ler

F32 = np.float32
LONG, SAMPLES = 512, 600                                                  # xrl_embed.h: kEmbedDenseLong
ROW_LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 129, LONG - 1, LONG, LONG + 45)  # look-ahead (8; long form 32), staging (64) and long-form steps
ORDER_LABEL, EMPTY_LABEL = len(ROW_LENGTHS), len(ROW_LENGTHS) + 2
COLS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 768, 1025, 4097)            # lane, slab and workgroup-loop (4096) edges


def product(A, X, fused=False):
    """scipy's csr_matvecs: one fp32 chain from +0.0 per element over the row's stored entries, product and sum rounded (fused: the sum only)"""
    X = np.asarray(X, dtype=F32)
    P = np.zeros((A.shape[0], X.shape[1]), dtype=F32)
    with np.errstate(all="ignore"):
        for r in range(A.shape[0]):
            y = P[r]
            for p in range(int(A.indptr[r]), int(A.indptr[r + 1])):
                a, x = A.data[p], X[int(A.indices[p])]
                if fused:
                    y = (y.astype(np.float64) + np.float64(a) * x.astype(np.float64)).astype(F32)
                else:
                    y = (y + (a * x).astype(F32)).astype(F32)
            P[r] = y
    return P


def normalize(P):
    """R1 on the dense rows: every element a stored entry, in column order"""
    r, c = P.shape
    full = ler.csr(np.arange(r + 1, dtype=np.uint64) * c, np.tile(np.arange(c, dtype=np.uint32), r), P.reshape(-1).astype(F32), (r, c))
    return ler.normalize(full).data.reshape(P.shape)


def embedding(Y, X, Z=None, normalized_Y=True, fused=False):
    E = normalize(product(ler.transpose(ler.normalize(Y) if normalized_Y else Y), X, fused))
    return E if Z is None else np.hstack([E, np.asarray(Z, dtype=F32)])


def label_rows(seed=5):
    """YT's rows: a label per length of ROW_LENGTHS, ORDER_LABEL (samples 0, 1, 2 alone), one with sample 40 twice, EMPTY_LABEL without positives"""
    rng = np.random.default_rng(seed)
    rows = []
    for n in ROW_LENGTHS:
        rows.append([(int(i), F32(v)) for i, v in zip(np.sort(rng.choice(np.arange(3, SAMPLES), n, replace=False)), rng.uniform(0.5, 2.0, n))])
    rows.append([(0, F32(1.0)), (1, F32(1.0)), (2, F32(1.0))])
    rows.append([(30, F32(0.5)), (40, F32(1.0)), (40, F32(0.25)), (50, F32(2.0))])
    rows.append([])
    return rows


def case_Y():
    """samples x labels, built as the transpose of label_rows()"""
    return ler.transpose(ler.from_rows(label_rows(), SAMPLES))


def case_X(cols, zero=False):
    """column 0 of samples 0, 1, 2 holds 1e8, 1, -1e8: the order label's element is (1e8 + 1) - 1e8 = 0 in the rule's order"""
    X = np.zeros((SAMPLES, cols), dtype=F32) if zero else np.random.default_rng(cols).standard_normal((SAMPLES, cols)).astype(F32)
    if not zero:
        X[:3, 0] = (1e8, 1.0, -1e8)
    return X


def ulps(a, b):
    """the distance of two float32 arrays in units in the last place"""
    def key(v):
        i = np.ascontiguousarray(v, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
