"""Caller-owned buffers for the device-resident entry points (xrl_queries_from_device_*, xrl_queries_tfidf_device, xrl_queries_concat_device_ex,
xrl_predict_device[_rows]): every array a test hands over is carved out of a larger tensor the test owns,

        [ front band | payload | back band ]

with the payload at a chosen ELEMENT offset from a 16-byte boundary and the bands holding poison that changes the result if a kernel ever uses
it.  Poison can never produce an out-of-range address: values are quiet NaNs, feature ids are valid ids that carry weights (the cycle
0 .. D-1), row pointers are the valid offset 0.  Outputs are carved the same way and filled with a sentinel (SENT_IDX / SENT_VAL).

Also here, shared by the CPU and the GPU tests: the query rows whose tails end 0, 1, 7, 8, 9, 63, 64 and 65 entries into the last batch a
feature walk loads, and what a kernel that read on past a row's end would have computed (poisoned_rows), for the oracle to show that the poison
has teeth."""
import numpy as np
import scipy.sparse as smat

SENT_IDX = 0x5A5A5A5A          # the fillers of tests/test_gpu_ensemble.py
SENT_VAL = -7.0
BAND = 160                     # elements per band: more than a 64-feature chunk plus the widest batch (16) a feature walk runs ahead
TAIL_LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65)
SPARSE_OFFSETS = ((1, 2), (3, 0), (2, 3), (0, 1))        # element offsets of (col, val)
POISON_PAIRS = 8


def _torch():
    import torch
    return torch


def _pattern(fill, n, dtype):
    """n elements of the fill: a scalar, or a 1-D array repeated from its start."""
    f = np.asarray(fill)
    out = np.full(n, f, dtype=dtype) if f.ndim == 0 else np.resize(f.astype(dtype), n)
    return out if n else np.zeros(0, dtype=dtype)


def _bits(t):
    torch = _torch()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def banded(array, elem_offset, band, fill, device=None):
    """(whole, payload): `array` (numpy array or torch tensor, 4- or 8-byte elements, any shape) copied into the middle of a 1-D tensor `whole`
    on `device` (default: the array's own) whose other elements hold `fill`; payload is the view of the copy, shaped like the array, and
    payload.data_ptr() % 16 == elem_offset * itemsize % 16.  Both bands are at least `band` elements long and each starts at fill[0]."""
    torch = _torch()
    t = array if torch.is_tensor(array) else torch.from_numpy(np.ascontiguousarray(array))
    t = t.contiguous()
    isz, n = t.element_size(), t.numel()
    assert isz in (4, 8), "4- or 8-byte elements"
    per16 = 16 // isz
    dev = t.device if device is None else torch.device(device)
    raw = torch.empty(band + per16 + n + band, dtype=t.dtype, device=dev)
    assert raw.data_ptr() % isz == 0
    front = band + (elem_offset - raw.data_ptr() // isz - band) % per16
    whole = raw[: front + n + band]
    npdt = np.dtype(str(t.dtype).replace("torch.", ""))
    whole[:front] = torch.from_numpy(_pattern(fill, front, npdt)).to(dev)
    whole[front + n:] = torch.from_numpy(_pattern(fill, band, npdt)).to(dev)
    payload = whole[front: front + n]
    payload.copy_(t.reshape(-1))
    payload = payload.view(t.shape)
    assert addr(payload) % 16 == (elem_offset * isz) % 16
    return whole, payload


def addr(t):
    """Device (or host) address of a view's first element -- also of an EMPTY view, for which data_ptr() gives none."""
    return t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()


def payload_slice(whole, payload):
    b = payload.storage_offset() - whole.storage_offset()
    return slice(b, b + payload.numel())


def poison_like(kind, D=None):
    """The fill of a band: "value" -> quiet NaN (val, count, idf, emb, dense X); "index" -> the cycle 0 .. D-1 of valid feature ids;
    "rowptr" -> the valid offset 0."""
    if kind == "value":
        return np.float32(np.nan)
    if kind == "index":
        return np.arange(D, dtype=np.int32)
    if kind == "rowptr":
        return np.int64(0)
    raise ValueError(kind)


def assert_bands_intact(whole, payload, fill, what=""):
    """Both bands of `whole` still hold `fill`, bit for bit (payload: the view banded() returned, or its slice of whole)."""
    torch = _torch()
    sl = payload if isinstance(payload, slice) else payload_slice(whole, payload)
    npdt = np.dtype(str(whole.dtype).replace("torch.", ""))
    for name, part in (("front", whole[: sl.start]), ("back", whole[sl.stop:])):
        want = torch.from_numpy(_pattern(fill, part.numel(), npdt))
        same = _bits(part.detach().cpu()) == _bits(want)
        assert bool(same.all()), f"{what}: {name} band: element {int((~same).nonzero()[0])} of {part.numel()} was overwritten"


def sentinel_out(n_rows, stride, elem_offsets=(0, 0, 0), band=BAND, device="cuda"):
    """Banded result buffers [n_rows, stride] (labels, scores) and [n_rows] (counts) full of the sentinel: ((whole, view), ...) for idx, val, cnt."""
    idx = banded(np.full((n_rows, stride), SENT_IDX, np.int32), elem_offsets[0], band, np.int32(SENT_IDX), device)
    val = banded(np.full((n_rows, stride), SENT_VAL, np.float32), elem_offsets[1], band, np.float32(SENT_VAL), device)
    cnt = banded(np.full((n_rows,), SENT_IDX, np.int32), elem_offsets[2], band, np.int32(SENT_IDX), device)
    return idx, val, cnt


# ------------------------------------------------------------------------------------------------------------------ the query rows
def tail_rows(D, seed=20):
    """8 seeded rows of TAIL_LENGTHS entries (sorted distinct feature ids < D, values away from zero)."""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(TAIL_LENGTHS)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(D, n, replace=False)) for n in TAIL_LENGTHS]).astype(np.int32)
    val = (rng.uniform(0.05, 0.5, indptr[-1]) * rng.choice([-1.0, 1.0], indptr[-1])).astype(np.float32)
    X = smat.csr_matrix((val, idx, indptr), shape=(len(TAIL_LENGTHS), D), dtype=np.float32)
    X.sort_indices()
    return X


def with_tails(X):
    """(golden X followed by the 8 tail rows, the cut points R: X[:R] ends with a tail row)."""
    n0 = X.shape[0]
    Xt = smat.vstack([X.astype(np.float32), tail_rows(X.shape[1])]).tocsr().astype(np.float32)
    Xt.sort_indices()
    return Xt, [n0 + 1 + i for i in range(len(TAIL_LENGTHS))]


def poisoned_rows(X, R, pairs=POISON_PAIRS):
    """X[:R] as a kernel would see it that took the first `pairs` (feature id, value) pairs of the back bands for entries of row R - 1:
    ids 0 .. pairs-1 with NaN values behind the row's own entries (stored order, as the arrays hold them)."""
    D = X.shape[1]
    nnz = int(X.indptr[R])
    idx = np.concatenate([X.indices[:nnz], _pattern(poison_like("index", D), pairs, np.int32)]).astype(np.int32)
    val = np.concatenate([X.data[:nnz], _pattern(poison_like("value"), pairs, np.float32)]).astype(np.float32)
    indptr = X.indptr[: R + 1].astype(np.int64).copy()
    indptr[R] += pairs
    P = smat.csr_matrix((R, D), dtype=np.float32)
    P.indptr, P.indices, P.data = indptr, idx.astype(np.int64), val             # assigned directly: the order and the NaNs stay as they are
    return P


def shifted_dense_row(row, by):
    """A dense row read `by` elements too early (by < 0) or too late (by > 0) inside a NaN-filled buffer whose next row is all poison."""
    out = np.full_like(row, np.nan)
    if by > 0:
        out[: len(row) - by] = row[by:]
    else:
        out[-by:] = row[: len(row) + by]
    return out


def differs(a, b):
    """Two predictions (CSR, score-sorted rows) are not the same answer: row lengths, labels, order or score bits."""
    return not (np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
                and np.array_equal(a.data.astype(np.float32).view(np.uint32), b.data.astype(np.float32).view(np.uint32)))
