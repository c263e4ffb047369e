"""Label embeddings over DENSE features on the MI355X (K12D): ``normalize(normalize(Y)^T * X)`` for a dense ``X`` resident in HBM, in the
reference's order of additions (``YT.dot(X)``, pecos/xmc/base.py:1967-1975) with the row normalisation fused behind the product, written
once as the dense row-major tensor :func:`~pecos_amd.indexer.run_clustering_device` takes as it is.

The rule R3D is stated at ``xrl_label_embedding_dense_device`` in include/xrl_abi.h.  These are the served names;
``pecos_amd.indexer.LabelEmbeddingFactory`` and ``label_embedding_device`` keep their pinned refusal of a dense ``X``, as
``pecos_amd.pairwise`` stands beside ``pecos_amd.ann``."""
import numpy as np
import scipy.sparse as smat

from . import indexer
from .core import clib

__all__ = ["LabelEmbeddingFactory", "label_embedding_dense_device", "sparse_dense_matmul_device"]


def _dense_operand(fn, name, T):
    """A dense operand as the kernels read it: (tensor, row stride in floats).  Read in place when its rows are contiguous and its row
    stride is at least its width; anything else goes through ``.contiguous()``.  Never changed."""
    import torch
    if not isinstance(T, torch.Tensor) or T.dim() != 2 or T.dtype != torch.float32 or not T.is_cuda:
        raise ValueError(f"{fn}: {name} must be a 2-D float32 CUDA tensor")
    if not _rows_in_place(T):
        T = T.contiguous()
    return T, _row_stride(T)


def _rows_in_place(T):
    rows, cols = T.shape
    return (cols <= 1 or T.stride(1) == 1) and (rows <= 1 or T.stride(0) >= cols)


def _row_stride(T):
    return T.stride(0) if T.shape[0] > 1 else T.shape[1]


def _result(fn, out, rows, cols, device):
    import torch
    if out is None:
        return torch.empty((rows, cols), dtype=torch.float32, device=device)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != device or tuple(out.shape) != (rows, cols):
        raise ValueError(f"{fn}: out must be a float32 tensor of shape ({rows}, {cols}) on {device}")
    if not _rows_in_place(out):
        raise ValueError(f"{fn}: out must have contiguous rows and a row stride of at least its width")
    return out


def _is_sparse(M):
    from .features import DeviceMatrix
    return smat.issparse(M) or isinstance(M, (DeviceMatrix, tuple, list))


def label_embedding_dense_device(Y, X, method="pifa", Z=None, normalized_Y=True, out=None, stream=None):
    """The label embedding of ``Y`` (samples x labels) over a dense ``X`` (samples x features), computed and left in HBM as a float32 CUDA
    tensor ``[labels, features (+ label-features)]``: ``method`` is ``"pifa"`` = normalize(normalize(Y)^T * X) or ``"pifa_lf_concat"`` =
    that next to the dense ``Z`` (labels x label-features).  ``X`` and ``Z`` are 2-D float32 CUDA tensors, read in place at any row stride
    of at least their width; ``Y`` is what :func:`~pecos_amd.indexer.label_embedding_device` takes (a DeviceMatrix, a float32 scipy sparse
    matrix, CSR tensors); none of them is changed.  ``out``: a tensor of the result's shape to write into (a window of a wider one is
    fine).  The product is scipy's ``YT.dot(X)`` bit for bit, the normalisation sklearn's CSR arithmetic (R3D).  The result feeds
    :func:`~pecos_amd.indexer.run_clustering_device`.  Runs on ``stream`` (default: torch's current one), which it synchronises."""
    import torch
    from .features import _as_device_matrix, _stream_or_current
    fn = "label_embedding_dense_device"
    method = str(method).lower()
    if method == "pifa_lf_convex_combine":
        raise NotImplementedError(f"{fn}: pifa_lf_convex_combine is not served on the device (its result is float64 in the reference)")
    if method not in clib.EMBED_DENSE_METHODS:
        raise NotImplementedError(f"{fn}: method '{method}' is not served over dense features; served: {sorted(clib.EMBED_DENSE_METHODS)}")
    concat = method == "pifa_lf_concat"
    if Y is None or X is None or (concat and Z is None):
        raise ValueError(f"{fn}: method '{method}' needs " + ("Y, X and Z" if concat else "Y and X"))
    if _is_sparse(X) or (concat and _is_sparse(Z)):
        raise NotImplementedError(f"{fn}: a dense / sparse mix of X and Z is not served (it needs dense_to_csr); a sparse X goes to label_embedding_device")
    X, x_stride = _dense_operand(fn, "X", X)
    dev = X.device
    z_cols = z_stride = 0
    if concat:
        Z, z_stride = _dense_operand(fn, "Z", Z)
        z_cols = Z.shape[1]
        if Z.device != dev:
            raise ValueError(f"{fn}: X and Z are on {dev} and {Z.device}")
    y = _as_device_matrix(indexer._embedding_operand("Y", Y), dev.index, None, stream)
    samples, labels = y.shape
    if samples != X.shape[0] or (concat and Z.shape[0] != labels):
        raise ValueError(f"{fn}: Y is {samples} x {labels}, X has {X.shape[0]} rows" + (f", Z has {Z.shape[0]} rows" if concat else ""))
    with torch.cuda.device(dev):
        out = _result(fn, out, labels, X.shape[1] + z_cols, dev)
    if stream is not None:
        torch.cuda.current_stream(dev).synchronize()       # the operands were made on torch's stream
    clib.label_embedding_dense_device(y.handle, X.data_ptr(), X.shape[1], x_stride, Z.data_ptr() if concat else None, z_cols, z_stride, method, normalized_Y,
                                      out.data_ptr(), _row_stride(out), stream=_stream_or_current(dev.index, stream))
    return out


def sparse_dense_matmul_device(A, X, out=None, stream=None):
    """``A * X`` for a sparse ``A`` (a DeviceMatrix, a float32 scipy sparse matrix or CSR tensors) and a dense 2-D float32 CUDA tensor ``X``,
    as a float32 CUDA tensor ``[A.rows, X.cols]``: every element one fp32 chain over the stored entries of ``A``'s row in stored order,
    bit for bit scipy's ``A.dot(X)`` (``xrl_smat_matmul_dense_device``) -- the roll-up of a dense embedding.  Runs on ``stream`` (default:
    torch's current one), which it synchronises."""
    import torch
    from .features import _as_device_matrix, _stream_or_current
    fn = "sparse_dense_matmul_device"
    X, x_stride = _dense_operand(fn, "X", X)
    dev = X.device
    if smat.issparse(A) and A.dtype != np.float32:
        raise ValueError(f"{fn}: A must be float32, got {A.dtype}")
    a = _as_device_matrix(A, dev.index, None, stream)
    rows, inner = a.shape
    if inner != X.shape[0]:
        raise ValueError(f"{fn}: A is {rows} x {inner}, X has {X.shape[0]} rows")
    with torch.cuda.device(dev):
        out = _result(fn, out, rows, X.shape[1], dev)
    if stream is not None:
        torch.cuda.current_stream(dev).synchronize()
    clib.smat_matmul_dense_device(a.handle, X.data_ptr(), X.shape[0], X.shape[1], x_stride, out.data_ptr(), _row_stride(out), 0, stream=_stream_or_current(dev.index, stream))
    return out


class LabelEmbeddingFactory(indexer.LabelEmbeddingFactory):
    """:class:`pecos_amd.indexer.LabelEmbeddingFactory` that also serves a dense ``X``: ``pifa`` and ``pifa_lf_concat`` over an ``ndarray`` ``X``
    (``Z`` an ``ndarray`` or absent) upload it once, run K12D and return an ``ndarray``, as the reference does; every other combination of
    operands goes to the parent.  A dense / sparse mix of ``X`` and ``Z`` and ``pifa_lf_convex_combine`` stay refused."""

    @staticmethod
    def create(Y=None, X=None, method="pifa", **kwargs):
        m = str(method).lower()
        if isinstance(X, np.ndarray) and m in ("pifa", "pifa_lf_concat"):
            return getattr(LabelEmbeddingFactory, m)(Y, X, **kwargs)
        return indexer.LabelEmbeddingFactory.create(Y, X, method, **kwargs)

    @staticmethod
    def _dense(method, Y, X, Z=None, normalized_Y=True):
        import torch
        if not smat.issparse(Y):
            raise NotImplementedError("type(Y) should be scipy.sparse.spmatrix")
        for name, M in (("X", X), ("Z", Z)):
            if M is not None and M.dtype != np.float32:
                raise ValueError(f"label embedding: {name} must be float32, got {M.dtype}")
        up = lambda M: None if M is None else torch.from_numpy(np.ascontiguousarray(M)).cuda()  # noqa: E731
        return label_embedding_dense_device(Y, up(X), method, up(Z), normalized_Y).cpu().numpy()

    @staticmethod
    def pifa(Y, X, threads=-1, normalized_Y=True):
        if isinstance(X, np.ndarray):
            return LabelEmbeddingFactory._dense("pifa", Y, X, normalized_Y=normalized_Y)
        return indexer.LabelEmbeddingFactory.pifa(Y, X, threads, normalized_Y)

    @staticmethod
    def pifa_lf_concat(Y, X, Z, threads=-1, normalized_Y=True):
        if isinstance(X, np.ndarray) != isinstance(Z, np.ndarray):
            raise NotImplementedError("LabelEmbeddingFactory: a dense / sparse mix of X and Z is not served on the device (it needs dense_to_csr)")
        if isinstance(X, np.ndarray):
            return LabelEmbeddingFactory._dense("pifa_lf_concat", Y, X, Z, normalized_Y)
        return indexer.LabelEmbeddingFactory.pifa_lf_concat(Y, X, Z, threads, normalized_Y)
