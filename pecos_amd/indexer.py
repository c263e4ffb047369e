"""Label indexing on the device: :class:`HierarchicalKMeans` (the surface of ``pecos.xmc.base.HierarchicalKMeans``: ``TrainParams``,
``gen``) over K11's balanced hierarchical 2-means, and :func:`run_clustering_device`, whose feature matrix and codes stay in HBM.
The codes are the reference's at ``threads = 1`` (``xrl_run_clustering_device`` in include/xrl_abi.h states the rule).
Ahead of it :class:`LabelEmbeddingFactory` (the surface of ``pecos.xmc.base.LabelEmbeddingFactory``) and
:func:`label_embedding_device` over K12 and K10: label matrix and features in, the PIFA / PII embedding out, which the clustering
takes as it is (``xrl_label_embedding_device`` states the rules)."""
import dataclasses as dc
import math

import numpy as np
import scipy.sparse as smat

from .core import ClusteringParam, ScipyCsrF32, ScipyDrmF32, clib


def codes_to_csc(codes, depth):
    """Leaf codes -> the binary ``len(codes) x 2^depth`` CSC with a 1 at ``(r, codes[r])``, rows ascending inside a column."""
    codes = np.asarray(codes).astype(np.int64)
    n_codes = 1 << depth
    indptr = np.zeros(n_codes + 1, dtype=np.int64)
    np.cumsum(np.bincount(codes, minlength=n_codes), out=indptr[1:])
    indices = np.argsort(codes, kind="stable")
    return smat.csc_matrix((np.ones(len(codes), dtype=np.float32), indices, indptr), shape=(len(codes), n_codes))


def chain_from_partial(C, min_codes=None, nr_splits=16):
    """The chain above a bottom clustering matrix ``C`` (labels x codes): code ``c`` of a level belongs to code ``c // nr_splits`` of the level
    above, until a level has at most ``min_codes`` codes (None: ``nr_splits``; <= 1: no level is added); a single root column tops every
    chain with more than one code.  Returns the list of ``csc_matrix``, root first (``ClusterChain.from_partial_chain``)."""
    if min_codes is None:
        min_codes = nr_splits
    chain = [smat.csc_matrix(C, dtype=np.float32)]
    if min_codes is None or min_codes <= 1:
        min_codes = chain[0].shape[1]
    while chain[0].shape[1] > min_codes:
        n = chain[0].shape[1]
        child = np.arange(n)
        parent = child // nr_splits
        chain.insert(0, smat.csc_matrix((np.ones(n, dtype=np.float32), (child, parent)), shape=(n, int(parent.max()) + 1), dtype=np.float32))
    if chain[0].shape[1] > 1:
        chain.insert(0, smat.csc_matrix(np.ones((chain[0].shape[1], 1), dtype=np.float32)))
    return chain


class HierarchicalKMeans(object):
    """Hierarchical 2-means label indexing (PECOS, Yu et al. 2020, Algorithm 1), clustered on the device."""

    KMEANS = 0
    SKMEANS = 5

    @dc.dataclass
    class TrainParams(object):
        """The reference's training parameters with its defaults (pecos/xmc/base.py:85-119)."""
        nr_splits: int = 16
        min_codes: int = None
        max_leaf_size: int = 100
        spherical: bool = True
        seed: int = 0
        kmeans_max_iter: int = 20
        threads: int = -1
        do_sample: bool = False
        max_sample_rate: float = 1.0
        min_sample_rate: float = 0.1
        warmup_ratio: float = 0.4

        @classmethod
        def from_dict(cls, param=None):
            if param is None:
                return cls()
            if isinstance(param, cls):
                return dc.replace(param)
            if isinstance(param, dict):
                names = {f.name for f in dc.fields(cls)}
                return cls(**{k: v for k, v in param.items() if k in names})
            raise ValueError(f"{cls} can only be created from a dict or an instance, got {type(param)}")

        def to_dict(self):
            return dict(__meta__={"class_fullname": "pecos.xmc.base###HierarchicalKMeans.TrainParams"}, **dc.asdict(self))

        def infer_binary_tree_depth(self, label_num):
            depth = max(1, int(math.ceil(math.log2(label_num / self.max_leaf_size))))
            if (2 ** depth) > label_num:
                raise ValueError(f"max_leaf_size > 1 is needed for feat_mat.shape[0] == {label_num} to avoid empty clusters")
            return depth

        def get_layer_sample_rate(self, cur_layer, binary_tree_depth):
            warmup_depth = int(self.warmup_ratio * binary_tree_depth)
            if cur_layer < warmup_depth:
                return self.min_sample_rate
            return self.min_sample_rate + (self.max_sample_rate - self.min_sample_rate) * float(cur_layer + 1 - warmup_depth) / float(
                binary_tree_depth - warmup_depth)

    @classmethod
    def gen(cls, feat_mat, train_params=None, dtype=np.float32, **kwargs):
        """The cluster chain of the label features ``feat_mat`` (float32 ``csr_matrix`` or ``ndarray``), as a list of ``csc_matrix``, root first."""
        p = cls.TrainParams.from_dict(kwargs if train_params is None else train_params)
        if p.min_codes is None:
            p.min_codes = p.nr_splits
        if not p.do_sample:
            p.warmup_ratio = 1.0
            p.min_sample_rate = 1.0
        n = feat_mat.shape[0]
        if p.max_leaf_size >= n:
            return chain_from_partial(smat.csc_matrix(np.ones((n, 1), dtype=np.float32)))
        p.depth = p.infer_binary_tree_depth(n)
        p.partition_algo = cls.SKMEANS if p.spherical else cls.KMEANS
        assert feat_mat.dtype == np.float32
        if isinstance(feat_mat, (smat.csr_matrix, ScipyCsrF32)):
            view = ScipyCsrF32.init_from(feat_mat)
        elif isinstance(feat_mat, (np.ndarray, ScipyDrmF32)):
            view = ScipyDrmF32.init_from(feat_mat)
        else:
            raise NotImplementedError("type(feat_mat) = {} is not supported.".format(type(feat_mat)))
        codes = clib.run_clustering(view, p)
        return chain_from_partial(codes_to_csc(codes, p.depth), min_codes=p.min_codes, nr_splits=p.nr_splits)


def run_clustering_device(feat, depth, partition_algo=HierarchicalKMeans.SKMEANS, seed=0, kmeans_max_iter=20, max_sample_rate=1.0, min_sample_rate=1.0,
                          warmup_ratio=1.0, return_scores=False, stream=None, dtype=None):
    """Leaf codes of the rows of ``feat`` -- a :class:`~pecos_amd.features.DeviceMatrix`, CSR tensors ``(crow, col, val, (rows, cols))`` or
    a scipy sparse matrix -- computed and left in HBM: an int32 tensor ``[rows]`` (``dtype=torch.uint32`` for that type), and with
    ``return_scores`` also the float32 ``[depth, rows]`` scores as they stand after each level.  Runs on ``stream`` (default: torch's
    current one), which it synchronises."""
    import torch
    from .features import _as_device_matrix, _operand_device, _stream_or_current
    dev = _operand_device(feat)
    m = _as_device_matrix(feat, 0 if dev is None else dev, None, stream)
    info = m.info
    tdev = torch.device("cuda", info["device"])
    codes = torch.zeros(info["rows"], dtype=torch.int32, device=tdev)
    scores = torch.zeros((depth, info["rows"]), dtype=torch.float32, device=tdev) if return_scores else None
    param = ClusteringParam(partition_algo=partition_algo, seed=seed, kmeans_max_iter=kmeans_max_iter, threads=1, max_sample_rate=max_sample_rate,
                            min_sample_rate=min_sample_rate, warmup_ratio=warmup_ratio)
    if stream is not None:
        torch.cuda.current_stream(tdev).synchronize()      # the zero fills above ran on torch's stream
    clib.run_clustering_device(m.handle, depth, param, codes.data_ptr(), scores.data_ptr() if return_scores else None,
                               stream=_stream_or_current(info["device"], stream))
    if dtype is not None:
        codes = codes.view(dtype)
    return (codes, scores) if return_scores else codes


def _embedding_operand(name, M):
    """An operand of a label embedding as the device form takes it; what is not served says so."""
    if isinstance(M, np.ndarray):
        raise NotImplementedError(f"label embedding: a dense {name} is not served on the device (CSR operands only)")
    if smat.issparse(M) and M.dtype != np.float32:
        raise ValueError(f"label embedding: {name} must be float32, got {M.dtype}")
    return M


def label_embedding_device(Y, X=None, method="pifa", Z=None, normalized_Y=True, stream=None):
    """The label embedding of ``Y`` (samples x labels) computed and left in HBM as a :class:`~pecos_amd.features.DeviceMatrix`
    (labels x features): ``method`` is ``"pifa"`` = normalize(normalize(Y)^T * X) over ``X`` (samples x features), ``"pifa_lf_concat"`` =
    that next to ``Z`` (labels x label-features), or ``"pii"`` = normalize(Y^T), in the reference's arithmetic bit for bit.  An operand is
    what :func:`~pecos_amd.features.sparse_matmul_device` accepts: a DeviceMatrix, a float32 scipy sparse matrix (uploaded), or CSR tensors
    ``(crow, col, val, (rows, cols))``; none of them is changed.  The result feeds :func:`run_clustering_device`.  Runs on ``stream``
    (default: torch's current one), which it synchronises."""
    from .features import DeviceMatrix, _as_device_matrix, _operand_device, _stream_or_current
    method = str(method).lower()
    if method == "pifa_lf_convex_combine":
        raise NotImplementedError("label embedding: pifa_lf_convex_combine is not served on the device")
    if method not in clib.EMBED_METHODS:
        raise NotImplementedError(f"label embedding method '{method}' is not implemented; served: {sorted(clib.EMBED_METHODS)}")
    if Y is None or (method != "pii" and X is None) or (method == "pifa_lf_concat" and Z is None):
        raise ValueError(f"label embedding: method '{method}' needs " + {"pii": "Y", "pifa": "Y and X", "pifa_lf_concat": "Y, X and Z"}[method])
    ops = [_embedding_operand("Y", Y), None if method == "pii" else _embedding_operand("X", X),
           _embedding_operand("Z", Z) if method == "pifa_lf_concat" else None]
    dev = next((d for d in (_operand_device(M) for M in ops if M is not None) if d is not None), 0)
    y, x, z = (None if M is None else _as_device_matrix(M, dev, None, stream) for M in ops)
    return DeviceMatrix(clib.label_embedding_device(y.handle, x and x.handle, z and z.handle, method, normalized_Y, stream=_stream_or_current(dev, stream)))


class LabelEmbeddingFactory(object):
    """The reference's ``LabelEmbeddingFactory`` (pecos/xmc/base.py:1903-2094) computed on the device: scipy matrices in, a scipy
    ``csr_matrix`` out, bit for bit the reference's at ``threads = 1``.  ``threads`` is accepted and ignored.  Dense ``X`` / ``Z`` and
    ``pifa_lf_convex_combine`` are not served."""

    @staticmethod
    def create(Y=None, X=None, method="pifa", **kwargs):
        mapping = {"pifa": LabelEmbeddingFactory.pifa, "pifa_lf_concat": LabelEmbeddingFactory.pifa_lf_concat,
                   "pifa_lf_convex_combine": LabelEmbeddingFactory.pifa_lf_convex_combine, "pii": LabelEmbeddingFactory.pii}
        m = str(method).lower()
        if m not in mapping:
            raise NotImplementedError(f"Label embedding method '{method}' is not implemented. Valid ones: {list(mapping)}")
        return mapping[m](Y) if m == "pii" else mapping[m](Y, X, **kwargs)

    @staticmethod
    def _run(method, Y, X=None, Z=None, normalized_Y=True):
        if not smat.issparse(Y):
            raise NotImplementedError("type(Y) should be scipy.sparse.spmatrix")
        for name, M in (("X", X), ("Z", Z)):
            if M is not None and not isinstance(M, (smat.csr_matrix, np.ndarray)):
                raise NotImplementedError(f"type({name}) should be row-major spmatrix or ndarray")
        return label_embedding_device(Y, X, method=method, Z=Z, normalized_Y=normalized_Y).download()

    @staticmethod
    def pifa(Y, X, threads=-1, normalized_Y=True):
        return LabelEmbeddingFactory._run("pifa", Y, X, normalized_Y=normalized_Y)

    @staticmethod
    def pifa_lf_concat(Y, X, Z, threads=-1, normalized_Y=True):
        return LabelEmbeddingFactory._run("pifa_lf_concat", Y, X, Z, normalized_Y=normalized_Y)

    @staticmethod
    def pifa_lf_convex_combine(Y, X, Z, alpha=0.5, threads=-1, normalized_Y=True):
        raise NotImplementedError("LabelEmbeddingFactory: pifa_lf_convex_combine is not served on the device")

    @staticmethod
    def pii(Y):
        return LabelEmbeddingFactory._run("pii", Y)
