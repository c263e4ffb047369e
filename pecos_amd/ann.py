"""``pecos.ann.hnsw.HNSW`` on the MI355X: a folder saved by the reference's ``HNSW.save`` is loaded into HBM and searched there (K17).

Search only.  Ids, order and distance bits are the reference's (sparse indexes on any x86 host, dense indexes the reference's avx512f
clone).  Training a graph, saving one, ``PairwiseANN`` and the product-quantised HNSW are refused by name."""
import contextlib
import copy
import dataclasses as dc
import json
import os

import numpy as np
import scipy.sparse as smat

from .core import ScipyCsrF32, ScipyDrmF32, clib

__all__ = ["HNSW", "PairwiseANN", "HNSWProductQuantizer4Bits", "hnsw_predict_device"]


@dc.dataclass
class _Params:
    @classmethod
    def from_dict(cls, param=None):
        if param is None:
            return cls()
        if isinstance(param, cls):
            return copy.deepcopy(param)
        if isinstance(param, dict):
            names = {f.name for f in dc.fields(cls)}
            return cls(**{k: v for k, v in param.items() if k in names})
        raise ValueError(f"{param} is not a valid parameter dictionary for {cls.__name__}")

    def to_dict(self):
        return dc.asdict(self)


class HNSW(object):
    """The reference's ``pecos.ann.hnsw.HNSW`` surface over an index in HBM."""

    @dc.dataclass
    class TrainParams(_Params):
        M: int = 32
        efC: int = 100
        threads: int = -1
        max_level_upper_bound: int = -1
        metric_type: str = "ip"

    @dc.dataclass
    class PredParams(_Params):
        efS: int = 100
        topk: int = 10
        threads: int = 1

    class Searchers(object):
        """Device scratch for ``num_searcher`` wavefronts: the reference's pre-allocated intermediate variables."""

        def __init__(self, model, num_searcher=1):
            self.searchers_ptr = clib.hnsw_searchers_create(model.model_ptr, num_searcher)

        def __del__(self):
            p, self.searchers_ptr = getattr(self, "searchers_ptr", None), None
            if p:
                clib.hnsw_searchers_destruct(p)

        def ctypes(self):
            return self.searchers_ptr

    def __init__(self, model_ptr, num_item, feat_dim, data_type, metric_type, pred_params=None):
        self.model_ptr, self.num_item, self.feat_dim = model_ptr, num_item, feat_dim
        self._data_type, self._metric_type = data_type, metric_type
        self.pred_params = self.PredParams.from_dict(pred_params)

    def __del__(self):
        p, self.model_ptr = getattr(self, "model_ptr", None), None
        if p:
            clib.hnsw_destruct(p)

    @property
    def data_type(self):
        return self._data_type

    @property
    def metric_type(self):
        return self._metric_type

    @property
    def info(self):
        return clib.hnsw_info(self.model_ptr)

    @staticmethod
    def create_pymat(X):
        if isinstance(X, (np.ndarray, ScipyDrmF32)):
            return ScipyDrmF32.init_from(X), "drm"
        if isinstance(X, (smat.csr_matrix, ScipyCsrF32)):
            return ScipyCsrF32.init_from(X), "csr"
        raise ValueError("type(X)={} is NOT supported!".format(type(X)))

    @classmethod
    def train(cls, X, train_params=None, pred_params=None):
        raise NotImplementedError("pecos_amd.HNSW.train: building the graph is not served on the device; train with pecos.ann.hnsw.HNSW, save, and load the folder here")

    def save(self, model_folder):
        raise NotImplementedError("pecos_amd.HNSW.save: the index in HBM is not written back; the folder it was loaded from is the saved model")

    @classmethod
    def load(cls, model_folder, lazy_load=False, device=0):
        """``lazy_load`` is accepted and ignored: the index is copied to HBM."""
        with open("{}/param.json".format(model_folder), "r") as fin:
            param = json.loads(fin.read())
        if param["model"] != cls.__name__:
            raise ValueError("param[model] != cls.__name__")
        if not ("data_type" in param and "metric_type" in param):
            raise ValueError("param.json did not have data_type or metric_type!")
        if param["data_type"] not in ("drm", "csr") or param["metric_type"] not in ("ip", "l2"):
            raise NotImplementedError("data_type={} and metric_type={} not implemented".format(param["data_type"], param["metric_type"]))
        c_model_dir = f"{model_folder}/c_model"
        if not os.path.isdir(c_model_dir):
            raise ValueError(f"c_model_dir did not exist: {c_model_dir}")
        model_ptr = clib.hnsw_load(c_model_dir, device)
        model = cls(model_ptr, param["num_item"], param["feat_dim"], param["data_type"], param["metric_type"], param["pred_kwargs"])
        i = model.info
        if (i["data_type"], i["metric_type"]) != (param["data_type"], param["metric_type"]):
            raise ValueError("param.json says {}/{}, c_model/config.json says {}/{}".format(param["data_type"], param["metric_type"], i["data_type"], i["metric_type"]))
        return model

    def searchers_create(self, num_searcher=1):
        if not self.model_ptr:
            raise ValueError("self.model_ptr must exist before using self.create_searcher()")
        if num_searcher <= 0:
            raise ValueError("num_searcher={} <= 0 is NOT valid".format(num_searcher))
        return HNSW.Searchers(self, num_searcher)

    def get_pred_params(self):
        return copy.deepcopy(self.pred_params)

    def predict(self, X, pred_params=None, searchers=None, ret_csr=True):
        pred_params = self.get_pred_params() if pred_params is None else pred_params
        pX, data_type = self.create_pymat(X)
        if data_type != self.data_type:
            raise ValueError("data_type={} is NOT consistent with self.data_type={}".format(data_type, self.data_type))
        if pX.cols != self.feat_dim:
            raise ValueError("pX.cols={} is NOT consistent with self.feat_dim={}".format(pX.cols, self.feat_dim))
        indices = np.zeros(pX.rows * pred_params.topk, dtype=np.uint32)
        distances = np.zeros(pX.rows * pred_params.topk, dtype=np.float32)
        clib.hnsw_predict(self.model_ptr, pX, data_type, indices, distances, pred_params.efS, pred_params.topk, pred_params.threads,
                          None if searchers is None else searchers.ctypes())
        if not ret_csr:
            return indices.reshape(pX.rows, pred_params.topk), distances.reshape(pX.rows, pred_params.topk)
        indptr = np.arange(0, pred_params.topk * (pX.rows + 1), pred_params.topk, dtype=np.uint64)
        return smat.csr_matrix((distances, indices, indptr), shape=(pX.rows, self.num_item), dtype=np.float32)


class PairwiseANN(object):
    def __init__(self, *a, **kw):
        raise NotImplementedError("pecos_amd.PairwiseANN: pairwise ANN search is not served on the device")

    train = load = classmethod(lambda cls, *a, **kw: cls())


class HNSWProductQuantizer4Bits(object):
    def __init__(self, *a, **kw):
        raise NotImplementedError("pecos_amd.HNSWProductQuantizer4Bits: the product-quantised HNSW is not served on the device")

    train = load = classmethod(lambda cls, *a, **kw: cls())


def hnsw_predict_device(model, X, efS=None, topk=None, searchers=None, stream=None):
    """The resident form: ``X`` is a CUDA float32 tensor ``[rows, feat_dim]`` (dense index; the last dimension contiguous, any row
    stride), a CSR ``(crow int64, col int32, val float32[, (rows, cols)])`` of CUDA tensors on one device or a :class:`DeviceMatrix` (sparse index).
    Returns ``(idx int32 [rows, topk], dist float32 [rows, topk], count int32 [rows])`` in HBM; row ``r`` holds ``count[r]`` entries,
    nearest first, and zeros after them."""
    import torch
    from .features import DeviceMatrix
    efS = model.pred_params.efS if efS is None else efS
    topk = model.pred_params.topk if topk is None else topk
    if isinstance(X, DeviceMatrix):
        crow, col, val, shape = X.to_torch(stream=stream)
        X = (crow, col, val)
        rows, cols = shape
    elif isinstance(X, (tuple, list)):
        if len(X) not in (3, 4):
            raise ValueError("hnsw_predict_device: a CSR is (crow, col, val) or (crow, col, val, (rows, cols))")
        crow, col, val = X[:3]
        if not all(torch.is_tensor(t) and t.is_cuda and t.dim() == 1 for t in (crow, col, val)) or col.device != crow.device or val.device != crow.device:
            raise ValueError("hnsw_predict_device: the three tensors of a CSR triple are one-dimensional CUDA tensors on one device")
        if not (crow.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32):
            raise ValueError("hnsw_predict_device: a CSR triple is (crow int64, col int32, val float32) of CUDA tensors")
        if crow.numel() < 1 or col.numel() != val.numel():
            raise ValueError("hnsw_predict_device: crow has rows + 1 entries, col and val one per stored entry")
        rows, cols = crow.numel() - 1, model.feat_dim       # a bare triple carries no width: the index's is taken, and the check kernel refuses an id that reaches it
        if len(X) == 4:
            if tuple(X[3])[0] != rows:
                raise ValueError("hnsw_predict_device: crow has {} entries, the shape says {} rows".format(crow.numel(), tuple(X[3])[0]))
            cols = tuple(X[3])[1]
        X = (crow, col, val)
    elif torch.is_tensor(X):
        if not (X.is_cuda and X.dtype == torch.float32 and X.dim() == 2):
            raise ValueError("hnsw_predict_device: a dense X is a CUDA float32 tensor [rows, feat_dim]")
        if X.shape[1] > 1 and X.stride(1) != 1:
            X = X.contiguous()
        rows, cols = X.shape
    else:
        raise ValueError("type(X)={} is NOT supported!".format(type(X)))
    sparse = isinstance(X, (tuple, list))
    if ("csr" if sparse else "drm") != model.data_type:
        raise ValueError("data_type={} is NOT consistent with self.data_type={}".format("csr" if sparse else "drm", model.data_type))
    if cols != model.feat_dim:
        raise ValueError("pX.cols={} is NOT consistent with self.feat_dim={}".format(cols, model.feat_dim))
    dev = (X[2] if sparse else X).device
    if not sparse and rows > 1 and X.stride(0) < cols:
        X = X.contiguous()
    with torch.cuda.device(dev), (torch.cuda.stream(torch.cuda.ExternalStream(stream)) if stream else contextlib.nullcontext()):
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        idx = torch.zeros((rows, topk), dtype=torch.int32, device=dev)
        dist = torch.zeros((rows, topk), dtype=torch.float32, device=dev)
        count = torch.zeros((rows,), dtype=torch.int32, device=dev)
        if sparse:
            crow, col, val = (t.contiguous() for t in X)
            clib.hnsw_predict_device(model.model_ptr, rows, cols, val.data_ptr(), 0, crow.data_ptr(), col.data_ptr(), val.numel(), efS, topk,
                                     idx.data_ptr(), dist.data_ptr(), count.data_ptr(), topk, None if searchers is None else searchers.ctypes(), s or None)
        else:
            clib.hnsw_predict_device(model.model_ptr, rows, cols, X.data_ptr(), X.stride(0) if rows > 1 else max(cols, 1), None, None, 0, efS, topk,
                                     idx.data_ptr(), dist.data_ptr(), count.data_ptr(), topk, None if searchers is None else searchers.ctypes(), s or None)
    return idx, dist, count
