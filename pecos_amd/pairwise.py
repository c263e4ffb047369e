"""``pecos.ann.pairwise.PairwiseANN`` on the MI355X: ``X_trn`` and ``Y_csc`` live in HBM and every ``(input row, label key)`` pair is an exact
scan of the label's column there (K18).

Row ids, order, distance bits and ``Y`` values are the reference's (sparse indexes on any x86 host, dense indexes the reference's avx512f clone;
DESIGN.md section 9).  This is the served class; ``pecos_amd.ann.PairwiseANN`` keeps its pinned refusal, as ``train_ext`` stands beside ``train``."""
import contextlib
import dataclasses as dc
import json
import os

import numpy as np
import scipy.sparse as smat

from .ann import _Params
from .core import ScipyCscF32, ScipyCsrF32, ScipyDrmF32, clib

__all__ = ["PairwiseANN", "pairwise_predict_device"]


class PairwiseANN(object):
    """The reference's ``pecos.ann.pairwise.PairwiseANN`` surface over an index in HBM."""

    @dc.dataclass
    class TrainParams(_Params):
        metric_type: str = "ip"

    @dc.dataclass
    class PredParams(_Params):
        batch_size: int = 1024
        only_topk: int = 10

    class Searchers(object):
        """``num_searcher`` wavefront slots with their device scratch, and the four host arrays a ``predict`` returns views of."""

        def __init__(self, model, pred_params, num_searcher=1):
            self.searchers_ptr = clib.pairwise_searchers_create(model.model_ptr, num_searcher)
            self.pred_params = pred_params
            max_nnz = pred_params.batch_size * pred_params.only_topk
            self.Imat = np.zeros(max_nnz, dtype=np.uint32)
            self.Mmat = np.zeros(max_nnz, dtype=np.uint32)
            self.Dmat = np.zeros(max_nnz, dtype=np.float32)
            self.Vmat = np.zeros(max_nnz, dtype=np.float32)

        def __del__(self):
            p, self.searchers_ptr = getattr(self, "searchers_ptr", None), None
            if p:
                clib.pairwise_searchers_destruct(p)

        def ctypes(self):
            return self.searchers_ptr

        def reset(self, reset_nnz):
            self.Imat[:reset_nnz].fill(0)
            self.Mmat[:reset_nnz].fill(0)
            self.Dmat[:reset_nnz].fill(0.0)
            self.Vmat[:reset_nnz].fill(0.0)

    def __init__(self, model_ptr, num_input_keys, num_label_keys, feat_dim, data_type, pred_params=None):
        self.model_ptr, self.num_input_keys, self.num_label_keys, self.feat_dim = model_ptr, num_input_keys, num_label_keys, feat_dim
        self._data_type = data_type
        self.pred_params = self.PredParams.from_dict(pred_params)

    def __del__(self):
        p, self.model_ptr = getattr(self, "model_ptr", None), None
        if p:
            clib.pairwise_destruct(p)

    @property
    def data_type(self):
        return self._data_type

    @property
    def metric_type(self):
        return "ip"

    @property
    def info(self):
        return clib.pairwise_info(self.model_ptr)

    @staticmethod
    def create_pymat(X):
        if isinstance(X, (np.ndarray, ScipyDrmF32)):
            return ScipyDrmF32.init_from(X), "drm"
        if isinstance(X, (smat.csr_matrix, ScipyCsrF32)):
            return ScipyCsrF32.init_from(X), "csr"
        raise ValueError("type(X)={} is NOT supported!".format(type(X)))

    @staticmethod
    def _check_metric(data_type, metric_type):
        if metric_type != "ip":                          # (pecos.core.clib.pairwise_ann_init's refusal)
            raise NotImplementedError("data_type={} and metric_type={} not implemented".format(data_type, metric_type))

    @classmethod
    def train(cls, X, Y, train_params=None, pred_params=None, device=0):
        train_params = cls.TrainParams.from_dict(train_params)
        pred_params = cls.PredParams.from_dict(pred_params)
        if not isinstance(Y, smat.csr_matrix) and not isinstance(Y, smat.csc_matrix):
            raise ValueError("type(Y) should be either a csr_matrix or csc_matrix.")
        pY = ScipyCscF32.init_from(Y.tocsc())
        pX, data_type = cls.create_pymat(X)
        cls._check_metric(data_type, train_params.metric_type)
        return cls(clib.pairwise_train(pX, data_type, pY, device), pY.rows, pY.cols, pX.cols, data_type, pred_params)

    @classmethod
    def train_device(cls, X, Y, train_params=None, pred_params=None, stream=None):
        """The resident build.  ``X``: a :class:`DeviceMatrix` (sparse index) or a CUDA float32 tensor ``[N, feat_dim]`` (dense index, last dimension
        contiguous); ``Y``: a :class:`DeviceMatrix` ``[N, L]``.  ``Y`` is transposed on the device (its rows become the columns the pairs scan, in
        scipy's ``tocsc()`` order) and both are copied device to device; nothing visits the host."""
        import torch
        from .features import DeviceMatrix
        cls._check_metric("csr" if isinstance(X, DeviceMatrix) else "drm", cls.TrainParams.from_dict(train_params).metric_type)
        if not isinstance(Y, DeviceMatrix):
            raise ValueError("type(Y) should be a DeviceMatrix.")
        n, n_label = Y.shape
        tcrow, tcol, tval, _ = Y.transpose(stream=stream).to_torch(stream=stream)
        dev = tcrow.device
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream().cuda_stream if stream is None else stream
            if isinstance(X, DeviceMatrix):
                crow, col, val, (rows, cols) = X.to_torch(stream=stream)
                x_args, data_type = (val.data_ptr(), 0, crow.data_ptr(), col.data_ptr(), val.numel()), "csr"
            elif torch.is_tensor(X) and X.is_cuda and X.dtype == torch.float32 and X.dim() == 2:
                X = X if (X.shape[1] <= 1 or X.stride(1) == 1) and (X.shape[0] <= 1 or X.stride(0) >= X.shape[1]) else X.contiguous()
                rows, cols = X.shape
                x_args, data_type = (X.data_ptr(), X.stride(0) if rows > 1 else max(cols, 1), 0, 0, 0), "drm"
            else:
                raise ValueError("type(X)={} is NOT supported!".format(type(X)))
            if rows != n:
                raise ValueError("X_trn.rows != Y_csc.rows")
            h = clib.pairwise_from_device(dev.index, rows, n_label, cols, *x_args, tcrow.data_ptr(), tcol.data_ptr(), tval.data_ptr(), tval.numel(), stream=s or None)
        return cls(h, rows, n_label, cols, data_type, pred_params)

    @classmethod
    def load(cls, model_folder, lazy_load=False, device=0):
        """``lazy_load`` is accepted and ignored: the index is copied to HBM."""
        with open("{}/param.json".format(model_folder), "r") as fin:
            param = json.loads(fin.read())
        if param["model"] != cls.__name__:
            raise ValueError("param[model] != cls.__name__")
        if not ("data_type" in param and "metric_type" in param):
            raise ValueError("param.json did not have data_type or metric_type!")
        if param["data_type"] not in ("drm", "csr"):
            raise NotImplementedError("data_type={} and metric_type={} not implemented".format(param["data_type"], param["metric_type"]))
        cls._check_metric(param["data_type"], param["metric_type"])
        c_model_dir = f"{model_folder}/c_model"
        if not os.path.isdir(c_model_dir):
            raise ValueError(f"c_model_dir did not exist: {c_model_dir}")
        model = cls(clib.pairwise_load(c_model_dir, device), param["num_input_keys"], param["num_label_keys"], param["feat_dim"], param["data_type"], param["pred_kwargs"])
        if model.info["data_type"] != param["data_type"]:
            raise ValueError("param.json says {}, c_model/config.json says {}".format(param["data_type"], model.info["data_type"]))
        return model

    def save(self, model_folder):
        os.makedirs(model_folder, exist_ok=True)
        param = {"model": self.__class__.__name__, "data_type": self.data_type, "metric_type": self.metric_type, "num_input_keys": self.num_input_keys,
                 "num_label_keys": self.num_label_keys, "feat_dim": self.feat_dim, "pred_kwargs": self.pred_params.to_dict()}
        with open("{}/param.json".format(model_folder), "w") as fout:
            fout.write(json.dumps(param, indent=True))
        clib.pairwise_save(self.model_ptr, f"{model_folder}/c_model")

    def get_pred_params(self):
        return self.PredParams.from_dict(self.pred_params)

    def searchers_create(self, pred_params=None, num_searcher=1):
        if not self.model_ptr:
            raise ValueError("self.model_ptr must exist before using searchers_create()")
        if num_searcher <= 0:
            raise ValueError("num_searcher={} <= 0 is NOT valid".format(num_searcher))
        return PairwiseANN.Searchers(self, self.get_pred_params() if pred_params is None else pred_params, num_searcher)

    def predict(self, input_feat, label_keys, searchers, is_same_input=False):
        """-> ``(Imat, Mmat, Dmat, Vmat)``, each ``[batch, only_topk]``: views of the searchers' arrays, as the reference returns them."""
        input_feat_py, data_type = self.create_pymat(input_feat)
        if data_type != self.data_type:
            raise ValueError("data_type={} is NOT consistent with self.data_type={}".format(data_type, self.data_type))
        if input_feat_py.cols != self.feat_dim:
            raise ValueError("input_feat_py.cols={} is NOT consistent with self.feat_dim={}".format(input_feat_py.cols, self.feat_dim))
        if not isinstance(label_keys, np.ndarray):
            raise TypeError("type(label_keys) != np.array")
        if not is_same_input and input_feat_py.rows != label_keys.shape[0]:
            raise ValueError("input_feat_py.rows != label_keys.shape[0]")
        cur_bsz = label_keys.shape[0]
        if cur_bsz > searchers.pred_params.batch_size:
            raise ValueError("cur_batch_size > searchers.batch_size!")
        only_topk = searchers.pred_params.only_topk
        cur_nnz = cur_bsz * only_topk
        searchers.reset(cur_nnz)
        keys = np.ascontiguousarray(label_keys, dtype=np.uint32)
        clib.pairwise_predict(self.model_ptr, searchers.ctypes(), cur_bsz, only_topk, input_feat_py, data_type, keys, searchers.Imat, searchers.Mmat, searchers.Dmat,
                              searchers.Vmat, is_same_input)
        return tuple(m[:cur_nnz].reshape(cur_bsz, only_topk) for m in (searchers.Imat, searchers.Mmat, searchers.Dmat, searchers.Vmat))


def pairwise_predict_device(model, Q, label_keys, only_topk=None, is_same_input=False, searchers=None, stream=None):
    """The resident form.  ``Q``: a CUDA float32 tensor ``[rows, feat_dim]`` (dense index; last dimension contiguous, any row stride), a CSR
    ``(crow int64, col int32, val float32)`` of CUDA tensors or a :class:`DeviceMatrix` (sparse index); ``label_keys``: a CUDA int32 tensor
    ``[batch]``.  Returns ``(Imat int32, Mmat int32, Dmat float32, Vmat float32)``, each ``[batch, only_topk]`` in HBM: pair ``b`` holds its
    entries nearest first, and zeros after them."""
    import torch
    from .features import DeviceMatrix
    only_topk = model.pred_params.only_topk if only_topk is None else only_topk
    if isinstance(Q, DeviceMatrix):
        Q = Q.to_torch(stream=stream)
    sparse = isinstance(Q, (tuple, list))
    if sparse:
        crow, col, val = (t.contiguous() for t in Q[:3])
        if not (crow.is_cuda and crow.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32 and crow.numel() >= 1 and col.numel() == val.numel()):
            raise ValueError("pairwise_predict_device: a CSR is (crow int64, col int32, val float32) of CUDA tensors")
        rows, cols = crow.numel() - 1, (tuple(Q[3])[1] if len(Q) == 4 else model.feat_dim)
        q_args = (val.data_ptr(), 0, crow.data_ptr(), col.data_ptr(), val.numel())
        dev = val.device
    elif torch.is_tensor(Q) and Q.is_cuda and Q.dtype == torch.float32 and Q.dim() == 2:
        Q = Q if (Q.shape[1] <= 1 or Q.stride(1) == 1) and (Q.shape[0] <= 1 or Q.stride(0) >= Q.shape[1]) else Q.contiguous()
        rows, cols = Q.shape
        q_args = (Q.data_ptr(), Q.stride(0) if rows > 1 else max(cols, 1), 0, 0, 0)
        dev = Q.device
    else:
        raise ValueError("type(X)={} is NOT supported!".format(type(Q)))
    if ("csr" if sparse else "drm") != model.data_type:
        raise ValueError("data_type={} is NOT consistent with self.data_type={}".format("csr" if sparse else "drm", model.data_type))
    if cols != model.feat_dim:
        raise ValueError("input_feat_py.cols={} is NOT consistent with self.feat_dim={}".format(cols, model.feat_dim))
    if not (torch.is_tensor(label_keys) and label_keys.is_cuda and label_keys.dtype == torch.int32 and label_keys.dim() == 1):
        raise TypeError("pairwise_predict_device: label_keys is a CUDA int32 tensor [batch]")
    if not is_same_input and rows != label_keys.shape[0]:
        raise ValueError("input_feat_py.rows != label_keys.shape[0]")
    batch = label_keys.shape[0]
    keys = label_keys.contiguous()
    with torch.cuda.device(dev), (torch.cuda.stream(torch.cuda.ExternalStream(stream)) if stream else contextlib.nullcontext()):
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        out = [torch.zeros((batch, only_topk), dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.float32, torch.float32)]
        clib.pairwise_predict_device(model.model_ptr, None if searchers is None else searchers.ctypes(), batch, only_topk, rows, cols, *q_args, keys.data_ptr(),
                                     *(t.data_ptr() for t in out), only_topk, is_same_input, stream=s or None)
    return tuple(out)
