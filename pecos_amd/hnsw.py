"""``pecos.ann.hnsw.HNSW`` with its graph built on the MI355X (K19): ``train`` and ``train_device`` run the reference's construction at
``threads = 1`` in HBM, ``save`` writes the reference's folder, and the loader and search surface are :class:`pecos_amd.ann.HNSW`'s.

A saved folder has the ``c_model/index.mmap_store`` and ``c_model/config.json`` of the reference's ``HNSW.train(...).save(...)`` on the same
items, byte for byte (sparse indexes on any x86 host, dense indexes the reference's avx512f clone).  This is the served
class; ``pecos_amd.ann.HNSW`` keeps its pinned refusals, as ``pecos_amd.pairwise.PairwiseANN`` stands beside ``pecos_amd.ann.PairwiseANN``."""
import json
import os

from . import ann
from .core import clib

__all__ = ["HNSW"]


class HNSW(ann.HNSW):
    """The reference's ``pecos.ann.hnsw.HNSW`` surface: train, save, load, predict."""

    @classmethod
    def train(cls, X, train_params=None, pred_params=None, device=0):
        """``threads`` is accepted and ignored: the graph is the reference's at ``threads = 1``."""
        train_params = cls.TrainParams.from_dict(train_params)
        pred_params = cls.PredParams.from_dict(pred_params)
        pX, data_type = cls.create_pymat(X)
        h = clib.hnsw_train(pX, data_type, train_params.M, train_params.efC, train_params.threads, train_params.max_level_upper_bound, train_params.metric_type, device)
        return cls(h, pX.rows, pX.cols, data_type, train_params.metric_type, pred_params)

    @classmethod
    def train_device(cls, X, train_params=None, pred_params=None, stream=None):
        """The resident build.  ``X``: a CUDA float32 tensor ``[N, feat_dim]`` (dense index; the last dimension contiguous, any row stride), a CSR
        ``(crow int64, col int32, val float32, (rows, cols))`` of CUDA tensors or a :class:`DeviceMatrix` (sparse index).  The items are copied
        device to device into the index; nothing visits the host."""
        import torch
        from .features import DeviceMatrix
        train_params = cls.TrainParams.from_dict(train_params)
        pred_params = cls.PredParams.from_dict(pred_params)
        tp = (train_params.M, train_params.efC, train_params.threads, train_params.max_level_upper_bound, train_params.metric_type)
        if isinstance(X, DeviceMatrix):
            rows, cols = X.shape
            dev = X.info["device"]
            with torch.cuda.device(dev):
                s = torch.cuda.current_stream().cuda_stream if stream is None else stream
                h = clib.hnsw_train_device(dev, 0, 0, 0, 0, 0, 0, 0, X.handle, *tp, stream=s or None)
            return cls(h, rows, cols, "csr", train_params.metric_type, pred_params)
        if isinstance(X, (tuple, list)):
            if len(X) != 4:
                raise ValueError("HNSW.train_device: a CSR is (crow, col, val, (rows, cols))")
            crow, col, val = (t.contiguous() for t in X[:3])
            if not (crow.is_cuda and crow.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32 and col.numel() == val.numel()):
                raise ValueError("HNSW.train_device: a CSR triple is (crow int64, col int32, val float32) of CUDA tensors")
            rows, cols = (int(v) for v in X[3])
            if crow.numel() != rows + 1:
                raise ValueError("HNSW.train_device: crow has {} entries, the shape says {} rows".format(crow.numel(), rows))
            args, data_type, dev = (val.data_ptr(), 0, crow.data_ptr(), col.data_ptr(), val.numel()), "csr", val.device
        elif torch.is_tensor(X) and X.is_cuda and X.dtype == torch.float32 and X.dim() == 2:
            X = X if (X.shape[1] <= 1 or X.stride(1) == 1) and (X.shape[0] <= 1 or X.stride(0) >= X.shape[1]) else X.contiguous()
            rows, cols = X.shape
            args, data_type, dev = (X.data_ptr(), X.stride(0) if rows > 1 else max(cols, 1), 0, 0, 0), "drm", X.device
        else:
            raise ValueError("type(X)={} is NOT supported!".format(type(X)))
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream().cuda_stream if stream is None else stream
            h = clib.hnsw_train_device(dev.index, rows, cols, *args, None, *tp, stream=s or None)
        return cls(h, rows, cols, data_type, train_params.metric_type, pred_params)

    def save(self, model_folder):
        """``param.json`` as the reference writes it, and ``c_model/``."""
        os.makedirs(model_folder, exist_ok=True)
        meta = "pecos.ann.hnsw.model###HNSW"
        param = {"__meta__": {"class_fullname": meta}, "model": "HNSW", "data_type": self.data_type, "metric_type": self.metric_type, "num_item": self.num_item,
                 "feat_dim": self.feat_dim, "pred_kwargs": dict({"__meta__": {"class_fullname": meta + ".PredParams"}}, **self.pred_params.to_dict())}
        with open("{}/param.json".format(model_folder), "w") as fout:
            fout.write(json.dumps(param, indent=True))
        clib.hnsw_save(self.model_ptr, f"{model_folder}/c_model")
