"""``XLinearModel`` -- the reference's user-facing XR-Linear API for the inference path, running
on MI355X through ``libxrl_amd.so``.

Surface kept from the reference (same names, kwargs and error behaviour):

* ``XLinearModel.load(model_folder, is_predict_only=True, **kwargs)``   pecos/xmc/xlinear/model.py:105-134
* ``XLinearModel.predict(X, pred_params=None, **kwargs)``               pecos/xmc/xlinear/model.py:480-550
  kwargs: beam_size, only_topk, post_processor, threads, max_pred_chunk
* ``HierarchicalMLModel.{load, predict, get_pred_params, PredParams}``  pecos/xmc/base.py:1090-1680
* ``MLModel.PredParams``                                                pecos/xmc/base.py:640-678

* ``MLProblem``, ``MLModel.{TrainParams, train, save}``, ``HierarchicalMLModel.{TrainParams, train, save}``,
  ``XLinearModel.{TrainParams, train, save}``                           pecos/xmc/base.py:488-880, 1371-1572
  training on the device (K13): a trained model predicts natively and saves the reference's folder layout
* ``XLinearModel.train_ext``: the reference's ``XLinearModel.train`` with relevance induction, user-supplied negatives and the
  ``matcher`` / ``ranker`` modes                                          pecos/xmc/xlinear/model.py:219-283

Pruning and the python (non predict-only) model chain stay in the reference: loading with
``is_predict_only=False`` raises ``NotImplementedError``, and a loaded model cannot be saved.
"""
import copy
import dataclasses as dc
import json
import os
import types
from glob import glob
from os import path

import numpy as np
import scipy.sparse as smat

from .core import ScipyCompressedSparseAllocator, ScipyCscF32, ScipyCsrF32, ScipyDrmF32, clib
from .training import _per_layer

VALID_POST_PROCESSORS = ["noop", "sigmoid", "log-sigmoid"] + \
    [f"l{p}-hinge" for p in range(1, 5)] + [f"log-l{p}-hinge" for p in range(1, 5)]  # xmc/base.py:456-475


class BaseParams:
    """Dataclass <-> dict helper with the reference's semantics (pecos/__init__.py:47-100)."""

    @classmethod
    def from_dict(cls, param=None):
        if param is None:
            return cls()
        if isinstance(param, cls):
            return copy.deepcopy(param)
        if isinstance(param, dict):
            names = {f.name for f in dc.fields(cls)}
            return cls(**{k: v for k, v in param.items() if k in names})
        raise ValueError(f"{type(param)} is not supported for {cls.__name__}.from_dict")

    def to_dict(self, with_meta=True):
        d = {}
        for f in dc.fields(self):
            v = getattr(self, f.name)
            if isinstance(v, BaseParams):
                v = v.to_dict(with_meta)
            elif isinstance(v, (list, tuple)):
                v = [x.to_dict(with_meta) if isinstance(x, BaseParams) else x for x in v]
            d[f.name] = v
        return d


class MLModel:
    @dc.dataclass
    class PredParams(BaseParams):
        only_topk: int = 20
        post_processor: str = "l3-hinge"

        def override_with_kwargs(self, pred_kwargs):
            if pred_kwargs is not None:
                if not isinstance(pred_kwargs, dict):
                    raise TypeError("type(pred_kwargs) must be dict")
                for k, v in pred_kwargs.items():
                    if k in ("only_topk", "post_processor") and v is not None:
                        setattr(self, k, v)
            return self

    @classmethod
    def load_pred_params(cls, folder):
        param = json.loads(open(f"{folder}/param.json", "r", encoding="utf-8").read())
        return cls.PredParams.from_dict(param["pred_kwargs"])

    @dc.dataclass
    class TrainParams(BaseParams):
        """pecos/xmc/base.py:616-647, the same names and defaults."""
        threshold: float = 0.1
        max_nonzeros_per_label: int = None  # type: ignore
        solver_type: str = "L2R_L2LOSS_SVC_DUAL"
        Cp: float = 1.0
        Cn: float = 1.0
        max_iter: int = 100
        eps: float = 0.1
        bias: float = 1.0
        threads: int = -1
        verbose: int = 0
        newton_eps: float = 0.01

    def __init__(self, W=None, C=None, bias=-1.0, pred_params=None, **kwargs):
        """One trained layer on the host: W ((features + (bias > 0)) x labels, CSC), C (labels x codes, CSC)."""
        self.W, self.C, self.bias = W, C, bias
        self.pred_params = self.PredParams.from_dict(pred_params)

    @property
    def nr_labels(self):
        return self.W.shape[1]

    @property
    def nr_codes(self):
        return self.C.shape[1]

    @property
    def nr_features(self):
        return self.W.shape[0] - (1 if self.bias > 0 else 0)

    @classmethod
    def train(cls, prob, train_params=None, pred_params=None, **kwargs):
        """One layer trained on the device (K13, or K16 for ``L2R_L2LOSS_SVC_PRIMAL``, which stops at ``newton_eps`` as in
        pecos/xmc/base.py:868-870; ``clib.xlinear_single_layer_train``) from an :class:`MLProblem`."""
        train_params = cls.TrainParams.from_dict(kwargs if train_params is None else train_params)
        if train_params.solver_type == "L2R_L2LOSS_SVC_PRIMAL":
            train_params.eps = train_params.newton_eps
        pred_params = cls.PredParams.from_dict(pred_params)
        pred_params.override_with_kwargs(kwargs.get("pred_kwargs", None))
        if pred_params.post_processor not in VALID_POST_PROCESSORS:
            raise ValueError("pred_params is not valid!")
        W = clib.xlinear_single_layer_train(prob.pX, prob.pY, prob.pC, prob.pM, prob.pR, **train_params.to_dict())
        return cls(W=W, C=prob.C, bias=train_params.bias, pred_params=pred_params)

    def get_pred_params(self):
        return copy.deepcopy(self.pred_params)

    def predict(self, X, csr_codes=None, pred_params=None, **kwargs):
        """This layer's prediction of ``X`` (csr_matrix or ndarray, float32), with ``csr_codes`` (instances x codes) the prediction of
        the layers above (pecos/xmc/base.py:890-949), through ``clib.xlinear_single_layer_predict``: a csr_matrix instances x labels, rows
        best first.  ``only_topk`` / ``post_processor`` keywords override ``pred_params``."""
        if X.shape[1] != self.nr_features:
            raise ValueError("Feature dimension of query matrix does not match weight matrix")
        pred_params = self.get_pred_params() if pred_params is None else self.PredParams.from_dict(pred_params)
        pred_params.override_with_kwargs(kwargs)
        if pred_params.post_processor not in VALID_POST_PROCESSORS:
            raise ValueError("pred_params is not valid!")
        pred_alloc = ScipyCompressedSparseAllocator()
        clib.xlinear_single_layer_predict(X, csr_codes, self.W, self.C, pred_params.post_processor, pred_params.only_topk if pred_params.only_topk else 0,
                                          kwargs.get("threads", -1), self.bias, pred_alloc)
        return pred_alloc.get()

    @classmethod
    def load(cls, folder):
        """A layer folder written by :meth:`save` here or by the reference: W and C as float32 CSC on the host."""
        param = json.loads(open(f"{folder}/param.json", "r", encoding="utf-8").read())
        W, C = (smat.csc_matrix(smat.load_npz(f"{folder}/{name}.npz"), dtype=np.float32) for name in ("W", "C"))
        return cls(W=W, C=C, bias=param["bias"], pred_params=param["pred_kwargs"])

    def save(self, folder):
        """The reference's layer folder (pecos/xmc/base.py:807-830): param.json, W.npz, C.npz."""
        os.makedirs(folder, exist_ok=True)
        param = {"__meta__": {"class_fullname": "pecos.xmc.base###MLModel"}, "model": "MLModel", "nr_labels": self.nr_labels, "nr_features": self.nr_features,
                 "nr_codes": self.nr_codes, "bias": self.bias, "pred_kwargs": self.pred_params.to_dict()}
        with open(f"{folder}/param.json", "w", encoding="utf-8") as f:
            f.write(json.dumps(param, indent=True))
        smat.save_npz(f"{folder}/W.npz", smat.csc_matrix(self.W, dtype=np.float32), compressed=False)
        smat.save_npz(f"{folder}/C.npz", smat.csc_matrix(self.C, dtype=np.float32), compressed=False)


def _ones_column(rows):
    """rows x 1, every entry stored with value 1: the one cluster every label (or instance) belongs to when no clustering is given."""
    return smat.csc_matrix((np.ones(rows, dtype=np.float32), np.arange(rows), np.array([0, rows])), shape=(rows, 1))


def _every_entry_csr(D):
    """A dense float32 array as the CSR that stores every entry, zeros included: what the dense training entry point trains on."""
    rows, cols = D.shape
    ids = np.int32 if D.size < 2 ** 31 else np.int64
    return smat.csr_matrix((np.ascontiguousarray(D).reshape(-1), np.tile(np.arange(cols, dtype=ids), rows), np.arange(rows + 1, dtype=ids) * cols), shape=D.shape)


def _csc_f32(A):
    """A sparse matrix as float32 CSC (a float32 CSC as it is, stored order kept)."""
    return A if isinstance(A, smat.csc_matrix) and A.dtype == np.float32 else A.tocsc().astype(np.float32)


def check_relevance(Y, R):
    """ValueError unless ``R`` stores exactly the entries of the label matrix ``Y`` (both read as float32 CSC) and no negative value."""
    labels, relevance = _csc_f32(Y), _csc_f32(R)
    for part in ("indptr", "indices"):
        if not np.array_equal(getattr(labels, part), getattr(relevance, part)):
            raise ValueError(f"Invalid relevance matrix: Y.{part} != R.{part}")
    if relevance.nnz and relevance.data.min() < 0:
        raise ValueError("Invalid relevance matrix: got value < 0")


class MLProblem(object):
    """The five matrices of one layer's training as the views the native call takes: ``pX`` (instances x features; CSR or dense),
    ``pY`` (instances x labels), ``pC`` (labels x clusters), ``pM`` (instances x clusters: whom a cluster's labels train against) and
    ``pR`` (the cost of every positive, or None), the last four column-major float32.  What is not given is filled in as the reference
    fills it in (pecos/xmc/base.py, MLProblem): without ``C`` all labels share one cluster; without ``M`` an instance is matched to
    the clusters of its own labels -- the pattern of ``Y * C``, by the device sparse product -- or, under a single cluster, to that
    cluster.  ``R`` must store exactly Y's entries and no negative value.  ``threads`` is accepted and ignored."""

    def __init__(self, X, Y, C=None, M=None, R=None, threads=8):
        self.dtype = np.float32
        self.pX = self._feature_view(X)
        labels = self._column_major("Y", Y)
        n_inst, n_labels = labels.shape
        clusters = _ones_column(n_labels) if C is None else self._column_major("C", C)
        if clusters.shape[0] != n_labels:
            raise ValueError(f"C has {clusters.shape[0]} rows, Y has {n_labels} labels")
        if M is not None:
            matching = self._column_major("M", M)
            if matching.shape != (n_inst, clusters.shape[1]):
                raise ValueError(f"M has shape {matching.shape}, Y and C need {(n_inst, clusters.shape[1])}")
        elif clusters.shape[1] > 1:
            matching = smat.csc_matrix(clib.sparse_matmul(labels, clusters), dtype=np.float32)
        else:
            matching = _ones_column(n_inst)
        if not matching.has_sorted_indices:
            matching = matching.sorted_indices()                      # (a copy: the caller's matrix stays as it is)
        relevance = None if R is None else self._column_major("R", R)
        if relevance is not None:
            check_relevance(labels, relevance)
        self.pY, self.pC, self.pM = (ScipyCscF32.init_from(A) for A in (labels, clusters, matching))
        self.pR = None if relevance is None else ScipyCscF32.init_from(relevance)

    def _feature_view(self, X):
        if isinstance(X, (ScipyCsrF32, ScipyDrmF32)):
            return X
        if X.dtype != self.dtype:
            raise ValueError(f"X must be float32, got {X.dtype}")
        if isinstance(X, smat.csr_matrix):
            return ScipyCsrF32(X)
        if isinstance(X, np.ndarray):
            return ScipyDrmF32(X)
        raise NotImplementedError("type(X) = {} is not supported.".format(type(X)))

    def _column_major(self, name, A):
        """A view's own matrix, or a sparse matrix as float32 CSC (a float32 CSC as it is, stored order kept)."""
        if isinstance(A, ScipyCscF32):
            return A.buf
        if not smat.issparse(A):
            raise NotImplementedError("type({}) = {} is not supported.".format(name, type(A)))
        return _csc_f32(A)

    X = property(lambda self: self.pX.buf)
    Y = property(lambda self: self.pY.buf)
    C = property(lambda self: self.pC.buf)
    M = property(lambda self: self.pM.buf)
    R = property(lambda self: None if self.pR is None else self.pR.buf)
    nr_labels = property(lambda self: self.pY.buf.shape[1])


class HierarchicalMLModel:
    """Predict-only hierarchical model: ``model_chain`` is the native handle (an int)."""

    @dc.dataclass
    class PredParams(BaseParams):
        model_chain: MLModel.PredParams = None  # type: ignore

        def __len__(self):
            return len(self.model_chain)

        @classmethod
        def from_dict(cls, param=None):
            if param is None:
                return cls()
            if isinstance(param, cls):
                return copy.deepcopy(param)
            chain = param.get("model_chain") if isinstance(param, dict) else None
            if isinstance(chain, (list, tuple)):
                chain = [MLModel.PredParams.from_dict(c) for c in chain]
            elif chain is not None:
                chain = MLModel.PredParams.from_dict(chain)
            return cls(model_chain=chain)

        def override_with_kwargs(self, pred_kwargs):
            # xmc/base.py:1140-1173: beam_size -> every layer but the last, only_topk -> last layer
            if pred_kwargs is None:
                return self
            if not isinstance(pred_kwargs, dict):
                raise TypeError("type(pred_kwargs) must be dict")
            beam = pred_kwargs.get("beam_size", None)
            topk = pred_kwargs.get("only_topk", None)
            pp = pred_kwargs.get("post_processor", None)
            if isinstance(self.model_chain, (list, tuple)):
                depth = len(self.model_chain)
                for d in range(depth):
                    if beam and d < depth - 1:
                        self.model_chain[d].only_topk = beam
                    if topk and d == depth - 1:
                        self.model_chain[d].only_topk = topk
                    if pp:
                        self.model_chain[d].post_processor = pp
            elif isinstance(self.model_chain, MLModel.PredParams):
                if topk:
                    self.model_chain.only_topk = topk
                if pp:
                    self.model_chain.post_processor = pp
            return self

    def __init__(self, model_chain, pred_params=None, is_predict_only=True, **kwargs):
        if not isinstance(model_chain, int):
            raise NotImplementedError("pecos_amd only wraps native (predict-only) model handles")
        self.model_chain = model_chain
        self.pred_params = self.PredParams.from_dict(pred_params)
        self.pred_params.override_with_kwargs(kwargs.get("pred_kwargs", None))
        self.is_predict_only = True

    def __del__(self):
        try:
            if getattr(self, "model_chain", None):
                clib.xlinear_destruct_model(self.model_chain)
                self.model_chain = None
        except Exception:
            pass

    @property
    def depth(self):
        return clib.xlinear_get_int_attr(self.model_chain, "depth")

    @property
    def nr_features(self):
        return clib.xlinear_get_int_attr(self.model_chain, "nr_features")

    @property
    def nr_codes(self):
        return clib.xlinear_get_int_attr(self.model_chain, "nr_codes")

    @property
    def nr_labels(self):
        return clib.xlinear_get_int_attr(self.model_chain, "nr_labels")

    @property
    def nr_pred_cols(self):
        """Column count of predict()'s CSR (== C.rows of the last layer; differs from nr_labels only
        for pruned trees, inference.hpp:1776-1784)."""
        return clib.xlinear_get_int_attr(self.model_chain, "nr_pred_cols")

    def get_pred_params(self):
        return copy.deepcopy(self.pred_params)

    def set_output_constraint(self, labels_to_keep):
        """Restrict predict() to the labels in ``labels_to_keep`` (xmc/base.py:1796-1824) -- here on the loaded, predict-only handle: the
        result equals a model whose C matrices were pruned by the reference's rule, saved and reloaded.  Any iterable of ints; a torch
        integer tensor on the model's device is read where it is (no host copy); ``None`` clears the constraint, and so does a set
        that covers every label.  Synchronous; not to be called while a predict of this model is running."""
        if labels_to_keep is None:
            clib.clear_output_constraint(self.model_chain)
            return
        if type(labels_to_keep).__module__.split(".")[0] == "torch" and hasattr(labels_to_keep, "data_ptr"):
            import torch
            t = labels_to_keep
            if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
                raise TypeError("can not convert labels_to_keep as set variable type!")
            if t.is_cuda and t.device.index == clib.xlinear_get_int_attr(self.model_chain, "device"):
                t = t.reshape(-1)
                if t.numel() and (int(t.min()) < 0 or int(t.max()) > 0xFFFFFFFF):
                    raise ValueError("labels_to_keep holds an id outside [0, 2^32)")
                # (the ids travel as 32-bit words: a reinterpreting view of an int32 tensor, a converted copy -- on the device -- of any other)
                t32 = t.contiguous() if t.dtype == torch.int32 else t.to(torch.int64).bitwise_and(0xFFFFFFFF).to(torch.int32).contiguous()
                stream = torch.cuda.current_stream(t.device).cuda_stream
                clib.set_output_constraint_device(self.model_chain, t32.data_ptr(), t32.numel(), stream=stream)
                return
            labels_to_keep = t.detach().cpu().reshape(-1).tolist()
        try:
            labels_to_keep = set(labels_to_keep)
        except TypeError:
            raise TypeError("can not convert labels_to_keep as set variable type!")
        ids = np.fromiter((int(v) for v in labels_to_keep), dtype=np.int64, count=len(labels_to_keep))
        if ids.size and (ids.min() < 0 or ids.max() > 0xFFFFFFFF):
            raise ValueError("labels_to_keep holds an id outside [0, 2^32)")
        clib.set_output_constraint(self.model_chain, ids.astype(np.uint32))

    @classmethod
    def load(cls, model_folder, is_predict_only=True, **kwargs):
        param = json.loads(open(f"{model_folder}/param.json", "r", encoding="utf-8").read())
        assert param["model"] == cls.__name__
        depth = int(param.get("depth", len(glob("{}/*.model".format(model_folder)))))
        if not is_predict_only:
            raise NotImplementedError(
                "pecos_amd accelerates the predict-only path; load with is_predict_only=True "
                "(training / pruning stay in the reference's CPU code)")
        if bool(param.get("is_mmap", False)):
            model = clib.xlinear_load_mmap(model_folder, **kwargs)
        else:
            model = clib.xlinear_load_predict_only(model_folder, **kwargs)
        pred_params = cls.PredParams(
            model_chain=[MLModel.load_pred_params(f"{model_folder}/{d}.model") for d in range(depth)])
        loaded = cls(model, pred_params=pred_params, is_predict_only=True)
        top = f"{model_folder}/0.model/C.npz"
        if not bool(param.get("is_mmap", False)) and path.exists(top) and smat.load_npz(top).shape[1] > 1:
            # a top layer of several clusters (a ranker-mode model): the beam search has no single root to start from; such a model
            # predicts layer by layer, the top layer without codes, as the reference's python path does
            loaded.layerwise = [MLModel.load(f"{model_folder}/{d}.model") for d in range(depth)]
        return loaded

    @dc.dataclass
    class TrainParams(BaseParams):
        """pecos/xmc/base.py:1101-1113: the negative sampling scheme and the solver parameters, one per layer or one for all."""
        neg_mining_chain: str = "tfn"
        model_chain: MLModel.TrainParams = None  # type: ignore

        @classmethod
        def from_dict(cls, param=None):
            if param is None:
                return cls()
            if isinstance(param, cls):
                return copy.deepcopy(param)
            chain = param.get("model_chain")
            chain = [MLModel.TrainParams.from_dict(c) for c in chain] if isinstance(chain, (list, tuple)) else MLModel.TrainParams.from_dict(chain)
            return cls(neg_mining_chain=param.get("neg_mining_chain", "tfn"), model_chain=chain)

    @classmethod
    def train(cls, prob, clustering=None, relevance_chain=None, matching_chain=None, train_params=None, pred_params=None, **kwargs):
        """The layers of a cluster chain (root first; None: one layer from the problem's own C and M, one-versus-all by default) trained on the device, top down
        (pecos/xmc/base.py:1412-1572), through :func:`pecos_amd.train_chain_device`: X (sparse, or dense as the CSR of all its entries), Y,
        the label chain ``Y * C_last * ... * C_(t+1)``, the matching matrices and the weights stay in HBM until the last layer is done, and
        the weights are downloaded once.  A layer's negatives are the instances matched to a label's cluster: ``tfn`` = the layer above's
        labels (teacher forcing), ``usn`` = ``matching_chain[t]``, or both.  A scheme with ``man`` (matcher-aware negatives) raises
        ``NotImplementedError`` here; :meth:`train_device` serves it.  Returns a model that predicts natively and can be saved."""
        return cls._train(False, prob, clustering, relevance_chain, matching_chain, train_params, pred_params, kwargs)

    @classmethod
    def train_device(cls, prob, clustering=None, relevance_chain=None, matching_chain=None, train_params=None, pred_params=None, **kwargs):
        """:meth:`train` with every scheme that is a sum of ``tfn``, ``usn`` and ``man`` (matcher-aware negatives: the layers trained so far
        predict X on the device and their prediction joins the next layer's matching matrix)."""
        return cls._train(True, prob, clustering, relevance_chain, matching_chain, train_params, pred_params, kwargs)

    @classmethod
    def _train(cls, serves_man, prob, clustering, relevance_chain, matching_chain, train_params, pred_params, kwargs):
        from .training import train_chain_device
        chain, depth, schemes, layer_params, pp = cls._training_setup(prob, clustering, train_params, pred_params, kwargs, serves_man)
        if chain[0] is None:                                 # one layer from the problem as it stands, as MLModel.train(prob) reads it
            relevance_chain, matching_chain = (None if prob.R is None else [prob.R]), None
            if prob.C.shape[1] > 1:                          # the problem's own clusters and matching matrix
                chain, matching_chain, schemes = [prob.C], [prob.M], ["usn"]
            elif prob.C.nnz != prob.nr_labels or prob.M.nnz != prob.Y.shape[0]:
                raise NotImplementedError("a one-versus-all layer from a problem whose single cluster leaves out a label, or whose M leaves out "
                                          "an instance, is not served on the device")
        X = prob.X if isinstance(prob.pX, ScipyCsrF32) else _every_entry_csr(prob.X)
        weights = train_chain_device(X, prob.Y, chain, schemes, matching_chain, relevance_chain, layer_params, pp.model_chain)
        return cls._from_weights(weights, [prob.C if C is None else C for C in chain], layer_params, pp)

    @classmethod
    def _from_weights(cls, weights, chain, layer_params, pp):
        """The model of a layer loop's resident weights (W^T per layer) over the host chain: the weights are downloaded once."""
        layers = []
        for t, wt in enumerate(weights):
            Wt = wt.download()                               # labels x (features + (bias > 0)) in CSR = the CSC arrays of W
            W = smat.csc_matrix((Wt.data, Wt.indices, Wt.indptr), shape=(Wt.shape[1], Wt.shape[0]), dtype=np.float32)
            layers.append(MLModel(W=W, C=chain[t], bias=layer_params[t].bias, pred_params=pp.model_chain[t]))
        return cls._from_layers(layers, pp)

    @classmethod
    def _training_setup(cls, prob, clustering, train_params, pred_params, kwargs, serves_man):
        """What :meth:`train` and :meth:`train_device` resolve, and refuse, before anything reaches a device: the chain as float32 CSC
        (``[None]``: one one-versus-all layer), its depth, the per-layer schemes, solver parameters and the prediction parameters.
        ``serves_man`` False refuses a scheme with ``man``."""
        chain = [None] if clustering is None or clustering is False else [smat.csc_matrix(C, dtype=np.float32) for C in clustering]
        depth = len(chain)
        if chain[0] is not None and chain[-1].shape[0] != prob.nr_labels:
            raise ValueError(f"the bottom clustering matrix has {chain[-1].shape[0]} rows, the problem {prob.nr_labels} labels")
        if train_params is None:
            tp = cls.TrainParams(neg_mining_chain=kwargs.get("negative_sampling_scheme", "tfn"), model_chain=MLModel.TrainParams.from_dict(kwargs))
        else:
            tp = cls.TrainParams.from_dict(train_params)
            if tp.neg_mining_chain is None:
                tp.neg_mining_chain = kwargs.get("negative_sampling_scheme", "tfn")
        schemes = [s.lower() for s in _per_layer(tp.neg_mining_chain, depth, "neg_mining_chain")]
        layer_params = _per_layer(tp.model_chain if tp.model_chain is not None else MLModel.TrainParams(), depth, "model_chain")
        for s in schemes:
            if "man" in s and not serves_man:
                raise NotImplementedError(f"negative sampling scheme '{s}': matcher-aware negatives (man) need a prediction of the half-trained chain, "
                                          "which this library does not run during training; use tfn, usn or tfn+usn")
        pp = cls.PredParams(model_chain=MLModel.PredParams()) if pred_params is None else cls.PredParams.from_dict(pred_params)
        pp.model_chain = _per_layer(pp.model_chain if pp.model_chain is not None else MLModel.PredParams(), depth, "pred_params.model_chain")
        pp.override_with_kwargs(kwargs.get("pred_kwargs", None))
        for p in pp.model_chain:
            if p.post_processor not in VALID_POST_PROCESSORS:
                raise ValueError("pred_params is not valid!")
        return chain, depth, schemes, layer_params, pp

    @classmethod
    def _from_layers(cls, layers, pred_params):
        """Trained layers as a model: written once in the reference's layout and loaded natively; the layers stay for :meth:`save`."""
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            cls._write(tmp, layers)
            model = cls.load(tmp)
        model.layers = layers
        model.pred_params = pred_params
        return model

    @staticmethod
    def _write(folder, layers):
        os.makedirs(folder, exist_ok=True)
        param = {"__meta__": {"class_fullname": "pecos.xmc.base###HierarchicalMLModel"}, "model": "HierarchicalMLModel", "depth": len(layers),
                 "nr_features": layers[-1].nr_features, "nr_codes": layers[-1].nr_codes, "nr_labels": layers[-1].nr_labels}
        open(f"{folder}/param.json", "w", encoding="utf-8").write(json.dumps(param, indent=True))
        for d, layer in enumerate(layers):
            layer.save(f"{folder}/{d}.model")

    def save(self, folder):
        """The reference's folder layout (pecos/xmc/base.py:1371-1395), which :meth:`load` here and in the reference read.  Only a model
        that was trained in this process holds its weights on the host; a loaded one is predict-only."""
        if getattr(self, "layers", None) is None:
            raise Exception("Model is predict only! save not supported!")
        self._write(folder, self.layers)

    def _resolve_overrides(self, pred_params, kwargs):
        """xmc/base.py:1609-1654: merge kwargs, then only UNIFORM overrides are expressible natively."""
        pred_params = self._merged_pred_params(pred_params, kwargs)
        old_chain = self.get_pred_params().model_chain
        new_chain = pred_params.model_chain
        if all(o.post_processor == n.post_processor for o, n in zip(old_chain, new_chain)):
            pp = None
        elif all(new_chain[0].post_processor == n.post_processor for n in new_chain):
            pp = new_chain[0].post_processor
        else:
            raise NotImplementedError("when is_predict_only=True, post_processor is not supported for overriddng")
        if all(o.only_topk == n.only_topk for o, n in zip(old_chain[:-1], new_chain[:-1])):
            beam = None
        elif all(new_chain[0].only_topk == n.only_topk for n in new_chain[:-1]):
            beam = new_chain[0].only_topk
        else:
            raise NotImplementedError("when is_predict_only=True, beam_size is not supported for overriding")
        return beam, pp, new_chain[-1].only_topk

    def _merged_pred_params(self, pred_params, kwargs):
        """xmc/base.py:1609-1619: the model's own prediction parameters, or the given ones per layer, overridden by the keywords."""
        if pred_params is None:
            pred_params = self.get_pred_params()
        elif isinstance(pred_params, self.PredParams):
            pred_params = self.PredParams.from_dict(pred_params)
            if isinstance(pred_params.model_chain, MLModel.PredParams):
                pred_params.model_chain = [copy.deepcopy(pred_params.model_chain) for _ in range(self.depth)]
            elif len(pred_params.model_chain) != self.depth:
                raise ValueError(f"len(params.model_chain)={len(pred_params.model_chain)} != {self.depth}")
        else:
            raise ValueError("unknown type(pred_params)!!")
        pred_params.override_with_kwargs(kwargs)
        return pred_params

    def predict(self, X, csr_codes=None, pred_params=None, **kwargs):
        assert X.dtype == np.float32
        assert isinstance(X, smat.csr_matrix) or (isinstance(X, np.ndarray) and X.flags["C_CONTIGUOUS"])
        assert X.shape[1] == self.nr_features
        if getattr(self, "layerwise", None):                 # (xmc/base.py:1670-1680: a top layer of several clusters has no single root)
            chain = self._merged_pred_params(pred_params, kwargs).model_chain
            for layer, pp in zip(self.layerwise, chain):
                csr_codes = layer.predict(X, csr_codes=csr_codes, pred_params=pp, threads=kwargs.get("threads", -1))
            return csr_codes
        if csr_codes is not None:
            raise NotImplementedError("is_predict_only=True did not support csr_codes being not None")
        beam, pp, topk = self._resolve_overrides(pred_params, kwargs)
        pred_alloc = ScipyCompressedSparseAllocator()
        clib.xlinear_predict(self.model_chain, X, beam, pp, topk, kwargs.get("threads", -1), pred_alloc)
        return pred_alloc.get()


def _selected(self, X, selected_outputs_csr, pred_params=None, **kwargs):
    """HierarchicalMLModel.predict_on_selected_outputs, pecos/xmc/base.py:1682-1790."""
    if X.dtype != np.float32:
        raise ValueError("X.dtype = {} is not supported".format(X.dtype))
    if not isinstance(X, smat.csr_matrix) and not (isinstance(X, np.ndarray) and X.flags["C_CONTIGUOUS"]):
        raise ValueError("type(X) = {} is not supported".format(type(X)))
    if X.shape[1] != self.nr_features:
        raise ValueError("Feature dimension of query matrix does not match weight matrix")
    if not isinstance(selected_outputs_csr, smat.csr_matrix):
        raise ValueError("type(selected_outputs_csr) = {} is not supported".format(type(selected_outputs_csr)))
    if selected_outputs_csr.shape[1] != self.nr_pred_cols:
        raise ValueError("Label dimension of selected output matrix does not match")
    if X.shape[0] != selected_outputs_csr.shape[0]:
        raise ValueError("Instance dimension of query and selected output matrix do not match")
    _, pp, _ = self._resolve_overrides(pred_params, {k: v for k, v in kwargs.items() if k == "post_processor"})
    pred_alloc = ScipyCompressedSparseAllocator()
    clib.xlinear_predict_on_selected_outputs(self.model_chain, X, selected_outputs_csr, pp, kwargs.get("threads", -1), pred_alloc)
    return pred_alloc.get()


HierarchicalMLModel.predict_on_selected_outputs = _selected


def vstack_csr(matrices):
    """Row-stack CSR blocks keeping the (score-sorted) order inside rows (smat_util.py:343-390)."""
    indptr = [np.zeros(1, dtype=np.int64)]
    base = 0
    for m in matrices:
        indptr.append(m.indptr[1:].astype(np.int64) + base)
        base += int(m.indptr[-1])
    return smat.csr_matrix((np.concatenate([m.data for m in matrices]),
                            np.concatenate([m.indices for m in matrices]).astype(np.int64),
                            np.concatenate(indptr)),
                           shape=(sum(m.shape[0] for m in matrices), matrices[0].shape[1]))


class XLinearModel:
    """Drop-in for ``pecos.xmc.xlinear.XLinearModel`` on the predict path."""

    @dc.dataclass
    class PredParams(BaseParams):
        hlm_args: HierarchicalMLModel.PredParams = None  # type: ignore

        def override_with_kwargs(self, pred_kwargs):
            self.hlm_args.override_with_kwargs(pred_kwargs)
            return self

    def __init__(self, model=None):
        self.model = model

    @property
    def depth(self):
        return self.model.depth

    @property
    def nr_features(self):
        return self.model.nr_features

    @property
    def nr_labels(self):
        return self.model.nr_labels

    @property
    def nr_codes(self):
        return self.model.nr_codes

    @property
    def nr_pred_cols(self):
        return self.model.nr_pred_cols

    @property
    def is_predict_only(self):
        return True

    @classmethod
    def load(cls, model_folder, is_predict_only=True, **kwargs):
        """kwargs: weight_matrix_type in {"BINARY_SEARCH_CHUNKED", "HASH_CHUNKED", "CSC"} (pecos/core/base.py:49).
        "CSC" runs the reference's CSC arithmetic (bias first, dot product summed separately, inference.hpp:1018-1149) and is
        bit-identical to the reference loaded with the same type.  The two chunked types share one device layout; with SPARSE
        queries "HASH_CHUNKED" takes that layout's arithmetic (bias first, then the query's features ascending,
        inference.hpp:705-735) and is bit-identical to the reference loaded as HASH_CHUNKED too; with DENSE queries the reference's
        hash layout walks its hash map in the map's own order (:737-768), which no other implementation can reproduce -- dense
        queries get the BINARY_SEARCH_CHUNKED arithmetic there (same labels, scores within ~3e-6 relative of the hash layout's)."""
        model = HierarchicalMLModel.load(path.join(model_folder, "ranker"), is_predict_only, **kwargs)
        return cls(model)

    @dc.dataclass
    class TrainParams(BaseParams):
        """The part of pecos/xmc/xlinear/model.py:33-70 that is served: the full model, no relevance induction."""
        mode: str = "full-model"
        ranker_level: int = 1
        nr_splits: int = 16
        min_codes: int = None  # type: ignore
        shallow: bool = False
        rel_mode: str = "disable"
        rel_norm: str = "no-norm"
        hlm_args: HierarchicalMLModel.TrainParams = None  # type: ignore

    @classmethod
    def train(cls, X, Y, C=None, R=None, user_supplied_negatives=None, train_params=None, pred_params=None, **kwargs):
        """An XR-Linear model trained on the device (pecos/xmc/xlinear/model.py:167-283): ``C`` is None (one-versus-all; ``R`` then gives
        the costs), the bottom clustering matrix (labels x codes) or a chain, root first.  Solver parameters come as keywords
        (``threshold``, ``solver_type``, ``Cp``, ``max_iter``, ``negative_sampling_scheme``, ...) or in ``train_params``;
        ``beam_size`` / ``only_topk`` / ``post_processor`` or ``pred_kwargs`` set the saved prediction parameters.  Not served, and refused
        by name: the ``matcher`` / ``ranker`` modes, relevance induction (``rel_mode`` other than ``disable``), user-supplied negatives."""
        return cls._train_through(HierarchicalMLModel.train, X, Y, C, R, user_supplied_negatives, train_params, pred_params, kwargs)

    @classmethod
    def train_device(cls, X, Y, C=None, R=None, train_params=None, pred_params=None, **kwargs):
        """:meth:`train` through :meth:`HierarchicalMLModel.train_device`: the same arguments and refusals, the whole layer loop resident in
        HBM, and ``negative_sampling_scheme`` may be any sum of ``tfn``, ``usn`` and ``man`` (``tfn+man`` is the reference CLI's
        ``-ns tfn+man``).  The result saves, loads and predicts like :meth:`train`'s."""
        return cls._train_through(HierarchicalMLModel.train_device, X, Y, C, R, kwargs.pop("user_supplied_negatives", None), train_params, pred_params, kwargs)

    @classmethod
    def _resolved_train_params(cls, train_params, kwargs):
        """The ``TrainParams`` of a train call from ``train_params`` or, without them, from the keywords (model.py:199-206)."""
        if train_params is None:
            tp = cls.TrainParams.from_dict(kwargs)
            tp.hlm_args = HierarchicalMLModel.TrainParams(neg_mining_chain=kwargs.get("negative_sampling_scheme", "tfn"), model_chain=MLModel.TrainParams.from_dict(kwargs))
        else:
            tp = cls.TrainParams.from_dict(train_params)
            if isinstance(tp.hlm_args, dict):
                tp.hlm_args = HierarchicalMLModel.TrainParams.from_dict(tp.hlm_args)
        return tp

    @classmethod
    def _resolved_pred_params(cls, pred_params, kwargs):
        """The ``HierarchicalMLModel.PredParams`` of a train call, or None (model.py:208-217); ``kwargs`` gets its ``pred_kwargs``."""
        hp = None
        if pred_params is not None:
            hp = cls.PredParams.from_dict(pred_params).hlm_args
        if kwargs.get("pred_kwargs", None) is None:
            kwargs["pred_kwargs"] = {k: kwargs.get(k, None) for k in ("beam_size", "only_topk", "post_processor")}
        return hp

    @classmethod
    def train_ext(cls, X, Y, C=None, R=None, user_supplied_negatives=None, train_params=None, pred_params=None, **kwargs):
        """:meth:`train_device` with every option of the reference's ``XLinearModel.train`` (pecos/xmc/xlinear/model.py:219-283):
        ``rel_mode`` ``induce`` / ``ranker-only`` with ``rel_norm`` ``l1`` / ``l2`` / ``max`` / ``no-norm`` (cost-sensitive training from
        ``R``, or from the binarized ``Y``), ``user_supplied_negatives`` (a dict of matching matrices keyed by layers above the leaves,
        for schemes with ``usn``), and the ``matcher`` / ``ranker`` modes with ``ranker_level``.  The chain is completed from a partial
        one (``shallow``, ``min_codes``, ``nr_splits``); X, Y and the chain are uploaded once; the matching and relevance chains are
        built in HBM (:func:`pecos_amd.training.matching_chain_device`, ``relevance_chain_device``) and never visit the host; a relevance
        level the caller gave is checked against the loop's ``Y_t`` by the device check (:meth:`DeviceMatrix.check_relevance`) before
        the first layer is trained.  Every ``ValueError`` of the reference comes before a device is touched.  Without ``C`` this is
        :meth:`train_device` (``R`` gives the one-versus-all costs).  The result saves, loads and predicts like :meth:`train_device`'s;
        a ``ranker``-mode model has a top layer of several clusters and predicts without codes as the reference does."""
        from .cluster_chain import ClusterChain
        from .features import DeviceMatrix, _as_device_matrix, _stream_or_current
        from .training import _device_of, _partial_chain_check, matching_chain_device, relevance_chain_device, train_chain_device
        tp, hp = cls._resolved_train_params(train_params, kwargs), cls._resolved_pred_params(pred_params, kwargs)
        no_chain =C is None or (isinstance(C, (list, tuple)) and len(C) == 0)
        if tp.mode not in ("full-model", "matcher", "ranker"):
            raise ValueError(f"Wrong value for the mode attribute: {tp.mode}")
        if no_chain:
            if tp.mode != "full-model":
                raise ValueError(f"Expect non-trivial clustering for {tp.mode} mode")
            return cls(HierarchicalMLModel.train_device(MLProblem(X, Y, R=R), clustering=None, train_params=tp.hlm_args, pred_params=hp, **kwargs))
        if tp.rel_mode not in ("disable", "induce", "ranker-only"):
            raise ValueError(f"Wrong value for rel_mode: {tp.rel_mode}")
        min_codes, nr_splits = (None, 16) if tp.shallow else (tp.min_codes or tp.nr_splits, tp.nr_splits)
        chain = ClusterChain.from_partial_chain(C.chain if isinstance(C, ClusterChain) else C, min_codes=min_codes, nr_splits=nr_splits)
        level = int(tp.ranker_level)
        if tp.mode != "full-model" and not 0 < level < len(chain) + (tp.mode == "ranker"):
            raise ValueError(f"ranker_level = {level} leaves no layer to train in {tp.mode} mode: the chain has {len(chain)} layers")
        if not isinstance(X, np.ndarray) and not smat.issparse(X):
            raise NotImplementedError("type(X) = {} is not supported.".format(type(X)))
        if X.dtype != np.float32:
            raise ValueError(f"X must be float32, got {X.dtype}")
        if chain[-1].shape[0] != Y.shape[1]:
            raise ValueError(f"the bottom clustering matrix has {chain[-1].shape[0]} rows, the problem {Y.shape[1]} labels")
        usn = user_supplied_negatives
        for D in (usn, None if R is None else {0: R}):
            if D is not None and not all(D[k] is None for k in D) and _partial_chain_check(D, chain)[0] != Y.shape[0]:
                raise ValueError("M_dict first dim do not match")
        cut = slice(None) if tp.mode == "full-model" else slice(None, -level) if tp.mode == "matcher" else slice(-level, None)
        host_chain = list(chain)[cut]

        labels = types.SimpleNamespace(nr_labels=host_chain[-1].shape[0])        # what _training_setup reads of a problem
        _, _, schemes, layer_params, pp = HierarchicalMLModel._training_setup(labels, host_chain, tp.hlm_args, hp, kwargs, True)

        dev = _device_of([X, Y, R] + list((usn or {}).values()))
        s = _stream_or_current(dev, None)
        x = _as_device_matrix(X if smat.issparse(X) else _every_entry_csr(X), dev, None, None)
        y = _as_device_matrix(Y, dev, None, None)
        cs = [DeviceMatrix.upload(c, dev) for c in chain]
        matching = matching_chain_device(usn, cs, stream=s)
        given = None
        if tp.rel_mode == "disable" or (tp.rel_mode == "ranker-only" and R is None):      # ({0: None}: nothing given, a chain of None)
            relevance = [None] * len(cs)
        else:
            given = None if R is None else _as_device_matrix(R, dev, None, None)
            level0 = given if given is not None else DeviceMatrix.pattern_union([y], stream=s)          # binarized(Y)
            relevance = relevance_chain_device({0: level0}, cs, tp.rel_norm, tp.rel_mode == "induce", stream=s)
        if tp.mode == "matcher":
            for c in reversed(cs[-level:]):
                y = y.multiply(c, stream=s)
        elif given is not None:                             # the caller's level is the leaves': against the loop's own Y there
            DeviceMatrix.check_relevance(y, relevance[-1], stream=s)
        weights = train_chain_device(x, y, cs[cut], schemes, matching[cut], relevance[cut], layer_params, pp.model_chain, stream=s)
        return cls(HierarchicalMLModel._from_weights(weights, host_chain, layer_params, pp))

    @classmethod
    def _train_through(cls, train_chain, X, Y, C, R, user_supplied_negatives, train_params, pred_params, kwargs):
        from .indexer import chain_from_partial
        tp = cls._resolved_train_params(train_params, kwargs)
        for what, bad in (("mode", tp.mode != "full-model"), ("rel_mode", tp.rel_mode != "disable"), ("user_supplied_negatives", user_supplied_negatives is not None)):
            if bad:
                raise NotImplementedError(f"XLinearModel.train: {what} = {getattr(tp, what, user_supplied_negatives)!r} is not served on the device")
        hp = cls._resolved_pred_params(pred_params, kwargs)
        if C is None or (isinstance(C, (list, tuple)) and len(C) == 0):
            clustering = None
        else:                                                   # the given levels, completed upwards to a single root (ClusterChain.from_partial_chain)
            top, rest = (C[0], [smat.csc_matrix(c, dtype=np.float32) for c in C[1:]]) if isinstance(C, (list, tuple)) else (C, [])
            min_codes, nr_splits = (None, 16) if tp.shallow else (tp.min_codes or tp.nr_splits, tp.nr_splits)
            clustering = chain_from_partial(top, min_codes=min_codes, nr_splits=nr_splits) + rest
        prob = MLProblem(X, Y, R=R if clustering is None else None)
        return cls(train_chain(prob, clustering=clustering, train_params=tp.hlm_args, pred_params=hp, **kwargs))

    def save(self, model_folder):
        """``model_folder/param.json`` and ``model_folder/ranker`` in the reference's layout (pecos/xmc/xlinear/model.py:92-103)."""
        os.makedirs(model_folder, exist_ok=True)
        with open(f"{model_folder}/param.json", "w", encoding="utf-8") as fout:
            fout.write(json.dumps({"__meta__": {"class_fullname": "pecos.xmc.xlinear.model###XLinearModel"}, "model": "XLinearModel"}, indent=True))
        self.model.save(path.join(model_folder, "ranker"))

    @classmethod
    def compile_mmap_model(cls, npz_folder, mmap_folder):
        """npz model folder -> memory-mapped model folder (pecos/xmc/xlinear/model.py:136-152)."""
        import shutil
        os.makedirs(mmap_folder, exist_ok=True)
        shutil.copy(path.join(npz_folder, "param.json"), path.join(mmap_folder, "param.json"))
        clib.xlinear_compile_mmap_model(path.join(npz_folder, "ranker"), path.join(mmap_folder, "ranker"))

    # ---- query / label matrix files as the reference's predict CLI reads and writes them (pecos/xmc/xlinear/model.py:424-467,
    #      pecos/utils/smat_util.py:60-150): .npy = dense, scipy .npz = sparse
    @staticmethod
    def _load_matrix(src):
        if not isinstance(src, str):
            raise ValueError("src for load_matrix must be a str")
        mat = np.load(src)
        if isinstance(mat, np.ndarray):
            return mat
        fmt = mat["format"].item()
        fmt = fmt if isinstance(fmt, str) else fmt.decode("ascii")
        if fmt in ("csc", "csr", "bsr"):
            out = getattr(smat, fmt + "_matrix")((mat["data"], mat["indices"], mat["indptr"]), shape=mat["shape"])
            out.sort_indices()
            return out
        if fmt == "coo":
            return smat.coo_matrix((mat["data"], (mat["row"], mat["col"])), shape=mat["shape"])
        if fmt == "dia":
            return smat.dia_matrix((mat["data"], mat["offsets"]), shape=mat["shape"])
        raise ValueError("Unknown matrix format {}".format(fmt))

    @staticmethod
    def save_feature_matrix(tgt, feat_mat):
        """dense -> .npy stream, sparse -> scipy .npz (uncompressed, like the reference's save_matrix)."""
        if isinstance(feat_mat, np.ndarray):
            np.save(tgt, feat_mat, allow_pickle=False)
        elif smat.issparse(feat_mat):
            smat.save_npz(tgt, feat_mat, compressed=False)
        else:
            raise NotImplementedError("Save not implemented for matrix type {}".format(type(feat_mat)))

    @staticmethod
    def load_feature_matrix(src):
        """csr_matrix with sorted indices, or a C-contiguous ndarray (what predict() accepts)."""
        feat_mat = XLinearModel._load_matrix(src)
        if isinstance(feat_mat, np.ndarray):
            return np.ascontiguousarray(feat_mat)
        feat_mat = feat_mat.tocsr()
        feat_mat.sort_indices()
        return feat_mat

    @staticmethod
    def load_label_matrix(src, for_training=False):
        assert isinstance(src, str), "src for load_label_matrix must be a str"
        lab = XLinearModel._load_matrix(src)
        lab = smat.csc_matrix(lab) if for_training else smat.csr_matrix(lab)
        return lab.astype(np.float32)

    def get_pred_params(self):
        return self.PredParams(hlm_args=self.model.get_pred_params())

    def set_output_constraint(self, labels_to_keep):
        """Prune the tree to the labels in ``labels_to_keep`` (pecos/xmc/xlinear/model.py:285-293); works on the predict-only model,
        ``None`` clears (HierarchicalMLModel.set_output_constraint)."""
        self.model.set_output_constraint(labels_to_keep)

    def predict(self, X, pred_params=None, selected_outputs_csr=None, **kwargs):
        if (pred_params is not None) and (not isinstance(pred_params, self.PredParams)):
            raise TypeError("type(pred_kwargs) is not supported")
        max_pred_chunk = kwargs.get("max_pred_chunk", 10**7)
        if not (max_pred_chunk is None or isinstance(max_pred_chunk, int)):
            raise TypeError("type(max_pred_chunk) is not supported.")
        if max_pred_chunk is None or max_pred_chunk >= X.shape[0]:
            kw = {k: v for k, v in kwargs.items() if k != "max_pred_chunk"}
            hp = None if pred_params is None else pred_params.hlm_args
            if selected_outputs_csr is None:
                return self.model.predict(X, pred_params=hp, **kw)
            return self.model.predict_on_selected_outputs(X, selected_outputs_csr, pred_params=hp, **kw)
        new_kwargs = kwargs.copy()
        new_kwargs.pop("max_pred_chunk", None)
        Ys = [self.predict(X[i: i + max_pred_chunk, :], pred_params=pred_params,
                           selected_outputs_csr=(selected_outputs_csr[i: i + max_pred_chunk, :]
                                                 if selected_outputs_csr is not None else None), **new_kwargs)
              for i in range(0, X.shape[0], max_pred_chunk)]
        return vstack_csr(Ys)
