"""Ranker training with the operands and the weights resident in HBM: :func:`train_layer_device` (K13), the last link of
``label_embedding_device -> run_clustering_device -> train_layer_device``; :func:`single_layer_predict_device`, a trained layer's
prediction from HBM; and :func:`train_chain_device`, the reference's layer loop (pecos/xmc/base.py:1512-1572) with X, Y, the label chain,
the matching matrices (K14), the predictions and the weights in HBM from the first layer to the last -- which is what serves matcher-aware
negatives (``man``).  The weights are the reference's at ``threads = 1`` bit for bit (``xrl_train_layer_device``,
``xrl_smat_pattern_union_device`` and ``xrl_single_layer_predict_device`` in include/xrl_abi.h state the rules)."""
import copy

from .core import clib

TRAIN_KEYS = ("threshold", "max_nonzeros_per_label", "solver_type", "Cp", "Cn", "max_iter", "eps", "bias")


def _device_of(operands, default=0):
    """The device of the first operand that lives on one (a :class:`DeviceMatrix` or CUDA tensors), else ``default``."""
    from .features import _operand_device
    return next((d for d in (_operand_device(o) for o in operands if o is not None) if d is not None), default)


def _train_transposed(x, yt, ct, mt, rt, stream, **params):
    """K13 over :class:`DeviceMatrix` operands that are transposed already."""
    from .features import DeviceMatrix
    return DeviceMatrix(clib.train_layer_device(x.handle, yt.handle, ct and ct.handle, mt and mt.handle, rt and rt.handle, stream=stream, **params))


def train_layer_device(X, Y, C=None, M=None, R=None, threshold=0.1, max_nonzeros_per_label=None, solver_type="L2R_L2LOSS_SVC_DUAL", Cp=1.0, Cn=1.0,
                       max_iter=100, eps=0.1, bias=1.0, stream=None):
    """One layer's weights from ``X`` (instances x features), ``Y`` (instances x labels), the label-to-cluster matrix ``C`` (labels x
    clusters; None: pure multi-label), the matching matrix ``M`` (instances x clusters; None with C: ``Y * C`` by the device sparse
    product) and the relevance ``R`` (Y's pattern; None: every positive costs 1).  An operand is a
    :class:`~pecos_amd.features.DeviceMatrix`, CSR tensors ``(crow, col, val, (rows, cols))`` or a float32 scipy sparse matrix (uploaded
    in CSR form); none of them is changed.  The solver reads columns, so Y, C, M and R are transposed on the device
    (:meth:`DeviceMatrix.transpose`, scipy's stable order: a column's entries by ascending row).  Returns W^T as a new
    :class:`~pecos_amd.features.DeviceMatrix`: labels x (features + (bias > 0)) in CSR, which is the CSC of W.  Runs on ``stream``
    (default: torch's current one), which it synchronises."""
    from .features import _as_device_matrix, _stream_or_current
    ops = [X, Y, C, M, R]
    dev = _device_of(ops)
    s = _stream_or_current(dev, stream)
    x, y, c, m, r = (None if o is None else _as_device_matrix(o, dev, None, stream) for o in ops)
    if c is not None and m is None:
        m = y.multiply(c, stream=s)
    if c is None:
        m = None
    yt = y.transpose(stream=s)
    ct, mt, rt = (None if o is None else o.transpose(stream=s) for o in (c, m, r))
    return _train_transposed(x, yt, ct, mt, rt, s, threshold=threshold, max_nonzeros_per_label=max_nonzeros_per_label, solver_type=solver_type, Cp=Cp, Cn=Cn,
                             max_iter=max_iter, eps=eps, bias=bias)


def _predict_transposed(x, wt, ct, codes, post_processor, only_topk, bias, stream, out_stride=None):
    """``xrl_single_layer_predict_device`` over :class:`DeviceMatrix` operands (``ct`` = C^T or None) and a codes triple or None: a new
    zeroed result triple of ``out_stride`` (default ``only_topk``) cells per row."""
    import torch
    from .features import result_buffers
    info = x.info
    rows, dev = info["rows"], torch.device("cuda", info["device"])
    stride = only_topk if out_stride is None else out_stride
    with torch.cuda.device(dev):
        out = result_buffers(rows, max(int(stride), 0), dev, sync=True)
        if codes is None:
            ci = cv = cc = None
            c_stride = 0
        else:
            ci, cv, cc = codes[:3]
            if ci.dim() != 2 or ci.shape != cv.shape or ci.dtype != torch.int32 or cv.dtype != torch.float32:
                raise ValueError("single_layer_predict_device: codes are (labels int32 [rows, k], scores float32 [rows, k], counts int32 [rows] or None)")
            if ci.shape[0] != rows:
                raise ValueError("single_layer_predict_device: Instance dimension of query and prev_layer_pred matrix do not match")
            n_parents = 1 if ct is None else ct.shape[0]
            if len(codes) > 3 and codes[3] is not None and codes[3] != n_parents:
                raise ValueError("single_layer_predict_device: Label dimension of prev_layer_pred and C matrix do not match")
            ci, cv = ci.contiguous(), cv.contiguous()
            c_stride = ci.shape[1]
            cc = torch.full((rows,), c_stride, dtype=torch.int32, device=dev) if cc is None else cc.contiguous()
            if cc.dtype != torch.int32 or cc.shape != (rows,):
                raise ValueError("single_layer_predict_device: counts are int32 [rows]")
            torch.cuda.current_stream().synchronize()
        clib.single_layer_predict_device(x.handle, wt.handle, ct and ct.handle, None if ci is None else ci.data_ptr(), None if cv is None else cv.data_ptr(),
                                         None if cc is None else cc.data_ptr(), c_stride, post_processor, only_topk, bias,
                                         out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stride, stream=stream)
    return out


def single_layer_predict_device(X, Wt, C=None, codes=None, post_processor="l3-hinge", only_topk=20, bias=1.0, stream=None, out_stride=None):
    """One layer's prediction with every operand in HBM: the resident form of ``clib.xlinear_single_layer_predict`` (the reference's
    ``MLModel.predict`` on sparse X), the same bits.  ``X`` (instances x features) and ``C`` (labels x clusters; None: one cluster) are
    operands as :func:`train_layer_device` takes them; ``Wt`` is that function's result (or any labels x (features + (bias > 0)) CSR
    operand); ``codes`` is None or a result triple ``(parents int32 [rows, k], scores float32 [rows, k], counts int32 [rows] or None)``
    -- this function's own output, fed back -- optionally with the parents' count as a fourth element.  Returns a result triple
    ``(labels int32 [rows, out_stride], scores float32, counts int32 [rows])``, rows best first, on the operands' device.  Runs on
    ``stream`` (default: torch's current one), which it synchronises."""
    from .features import _as_device_matrix, _stream_or_current
    ops = [X, Wt, C]
    dev = _device_of(ops, default=codes[0].device.index if codes is not None else 0)
    s = _stream_or_current(dev, stream)
    x, wt, c = (None if o is None else _as_device_matrix(o, dev, None, stream) for o in ops)
    ct = None if c is None else c.transpose(stream=s)
    return _predict_transposed(x, wt, ct, codes, post_processor, only_topk, bias, s, out_stride)


def _per_layer(value, depth, name):
    if isinstance(value, (list, tuple)):
        if len(value) != depth:
            raise ValueError(f"len({name})={len(value)} != {depth}")
        return list(value)
    return [copy.deepcopy(value) for _ in range(depth)]


def _params_dict(p):
    """A layer's solver keywords.  The primal solver stops at ``newton_eps`` (0.01 unless given), not at ``eps`` (pecos/xmc/base.py:868-870)."""
    d = p if isinstance(p, dict) else p.to_dict()
    out = {k: d[k] for k in TRAIN_KEYS if k in d}
    if clib._solver_number(out.get("solver_type", 1)) == 2:
        out["eps"] = d.get("newton_eps", 0.01)
    return out


def _label_chain(y, cs, stream):
    """``Y_t = Y_(t+1) * C_(t+1)`` by the device sparse product, bottom up: one matrix per layer, the leaves' ``y`` last."""
    labels_of = [y]
    for c in reversed(cs[1:]):
        labels_of.insert(0, labels_of[0].multiply(c, stream=stream))
    return labels_of


def _union_of_sources(t, scheme, labels_of, c, user_supplied, m_pred, stream):
    """Layer t's matching matrix (instances x clusters of layer t): K14's union of the sources ``scheme`` names.  ``tfn``: the clusters that
    hold one of an instance's own nodes -- the layer above's labels, which for the top layer is one more product; ``usn``: the caller's
    matrix; ``man``: the prediction ``m_pred`` of the layers above.  None for a layer without ``c`` and for a root that is a single cluster
    (every instance then trains every node); a scheme that names no source, or only absent ones, gives an empty M, as in the reference."""
    from .features import DeviceMatrix
    if c is None or (t == 0 and c.shape[1] == 1):
        return None
    shape = (labels_of[t].shape[0], c.shape[1])
    parts = []
    if "usn" in scheme and user_supplied is not None:
        if user_supplied.shape != shape:
            raise ValueError(f"a matching matrix has shape {user_supplied.shape}, the layer needs {shape}")
        parts.append(user_supplied)
    if "tfn" in scheme:
        parts.append(labels_of[t - 1] if t else labels_of[0].multiply(c, stream=stream))
    if "man" in scheme and t > 0:
        parts.append(DeviceMatrix.from_result(m_pred, shape[1], stream=stream))
    if not parts:
        import scipy.sparse as smat
        parts.append(DeviceMatrix.upload(smat.csr_matrix(shape, dtype="float32"), c.info["device"]))
    return DeviceMatrix.pattern_union(parts, stream=stream)


def _shape_of(o):
    """(rows, cols) of an operand: a scipy matrix or :class:`DeviceMatrix` (``.shape``), or CSR tensors ``(crow, col, val, (rows, cols))``."""
    return tuple(int(v) for v in (o[3] if isinstance(o, (tuple, list)) else o.shape))


class _Shaped(object):
    """Stands in for a matrix where only its shape is read."""

    def __init__(self, shape):
        self.shape = shape


def _partial_chain_check(D, chain):
    """``ClusterChain.matrix_chain_dimension_check`` over operands of any served kind, from their shapes alone: ``(nr_insts, nr_labels)``."""
    from .cluster_chain import ClusterChain
    shapes = {k: None if v is None else _Shaped(_shape_of(v)) for k, v in D.items()}
    return ClusterChain([_Shaped(_shape_of(c)) for c in chain]).matrix_chain_dimension_check(shapes)


def _nothing_given(D):
    return D is None or all(D[k] is None for k in D)


def relevance_chain_device(R_dict, chain, norm_type, induce, stream=None):
    """``ClusterChain.generate_relevance_chain`` (pecos/utils/cluster_util.py:240-281) with every matrix resident in HBM.  ``R_dict`` maps
    layers above the leaves (0: instances x labels) to relevance matrices; ``chain`` is the list of ``C``, root first; operands are scipy
    matrices (uploaded as CSR), CSR tensors or :class:`~pecos_amd.features.DeviceMatrix`.  Level 0 is ``R_dict.get(0)``; level i is
    ``R_dict[i]`` when given, else under ``induce`` the device product of level i-1 and ``chain[-i]`` (K10, explicit zeros kept, rows
    sorted), else None; the levels are then normalised by row under ``norm_type`` (``l1``, ``l2``, ``max``; None and ``no-norm``: as they
    are) by K12 -- a caller's level into a copy, never in place -- and returned root side first without the root: a list of ``len(chain)``
    :class:`DeviceMatrix` or None, which :func:`train_chain_device` takes as ``relevance_chain``.  Dimension errors are the reference's,
    as ``ValueError``, before a device is touched.  Runs on ``stream`` (default: torch's current one), which every step synchronises."""
    from .core import clib as _clib
    from .features import _as_device_matrix, _stream_or_current
    chain = list(chain)
    if _nothing_given(R_dict):
        return [None] * len(chain)
    _partial_chain_check(R_dict, chain)
    if norm_type not in (None, "no-norm") and norm_type not in _clib.ROW_NORMS:
        raise ValueError(f"'{norm_type}' is not a supported norm")
    dev = _device_of(list(R_dict.values()) + chain)
    s = _stream_or_current(dev, stream)
    levels, given = [], []
    for i in range(len(chain) + 1):
        if R_dict.get(i, None) is not None:
            levels.append(_as_device_matrix(R_dict[i], dev, None, stream))
            given.append(True)
        elif i > 0 and levels[i - 1] is not None and induce:
            levels.append(levels[i - 1].multiply(_as_device_matrix(chain[-i], dev, None, stream), eliminate_zeros=False, sorted_indices=True, stream=s))
            given.append(False)
        else:
            levels.append(None)
            given.append(False)
    if norm_type not in (None, "no-norm"):                  # (after the last product: a level is induced from the one below as it was given)
        levels = [None if m is None else m.normalize_rows(in_place=not own, stream=s, norm=norm_type) for m, own in zip(levels, given)]
    levels.reverse()
    return levels[1:]


def matching_chain_device(M_dict, chain, stream=None):
    """``ClusterChain.generate_matching_chain`` (pecos/utils/cluster_util.py:206-238) with every matrix resident in HBM: the chain of
    instance-to-cluster matching matrices of user-supplied negatives.  Level 0 is the pattern of ``M_dict[0]`` (instances x labels), or
    empty; level i is the pattern of the device product of level i-1 and ``chain[-i]`` (K10), united with ``M_dict[i]`` when given (K14).
    Only the pattern is the contract: the trainer reads nothing else of a matching matrix.  Returns the levels root side first without the
    label level: a list of ``len(chain)`` :class:`DeviceMatrix` (all None when nothing is given), which :func:`train_chain_device` takes
    as ``matching_chain``.  Operands, errors and the stream are :func:`relevance_chain_device`'s."""
    import scipy.sparse as smat
    from .features import DeviceMatrix, _as_device_matrix, _stream_or_current
    chain = list(chain)
    if _nothing_given(M_dict):
        return [None] * len(chain)
    nr_insts, nr_labels = _partial_chain_check(M_dict, chain)
    dev = _device_of(list(M_dict.values()) + chain)
    s = _stream_or_current(dev, stream)

    def given(i):
        return None if M_dict.get(i, None) is None else _as_device_matrix(M_dict[i], dev, None, stream)

    level = given(0)
    if level is None:
        level = DeviceMatrix.upload(smat.csr_matrix((nr_insts, nr_labels), dtype="float32"), dev)
    levels = []
    for i in range(1, len(chain) + 1):
        level = level.multiply(_as_device_matrix(chain[-i], dev, None, stream), eliminate_zeros=False, sorted_indices=True, stream=s)
        own = given(i)
        level = DeviceMatrix.pattern_union([level] if own is None else [level, own], stream=s)
        levels.append(level)
    levels.reverse()
    return levels


def train_chain_device(X, Y, chain, neg_mining_chain="tfn", matching_chain=None, relevance_chain=None, train_params=None, pred_params=None,
                       return_matching=False, stream=None):
    """The layers of a cluster chain trained top down with everything resident in HBM (pecos/xmc/base.py:1512-1572).  ``X`` (instances x
    features) and ``Y`` (instances x labels) are operands as :func:`train_layer_device` takes them; ``chain`` is the list of ``C``
    matrices, root first (an entry None: a one-versus-all layer, only as a one-element chain); ``neg_mining_chain`` is one scheme or one
    per layer, a sum of ``tfn`` (the layer above's labels), ``usn`` (``matching_chain[t]``) and ``man`` (the prediction of the layers
    trained so far, with layer t-1's own ``only_topk`` and ``post_processor`` from ``pred_params``); ``train_params`` / ``pred_params`` are
    one ``MLModel.TrainParams`` / ``PredParams`` (or dict) or one per layer.  A ``relevance_chain[t]`` given as a host matrix is checked
    as :class:`~pecos_amd.xlinear.MLProblem` checks R (``Y_t``'s pattern, no negative value; above the leaves ``Y_t`` is downloaded for
    it) before any layer is trained.  This is the package's one layer loop: ``HierarchicalMLModel.train`` and ``train_device`` run it.
    The label chain is ``Y_t = Y_(t+1) * C_(t+1)`` by the device sparse product; layer t's matching matrix is K14's union of its sources,
    and the half-trained chain predicts X layer by layer through :func:`single_layer_predict_device` whenever a scheme from layer t on
    contains ``man``, each result fed back as the next codes without leaving HBM.  Returns the list of W^T as
    :class:`~pecos_amd.features.DeviceMatrix`; with ``return_matching`` also the list of matching matrices (None where a layer has none)
    and the list of predictions that entered them (result triples, None where none was run).  X is uploaded once; nothing but each ``C``
    (a predict's tree bookkeeping) and 8-byte bounds and counters crosses to the host."""
    import scipy.sparse as smat
    from .features import _as_device_matrix, _stream_or_current
    from .xlinear import MLModel, check_relevance
    chain = list(chain)
    depth = len(chain)
    if depth == 0:
        raise ValueError("train_chain_device: an empty chain")
    if any(C is None for C in chain) and depth != 1:
        raise ValueError("train_chain_device: a layer without C is a one-element chain")
    for name, given in (("matching_chain", matching_chain), ("relevance_chain", relevance_chain)):
        if given is not None and len(given) != depth:
            raise ValueError(f"len({name})={len(given)} != {depth}")
    schemes = [s.lower() for s in _per_layer(neg_mining_chain, depth, "neg_mining_chain")]
    tps = [_params_dict(MLModel.TrainParams.from_dict(p)) for p in _per_layer(MLModel.TrainParams() if train_params is None else train_params, depth, "train_params")]
    pps = [MLModel.PredParams.from_dict(p) for p in _per_layer(MLModel.PredParams() if pred_params is None else pred_params, depth, "pred_params")]
    host_leaves = relevance_chain is not None and smat.issparse(relevance_chain[-1]) and smat.issparse(Y)
    if host_leaves:                                         # the leaves' relevance against the caller's own Y: checked before anything is uploaded
        check_relevance(Y, relevance_chain[-1])
    dev = _device_of([X, Y] + chain + list(matching_chain or []) + list(relevance_chain or []))
    s = _stream_or_current(dev, stream)

    def resident(o):
        return None if o is None else _as_device_matrix(o, dev, None, stream)

    x, cs = resident(X), [resident(C) for C in chain]
    usn = [resident(m) for m in matching_chain] if matching_chain is not None else [None] * depth
    labels_of = _label_chain(resident(Y), cs, s)
    for t, R in enumerate(relevance_chain or []):           # every other host matrix of the caller's before any layer is trained; Y_t comes down for it
        if smat.issparse(R) and not (host_leaves and t == depth - 1):
            check_relevance(labels_of[t].download(), R)
    rel = [resident(r) for r in relevance_chain] if relevance_chain is not None else [None] * depth
    cts = [None if c is None else c.transpose(stream=s) for c in cs]
    weights, matchings, predictions = [], [], []
    m_pred = None
    for t in range(depth):
        pred_t = None
        if t > 0 and any("man" in sc for sc in schemes[t:]):
            m_pred = _predict_transposed(x, weights[t - 1], cts[t - 1], m_pred, pps[t - 1].post_processor, pps[t - 1].only_topk, tps[t - 1]["bias"], s)
            pred_t = m_pred
        m = _union_of_sources(t, schemes[t], labels_of, cs[t], usn[t], m_pred, s)
        yt = labels_of[t].transpose(stream=s)
        mt = None if m is None else m.transpose(stream=s)
        rt = None if rel[t] is None else rel[t].transpose(stream=s)
        weights.append(_train_transposed(x, yt, cts[t] if m is not None else None, mt, rt, s, **tps[t]))
        matchings.append(m)
        predictions.append(pred_t)
    return (weights, matchings, predictions) if return_matching else weights
