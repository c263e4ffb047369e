"""Ranker training with the operands and the weights resident in HBM (K13): :func:`train_layer_device`, the last link of
``label_embedding_device -> run_clustering_device -> train_layer_device``.  The weights are the reference's at ``threads = 1`` bit for
bit (``xrl_train_layer_device`` in include/xrl_abi.h states the rule)."""
from .core import clib


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
    from .features import DeviceMatrix, _as_device_matrix, _operand_device, _stream_or_current
    ops = [X, Y, C, M, R]
    dev = next((d for d in (_operand_device(o) for o in ops if o is not None) if d is not None), 0)
    s = _stream_or_current(dev, stream)
    x, y, c, m, r = (None if o is None else _as_device_matrix(o, dev, None, stream) for o in ops)
    if c is not None and m is None:
        m = y.multiply(c, stream=s)
    if c is None:
        m = None
    yt = y.transpose(stream=s)
    ct, mt, rt = (None if o is None else o.transpose(stream=s) for o in (c, m, r))
    h = clib.train_layer_device(x.handle, yt.handle, ct and ct.handle, mt and mt.handle, rt and rt.handle, threshold=threshold,
                                max_nonzeros_per_label=max_nonzeros_per_label, solver_type=solver_type, Cp=Cp, Cn=Cn, max_iter=max_iter, eps=eps, bias=bias, stream=s)
    return DeviceMatrix(h)
