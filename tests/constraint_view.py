"""The reference's set_output_constraint rule (pecos/xmc/base.py:1796-1824) in numpy -- what the device form of the output constraint
(xrl_set_output_constraint, pecos_amd/csrc/xrl_constrain.hip) is held against.

Bottom-up over the layers: if the kept set has as many members as C has rows, stop (this layer and every layer above keep their C);
otherwise delete from C every entry whose row is not kept -- the stored order of the survivors does not change -- and the kept set of the layer
above is the set of columns that still hold an entry.

  prune_layers   the rule on the list of layers oracle.xrl_oracle.load_model_folder returns
  prune_folder   the rule on a model folder: C.npz rewritten in the format in which it was stored, everything else copied
  view_arrays    per layer the (chunk_col', perm_inv') pair the device builds, None for a layer that keeps its own arrays
  kept_sets      the kept sets the tests share
"""
import os
import shutil

import numpy as np
import scipy.sparse as smat


def _stored_csc(C):
    """C as CSC in its STORED order (no sort, no duplicate merging): what the loaders see."""
    C = C if smat.isspmatrix_csc(C) else smat.csc_matrix(C)
    return C


def prune_C(C, kept):
    """(C without the entries whose row is not in `kept`, columns that still hold an entry); survivors keep their stored order."""
    C = _stored_csc(C)
    mask = np.isin(C.indices, np.fromiter(kept, dtype=np.int64, count=len(kept)))
    csum = np.concatenate([[0], np.cumsum(mask)]).astype(np.int64)
    per_col = csum[C.indptr[1:]] - csum[C.indptr[:-1]]
    indptr = np.concatenate([[0], np.cumsum(per_col)]).astype(C.indptr.dtype)
    out = smat.csc_matrix((C.data[mask], C.indices[mask], indptr), shape=C.shape)
    return out, set(np.nonzero(per_col)[0].tolist())


def prune_layers(layers, labels_to_keep, early_stop=True):
    """(new list of layers, index of the layer at which the rule stopped or -1).  early_stop=False: the rule WITHOUT its stop (every layer
    pruned) -- only to show that the stop matters."""
    kept = set(int(v) for v in labels_to_keep)
    out = [dict(L) for L in layers]
    stopped = -1
    for l in range(len(layers) - 1, -1, -1):
        C = _stored_csc(layers[l]["C"])
        if early_stop and len(kept) == C.shape[0]:
            stopped = l
            break
        out[l]["C"], kept = prune_C(C, kept)
    return out, stopped


def prune_folder(src, dst, labels_to_keep):
    """Copy the model folder `src` (the XLinearModel folder, with ranker/) to `dst` with every C.npz rewritten by the rule, in the format in
    which it was stored; returns dst."""
    shutil.copytree(src, dst)
    ranker = os.path.join(dst, "ranker")
    depth = len([d for d in os.listdir(ranker) if d.endswith(".model")])
    kept = set(int(v) for v in labels_to_keep)
    for l in range(depth - 1, -1, -1):
        lf = os.path.join(ranker, f"{l}.model")
        cpath = os.path.join(lf, "C.npz")
        if os.path.exists(cpath):
            M = smat.load_npz(cpath)
            fmt = M.format
        else:                                                 # a root without codes: one parent over every column of W
            M = smat.csc_matrix(np.ones((smat.load_npz(os.path.join(lf, "W.npz")).shape[1], 1), dtype=np.float32))
            fmt = "csc"
        C = _stored_csc(M)
        if len(kept) == C.shape[0]:
            break
        pruned, kept = prune_C(C, kept)
        smat.save_npz(cpath, pruned if fmt == "csc" else pruned.asformat(fmt), compressed=False)
    return dst


def view_arrays(layers, labels_to_keep):
    """Per layer (chunk_col' uint32 [parents + 1], perm_inv' uint32 [kept]) of the pruned C, or None where the rule left C alone; and
    the kept children per layer (all of them where C was left alone)."""
    pruned, stopped = prune_layers(layers, labels_to_keep)
    views, kept = [], []
    for l, L in enumerate(pruned):
        C = _stored_csc(L["C"])
        kept.append(int(C.nnz))
        views.append(None if l <= stopped else (C.indptr.astype(np.uint32), C.indices.astype(np.uint32)))
    return views, kept


def kept_sets(nr_labels, seed=7, in_tree=None):
    """name -> label ids: a random 10 %, one label, all but one, every second label, six labels.  The one label is drawn from `in_tree` (the
    labels the loaded tree holds) where given: a kept set without any label of the tree empties the model, which is a case of its own."""
    rng = np.random.default_rng(seed)
    ten = np.sort(rng.choice(nr_labels, max(1, nr_labels // 10), replace=False))
    pool = np.arange(nr_labels) if in_tree is None else np.unique(np.asarray(in_tree))
    return {
        "ten_percent": ten,
        "one_label": np.array([int(pool[int(rng.integers(0, len(pool)))])]),
        "all_but_one": np.delete(np.arange(nr_labels), nr_labels // 3),
        "every_second": np.arange(0, nr_labels, 2),
        "six_labels": np.sort(rng.choice(nr_labels, 6, replace=False)),
    }


SPARSE_SETS = ("one_label", "six_labels")                     # leave every row with fewer than k = 10 results
CHANGING_SETS = ("ten_percent", "every_second")               # change (nearly) every row of the answer
