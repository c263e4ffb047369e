"""The plan of K7 (xrl_select_plan.hip) in numpy: for one row's set of labels, the nodes of every layer in the order the reference's walk emits
them (prolongate_sparse_predictions, inference.hpp:1302-1358) and, for every node, the position of its parent in the previous layer's list.

In a tree every node has one parent, so with A[T-1] = the sorted labels and A[l-1] = the sorted distinct parents of A[l], the walk emits layer
l in ascending order of the key (position of the node's parent in the ORDERED list of layer l-1, position of the node inside its parent's
column of C as stored); layer 0 hangs under the implicit root at position 0.  The steps and the 64-bit key (10 | 32 | 10 bits) are the
kernel's; the CPU tests hold this statement against the oracle's predict_on_selected_outputs, the GPU tests hold the kernel against both."""
import numpy as np
import scipy.sparse as smat

NONE = 0xFFFFFFFF
OK, OUT_OF_RANGE, TWICE, NO_PARENT = 0, 1, 2, 3
MAX_STRIDE = 1024


def tree_arrays(layers):
    """[(parent u32[c_rows], crank u32[c_rows])] per layer from the layers' C (CSC, STORED order; oracle.load_model_folder's dicts or matrices)."""
    out = []
    for l, L in enumerate(layers):
        C = smat.csc_matrix(L["C"] if isinstance(L, dict) else L)
        parent = np.full(C.shape[0], NONE, np.uint32)
        crank = np.zeros(C.shape[0], np.uint32)
        for p in range(C.shape[1]):
            kids = C.indices[C.indptr[p]: C.indptr[p + 1]]
            assert (parent[kids] == NONE).all() and len(set(kids.tolist())) == len(kids), "C is not a tree"
            parent[kids] = p if (l > 0 or p == 0) else NONE
            crank[kids] = np.arange(len(kids), dtype=np.uint32)
        out.append((parent, crank))
    return out


def plan_row(tree, labels, nr_labels):
    """(code, nodes, ppos): per layer the ordered nodes and parent positions of one row; a bad row gives (code, None, None)."""
    labels = np.asarray(labels, dtype=np.uint32)
    assert len(labels) <= MAX_STRIDE
    T = len(tree)
    cur = np.sort(labels)
    if len(np.unique(cur)) != len(cur):
        return TWICE, None, None
    if len(cur) and cur[-1] >= nr_labels:
        return OUT_OF_RANGE, None, None
    A = [None] * T
    for l in range(T - 1, -1, -1):                      # bottom-up
        parent = tree[l][0]
        A[l] = cur
        if (cur >= len(parent)).any() or (parent[cur] == NONE).any():
            return NO_PARENT, None, None
        cur = np.unique(parent[cur])
    nodes, ppos = [None] * T, [None] * T
    pos_prev = None
    for l in range(T):                                  # top-down
        parent, crank = tree[l]
        a = A[l]
        if l == 0:
            pp = np.zeros(len(a), np.uint64)
        else:
            rank = np.searchsorted(A[l - 1], parent[a])
            pp = pos_prev[rank].astype(np.uint64)
        key = (pp << np.uint64(42)) | (crank[a].astype(np.uint64) << np.uint64(10)) | np.arange(len(a), dtype=np.uint64)
        key = np.sort(key)
        idx = (key & np.uint64(1023)).astype(np.int64)
        nodes[l] = a[idx]
        ppos[l] = (key >> np.uint64(42)).astype(np.uint32)
        pos_prev = np.empty(len(a), np.int64)
        pos_prev[idx] = np.arange(len(a))
    return OK, nodes, ppos


def plan_order(tree, labels, nr_labels):
    """The reference's output order of one row's labels."""
    code, nodes, _ = plan_row(tree, labels, nr_labels)
    assert code == OK, f"bad row, code {code}"
    return nodes[-1]


def rooted_labels(tree):
    """Labels whose chain of parents reaches the root (what a pruned tree leaves selectable)."""
    ok = None
    for l, (parent, _) in enumerate(tree):
        has = parent != NONE
        if l > 0:
            has &= np.where(parent != NONE, ok[np.minimum(parent, len(ok) - 1)], False)
        ok = has
    return np.flatnonzero(ok).astype(np.uint32)


ROW_LENGTHS = (0, 1, 2, 63, 64, 65, 200, 1023, 1024)


def random_rows(pool, lengths=ROW_LENGTHS, seed=0):
    """One row per length (capped at the pool's size) of distinct labels drawn from `pool`, in shuffled order."""
    rng = np.random.default_rng(seed)
    return [rng.permutation(rng.choice(pool, min(n, len(pool)), replace=False)).astype(np.uint32) for n in lengths]


def rows_to_csr(rows, n_cols):
    """scipy CSR pattern (sorted inside every row, the form the host entry point takes) of a list of label rows."""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate([np.sort(r) for r in rows]).astype(np.int64) if len(rows) else np.zeros(0, np.int64)
    S = smat.csr_matrix((len(rows), n_cols), dtype=np.float32)
    S.indptr, S.indices, S.data = indptr, idx, np.ones(len(idx), np.float32)
    return S


def fixed_stride(rows, stride, fill=0):
    """(idx int32 [n, stride], cnt int32 [n]) of a list of label rows: the layout xrl_predict_selected_device reads."""
    idx = np.full((len(rows), stride), fill, np.uint32)
    for r, lab in enumerate(rows):
        idx[r, : len(lab)] = lab
    return idx.view(np.int32), np.array([len(r) for r in rows], np.int32)
