"""What the ensemble tests (test_ensemble_cpu.py, test_gpu_ensemble.py) and the fixture generator (golden/make_golden_ensemble.py) share:
the case list, the `finish` settings, and the fixtures' array forms.

A fixture tests/golden/ensemble/<case>.npz holds, per model m, the fixed-stride arrays K6 reads (idx<m> u32 [rows, stride_m], val<m> f32,
cnt<m> u32 [rows]; entries beyond cnt are filler), n_cols, and the reference's outputs as raw CSR triplets (<name>_indptr / _indices /
_data, rows in the reference's order): "average", "rank_average" (float64 data, as the reference returns it) and "finish<i>" for
FINISH[i]."""
import os

import numpy as np
import scipy.sparse as smat

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ensemble")
CASES = ("a", "b", "c", "d", "e")
# (threshold, only_topk) of Text2Text.predict; 0.2 is a quotient that occurs in the data (0.4 / 2), 0.0 meets the explicit zeros
FINISH = ((None, None), (0.2, 4), (0.0, 1), (None, 100), (-1.0, 3))


def fixed_to_csr(idx, val, cnt, n_cols):
    """Fixed-stride rows -> scipy CSR with exactly the stored entries in the stored order (explicit zeros kept)."""
    rows, stride = idx.shape
    cnt = np.minimum(cnt.astype(np.int64), stride)
    mask = np.arange(stride)[None, :] < cnt[:, None]
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    m = smat.csr_matrix((rows, n_cols), dtype=np.float32)
    m.indptr, m.indices, m.data = indptr, idx[mask].astype(np.int64), val[mask].astype(np.float32)
    return m


def compact_labels(idx, cnt):
    """scipy adds CSR matrices with unsorted rows through work arrays of n_cols entries, so label ids near 2^32 cannot go through the
    host code (ours or the reference's) as they are.  The merge depends on the labels only through their ORDER: the ids in use are
    replaced by their ranks (order-preserving), the host code runs on those, and `table[indices]` maps its output back.
    Returns (remapped idx arrays, table)."""
    used = [i[np.arange(i.shape[1])[None, :] < np.minimum(c, i.shape[1])[:, None]] for i, c in zip(idx, cnt)]
    table = np.unique(np.concatenate(used))
    return [np.searchsorted(table, i).astype(np.uint32) for i in idx], table


class Case:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        self.name = name
        self.n_models = int(z["n_models"])
        self.n_cols = int(z["n_cols"])
        self.idx = [z[f"idx{m}"] for m in range(self.n_models)]
        self.val = [z[f"val{m}"] for m in range(self.n_models)]
        self.cnt = [z[f"cnt{m}"] for m in range(self.n_models)]
        self.rows = self.idx[0].shape[0]
        self.out = {k[:-7]: (z[k], z[k[:-7] + "_indices"], z[k[:-7] + "_data"]) for k in z.files if k.endswith("_indptr")}

    def host_inputs(self):
        """(the models' results as CSR for the host code, table): output label = indices if table is None else table[indices]."""
        idx, table, n_cols = self.idx, None, self.n_cols
        if n_cols > 1 << 31:
            idx, table = compact_labels(self.idx, self.cnt)
            n_cols = len(table)
        return [fixed_to_csr(i, v, c, n_cols) for i, v, c in zip(idx, self.val, self.cnt)], table

    def expected(self, name):
        """(indptr int64, indices uint32, fp32 value bits) of a recorded output; the float64 of rank_average cast like K6 casts it."""
        ip, ix, dv = self.out[name]
        return ip.astype(np.int64), ix.astype(np.uint32), dv.astype(np.float32)


def same_rows(got, want, what=""):
    """Row lengths, labels in order and fp32 value BITS (so the sign of zero counts), NaN equal to NaN whatever its payload."""
    (gp, gi, gv), (wp, wi, wv) = got, want
    assert np.array_equal(gp, wp), f"{what}: row lengths differ"
    assert np.array_equal(gi, wi), f"{what}: labels or their order differ"
    gv, wv = np.asarray(gv, np.float32), np.asarray(wv, np.float32)
    nan = np.isnan(wv)
    assert np.array_equal(np.isnan(gv), nan), f"{what}: NaN positions differ"
    assert np.array_equal(gv.view(np.uint32)[~nan], wv.view(np.uint32)[~nan]), f"{what}: value bits differ"
