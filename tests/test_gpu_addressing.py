"""GPU (-m gpu): models whose weight matrices have 2^24 feature rows and more -- where 32-bit byte offsets into a dense-format matrix end.

The dense row format holds a level as (w_rows + 1) rows of d_ld floats.  K1Q reads a row through a raw buffer load whose num_records and
scalar offset are 32-bit BYTE counts (k1q_load_w<BIGW = false>); matrices of 4 GiB and more take the BIGW instantiations (a 64-bit base
per row).  The merged level-0/1 matrix (LayerDev::wd01, 64 columns = 256 bytes per row) is read by k1q_layer01m, which has no BIGW form:
with w_rows + 1 == 2^24 its num_records is exactly 0 (every level-0/1 weight reads as 0), above that it wraps and aliases onto low rows
-- while levels 0 and 1 themselves (d_ld = 32, 2.1 GB each) stay under 4 GiB, so nothing else in the launch asks for BIGW.  The model
compiler must therefore not build / use the merged matrix unless (w_rows + 2) * 256 < 0xFFFFFFF0 (attribute "merged01" says whether it did).

Three hand-built models, tree [2, 8, 64], bias 1.0, 300 weights per column drawn from a pool of ~3 100 features: the 40 lowest ids, 40 around
2^23, the 40 highest and 3 000 random ones; 300 queries of 60 features from the same pool (about half of them >= 2^23):
  D = 2^24 - 4     the last size at which the merged matrix is still addressable: merged01 == 1, the merged path must be taken
  D = 2^24 - 2     w_rows + 1 == 2^24
  D = 2^24 + 1000  past the limit
On the device levels 0 and 1 take 2.1 GB each, level 2 (d_ld = 64) 4.3 GB -- its launches are BIGW --, the merged matrix 4.29 GB where it is
built: about 13 GB per model.  Generation, the oracle and its predicts cost under a second on the CPU; the model load does host work
proportional to the row count and is printed by the test (not yet measured on a GPU host: if it exceeds a minute, shrink the feature pool, not D).

Expected on a library without the guard: with D = 2^24 - 2 and D = 2^24 + 1000 the default path (XRL_K1Q_FUSE01 unset) reads zeros / aliased rows
for levels 0 and 1 and returns wrong beams, and merged01 reads 1; XRL_K1Q_FUSE01 = 0 / 1 and dense_layers = 0 do not touch the merged matrix.
"""
import json
import os
import time

import numpy as np
import pytest
import scipy.sparse as smat

from conftest import assert_same_topk

pytestmark = pytest.mark.gpu

SHAPE = (2, 8, 64)
PER_COL = 300
MIN_FREE_GB = 64


def feature_pool(D, rng):
    mid = 1 << 23
    pool = np.concatenate([np.arange(40), np.arange(mid - 20, mid + 20), np.arange(D - 40, D), rng.integers(0, D, 3000)])
    return np.unique(pool[pool < D]).astype(np.int64)


def huge_model(folder, D, seed=7):
    rng = np.random.default_rng(seed)
    pool = feature_pool(D, rng)
    prev_k = 1
    for d, K in enumerate(SHAPE):
        lf = os.path.join(folder, "ranker", f"{d}.model"); os.makedirs(lf, exist_ok=True)
        cols, ptr = [], [0]
        for c in range(K):
            ids = np.sort(rng.choice(pool, PER_COL, replace=False))
            # the pool's extremes in many columns: the lowest / highest ids and the ones around 2^23 are where a wrapped offset aliases
            cols.append(np.concatenate([ids, [D]]))            # bias row last
            ptr.append(ptr[-1] + len(ids) + 1)
        idx = np.concatenate(cols)
        val = rng.standard_normal(len(idx)).astype(np.float32)
        W = smat.csc_matrix((val, idx.astype(np.int32), np.array(ptr, np.int64)), shape=(D + 1, K))
        smat.save_npz(os.path.join(lf, "W.npz"), W, compressed=False)
        par = np.arange(K) * prev_k // K
        C = smat.csc_matrix((np.ones(K, np.float32), (np.arange(K), par)), shape=(K, prev_k))
        smat.save_npz(os.path.join(lf, "C.npz"), C, compressed=False)
        json.dump({"model": "MLModel", "bias": 1.0, "pred_kwargs": {"only_topk": 20, "post_processor": "l3-hinge"}},
                  open(os.path.join(lf, "param.json"), "w"))
        prev_k = K
    json.dump({"model": "HierarchicalMLModel", "depth": len(SHAPE)}, open(os.path.join(folder, "ranker", "param.json"), "w"))
    json.dump({"model": "XLinearModel"}, open(os.path.join(folder, "param.json"), "w"))
    return pool


def huge_queries(D, pool, seed=8, n=300, per_row=60):
    rng = np.random.default_rng(seed)
    idx = np.concatenate([np.sort(rng.choice(pool, per_row, replace=False)) for _ in range(n)])
    val = (np.abs(rng.standard_normal(len(idx))) + 0.05).astype(np.float32)
    X = smat.csr_matrix((val, idx.astype(np.int32), np.arange(0, len(idx) + 1, per_row)), shape=(n, D))
    X.data /= np.repeat(np.sqrt(np.asarray(X.multiply(X).sum(axis=1)).ravel()), per_row).astype(np.float32)
    X.has_sorted_indices = True
    return X


# option settings under which the comparison runs: (name, options, XRL_K1Q_FUSE01)
SETTINGS = [
    ("defaults", {}, None),
    ("XRL_K1Q_FUSE01=0", {}, "0"),
    ("XRL_K1Q_FUSE01=1", {}, "1"),
    ("dense_layers=2", {"dense_layers": 2}, None),
    ("dense_layers=0", {"dense_layers": 0}, None),
    ("presence=0", {"presence": 0}, None),
    ("presence=2", {"presence": 2}, None),
    ("dense_layers=0 tile_rows=0", {"dense_layers": 0, "tile_rows": 0}, None),
    ("dense_layers=0 tile_rows=2", {"dense_layers": 0, "tile_rows": 2}, None),
    ("sorted launch", {"qsort": 1, "qsort_min_rows": 1, "qsort_min_parents": 2}, None),
]
DEFAULTS = {"dense_layers": 1, "presence": 1, "tile_rows": 1, "qsort": 1, "qsort_min_rows": 131072, "qsort_min_parents": 64}


@pytest.mark.parametrize("D,merged", [((1 << 24) - 4, 1), ((1 << 24) - 2, 0), ((1 << 24) + 1000, 0)], ids=["2^24-4", "2^24-2", "2^24+1000"])
def test_feature_rows_at_the_32bit_offset_limit(D, merged, oracle_mod, tmp_path):
    import torch
    from pecos_amd import XLinearModel, clib
    free_b, _ = torch.cuda.mem_get_info()
    if free_b < MIN_FREE_GB << 30:
        pytest.skip(f"needs {MIN_FREE_GB} GB of free HBM (the dense format's cap is a quarter of what is free; the model takes ~13 GB): {free_b >> 30} GB free")
    folder = str(tmp_path / "m")
    pool = huge_model(folder, D)
    X = huge_queries(D, pool)
    assert 0.35 < np.mean(X.indices >= (1 << 23)) < 0.65 and X.indices.max() == D - 1 and X.indices.min() == 0
    om = oracle_mod.OracleModel.load(folder)
    kws = (dict(beam_size=4, only_topk=10), dict(beam_size=8, only_topk=64, post_processor="noop"))
    wants = [om.predict(X, **kw) for kw in kws]
    if oracle_mod.ref_available():
        rm = oracle_mod.RefModel(folder)
        for kw, want in zip(kws, wants):
            assert_same_topk(rm.predict(X, **kw), want, exact_scores=True, what=f"D={D}: compiled reference vs restatement {kw}")
    t0 = time.time()
    m = XLinearModel.load(folder)
    print(f"\nD={D}: model load {time.time() - t0:.1f} s")
    h = m.model.model_chain
    assert clib.xlinear_get_int_attr(h, "nr_dense_layers") == 3            # the dense row format is really in play
    assert clib.xlinear_get_int_attr(h, "merged01") == merged, "merged level-0/1 matrix: built exactly while (w_rows + 2) * 256 < 0xFFFFFFF0"
    wrong = []
    try:
        for name, opts, fuse in SETTINGS:
            for o, v in opts.items():
                clib.set_option(h, o, v)
            if fuse is not None:
                os.environ["XRL_K1Q_FUSE01"] = fuse
            try:
                if name == "defaults" and merged:      # just under the limit the merged walk must still be the one that runs
                    clib.profile_enable(h, True); clib.profile_reset(h)
                    m.predict(X, **kws[0])
                    names = {r["name"] for r in clib.profile_get(h)}
                    clib.profile_enable(h, False)
                    assert any(n.startswith("k1q_fused_0_") for n in names), names
                for kw, want in zip(kws, wants):
                    got = m.predict(X, **kw)
                    try:
                        assert_same_topk(got, want, exact_scores=True, what=f"D={D} {name} {kw}")
                    except AssertionError as e:      # collect: the report names every setting that is wrong, not the first
                        wrong.append(str(e).splitlines()[0])
            finally:
                os.environ.pop("XRL_K1Q_FUSE01", None)
                for o in opts:
                    clib.set_option(h, o, DEFAULTS[o])
    finally:
        del m
    assert not wrong, "\n".join(wrong)
