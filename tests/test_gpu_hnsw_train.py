"""HNSW graph construction on the device (K19): a folder saved after pecos_amd.hnsw.HNSW.train / train_device against the reference's bytes --
the recordings under tests/golden/hnsw/ (trained by the reference with M = 8, efC = 100, threads = 1) and the compiled reference when
oracle/_ref is there (dense under the avx512f gate)."""
import os

import numpy as np
import pytest
import scipy.sparse as smat

import hnsw_rule as hr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hnsw")
FILES = ("c_model/index.mmap_store", "c_model/config.json")


def HNSW():
    import pecos_amd
    return pecos_amd.hnsw.HNSW


def on_device(X):
    import torch
    if smat.issparse(X):
        X = X.tocsr()
        return (torch.from_numpy(X.indptr.astype(np.int64)).cuda(), torch.from_numpy(X.indices.astype(np.int32)).cuda(), torch.from_numpy(X.data.astype(np.float32)).cuda(), X.shape)
    return torch.from_numpy(np.ascontiguousarray(X)).cuda()


def train(X, folder, metric, M, efC, bound=-1, device_form=False):
    params = dict(M=M, efC=efC, threads=1, max_level_upper_bound=bound, metric_type=metric)
    m = HNSW().train_device(on_device(X), params) if device_form else HNSW().train(X, params)
    m.save(folder)
    return m


def same_bytes(got, want):
    """None, or where the first of the two files differs."""
    for f in FILES:
        a, b = open(os.path.join(got, f), "rb").read(), open(os.path.join(want, f), "rb").read()
        if a != b:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            return "%s differs: %d and %d bytes, first at byte %d" % (f, len(a), len(b), first)
    return None


# ------------------------------------------------------------------------------------------------ the recordings
@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["csr_ip", "csr_l2", "drm_ip", "drm_l2"])
def test_goldens(tmp_path, name, device_form):
    want = os.path.join(GOLDEN, name)
    ix = hr.read_folder(want)
    train(ix.items, str(tmp_path / "m"), ix.metric, 8, 100, device_form=device_form)
    assert same_bytes(str(tmp_path / "m"), want) is None, same_bytes(str(tmp_path / "m"), want)


# ------------------------------------------------------------------------------------------------ the live reference
def disjoint_rows(n):
    """Rows that share no id: every distance is 1.0 (ip) or 0.0 (l2), every heap, heuristic and sort decision a tie."""
    return smat.csr_matrix((np.linspace(0.5, 1.5, n).astype(np.float32), np.arange(n), np.arange(n + 1)), shape=(n, n))


def items_of(kind, n, dim, seed):
    return hr.sparse_items(n, dim, min(dim, 9), seed) if kind == "csr" else hr.dense_items(n, dim, seed)


# kind, metric, rows, dim, M, efC, max_level_upper_bound: rows 1, 2, 3, M + 1, 2 M + 1, 300, 1500, 4200; M 2, 8, 12 (maxM0 24: introsort), 32 (64);
# efC 1, M - 1, M, 100; the bound 0, 1, -1; dense dimensions 3, 16, 35, 130
LIVE = [("csr", "ip", 1, 40, 8, 100, -1), ("drm", "l2", 2, 3, 8, 100, -1), ("csr", "l2", 3, 40, 2, 1, -1), ("drm", "ip", 3, 16, 2, 2, 0), ("drm", "ip", 9, 16, 8, 7, -1),
        ("csr", "ip", 17, 40, 8, 8, 0), ("drm", "l2", 5, 35, 2, 2, 1), ("csr", "l2", 25, 30, 12, 11, 1), ("drm", "l2", 65, 130, 32, 31, -1),
        ("csr", "ip", 300, 60, 12, 100, -1), ("drm", "l2", 300, 130, 12, 12, -1), ("drm", "ip", 300, 35, 32, 100, 1), ("csr", "l2", 300, 60, 32, 32, 0),
        ("drm", "ip", 300, 3, 2, 1, -1), ("drm", "ip", 1500, 16, 8, 100, -1), ("csr", "l2", 1500, 80, 2, 100, -1), ("csr", "ip", 1500, 80, 8, 100, 1),
        ("csr", "ip", 4200, 80, 8, 20, -1)]                   # (above 4096 nodes the cand heap of a search is in HBM)


def against_reference(tmp_path, X, metric, M, efC, bound):
    kind = "csr" if smat.issparse(X) else "drm"
    if not hr.have_reference():
        pytest.skip("the compiled reference (oracle/_ref) is not here")
    if kind == "drm" and not hr.host_has_avx512f():
        pytest.skip("dense indexes are pinned to the reference's avx512f clone; this host has no avx512f")
    want = hr.train_reference(X, str(tmp_path / "ref"), metric=metric, M=M, efC=efC, threads=1, max_level_upper_bound=bound)
    train(X, str(tmp_path / "m"), metric, M, efC, bound)
    assert same_bytes(str(tmp_path / "m"), want) is None, same_bytes(str(tmp_path / "m"), want)


@pytest.mark.parametrize("case", LIVE, ids=lambda c: "-".join(str(v) for v in c))
def test_live_reference(tmp_path, case):
    kind, metric, n, dim, M, efC, bound = case
    against_reference(tmp_path, items_of(kind, n, dim, 7 * n + dim + M), metric, M, efC, bound)


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("kind", ["csr", "drm"])
def test_duplicated_rows(tmp_path, kind, metric):
    X = items_of(kind, 20, 16, 3)[np.arange(200) % 20]
    against_reference(tmp_path, X, metric, 8, 100, -1)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_every_decision_a_tie(tmp_path, metric):
    against_reference(tmp_path, disjoint_rows(150), metric, 12, 100, -1)


# ------------------------------------------------------------------------------------------------ the sort forms, search, end to end
def test_sort_forms(tmp_path):
    clib = __import__("pecos_amd").clib
    clib.debug_hnsw_train_counters(reset=True)
    train(disjoint_rows(60), str(tmp_path / "t"), "ip", 12, 100)
    c = clib.debug_hnsw_train_counters(reset=True)
    assert c["sort_replay"] > 0 and c["rewritten"] > 0, c
    train(hr.dense_items(200, 35, 11), str(tmp_path / "g"), "ip", 8, 100)
    c = clib.debug_hnsw_train_counters()
    assert c["sort_replay"] == 0 and c["sort_rank"] >= 200 and min(c["dist_search"], c["dist_select"], c["dist_reverse"]) > 0, c


def test_search_on_a_trained_index(tmp_path):
    X, Q = hr.sparse_items(400, 50, 8, 21), hr.sparse_items(30, 50, 8, 22)
    m = train(X, str(tmp_path / "m"), "ip", 8, 100)
    loaded = HNSW().load(str(tmp_path / "m"))
    pp = m.PredParams(efS=40, topk=10)
    a, b = m.predict(Q, pred_params=pp, ret_csr=False), loaded.predict(Q, pred_params=pp, ret_csr=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert len(set(a[0][0])) == 10


def test_label_embedding_to_predict_without_a_host_copy(tmp_path):
    import pecos_amd
    Y = hr.sparse_items(300, 120, 3, 31)                       # samples x labels
    Xf = hr.sparse_items(300, 64, 6, 32)                       # samples x features
    emb = pecos_amd.label_embedding_device(Y, Xf, method="pifa")
    params = dict(M=8, efC=100, metric_type="ip")
    m = HNSW().train_device(emb, params)
    idx, dist, count = pecos_amd.hnsw_predict_device(m, emb, efS=30, topk=5)
    host = emb.download()                                      # the folder path: the same embedding through train, save, load, predict
    train(host, str(tmp_path / "m"), "ip", 8, 100)
    want = HNSW().load(str(tmp_path / "m")).predict(host, pred_params=m.PredParams(efS=30, topk=5), ret_csr=False)
    assert np.array_equal(idx.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(dist.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    assert int(count.min()) == 5
