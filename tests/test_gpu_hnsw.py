"""HNSW search on the device (K17) against the numpy statement of the rule (tests/hnsw_rule.py), the recording under tests/golden/hnsw/ and
the compiled reference when oracle/_ref is there (dense under the avx512f gate): ids, order, distance bits, counts, untouched tails, and the
counters -- distance evaluations, pops, admissions, upper-level passes, the largest cand size, the heap form -- so that "the same traversal"
is checked and not only "the same answer"."""
import ctypes
import json
import os

import numpy as np
import pytest
import scipy.sparse as smat

import hnsw_rule as hr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hnsw")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
PI, PF = 0xDEADBEEF, np.float32(-7.5)            # what the outputs hold before a call: a row's tail keeps it
TRACED = ("dist", "pops", "admissions", "passes", "max_cand")


def live(kind):
    return hr.have_reference() and (kind == "csr" or hr.host_has_avx512f())


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def first_difference(got, want):
    """(row, position, got bits, wanted bits) of the first entry whose bits differ, for the assertion's message."""
    g, w = got.view(np.uint32), want.view(np.uint32)
    r, k = np.argwhere(g != w)[0]
    return int(r), int(k), hex(g[r, k]), hex(w[r, k])


def check(folder, ix, Q, efS, topk, m=None, searchers=None, form=None, what=""):
    """One host call against the statement (answer, tails, counters) and the live reference; -> the counters."""
    own = m is None
    m = m or hr.Ours(folder)
    assert m.error is None, m.error
    try:
        hr.counters(reset=True)
        idx, dist, err = m.predict(Q, efS, topk, searchers=searchers, fill_idx=PI, fill_val=PF)
        c = hr.counters()
        assert err is None, err
        want = hr.statement(ix, Q, efS, topk, fill_idx=PI, fill_val=PF)
        assert np.array_equal(idx, want[0]), (what, "ids, order or untouched tails differ from the statement")
        assert np.array_equal(dist.view(np.uint32), want[1].view(np.uint32)), (what, "distance bits differ from the statement", first_difference(dist, want[1]))
        assert {k: c[k] for k in TRACED} == {k: want[3][k] for k in TRACED} or Q.shape[0] == 0, (what, c, want[3])
        cap = hr.caps()["CAP"]
        rows = Q.shape[0]
        assert (c["lds_queries"], c["hbm_queries"]) == ((rows, 0) if max(efS, topk) <= cap else (0, rows)), (what, c)
        if form:
            assert c[form + "_queries"] == rows
        if live(ix.data_type):
            assert same((idx, dist), hr.run_reference(folder, Q, efS, topk, fill_idx=PI, fill_val=PF)), (what, "differs from the live reference")
        return c
    finally:
        if own:
            m.close()


def graph_index(items, deg, seed, metric, levels=0, maxM0=None, maxM=None):
    l0, l1, lv, init = hr.random_graph(items.shape[0], deg, seed, levels=levels, maxM=maxM)
    return hr.Index(items, l0, l1, maxM=maxM, maxM0=maxM0, max_level=lv, init_node=init, metric=metric)


# ------------------------------------------------------------------------------------------------ distances
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("ln", [1, 3, 4, 15, 16, 17, 19, 35, 64, 67, 130])
def test_dense_lengths(tmp_path, ln, metric):
    ix = graph_index(hr.dense_items(40, ln, 100 + ln), 6, ln, metric, levels=1)
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    check(folder, ix, hr.dense_items(5, ln, 200 + ln), 10, 5)
    full = hr.Index(ix.items[:9], hr.full_graph(9), metric=metric)        # every item returned: the answer reads every distance
    check(hr.write_folder(full, str(tmp_path / "f")), full, hr.dense_items(3, ln, 300 + ln), 9, 9)


SPARSE_LENS = [0, 1, 3, 4, 5, 63, 64, 65, 129]


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_sparse_row_lengths_and_a_query_sharing_no_id(tmp_path, metric):
    n = 3 * len(SPARSE_LENS)
    items = hr.sparse_items(n, 400, 0, 7, lengths=SPARSE_LENS * 3)
    items.resize((n, 420))                                                 # ids 400 .. 419 belong to no item
    Q = hr.sparse_items(len(SPARSE_LENS), 400, 0, 8, lengths=SPARSE_LENS)
    Q.resize((Q.shape[0], 420))
    lone = smat.csr_matrix((np.ones(5, np.float32), (np.zeros(5, int), np.arange(405, 410))), shape=(1, 420))
    Q = smat.vstack([Q, lone]).tocsr().astype(np.float32)
    ix = hr.Index(items, hr.full_graph(n), metric=metric)
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    check(folder, ix, Q, n, n)
    m = hr.Ours(folder)
    idx, dist, err = m.predict(Q[-1], n, n)
    m.close()
    assert err is None and set(dist[0].tolist()) == ({0.0} if metric == "l2" else {1.0})


# ------------------------------------------------------------------------------------------------ graph shapes
@pytest.mark.parametrize("kind", ["drm", "csr"])
def test_degrees_under_maxM0_128(tmp_path, kind):
    n = 200
    items = hr.dense_items(n, 6, 3) if kind == "drm" else hr.sparse_items(n, 30, 5, 3)
    degs = [0, 1, 127, 128, 63, 64, 65]
    rs = np.random.RandomState(4)
    l0 = []
    for i in range(n):
        d = degs[i % len(degs)] if i else 128
        l0.append(np.array([j for j in rs.permutation(n) if j != i][:d], dtype=np.uint32))
    ix = hr.Index(items, l0, maxM0=128, metric="l2" if kind == "drm" else "ip")
    Q = hr.dense_items(6, 6, 5) if kind == "drm" else hr.sparse_items(6, 30, 6, 5)
    check(hr.write_folder(ix, str(tmp_path / "m")), ix, Q, 30, 10)


def test_degrees_at_maxM0_and_below(tmp_path):
    items = hr.dense_items(30, 5, 3)
    l0 = [np.array([j for j in range(30) if j != i][:(8, 7, 1, 0)[i % 4] if i else 8], dtype=np.uint32) for i in range(30)]
    ix = hr.Index(items, l0, maxM0=8, metric="ip")
    check(hr.write_folder(ix, str(tmp_path / "m")), ix, hr.dense_items(4, 5, 6), 12, 6)


def test_a_neighbourhood_above_the_lds_degree(tmp_path):
    n = hr.caps()["lds_degree"] + 44
    ix = hr.Index(hr.dense_items(n, 3, 1), hr.full_graph(n), metric="l2")
    check(hr.write_folder(ix, str(tmp_path / "m")), ix, hr.dense_items(2, 3, 2), 20, 20)


@pytest.mark.parametrize("levels", [0, 1, 4])
@pytest.mark.parametrize("kind", ["drm", "csr"])
def test_max_level(tmp_path, levels, kind):
    items = hr.dense_items(80, 7, 11) if kind == "drm" else hr.sparse_items(80, 40, 6, 11)
    ix = graph_index(items, 5, 12, "ip", levels=levels, maxM=3)
    Q = hr.dense_items(6, 7, 13) if kind == "drm" else hr.sparse_items(6, 40, 8, 13)
    c = check(hr.write_folder(ix, str(tmp_path / "m")), ix, Q, 8, 4)
    assert (c["passes"] >= 6 * levels) and (levels or c["passes"] == 0)


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_nodes(tmp_path, n):
    ix = hr.Index(hr.dense_items(n, 4, 1), hr.full_graph(n), maxM0=2, metric="l2")
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    for efS, topk in ((1, 1), (5, 3), (3, 5)):
        check(folder, ix, hr.dense_items(3, 4, 2), efS, topk, what=(n, efS, topk))


def test_topk_and_efS(tmp_path):
    ix = graph_index(hr.dense_items(50, 9, 21), 6, 22, "ip", levels=1)
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    Q = hr.dense_items(5, 9, 23)
    m = hr.Ours(folder)
    for efS, topk in ((1, 1), (1, 7), (7, 7), (20, 7), (7, 20), (60, 60), (10, 80)):      # 80 > num_node: tails stay untouched
        check(folder, ix, Q, efS, topk, m=m, what=(efS, topk))
    m.close()


def test_heap_forms_at_cap(tmp_path):
    cap = hr.caps()["CAP"]
    n = cap + 76
    ix = graph_index(hr.dense_items(n, 4, 31), 8, 32, "l2")
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    Q = hr.dense_items(2, 4, 33)
    m = hr.Ours(folder)
    for ef, form in ((cap - 1, "lds"), (cap, "lds"), (cap + 1, "hbm")):
        check(folder, ix, Q, ef, 10, m=m, form=form, what=ef)
    check(folder, ix, Q, 5, cap + 1, m=m, form="hbm", what="topk above CAP")
    m.close()


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("kind", ["drm", "csr"])
def test_an_index_of_identical_items(tmp_path, kind):
    n = 70
    one = hr.dense_items(1, 5, 3) if kind == "drm" else hr.sparse_items(1, 20, 4, 3)
    items = np.tile(one, (n, 1)) if kind == "drm" else smat.vstack([one] * n).tocsr()
    ix = graph_index(items, 9, 5, "ip", levels=1)
    Q = hr.dense_items(3, 5, 4) if kind == "drm" else hr.sparse_items(3, 20, 6, 4)
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    for efS, topk in ((70, 70), (20, 10), (5, 30)):
        check(folder, ix, Q, efS, topk, what=(efS, topk))


def test_two_clumps_of_duplicates_and_a_disconnected_component(tmp_path):
    a, b = hr.dense_items(2, 6, 9)
    items = np.vstack([np.tile(a, (20, 1)), np.tile(b, (20, 1)), hr.dense_items(10, 6, 10)])
    l0, _, _, _ = hr.random_graph(40, 6, 11)
    l0 += [np.array([40 + (i + 1) % 10, 40 + (i + 3) % 10], dtype=np.uint32) for i in range(10)]       # nodes 40 .. 49: reachable from nowhere
    ix = hr.Index(items, l0, maxM0=8, metric="l2")
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    Q = np.vstack([a, b, hr.dense_items(2, 6, 12)]).astype(np.float32)
    for efS, topk in ((50, 50), (30, 10), (3, 45)):           # topk 50 > the 40 reachable nodes: 40 entries, the rest untouched
        c = check(folder, ix, Q, efS, topk, what=(efS, topk))
    m = hr.Ours(folder)
    idx, dist, err = m.predict(Q, 50, 50, fill_idx=PI, fill_val=PF)
    m.close()
    assert (idx[:, 40:] == PI).all() and (idx[:, :40] < 40).all()


def test_upper_level_best_neighbour_ties_with_the_current_node(tmp_path):
    """Level 1: node 0 lists [1, 2, 3]; 1 ties with 0 (not taken: the test is strict), 2 and 3 tie below it (the first j wins)."""
    items = np.array([[4.0], [4.0], [2.0], [2.0]], dtype=np.float32)
    l0 = [[], [], [], []]                                   # level 0 adds nothing: the answer is where the upper level ended
    ix = hr.Index(items, l0, {(0, 1): [1, 2, 3], (1, 1): [0], (2, 1): [3], (3, 1): [2]}, maxM=3, maxM0=4, max_level=1, init_node=0, metric="l2")
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    Q = np.zeros((1, 1), dtype=np.float32)
    check(folder, ix, Q, 1, 1)
    assert hr.statement(ix, Q, 1, 1)[0][0, 0] == 2


def test_per_pass_upper_level_update(tmp_path):
    items = np.array([[4.0], [3.0], [2.0], [2.5]], dtype=np.float32)
    ix = hr.Index(items, [[], [], [], []], {(0, 1): [1, 2], (1, 1): [3]}, maxM=2, maxM0=4, max_level=1, init_node=0, metric="l2")
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    m = hr.Ours(folder)
    idx, _, err = m.predict(np.zeros((1, 1), dtype=np.float32), 1, 1)
    m.close()
    assert err is None and idx[0, 0] == 2


# ------------------------------------------------------------------------------------------------ scratch and slots
def test_a_small_cand_capacity_makes_queries_run_again(tmp_path, monkeypatch):
    ix = graph_index(hr.dense_items(120, 8, 41), 8, 42, "ip", levels=1)
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    Q = hr.dense_items(9, 8, 43)
    monkeypatch.setenv("XRL_HNSW_CAND_CAP", "6")
    c = check(folder, ix, Q, 40, 10)
    assert c["rerun"] > 0 and c["max_cand"] > 6
    monkeypatch.delenv("XRL_HNSW_CAND_CAP")
    assert check(folder, ix, Q, 40, 10)["rerun"] == 0


@pytest.mark.parametrize("kind", ["drm", "csr"])
def test_more_queries_than_slots_and_searchers_reused(tmp_path, kind):
    items = hr.dense_items(90, 10, 51) if kind == "drm" else hr.sparse_items(90, 50, 6, 51)
    ix = graph_index(items, 7, 52, "l2", levels=1)
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    Q = hr.dense_items(65, 10, 53) if kind == "drm" else hr.sparse_items(65, 50, 8, 53)
    m = hr.Ours(folder)
    s = m.searchers(3)
    assert s
    cap = hr.caps()["CAP"]
    for efS, topk in ((5, 5), (50, 10), (cap + 5, 3), (7, 2)):             # a clean visited set on every reuse, across heap forms
        check(folder, ix, Q, efS, topk, m=m, searchers=s, what=(efS, topk))
    m.free_searchers(s)
    m.close()


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 1000])
def test_query_row_counts(tmp_path, rows):
    ix = graph_index(hr.dense_items(40, 6, 61), 5, 62, "ip")
    check(hr.write_folder(ix, str(tmp_path / "m")), ix, hr.dense_items(rows, 6, 63).reshape(rows, 6), 5, 3)


# ------------------------------------------------------------------------------------------------ the resident form
def test_resident_form_caller_buffers_strides_and_a_side_stream(tmp_path):
    import torch
    from pecos_amd import clib
    ix = graph_index(hr.dense_items(60, 7, 71), 6, 72, "l2", levels=1)
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    Q = hr.dense_items(33, 7, 73)
    rows, dim, topk, xs, os_ = 33, 7, 6, 12, 9
    h = clib.hnsw_load(os.path.join(folder, "c_model"), 0)
    dev = torch.device("cuda:0")
    xbuf = torch.full((1 + rows * xs + 3,), float("nan"), dtype=torch.float32, device=dev)            # poison between the rows
    xview = xbuf[1:1 + rows * xs].view(rows, xs)
    xview[:, :dim] = torch.from_numpy(Q).to(dev)
    ibuf = torch.full((1 + rows * os_ + 2,), -559038737, dtype=torch.int32, device=dev)
    dbuf = torch.full((1 + rows * os_ + 2,), -7.5, dtype=torch.float32, device=dev)
    cbuf = torch.full((rows + 2,), -3, dtype=torch.int32, device=dev)
    want = hr.statement(ix, Q, 20, topk)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    s = clib.hnsw_searchers_create(h, 4)
    for stream, searchers in ((None, None), (side.cuda_stream, None), (side.cuda_stream, s)):
        ibuf.fill_(-559038737), dbuf.fill_(-7.5), cbuf.fill_(-3)
        torch.cuda.synchronize()
        clib.hnsw_predict_device(h, rows, dim, xbuf.data_ptr() + 4, xs, None, None, 0, 20, topk, ibuf.data_ptr() + 4, dbuf.data_ptr() + 4, cbuf.data_ptr() + 4, os_,
                                 searchers=searchers, stream=stream)
        i, d, c = ibuf.cpu().numpy(), dbuf.cpu().numpy(), cbuf.cpu().numpy()
        assert i[0] == -559038737 and (i[1 + rows * os_:] == -559038737).all() and d[0] == -7.5 and c[0] == -3 and c[-1] == -3
        iv, dv = i[1:1 + rows * os_].reshape(rows, os_), d[1:1 + rows * os_].reshape(rows, os_)
        assert np.array_equal(iv[:, :topk].view(np.uint32), want[0]) and np.array_equal(dv[:, :topk].view(np.uint32), want[1].view(np.uint32))
        assert (iv[:, topk:] == -559038737).all() and (dv[:, topk:] == -7.5).all()                      # the sentinels of the wider stride
        assert np.array_equal(c[1:1 + rows], want[2].astype(np.int32))
    clib.hnsw_searchers_destruct(s)
    clib.hnsw_destruct(h)


def test_python_class_and_resident_csr(tmp_path):
    import torch
    import pecos_amd
    items = hr.sparse_items(70, 40, 6, 81)
    ix = graph_index(items, 6, 82, "ip", levels=1)
    folder = hr.write_folder(ix, str(tmp_path / "m"), pred_kwargs={"efS": 30, "topk": 8})
    Q = hr.sparse_items(9, 40, 7, 83)
    m = pecos_amd.HNSW.load(folder, lazy_load=True)
    assert (m.data_type, m.metric_type, m.num_item, m.feat_dim) == ("csr", "ip", 70, 40) and m.info["num_node"] == 70
    want = hr.statement(ix, Q, 30, 8)
    Yp = m.predict(Q)
    assert Yp.shape == (9, 70) and np.array_equal(Yp.indptr, np.arange(0, 80, 8)) and np.array_equal(Yp.indices.reshape(9, 8), want[0])
    assert np.array_equal(Yp.data.reshape(9, 8).view(np.uint32), want[1].view(np.uint32))
    s = m.searchers_create(2)
    i2, d2 = m.predict(Q, pred_params=m.PredParams(efS=5, topk=12, threads=3), searchers=s, ret_csr=False)
    w2 = hr.statement(ix, Q, 5, 12)
    assert np.array_equal(i2, w2[0]) and np.array_equal(d2.view(np.uint32), w2[1].view(np.uint32))
    dev = "cuda:0"
    triple = (torch.from_numpy(Q.indptr.astype(np.int64)).to(dev), torch.from_numpy(Q.indices.astype(np.int32)).to(dev), torch.from_numpy(Q.data).to(dev))
    for X in (triple, pecos_amd.DeviceMatrix.upload(Q)):
        idx, dist, cnt = pecos_amd.hnsw_predict_device(m, X, searchers=s)
        assert np.array_equal(idx.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(dist.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
        assert np.array_equal(cnt.cpu().numpy(), want[2].astype(np.int32))
    with pytest.raises(ValueError, match="data_type=drm is NOT consistent"):
        pecos_amd.hnsw_predict_device(m, torch.zeros((2, 40), device=dev))


def test_label_embedding_as_the_queries_of_a_sparse_index(tmp_path):
    import pecos_amd
    rs = np.random.RandomState(5)
    Y = smat.random(60, 12, density=0.2, format="csr", dtype=np.float32, random_state=rs)
    X = hr.sparse_items(60, 50, 6, 91)
    ix = graph_index(hr.sparse_items(100, 50, 7, 92), 6, 93, "ip", levels=1)
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    m = pecos_amd.HNSW.load(folder)
    E = pecos_amd.label_embedding_device(Y, X)                              # labels x features, left in HBM
    idx, dist, cnt = pecos_amd.hnsw_predict_device(m, E, efS=20, topk=5)
    Eh = E.download()
    Eh.sort_indices()
    i2, d2 = m.predict(Eh, pred_params=m.PredParams(efS=20, topk=5), ret_csr=False)
    assert np.array_equal(idx.cpu().numpy().view(np.uint32), i2) and np.array_equal(dist.cpu().numpy().view(np.uint32), d2.view(np.uint32))
    want = hr.statement(ix, Eh, 20, 5)
    assert np.array_equal(i2, want[0]) and np.array_equal(d2.view(np.uint32), want[1].view(np.uint32))


# ------------------------------------------------------------------------------------------------ the recording and the live reference
@pytest.mark.parametrize("name", sorted(MANIFEST["cases"]))
def test_every_golden_index_at_every_recorded_setting(name):
    folder = os.path.join(GOLDEN, name)
    kind = MANIFEST["cases"][name]["data_type"]
    Q = np.load(os.path.join(folder, "queries.npy")) if kind == "drm" else smat.load_npz(os.path.join(folder, "queries.npz")).tocsr()
    exp = np.load(os.path.join(folder, "expected.npz"))
    m = hr.Ours(folder)
    assert m.error is None, m.error
    for efS, topk in MANIFEST["settings"]:
        idx, dist, err = m.predict(Q, efS, topk)
        assert err is None and np.array_equal(idx, exp["idx_%d_%d" % (efS, topk)]), (name, efS, topk)
        assert np.array_equal(dist.view(np.uint32), exp["bits_%d_%d" % (efS, topk)]), (name, efS, topk)
    m.close()


@pytest.mark.parametrize("kind", ["drm", "csr"])
def test_5000_items_trained_by_the_live_reference(tmp_path, kind):
    if not live(kind):
        pytest.skip("needs the compiled reference" + (" and avx512f on this host" if kind == "drm" else ""))
    items = hr.dense_items(5000, 32, 101) if kind == "drm" else hr.sparse_items(5000, 500, 12, 101)
    Q = hr.dense_items(16, 32, 102) if kind == "drm" else hr.sparse_items(16, 500, 14, 102)
    folder = hr.train_reference(items, str(tmp_path / "m"), metric="l2" if kind == "drm" else "ip", M=8)
    ix = hr.read_folder(folder)
    check(folder, ix, Q, 50, 10)


# ------------------------------------------------------------------------------------------------ refusals, outputs unchanged
def test_refusals_leave_the_outputs_unchanged(tmp_path):
    dense = graph_index(hr.dense_items(20, 4, 1), 4, 2, "ip")
    sparse = graph_index(hr.sparse_items(20, 10, 3, 1), 4, 2, "ip")
    md, ms = hr.Ours(hr.write_folder(dense, str(tmp_path / "d"))), hr.Ours(hr.write_folder(sparse, str(tmp_path / "s")))
    Qd, Qs = hr.dense_items(3, 4, 5), hr.sparse_items(3, 10, 4, 5)

    def refused(m, Q, efS, topk, words):
        idx, dist = np.full((Q.shape[0], 2), PI, np.uint32), np.full((Q.shape[0], 2), PF, np.float32)
        view, keep, kind = hr._view(Q)
        rc = getattr(m.lib, "xrl_hnsw_predict_%s_f32" % kind)(m.h, ctypes.byref(view), idx.ctypes.data, dist.ctypes.data, efS, topk, 1, None)
        err = hr.last_error(m.lib) if rc else None
        assert err is not None and err.startswith("xrl_hnsw_predict_") and words in err, err
        assert (idx == PI).all() and (dist == PF).all()

    refused(md, Qs[:, :4], 5, 2, "the index holds drm items, the queries are csr")
    refused(ms, Qd, 5, 2, "the index holds csr items, the queries are drm")
    refused(md, hr.dense_items(3, 5, 5), 5, 2, "X has 5 columns, the index has feat_dim = 4")
    refused(md, Qd, 0, 2, "efS == 0")
    refused(md, Qd, 5, 0, "topk == 0")
    bad = Qd.copy()
    bad[1, 2] = np.nan
    refused(md, bad, 5, 2, "a query value is not finite")
    bad = Qs.copy()
    bad.data[1] = np.inf
    refused(ms, bad, 5, 2, "a query value is not finite")
    bad = Qs.copy()
    bad.indices[0:2] = bad.indices[0:2][::-1].copy()
    refused(ms, bad, 5, 2, "unsorted or repeated column ids")
    bad = Qs.copy()
    bad.indices[1] = bad.indices[0]
    refused(ms, bad, 5, 2, "unsorted or repeated column ids")
    bad = Qs.copy()
    bad.indices[3] = 10
    refused(ms, bad, 5, 2, "a column id at or above feat_dim = 10")
    check(str(tmp_path / "d"), dense, Qd, 5, 2, m=md)                       # and the handles still serve
    md.close(), ms.close()


def test_resident_form_refusals_leave_the_outputs_unchanged(tmp_path):
    import torch
    from pecos_amd import clib
    dev = torch.device("cuda:0")
    dense = graph_index(hr.dense_items(20, 4, 1), 4, 2, "ip")
    sparse = graph_index(hr.sparse_items(20, 10, 3, 1), 4, 2, "ip")
    hd = clib.hnsw_load(os.path.join(hr.write_folder(dense, str(tmp_path / "d")), "c_model"), 0)
    hs = clib.hnsw_load(os.path.join(hr.write_folder(sparse, str(tmp_path / "s")), "c_model"), 0)
    h2 = clib.hnsw_load(os.path.join(str(tmp_path / "d"), "c_model"), 0)        # the same folder loaded again: another index
    Qd, Qs = hr.dense_items(3, 4, 5), hr.sparse_items(3, 10, 4, 5)
    xd = torch.from_numpy(Qd).to(dev)
    crow, col, val = (torch.from_numpy(a).to(dev) for a in (Qs.indptr.astype(np.int64), Qs.indices.astype(np.int32), Qs.data))
    rows, topk, stride = 3, 2, 4
    idx = torch.full((rows, stride), -559038737, dtype=torch.int32, device=dev)
    dist = torch.full((rows, stride), -7.5, dtype=torch.float32, device=dev)
    cnt = torch.full((rows,), -3, dtype=torch.int32, device=dev)
    s_d = clib.hnsw_searchers_create(hd, 2)

    def refused(words, h=hd, X=None, row_stride=4, out=None, out_stride=stride, searchers=None, cols=None):
        o = out or (idx.data_ptr(), dist.data_ptr(), cnt.data_ptr())
        with pytest.raises(RuntimeError, match=words) as e:
            if X is None:
                clib.hnsw_predict_device(h, rows, cols or 4, xd.data_ptr(), row_stride, None, None, 0, 5, topk, o[0], o[1], o[2], out_stride, searchers=searchers)
            else:
                clib.hnsw_predict_device(h, rows, cols or 10, X[2].data_ptr(), 0, X[0].data_ptr(), X[1].data_ptr(), X[2].numel(), 5, topk, o[0], o[1], o[2], out_stride,
                                         searchers=searchers)
        assert str(e.value).startswith("xrl_hnsw_predict_device: ")
        torch.cuda.synchronize()
        assert bool((idx == -559038737).all()) and bool((dist == -7.5).all()) and bool((cnt == -3).all())

    refused("out_stride = 1 is below topk = 2", out_stride=1)
    refused("row_stride = 3 is below feat_dim = 4", row_stride=3)
    refused("null argument \\(d_idx / d_dist / d_count\\)", out=(0, dist.data_ptr(), cnt.data_ptr()))
    refused("null argument \\(d_idx / d_dist / d_count\\)", out=(idx.data_ptr(), 0, cnt.data_ptr()))
    refused("null argument \\(d_idx / d_dist / d_count\\)", out=(idx.data_ptr(), dist.data_ptr(), 0))
    refused("the searchers belong to another index", h=h2, searchers=s_d)
    refused("the searchers belong to another index", h=hs, X=(crow, col, val), searchers=s_d)
    refused("the index holds drm items, the queries are csr", X=(crow, col, val), cols=4)
    refused("X has 9 columns, the index has feat_dim = 10", h=hs, X=(crow, col, val), cols=9)
    down = crow.clone()
    down[1], down[2] = int(crow[2]), int(crow[1])                                # [0, 8, 4, 12]: the row pointers go down
    refused("the row pointers of X are not ascending within its stored entries", h=hs, X=(down, col, val))
    beyond = crow.clone()
    beyond[3] = int(crow[3]) + 5                                                 # the last row ends past nnz
    refused("the row pointers of X are not ascending within its stored entries", h=hs, X=(beyond, col, val))
    bad = val.clone()
    bad[1] = float("nan")
    refused("a query value is not finite", h=hs, X=(crow, col, bad))
    # the handles and the searchers still serve
    clib.hnsw_predict_device(hd, rows, 4, xd.data_ptr(), 4, None, None, 0, 5, topk, idx.data_ptr(), dist.data_ptr(), cnt.data_ptr(), stride, searchers=s_d)
    want = hr.statement(dense, Qd, 5, topk)
    assert np.array_equal(idx.cpu().numpy()[:, :topk].view(np.uint32), want[0]) and bool((idx[:, topk:] == -559038737).all())
    import pecos_amd
    with pytest.raises(ValueError, match="one-dimensional CUDA tensors on one device"):
        pecos_amd.hnsw_predict_device(pecos_amd.HNSW(None, 20, 10, "csr", "ip"), (crow, col.cpu(), val))
    with pytest.raises(ValueError, match="col and val one per stored entry"):
        pecos_amd.hnsw_predict_device(pecos_amd.HNSW(None, 20, 10, "csr", "ip"), (crow, col[:-1], val))
    clib.hnsw_searchers_destruct(s_d)
    for h in (hd, hs, h2):
        clib.hnsw_destruct(h)
