"""PairwiseANN on the device (K18) against the numpy statement of the rule (test_pairwise_cpu.statement): row ids, mask, distance bits, Y values
and the form counters, exactly; the compiled reference on the same inputs as a second witness where it is present.

+0 against -0 distances: the data cannot produce them.  A distance is (float)(1.0 - (double)dot), and in round-to-nearest a difference is -0
only for (-0) - (+0); 1.0 - 1.0 is +0.  The case is dropped; the kernel's tie test treats the two zeros as equal all the same."""
import filecmp

import numpy as np
import pytest
import scipy.sparse as smat

import hnsw_rule as hr
import test_pairwise_cpu as pc
from test_pairwise_cpu import CAP, KEEP, KINDS

pytestmark = pytest.mark.gpu
FORMS = ("sorted", "stream", "replay", "second_pass")


def check(model, X, Yc, Q, keys, k, same=False, searchers=None, witness=True):
    """One predict through the host entry point against the statement (and the reference) -> the counters."""
    from pecos_amd import clib
    keys = np.asarray(keys, dtype=np.uint32)
    want, forms = pc.statement(X, Yc, Q, keys, k, same)
    s = searchers or model.searchers_create(model.PredParams(batch_size=len(keys), only_topk=k))
    clib.debug_pairwise_counters(reset=True)
    got = model.predict(Q, keys, s, is_same_input=same)
    c = clib.debug_pairwise_counters()
    assert pc.same_outputs(got, want), [np.flatnonzero((np.asarray(g).view(np.uint32) != w.view(np.uint32)).any(axis=1)) for g, w in zip(got, want)]
    assert tuple(c[f] for f in FORMS) == forms
    if witness and pc.can_witness(model.data_type):
        assert pc.same_outputs(pc.Reference(model.data_type, X, Yc).predict(Q, keys, k, same), want)
    return c


def trained(kind, X, Yc):
    from pecos_amd.pairwise import PairwiseANN
    return PairwiseANN.train(X, Yc)


def test_caps_are_the_statements():
    from pecos_amd import clib
    caps = clib.debug_pairwise_caps()
    assert (caps["CAP"], caps["KEEP"]) == (CAP, KEEP) and CAP >= 1024


@pytest.mark.parametrize("k", (1, 10))
@pytest.mark.parametrize("kind", KINDS)
def test_distinct_distances_are_served_in_parallel(kind, k):
    lengths = sorted({0, 1, 2, k - 1, k, k + 1, 63, 64, 65, CAP - 1, CAP, CAP + 1, 3 * CAP + 5})
    X, Yc, Q = pc.items(kind, 3 * CAP + 5, 19, 1), pc.columns(3 * CAP + 5, lengths, 2), pc.items(kind, len(lengths), 19, 3)
    c = check(trained(kind, X, Yc), X, Yc, Q, np.arange(len(lengths)), k)
    assert c["replay"] == 0 and c["stream"] == 2 and c["max_col"] == 3 * CAP + 5 and c["dist"] == sum(lengths)


@pytest.mark.parametrize("n", (40, CAP + 40))
@pytest.mark.parametrize("where", ("inside", "across", "beyond", "everywhere"))
@pytest.mark.parametrize("kind", KINDS)
def test_ties_replay_only_where_they_show(kind, where, n):
    X, Yc, Q = pc.tie_case(kind, where, n)
    c = check(trained(kind, X, Yc), X, Yc, Q, [0], 10)
    assert c["replay"] == (0 if where == "beyond" else 1) and c["second_pass"] == (1 if where != "beyond" and n > CAP else 0)


@pytest.mark.parametrize("kind", KINDS)
def test_forced_replay_by_topk_and_by_nan(kind):
    X, Yc, Q = pc.items(kind, CAP + 1, 19, 4), pc.columns(CAP + 1, [CAP + 1], 5), pc.items(kind, 1, 19, 6)
    model = trained(kind, X, Yc)
    assert check(model, X, Yc, Q, [0], KEEP - 1, witness=False)["stream"] == 1         # only_topk + 1 = KEEP
    c = check(model, X, Yc, Q, [0], KEEP)                                               # KEEP + 1: replayed at once, no second pass
    assert (c["replay"], c["second_pass"]) == (1, 0)
    X, Yc, Q = pc.nan_case(kind)                                                        # an overflow-born NaN (inf + -inf) among the distances
    for k in (3, 8):
        c = check(trained(kind, X, Yc), X, Yc, Q, [0, 1, 0, 1], k, same=True)
        assert c["replay"] >= 2


def test_sparse_rows_of_every_length_and_a_query_that_shares_nothing():
    lens = [0, 1, 63, 64, 65, 5, 7, 9, 600]
    X = hr.sparse_items(len(lens), 700, 0, 1, lengths=lens)
    Q = smat.vstack([hr.sparse_items(len(lens), 700, 0, 2, lengths=lens), smat.csr_matrix(([1.0], ([0], [699])), shape=(1, 700), dtype=np.float32)]).tocsr().astype(np.float32)
    Xz = smat.vstack([X, smat.csr_matrix((20, 700), dtype=np.float32)]).tocsr()        # twenty empty rows: distance 1.0 to every query
    Yc = pc.columns(Xz.shape[0], [len(lens)], 4)
    Yc = smat.hstack([Yc, smat.csc_matrix((np.ones(20, np.float32), (np.arange(9, 29), np.zeros(20, int))), shape=(29, 1)),
                      smat.csc_matrix((np.ones(6, np.float32), (np.arange(9, 15), np.zeros(6, int))), shape=(29, 1))]).tocsc().astype(np.float32)
    model = trained("csr", Xz, Yc)
    check(model, Xz, Yc, Q[:len(lens)], np.zeros(len(lens), int), 10)
    c = check(model, Xz, Yc, Q[len(lens):], [1, 2], 10, same=True)                      # all distances 1.0: n = 20 > k and n = 6 <= k
    assert c["replay"] == 2 and c["dist"] == 26


@pytest.mark.parametrize("dim", (19, 67, 1100))
def test_dense_widths(dim):
    """19 and 67: one width per tail kind of the avx512f clone; 1100: a query too wide for its LDS stage."""
    X, Yc, Q = pc.items("drm", 70, dim, 1), pc.columns(70, [70, 5], 2), pc.items("drm", 2, dim, 3)
    check(trained("drm", X, Yc), X, Yc, Q, [0, 1], 10)


@pytest.mark.parametrize("kind", KINDS)
def test_y_values_explicit_zeros_and_a_row_stored_twice(kind):
    X, Q = pc.items(kind, 12, 19, 1), pc.items(kind, 3, 19, 2)
    ind = np.array([3, 7, 3, 1, 7, 7, 0, 2, 4, 5, 6, 8, 9, 10, 11, 3], dtype=np.int32)                   # row 3 twice in column 0, row 7 three times
    data = np.array([5.0, 0.0, 5.0, -0.0, 2.0, 0.0] + [0.0] * 10, dtype=np.float32)
    Yc = smat.csc_matrix((data, ind, [0, 6, 6, 16]), shape=(12, 3))
    c = check(trained(kind, X, Yc), X, Yc, Q, [0, 1, 2], 4)
    assert c["replay"] == 1                                                                             # column 0: its equal rows tie


@pytest.mark.parametrize("kind", KINDS)
def test_batches_same_input_repeated_labels_and_reused_searchers(kind):
    X, Yc = pc.tie_case(kind, "inside", 200)[0], pc.columns(200, [0, 3, 70, 200, 12], 2)       # two equal rows: the forms change from pair to pair
    model = trained(kind, X, Yc)
    few = model.searchers_create(model.PredParams(batch_size=65, only_topk=10), num_searcher=2)        # more pairs than slots
    for batch in (1, 63, 64, 65):
        keys = np.random.RandomState(batch).randint(0, 5, size=batch)                                   # labels repeat
        Q = pc.items(kind, batch, 19, 10 + batch)
        check(model, X, Yc, Q, keys, 10, searchers=few, witness=batch == 65)
        check(model, X, Yc, Q[:1], keys, 10, same=True, searchers=few, witness=batch == 65)


@pytest.mark.parametrize("kind", KINDS)
def test_resident_form_caller_buffers_and_train_device(kind):
    import torch
    from pecos_amd import DeviceMatrix, clib, pairwise_predict_device
    from pecos_amd.pairwise import PairwiseANN
    X, Yc, Q = pc.items(kind, 300, 19, 1), pc.columns(300, [0, 5, 64, 300], 2), pc.items(kind, 6, 19, 3)
    keys, k, stride = np.array([3, 0, 2, 1, 3, 2], dtype=np.uint32), 10, 13
    want, forms = pc.statement(X, Yc, Q, keys, k)
    dev = torch.device("cuda", 0)
    dX = DeviceMatrix.upload(X) if kind == "csr" else torch.from_numpy(X).to(dev)
    resident = PairwiseANN.train_device(dX, DeviceMatrix.upload(Yc.tocsr()))
    host = trained(kind, X, Yc)
    assert resident.info == host.info
    dkeys = torch.from_numpy(keys.view(np.int32)).to(dev)
    dQ = DeviceMatrix.upload(Q) if kind == "csr" else torch.from_numpy(Q).to(dev)
    for model in (resident, host):
        got = pairwise_predict_device(model, dQ, dkeys, only_topk=k)
        assert pc.same_outputs([g.cpu().numpy() for g in got], want)
    # the caller's buffers: outputs at odd offsets between poison with a wider stride, dense queries with a wider stride, a side stream
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        pool = torch.full((4, 1 + len(keys) * stride + 5), 0x7B7B7B7B, dtype=torch.int32, device=dev)
        if kind == "csr":
            crow, col, val, _ = dQ.to_torch(stream=side.cuda_stream)
            q_args = (6, 19, val.data_ptr(), 0, crow.data_ptr(), col.data_ptr(), val.numel())
        else:
            wide = torch.full((6, 19 + 4), float("nan"), device=dev)
            wide[:, :19] = dQ
            q_args = (6, 19, wide.data_ptr(), 19 + 4, 0, 0, 0)
        clib.debug_pairwise_counters(reset=True)
        clib.pairwise_predict_device(host.model_ptr, None, len(keys), k, *q_args, dkeys.data_ptr(), *(pool[j, 1:].data_ptr() for j in range(4)), stride, False,
                                     stream=side.cuda_stream)
    after = pool.cpu().numpy()
    assert tuple(clib.debug_pairwise_counters()[f] for f in FORMS) == forms
    for j in range(4):
        rows = after[j, 1:1 + len(keys) * stride].reshape(len(keys), stride)
        reached = want[1].astype(bool)
        assert np.array_equal(rows[:, :k][reached], want[j].view(np.int32)[reached])
        rows[:, :k][reached] = 0x7B7B7B7B
    assert (after == 0x7B7B7B7B).all()                                      # nothing else was touched


@pytest.mark.parametrize("kind", KINDS)
def test_save_load_and_the_references_folder(kind, tmp_path):
    from pecos_amd.pairwise import PairwiseANN
    X, Yc, Q = pc.items(kind, 90, 19, 1), pc.columns(90, [0, 5, 90], 2), pc.items(kind, 3, 19, 3)
    model = trained(kind, X, Yc)
    model.save(str(tmp_path / "ours"))
    loaded = PairwiseANN.load(str(tmp_path / "ours"))
    assert loaded.info == model.info and (loaded.num_input_keys, loaded.num_label_keys, loaded.feat_dim, loaded.data_type) == (90, 3, 19, kind)
    check(loaded, X, Yc, Q, [2, 1, 0], 10)
    if hr.have_reference():
        pc.Reference(kind, X, Yc).save(str(tmp_path / "ref"))
        for name in ("config.json", "index.mmap_store"):
            assert filecmp.cmp(tmp_path / "ours" / "c_model" / name, tmp_path / "ref" / "c_model" / name, shallow=False), name
        if pc.can_witness(kind):
            assert pc.same_outputs(pc.Reference(kind, folder=str(tmp_path / "ours")).predict(Q, np.array([2, 1, 0], np.uint32), 10), pc.statement(X, Yc, Q, [2, 1, 0], 10)[0])


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_outputs_and_index_unchanged(kind):
    from pecos_amd.pairwise import PairwiseANN
    X, Yc, Q = pc.items(kind, 30, 19, 1), pc.columns(30, [4, 30], 2), pc.items(kind, 2, 19, 3)
    bad_y = Yc.copy()
    bad_y.indices[5] = 30
    with pytest.raises(RuntimeError, match="Y has a row id at or above X_trn.rows = 30"):
        PairwiseANN.train(X, bad_y)
    with pytest.raises(RuntimeError, match="X_trn.rows != Y_csc.rows"):
        PairwiseANN.train(X[:29], Yc)
    model = trained(kind, X, Yc)
    s = model.searchers_create(model.PredParams(batch_size=2, only_topk=5))

    def damaged(M, what):
        M = M.copy()
        if what == "value":
            (M.data if kind == "csr" else M)[1] = np.inf
        elif what == "order":
            r = int(np.argmax(np.diff(M.indptr) >= 2))
            M.indices[M.indptr[r] + 1] = M.indices[M.indptr[r]]
        else:
            M.indices[M.indptr[1] - 1] = 19
        return M

    cases = [("value", "is not finite")] + ([("order", "unsorted or repeated column ids"), ("range", "at or above feat_dim = 19")] if kind == "csr" else [])
    for what, message in cases:
        with pytest.raises(RuntimeError, match=message):
            PairwiseANN.train(damaged(X, what), Yc)
        with pytest.raises(RuntimeError, match=message):
            model.predict(damaged(Q, what), np.array([0, 1], np.uint32), s)
    for Qb, keys, same, message in ((Q, [0, 2], False, "a label key is at or above num_label_keys = 2"), (Q[:0], [0, 1], True, "is_same_input needs a first row"),
                                    (Q, [0], True, None)):
        s.Imat[:] = 77                                                      # (predict clears the cells it is about to use; the call must not reach them)
        if message is None:
            model.predict(Qb, np.array(keys, np.uint32), s, is_same_input=same)
            assert (s.Imat[5:] == 77).all()                                 # a batch of one writes its own row only
            continue
        with pytest.raises(RuntimeError, match=message):
            model.predict(Qb, np.array(keys, np.uint32), s, is_same_input=same)
        assert (s.Imat[:10] == 0).all() and (s.Mmat[:10] == 0).all()        # refused before any launch wrote
    from pecos_amd import clib
    with pytest.raises(RuntimeError, match="the queries have 2 rows, batch_size = 1"):
        clib.pairwise_predict(model.model_ptr, s.ctypes(), 1, 5, *model.create_pymat(Q), np.zeros(1, np.uint32), s.Imat, s.Mmat, s.Dmat, s.Vmat)
    check(model, X, Yc, Q, [1, 0], 5)                                       # the index still serves
    empty = model.searchers_create(model.PredParams(batch_size=2, only_topk=0))
    assert all(m.shape == (2, 0) for m in model.predict(Q, np.array([0, 1], np.uint32), empty))
