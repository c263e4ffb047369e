"""Cost-sensitive and user-negative training without a GPU: the numpy statements of R1a / R1b (tests/relevance_rule.py) against sklearn's
normalize bit for bit; the two wrong variants of l1 shown wrong; the scipy chain rules against the reference's ClusterChain, recorded
(tests/golden/relevance_chains_ref.npz) and live (where oracle/_ref is built); pecos_amd.ClusterChain's host half; every refusal of
XLinearModel.train_ext and of the two new entry points that needs no GPU; and that XLinearModel.train refuses what it refused."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as smat

import matching_rule as mr
import ranker_training_rule as rr
import relevance_rule as rl

RECORDED = np.load(rl.FIXTURE)
CHAIN = mr.recorded_chain(RECORDED)
GRID = [(ks, norm, induce) for ks in rl.KEYSETS for norm in rl.NORM_TYPES for induce in (True, False)]


# ------------------------------------------------------------------------------------------------ R1a, R1b
@pytest.mark.parametrize("norm", rl.NORMS)
@pytest.mark.parametrize("name", sorted(rl.norm_cases()))
def test_numpy_rule_equals_sklearn_normalize(name, norm):
    sklearn = pytest.importorskip("sklearn")
    from sklearn.preprocessing import normalize
    A = rl.norm_cases()[name]
    if A.shape[0] == 0:
        assert rl.normalize(A, norm).nnz == 0
        return
    with sklearn.config_context(assume_finite=True), np.errstate(all="ignore"):       # (the non-finite rows are part of the contract)
        want = normalize(A.copy(), norm=norm, axis=1)
    assert rl.same_normalized(rl.normalize(A, norm), want, norm), f"{name} under {norm}"
    assert np.array_equal(rl.bits(A.data), rl.bits(rl.norm_cases()[name].data)), "the rule changed its operand"


def test_max_nan_payload_is_numpys_reduction_order_not_the_contract():
    """Under max a row with a NaN becomes NaNs; which payload the others get follows numpy's reduction order, so the rule says 'a NaN'."""
    sklearn = pytest.importorskip("sklearn")
    from sklearn.preprocessing import normalize
    A = rl.norm_cases()["nan"]
    with sklearn.config_context(assume_finite=True), np.errstate(all="ignore"):
        want = normalize(A.copy(), norm="max", axis=1)
    assert np.isnan(want.data).all() and np.isnan(rl.normalize(A, "max").data).all()
    assert rl.same_normalized(rl.normalize(A, "l1"), normalize_l1(A), "l1", nan_rows_exact=True), "under l1 the NaN bits follow from IEEE rules: pinned"


def normalize_l1(A):
    import sklearn
    from sklearn.preprocessing import normalize
    with sklearn.config_context(assume_finite=True), np.errstate(all="ignore"):
        return normalize(A.copy(), norm="l1", axis=1)


@pytest.mark.parametrize("variant,row", [("f32sum", rl.L1_F32SUM_ROW), ("f32div", rl.L1_F32DIV_ROW)])
def test_wrong_l1_variants_differ_on_the_search_found_rows(variant, row):
    pytest.importorskip("sklearn")
    v = row.view(np.float32)
    A = mr.raw_csr((2, 200), [(np.arange(len(v)), v), (np.arange(130), np.resize(v, 130))])
    want = normalize_l1(A)
    assert rl.same_normalized(rl.normalize(A, "l1"), want, "l1")
    wrong = rl.normalize(A, "l1", variant)
    assert not np.array_equal(rl.bits(wrong.data[:len(v)]), rl.bits(want.data[:len(v)])), f"{variant} is not told from R1a by its row"
    found = rl.search_l1_rows()
    assert np.array_equal(found[variant], row), "the kept row is the one the search finds"


def test_sklearn_sums_repeated_ids_under_max_which_is_why_such_rows_are_refused():
    pytest.importorskip("sklearn")
    from sklearn.preprocessing import normalize
    D = rl.duplicate_ids_case()
    want = normalize(D.copy(), norm="max", axis=1)
    assert want.nnz == D.nnz - 1 and np.float32(want[1, 9]) == np.float32(1.0)         # 2.0 + 2.5 is the row's maximum there
    assert not np.array_equal(rl.normalize(D, "max").data[3:7], want.data[3:6])


def test_cases_hold_what_they_promise():
    c = rl.norm_cases()
    assert tuple(np.diff(c["lengths"].indptr)) == rl.LENGTHS
    for name, A in c.items():
        for r in range(A.shape[0]):
            assert np.all(np.diff(A.indices[A.indptr[r]:A.indptr[r + 1]]) > 0), f"{name}: row {r} is not strictly ascending"
    m = c["max_last_of_65"]
    assert np.diff(m.indptr)[0] == 65 and abs(m.data[64]) == np.abs(m.data[:65]).max() and m.data[129] < 0
    assert np.isinf(c["inf"].data).sum() == 5 and np.isnan(c["nan"].data).sum() >= 6
    assert (c["zero_rows"].data == 0).all() and c["zero_rows"].nnz == 74
    assert (np.abs(c["subnormal"].data) < np.finfo(np.float32).tiny).all()


# ------------------------------------------------------------------------------------------------ the check rule
def test_check_rule_orders_its_codes_as_check_relevance_does():
    from pecos_amd.xlinear import check_relevance
    _, Y, _, R = rl.fixture_problem()
    assert rl.check_rule(Y, R) == (0, 0)
    check_relevance(Y, R)
    moved = R.copy()
    moved.indices = moved.indices.copy()
    b = int(moved.indptr[7])
    free = sorted(set(range(rl.LABELS)) - set(moved.indices[b:int(moved.indptr[8])]))[0]
    moved.indices[b] = free
    assert rl.check_rule(Y, moved)[0] == 2 and rl.check_rule(Y, moved)[1] == 7
    with pytest.raises(ValueError, match="Invalid relevance matrix: Y.ind"):
        check_relevance(Y, moved)
    neg = R.copy()
    neg.data = neg.data.copy()
    neg.data[int(neg.indptr[9])] = -1.0
    assert rl.check_rule(Y, neg) == (3, 9)
    with pytest.raises(ValueError, match="got value < 0"):
        check_relevance(Y, neg)
    for v in (-0.0, np.nan):
        neg.data[int(neg.indptr[9])] = v
        assert rl.check_rule(Y, neg) == (0, 0)
        check_relevance(Y, neg)


# ------------------------------------------------------------------------------------------------ the chain rules
def _recorded(prefix):
    return [mr.get_sparse(RECORDED, f"{prefix}__{t}", smat.csr_matrix) for t in range(len(CHAIN))]


def _same_chain(got, want, values, what):
    assert len(got) == len(want) == len(CHAIN), what
    for t, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), f"{what}: level {t}"
        if g is not None:
            g, w = rl.canonical_csr(g), rl.canonical_csr(w)
            assert mr.same_bits(g, w) if values else mr.same_pattern(g, w), f"{what}: level {t}"


def test_fixture_preconditions():
    assert [c.shape for c in CHAIN] == [(4, 1), (16, 4), (48, 16)]
    assert os.path.getsize(rl.FIXTURE) <= os.path.getsize(os.path.join(os.path.dirname(rl.FIXTURE), "man_training_ref.npz"))
    X, Y, C, R = rl.fixture_problem()
    assert X.shape == (rl.N, rl.FEATURES) and Y.shape == (rl.N, rl.LABELS) and C.shape == (rl.LABELS, rl.CODES)
    l1, mx, no = (_recorded(f"rel__k0__{n}__1") for n in ("l1", "max", "no-norm"))
    assert all(m is not None for m in l1) and not mr.same_bits(l1[0], mx[0]) and not mr.same_bits(l1[0], no[0])
    assert _recorded("rel__k0__l1__0")[:2] == [None, None] and _recorded("rel__k1__l1__0")[2] is None
    assert all(m is None for m in _recorded("rel__none__l1__1")) and all(m is None for m in _recorded("match__none"))
    for name in rl.TRAIN_CONFIGS:
        depth = int(RECORDED[f"train__{name}__depth"][0])
        assert depth == {"matcher_1": 2, "matcher_2": 1, "ranker_1": 1, "ranker_2": 2}.get(name, 3), name
    W = lambda n, t: mr.get_sparse(RECORDED, f"train__{n}__W{t}", smat.csc_matrix)      # noqa: E731
    assert not mr.same_bits(W("induce_l1", 2), W("induce_max", 2)) and not mr.same_bits(W("induce_l1", 2), W("induce_l1_R", 2))
    assert not mr.same_bits(W("usn", 2), W("tfn_usn", 2)) and W("ranker_1", 0).shape[1] == rl.LABELS and W("ranker_2", 0).shape[1] == rl.CODES


@pytest.mark.parametrize("keyset,norm,induce", GRID)
def test_relevance_chain_rule_equals_the_recording(keyset, norm, induce):
    got = rl.relevance_chain_rule(rl.partial_dict(rl.KEYSETS[keyset], "R"), CHAIN, norm, induce)
    _same_chain(got, _recorded(f"rel__{keyset}__{norm}__{int(induce)}"), True, f"{keyset} {norm} {induce}")


@pytest.mark.parametrize("keyset", sorted(rl.KEYSETS))
def test_matching_chain_rule_equals_the_recording(keyset):
    got = rl.matching_chain_rule(rl.partial_dict(rl.KEYSETS[keyset], "M"), CHAIN)
    _same_chain(got, _recorded(f"match__{keyset}"), False, keyset)
    for m in got:
        assert m is None or (m.data == 1).all()


@pytest.mark.parametrize("keyset", sorted(rl.KEYSETS))
def test_the_live_reference_equals_the_recording(keyset):
    if not mr.refpy_available():
        pytest.skip("oracle/_ref (the compiled reference and its python package) is not built")
    mr.import_refpy()
    from pecos.utils.cluster_util import ClusterChain
    _, _, C, _ = rl.fixture_problem()
    chain = ClusterChain.from_partial_chain(C, min_codes=rl.NR_SPLITS, nr_splits=rl.NR_SPLITS)
    keys = rl.KEYSETS[keyset]
    for norm in rl.NORM_TYPES:
        for induce in (True, False):
            got = chain.generate_relevance_chain(rl.partial_dict(keys, "R"), norm_type=norm, induce=induce)
            _same_chain(got[-len(CHAIN):] if keys else got[:len(CHAIN)], _recorded(f"rel__{keyset}__{norm}__{int(induce)}"), True, f"{keyset} {norm} {induce}")
    _same_chain(chain.generate_matching_chain(rl.partial_dict(keys, "M"))[:len(CHAIN)], _recorded(f"match__{keyset}"), False, keyset)


# ------------------------------------------------------------------------------------------------ ClusterChain on the host
def test_cluster_chain_from_partial_save_load(tmp_path):
    from pecos_amd import ClusterChain
    _, _, C, _ = rl.fixture_problem()
    chain = ClusterChain.from_partial_chain(C, min_codes=rl.NR_SPLITS, nr_splits=rl.NR_SPLITS)
    assert len(chain) == 3 and [c.shape for c in chain] == [c.shape for c in CHAIN] and chain == ClusterChain(CHAIN)
    assert all(mr.same_bits(rl.canonical_csr(a), rl.canonical_csr(b)) for a, b in zip(chain, CHAIN))
    assert chain[2] is chain.chain[2] and [c.shape for c in chain[-2:]] == [(16, 4), (48, 16)]
    assert len(ClusterChain.from_partial_chain([chain[1], chain[2]], min_codes=rl.NR_SPLITS, nr_splits=rl.NR_SPLITS)) == 3
    assert len(ClusterChain.from_partial_chain(C, min_codes=None)) == 2 and len(ClusterChain(C)) == 1
    chain.save(str(tmp_path / "c"))
    assert sorted(os.listdir(tmp_path / "c")) == ["C0.npz", "C1.npz", "C2.npz", "config.json"]
    assert ClusterChain.load(str(tmp_path / "c")) == chain and ClusterChain.load(str(tmp_path / "c" / "C2.npz")) == ClusterChain.from_partial_chain(C)
    with pytest.raises(ValueError, match="does not exist"):
        ClusterChain.load(str(tmp_path / "nowhere"))
    with pytest.raises(AssertionError, match="valid hierarchical clustering chain"):
        ClusterChain([chain[0], chain[2]])
    if mr.refpy_available():
        mr.import_refpy()
        from pecos.utils.cluster_util import ClusterChain as Ref
        theirs = Ref.load(str(tmp_path / "c"))
        assert len(theirs) == 3 and all((a != b).nnz == 0 for a, b in zip(theirs, chain))
        theirs.save(str(tmp_path / "r"))
        assert ClusterChain.load(str(tmp_path / "r")) == chain


def test_dimension_errors_come_before_a_device():
    """Each of these is raised from the operands' shapes: the machine of this test has no device to touch."""
    from pecos_amd import ClusterChain, matching_chain_device, relevance_chain_device
    chain = ClusterChain(CHAIN)
    wide = smat.csr_matrix((rl.N, rl.LABELS + 1), dtype=np.float32)
    short = smat.csr_matrix((rl.N - 1, rl.CODES), dtype=np.float32)
    ok = smat.csr_matrix((rl.N, rl.LABELS), dtype=np.float32)
    for call in (lambda D: chain.generate_relevance_chain(D), lambda D: chain.generate_matching_chain(D), lambda D: relevance_chain_device(D, CHAIN, "l1", True),
                 lambda D: matching_chain_device(D, CHAIN), chain.matrix_chain_dimension_check):
        with pytest.raises(ValueError, match=r"0: \(200, 49\)!=\(48, 16\)"):
            call({0: wide})
        with pytest.raises(ValueError, match="M_dict first dim do not match"):
            call({0: ok, 1: short})
        with pytest.raises(ValueError, match="M_dict got invalid key"):
            call({4: ok})
        with pytest.raises(ValueError, match=r"2: \(200, 48\)!=\(16, 4\)"):
            call({2: ok})
    assert chain.matrix_chain_dimension_check({0: ok, 3: smat.csr_matrix((rl.N, 1), dtype=np.float32)}) == (rl.N, rl.LABELS)
    assert chain.generate_relevance_chain(None) == [None] * 3 and chain.generate_matching_chain({0: None}) == [None] * 3
    assert relevance_chain_device({}, CHAIN, "l1", True) == [None] * 3 and matching_chain_device(None, CHAIN) == [None] * 3
    with pytest.raises(ValueError, match="'l3' is not a supported norm"):
        relevance_chain_device({0: ok}, CHAIN, "l3", True)


# ------------------------------------------------------------------------------------------------ train_ext, train
def test_train_ext_refusals_need_no_gpu():
    from pecos_amd import XLinearModel
    X, Y, C, R = rl.fixture_problem()
    kw = dict(nr_splits=rl.NR_SPLITS, min_codes=rl.NR_SPLITS)
    for mode in ("matcher", "ranker"):
        with pytest.raises(ValueError, match=f"Expect non-trivial clustering for {mode} mode"):
            XLinearModel.train_ext(X, Y, mode=mode)
        with pytest.raises(ValueError, match=f"Expect non-trivial clustering for {mode} mode"):
            XLinearModel.train_ext(X, Y, C=[], mode=mode)
    for given in (None, C):
        with pytest.raises(ValueError, match="Wrong value for the mode attribute: both"):
            XLinearModel.train_ext(X, Y, C=given, mode="both")
    with pytest.raises(ValueError, match="Wrong value for rel_mode: always"):
        XLinearModel.train_ext(X, Y, C=C, rel_mode="always", **kw)
    for mode, level in (("matcher", 3), ("matcher", 0), ("ranker", 4), ("ranker", 0)):
        with pytest.raises(ValueError, match=f"ranker_level = {level} leaves no layer to train in {mode} mode: the chain has 3 layers"):
            XLinearModel.train_ext(X, Y, C=C, mode=mode, ranker_level=level, **kw)
    with pytest.raises(ValueError, match="the bottom clustering matrix has 48 rows, the problem 47 labels"):
        XLinearModel.train_ext(X, Y[:, :47], C=C, **kw)
    with pytest.raises(ValueError, match=r"0: \(200, 47\)!=\(48, 16\)"):
        XLinearModel.train_ext(X, Y, C=C, R=R[:, :47], rel_mode="induce", **kw)
    with pytest.raises(ValueError, match="M_dict first dim do not match"):
        XLinearModel.train_ext(X, Y, C=C, user_supplied_negatives={0: Y[:150]}, negative_sampling_scheme="usn", **kw)
    with pytest.raises(ValueError, match=r"1: \(200, 48\)!=\(48, 16\)"):
        XLinearModel.train_ext(X, Y, C=C, user_supplied_negatives={1: Y}, negative_sampling_scheme="usn", **kw)
    with pytest.raises(ValueError, match="X must be float32"):
        XLinearModel.train_ext(X.astype(np.float64), Y, C=C, **kw)
    with pytest.raises(ValueError, match="pred_params is not valid"):
        XLinearModel.train_ext(X, Y, C=C, post_processor="nope", **kw)
    with pytest.raises(ValueError, match=r"len\(neg_mining_chain\)=2 != 3"):
        XLinearModel.train_ext(X, Y, C=C, train_params=dict(nr_splits=4, min_codes=4, hlm_args=dict(neg_mining_chain=["tfn", "usn"], model_chain=dict())))


def test_train_and_train_device_still_refuse_these_options_by_name():
    from pecos_amd import XLinearModel
    X, Y, C, R = rl.fixture_problem()
    for train in (XLinearModel.train, XLinearModel.train_device):
        for kw, what in ((dict(mode="matcher"), "mode = 'matcher'"), (dict(mode="ranker"), "mode = 'ranker'"), (dict(rel_mode="induce"), "rel_mode = 'induce'"),
                         (dict(rel_mode="ranker-only"), "rel_mode = 'ranker-only'")):
            with pytest.raises(NotImplementedError) as e:
                train(X, Y, C=C, **kw)
            assert str(e.value) == f"XLinearModel.train: {what} is not served on the device"
        with pytest.raises(NotImplementedError, match="(?s)XLinearModel.train: user_supplied_negatives = .* is not served on the device"):
            train(X, Y, C=C, user_supplied_negatives={0: Y})


# ------------------------------------------------------------------------------------------------ the entry points
def _fake(lib, device, rows, cols, nnz=3):
    lib.xrl_smat_from_device_csr.restype = ctypes.c_void_p
    lib.xrl_smat_from_device_csr.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    h = lib.xrl_smat_from_device_csr(device, rows, cols, 0x1000, 0x1000, 0x1000, nnz)
    assert h
    return h


def test_entry_point_refusals_need_no_gpu():
    lib = rr.load(rr.OURS)
    norm, check = lib.xrl_smat_normalize_rows_norm_device, lib.xrl_smat_check_relevance_device
    norm.restype, norm.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p]
    check.restype, check.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    lib.xrl_smat_free.argtypes = [ctypes.c_void_p]
    made = [_fake(lib, 0, 5, 7), _fake(lib, 0, 5, 8), _fake(lib, 0, 6, 7), _fake(lib, 1, 5, 7)]
    out, status = ctypes.c_void_p(), (ctypes.c_uint64 * 2)()

    def refusal(rc):
        assert rc == -1
        return rr.last_error(lib)

    try:
        n = "xrl_smat_normalize_rows_norm_device: "
        for bad in (0, 4, -1):
            assert refusal(norm(made[0], bad, 0, ctypes.byref(out), None)) == n + f"unknown norm {bad} (1 = l1, 2 = l2, 3 = max)"
        assert refusal(norm(None, 1, 0, ctypes.byref(out), None)) == n + "null matrix handle (A)"
        assert refusal(norm(made[0], 3, 0, None, None)) == n + "null argument (out)"
        c = "xrl_smat_check_relevance_device: "
        assert refusal(check(None, made[0], status, None)) == c + "null matrix handle (Y)"
        assert refusal(check(made[0], None, status, None)) == c + "null matrix handle (R)"
        assert refusal(check(made[0], made[0], None, None)) == c + "null argument (status)"
        assert refusal(check(made[0], made[1], status, None)) == c + "R has shape 5 x 8, Y has 5 x 7"
        assert refusal(check(made[0], made[2], status, None)) == c + "R has shape 6 x 7, Y has 5 x 7"
        assert refusal(check(made[0], made[3], status, None)) == c + "Y and R are on devices 0 and 1"
    finally:
        for h in made:
            lib.xrl_smat_free(h)


def test_new_symbols_are_exported_and_bound():
    import pecos_amd
    from pecos_amd import DeviceMatrix, XLinearModel, clib
    for name in ("ClusterChain", "relevance_chain_device", "matching_chain_device"):
        assert name in pecos_amd.__all__ and callable(getattr(pecos_amd, name))
    from pecos_amd.training import matching_chain_device, relevance_chain_device
    assert relevance_chain_device is pecos_amd.relevance_chain_device and matching_chain_device is pecos_amd.matching_chain_device
    assert callable(XLinearModel.train_ext) and callable(DeviceMatrix.check_relevance) and clib.ROW_NORMS == {"l1": 1, "l2": 2, "max": 3}
    for name in ("xrl_smat_normalize_rows_norm_device", "xrl_smat_check_relevance_device"):
        assert getattr(clib.clib_float32, name).argtypes is not None
    header = open(os.path.join(rr.REPO, "include", "xrl_abi.h")).read()
    assert "int xrl_smat_normalize_rows_norm_device(void* A, int norm, int in_place, void** out, void* hip_stream);" in header
    assert "int xrl_smat_check_relevance_device(void* Y, void* R, uint64_t* status, void* hip_stream);" in header
    assert "int xrl_smat_normalize_rows_device(void* A, int in_place, void** out, void* hip_stream);" in header
    for rule in (" * R1a, ", " * R1b, ", " * Rule C, "):
        assert rule in header
    with pytest.raises(ValueError, match="'l3' is not a supported norm"):
        clib.smat_normalize_rows_device(1, norm="l3")
