"""Cost-sensitive and user-negative training on the device: K12 under l1 / l2 / max against the numpy statements of R1a / R1 / R1b bit for
bit (tests/relevance_rule.py); K14's relevance check against the check rule; relevance_chain_device / matching_chain_device and
ClusterChain.generate_* against the reference's chains as recorded in tests/golden/relevance_chains_ref.npz; XLinearModel.train_ext
against the reference's recorded XLinearModel.train, per layer and bit for bit, and a ranker-mode model saved, loaded here and in the live
reference (where oracle/_ref is built) and predicted."""
import numpy as np
import pytest
import scipy.sparse as smat

import device_views as dv
import matching_rule as mr
import relevance_rule as rl

pytestmark = pytest.mark.gpu

RECORDED = np.load(rl.FIXTURE)
CHAIN = mr.recorded_chain(RECORDED)
CASES = rl.norm_cases()
_WANT = {}


def want_of(name, norm):
    if (name, norm) not in _WANT:
        _WANT[name, norm] = rl.normalize(CASES[name], norm)
    return _WANT[name, norm]


def dm(M):
    from pecos_amd import DeviceMatrix
    return DeviceMatrix.upload(M)


def forms_of(run):
    from pecos_amd import clib
    a = clib.debug_embed_forms()
    out = run()
    b = clib.debug_embed_forms()
    return out, {k: b[k] - a[k] for k in ("n_lane", "n_wave")}


# ------------------------------------------------------------------------------------------------ K12 under l1, l2, max
@pytest.mark.parametrize("norm", rl.NORMS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_normalize_against_the_rule_in_and_out_of_place_on_a_side_stream(name, norm):
    import torch
    M, want = CASES[name], want_of(name, norm)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    D = dm(M)
    with torch.cuda.stream(side):
        N = D.normalize_rows(stream=side.cuda_stream, norm=norm)
    side.synchronize()
    assert rl.same_normalized(N.download(), want, norm), f"{name} under {norm}: a new handle"
    assert mr.same_bits(D.download(), M), "the operand of a new handle was changed"
    with torch.cuda.stream(side):
        assert D.normalize_rows(in_place=True, stream=side.cuda_stream, norm=norm) is D
    side.synchronize()
    assert rl.same_normalized(D.download(), want, norm), f"{name} under {norm}: in place"


@pytest.mark.parametrize("norm", rl.NORMS)
def test_which_form_serves_which_row(norm):
    M = CASES["lengths"]
    lens = np.diff(M.indptr)
    assert tuple(lens) == rl.LENGTHS
    D = dm(M)
    for r, n in enumerate(rl.LENGTHS):                      # a row at a time: the counters say which form served it
        one = dm(M[r])
        _, forms = forms_of(lambda: one.normalize_rows(norm=norm))
        assert forms == {"n_lane": int(0 < n < 64), "n_wave": int(n >= 64)}, f"{n} entries under {norm}"
    _, forms = forms_of(lambda: D.normalize_rows(norm=norm))
    assert forms == {"n_lane": 2, "n_wave": 6}


def test_l2_through_the_new_entry_point_is_byte_equal_to_the_old_one():
    from pecos_amd import DeviceMatrix, clib
    for name in ("lengths", "nan", "inf", "subnormal", "zero_rows"):
        D = dm(CASES[name])
        old = D.normalize_rows().download()
        out = DeviceMatrix(_norm_handle(clib, D.handle, 2)).download()
        assert mr.same_bits(out, old), name
        assert rl.same_normalized(old, want_of(name, "l2"), "l2"), name


def _norm_handle(clib, handle, norm):
    from ctypes import byref, c_void_p
    out = c_void_p()
    clib.clib_float32.xrl_smat_normalize_rows_norm_device(c_void_p(handle), norm, 0, byref(out), c_void_p(0))
    clib._check()
    return out.value


@pytest.mark.parametrize("norm", ("l1", "max"))
def test_normalize_caller_buffers_at_odd_offsets_between_poison(norm):
    import torch
    from pecos_amd import DeviceMatrix
    M = CASES["lengths"]
    fills = (np.int64(0), np.int32(0), np.float32(7.0))
    bands = [dv.banded(M.indptr.astype(np.int64), 1, dv.BAND, fills[0], "cuda"), dv.banded(M.indices.astype(np.int32), 3, dv.BAND, fills[1], "cuda"),
             dv.banded(np.asarray(M.data, np.float32), 1, dv.BAND, fills[2], "cuda")]
    assert bands[0][1].data_ptr() % 16 == 8 and bands[1][1].data_ptr() % 16 == 12 and bands[2][1].data_ptr() % 16 == 4
    D = DeviceMatrix.from_torch(bands[0][1], bands[1][1], bands[2][1], M.shape)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        N = D.normalize_rows(stream=side.cuda_stream, norm=norm)
        D.normalize_rows(in_place=True, stream=side.cuda_stream, norm=norm)
    side.synchronize()
    want = want_of("lengths", norm)
    assert rl.same_normalized(N.download(), want, norm)
    assert np.array_equal(rl.bits(bands[2][1].cpu().numpy()), rl.bits(want.data)), "the caller's array was not rewritten in place"
    for (whole, payload), fill in zip(bands, fills):
        dv.assert_bands_intact(whole, payload, fill, norm)


def test_max_refuses_a_row_that_is_not_strictly_ascending_and_leaves_it_as_it_was():
    M = rl.duplicate_ids_case()
    D = dm(M)
    for in_place in (False, True):
        with pytest.raises(RuntimeError, match="norm = max: row 1 does not store its column ids strictly ascending"):
            D.normalize_rows(in_place=in_place, norm="max")
    assert mr.same_bits(D.download(), M)
    for norm in ("l1", "l2"):                               # walked as stored
        assert rl.same_normalized(D.normalize_rows(norm=norm).download(), rl.normalize(M, norm), norm)
    with pytest.raises(RuntimeError, match="row 2 does not store"):
        dm(M[[0, 0, 2]]).normalize_rows(norm="max")


# ------------------------------------------------------------------------------------------------ the check kernel
def check_row():
    """Y: rows of 3, 129, 0, 5 and 129 entries; R: the same pattern with positive values."""
    Y = rl.rows_case((3, 129, 0, 5, 129), seed=8, cols=400, signs=False)
    R = Y.copy()
    R.data = np.random.RandomState(3).uniform(0.5, 2.0, Y.nnz).astype(np.float32)
    return Y, R


def status_of(Y, R):
    from pecos_amd import clib
    y, r = dm(Y), dm(R)
    return clib.smat_check_relevance_device(y.handle, r.handle)


def altered(R, indptr=None, index=None, value=None):
    out = smat.csr_matrix(R.shape, dtype=np.float32)
    out.indptr, out.indices, out.data = R.indptr.copy(), R.indices.copy(), R.data.copy()
    if indptr is not None:
        out.indptr[indptr[0]] += indptr[1]
    if index is not None:
        out.indices[index[0]] = index[1]
    if value is not None:
        out.data[value[0]] = value[1]
    return out


def free_id(R, at):
    """A column id that the row of position ``at`` does not store."""
    row = int(np.searchsorted(R.indptr, at, side="right") - 1)
    return sorted(set(range(R.shape[1])) - set(R.indices[R.indptr[row]:R.indptr[row + 1]].tolist()))[-1]


def test_check_equal_patterns_and_every_way_to_differ():
    Y, R = check_row()
    assert status_of(Y, R) == (0, 0) == rl.check_rule(Y, R)
    assert status_of(Y, Y) == (0, 0)
    # a row's end moved by one: the first, a middle and the last row (the last: one entry fewer in all)
    for row, by in ((0, -1), (0, 1), (3, -1), (3, 1)):
        bad = altered(R, indptr=(row + 1, by))
        assert status_of(Y, bad) == (1, row) == rl.check_rule(Y, bad), f"row {row} by {by}"
    last = smat.csr_matrix((R.data[:-1], R.indices[:-1], np.concatenate([R.indptr[:-1], [R.indptr[-1] - 1]])), shape=R.shape)
    assert status_of(Y, last) == (1, 4) == rl.check_rule(Y, last)
    # a column id changed in lane 0 / 63 / 64 of a 129-entry row
    b = int(R.indptr[1])
    for lane in (0, 63, 64, 128):
        bad = altered(R, index=(b + lane, free_id(R, b + lane)))
        assert status_of(Y, bad) == (2, 1) == rl.check_rule(Y, bad), f"lane {lane}"
    b4 = int(R.indptr[4])
    assert status_of(Y, altered(R, index=(b4 + 64, free_id(R, b4 + 64)))) == (2, 4)
    # values: below 0 is code 3; -0.0 and NaN are not below 0
    for at, row in ((0, 0), (b + 64, 1), (R.nnz - 1, 4)):
        assert status_of(Y, altered(R, value=(at, -1e-30))) == (3, row) == rl.check_rule(Y, altered(R, value=(at, -1e-30)))
        for v in (-0.0, np.nan, 0.0, np.inf):
            assert status_of(Y, altered(R, value=(at, v))) == (0, 0)
    assert status_of(Y, altered(R, value=(at, -np.inf))) == (3, 4)
    # the first failing check wins, then the first row
    both = altered(altered(R, value=(0, -1.0)), index=(b4, free_id(R, b4)))
    assert status_of(Y, both) == (2, 4) == rl.check_rule(Y, both)
    assert status_of(Y, altered(both, indptr=(4, -1))) == (1, 3)


def test_check_empty_matrices_and_refusals():
    from pecos_amd import DeviceMatrix, clib
    for shape in ((0, 9), (4, 9), (4, 0)):
        E = smat.csr_matrix(shape, dtype=np.float32)
        assert status_of(E, E) == (0, 0)
    Y, R = check_row()
    with pytest.raises(RuntimeError, match="xrl_smat_check_relevance_device: R has shape 5 x 399, Y has 5 x 400"):
        status_of(Y, smat.csr_matrix(R[:, :399]))
    with pytest.raises(ValueError, match="Invalid relevance matrix: R has shape"):
        DeviceMatrix.check_relevance(dm(Y), dm(smat.csr_matrix(R[:4])))
    # the Python form raises check_relevance's own words, read column-major as the host check reads
    from pecos_amd.xlinear import check_relevance
    DeviceMatrix.check_relevance(dm(Y), dm(R))
    b = int(R.indptr[1])
    for bad in (altered(R, index=(b, free_id(R, b))), altered(R, value=(5, -2.0))):
        with pytest.raises(ValueError) as host:
            check_relevance(Y, bad)
        with pytest.raises(ValueError) as device:
            DeviceMatrix.check_relevance(dm(Y), dm(bad))
        assert str(host.value) == str(device.value)
    with pytest.raises(ValueError, match="Invalid relevance matrix: Y.indices != R.indices"):
        DeviceMatrix.check_relevance(dm(Y), dm(altered(R, index=(b, free_id(R, b)))), by_columns=False)
    assert clib.smat_check_relevance_device(dm(Y).handle, dm(Y).handle) == (0, 0)


# ------------------------------------------------------------------------------------------------ the chains
GRID = [(ks, norm, induce) for ks in rl.KEYSETS for norm in rl.NORM_TYPES for induce in (True, False)]


def recorded(prefix):
    return [mr.get_sparse(RECORDED, f"{prefix}__{t}", smat.csr_matrix) for t in range(len(CHAIN))]


def assert_chain(got, want, values, what):
    assert len(got) == len(want) == len(CHAIN), what
    for t, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), f"{what}: level {t}"
        if g is not None:
            g = g if smat.issparse(g) else g.download()
            assert g.shape == w.shape
            if values:
                assert mr.same_bits(smat.csr_matrix(g), w), f"{what}: level {t}"          # as stored: ascending rows come out of the device
            else:
                assert mr.same_pattern(smat.csr_matrix(g), w), f"{what}: level {t}"


@pytest.mark.parametrize("keyset,norm,induce", GRID)
def test_relevance_chain_device_against_the_recorded_reference(keyset, norm, induce):
    from pecos_amd import ClusterChain, relevance_chain_device
    D = rl.partial_dict(rl.KEYSETS[keyset], "R")
    before = {k: v.copy() for k, v in D.items()}
    want = recorded(f"rel__{keyset}__{norm}__{int(induce)}")
    assert_chain(relevance_chain_device(D, CHAIN, norm, induce), want, True, "resident")
    assert_chain(ClusterChain(CHAIN).generate_relevance_chain(D, norm_type=norm, induce=induce), want, True, "ClusterChain")
    assert all(mr.same_bits(D[k], before[k]) for k in D), "an operand was changed"


def test_relevance_chain_device_leaves_resident_operands_as_they_are_and_takes_tensors():
    from pecos_amd import DeviceMatrix, relevance_chain_device
    D = rl.partial_dict((0, 2), "R")
    resident = {k: DeviceMatrix.upload(v) for k, v in D.items()}
    chain = [DeviceMatrix.upload(c) for c in CHAIN]
    want = recorded("rel__k02__l1__1")
    assert_chain(relevance_chain_device(resident, chain, "l1", True), want, True, "DeviceMatrix operands")
    assert all(mr.same_bits(resident[k].download(), D[k]) for k in D), "a caller's level was normalised in place"
    assert_chain(relevance_chain_device({k: v.to_torch() for k, v in resident.items()}, chain, "l1", True), want, True, "tensor operands")


@pytest.mark.parametrize("keyset", sorted(rl.KEYSETS))
def test_matching_chain_device_against_the_recorded_reference(keyset):
    from pecos_amd import ClusterChain, matching_chain_device
    D = rl.partial_dict(rl.KEYSETS[keyset], "M")
    want = recorded(f"match__{keyset}")
    got = matching_chain_device(D, CHAIN)
    assert_chain(got, want, False, "resident")
    assert all(m is None or (m.download().data == 1).all() for m in got)
    host = ClusterChain(CHAIN).generate_matching_chain(D)
    assert all(m is None or isinstance(m, smat.csc_matrix) for m in host)
    assert_chain([None if m is None else rl.canonical_csr(m) for m in host], want, False, "ClusterChain")


# ------------------------------------------------------------------------------------------------ train_ext
def recorded_weights(name):
    depth = int(RECORDED[f"train__{name}__depth"][0])
    return [mr.get_sparse(RECORDED, f"train__{name}__W{t}", smat.csc_matrix) for t in range(depth)]


@pytest.mark.parametrize("name", sorted(rl.TRAIN_CONFIGS))
def test_train_ext_against_the_recorded_reference(name):
    from pecos_amd import XLinearModel
    X, Y, C, R, usn, kw = rl.train_kwargs(name)
    model = XLinearModel.train_ext(X, Y, C=C, R=R, user_supplied_negatives=usn, **kw)
    want = recorded_weights(name)
    assert model.depth == len(want)
    for t, layer in enumerate(model.model.layers):
        got = smat.csc_matrix(layer.W)
        got.sort_indices()
        assert got.shape == want[t].shape and mr.same_bits(got, want[t]), f"{name}: layer {t}: the weights differ from the reference's"


def test_train_ext_without_c_is_train_device():
    from pecos_amd import XLinearModel
    X, Y, C, R = rl.fixture_problem()
    a = XLinearModel.train_ext(X[:60], smat.csc_matrix(Y[:60]), R=smat.csc_matrix(R[:60]), **rl.TRAIN_KW)
    b = XLinearModel.train_device(X[:60], smat.csc_matrix(Y[:60]), R=smat.csc_matrix(R[:60]), **rl.TRAIN_KW)
    assert a.depth == b.depth == 1 and mr.same_bits(smat.csc_matrix(a.model.layers[0].W), smat.csc_matrix(b.model.layers[0].W))


def ranker_model(folder):
    from pecos_amd import XLinearModel
    X, Y, C, R, usn, kw = rl.train_kwargs("ranker_2")
    model = XLinearModel.train_ext(X, Y, C=C, beam_size=3, only_topk=4, **kw)
    model.save(folder)
    return model, XLinearModel.load(folder), X[:70]


def test_ranker_mode_save_load_predict(tmp_path):
    """A ranker-mode model's top layer has four clusters: it predicts layer by layer, the top layer without codes (every cluster, score 1)."""
    model, loaded, Xq = ranker_model(str(tmp_path / "m"))
    assert model.depth == 2 and model.model.layers[0].C.shape == (16, 4)
    assert (loaded.depth, loaded.nr_features, loaded.nr_labels) == (2, rl.FEATURES, rl.LABELS)
    assert len(loaded.model.layerwise) == 2 and loaded.model.layerwise[0].C.shape == (16, 4)
    a, b = loaded.predict(Xq), model.predict(Xq)
    assert a.shape == (70, rl.LABELS) and a.nnz == 70 * 4 and mr.same_bits(smat.csr_matrix(a), smat.csr_matrix(b))
    p0 = model.model.layers[0].predict(Xq, only_topk=3)
    assert p0.shape == (70, 16) and p0.nnz == 70 * 3
    assert mr.same_bits(smat.csr_matrix(model.model.layers[1].predict(Xq, csr_codes=p0, only_topk=4)), smat.csr_matrix(a))
    wide = loaded.predict(Xq, beam_size=16, only_topk=48)
    assert wide.nnz == 70 * 48 and not mr.same_pattern(rl.canonical_csr(wide), rl.canonical_csr(a))


def test_ranker_mode_folder_loads_and_predicts_in_the_live_reference(tmp_path):
    if not mr.refpy_available():
        pytest.skip("oracle/_ref (the compiled reference and its python package) is not built")
    model, loaded, Xq = ranker_model(str(tmp_path / "m"))
    mr.import_refpy()
    from pecos.xmc.xlinear.model import XLinearModel as RefModel
    ref = RefModel.load(str(tmp_path / "m"), is_predict_only=False)
    assert len(ref.model.model_chain) == 2 and ref.model.model_chain[0].C.shape == (16, 4)
    want = smat.csr_matrix(ref.predict(Xq, threads=1))
    for got in (loaded.predict(Xq), model.predict(Xq)):
        assert mr.same_bits(smat.csr_matrix(got), want), "the reference predicts something else from the saved folder"


def test_a_moved_relevance_entry_is_refused_by_the_device_check():
    from pecos_amd import XLinearModel
    from pecos_amd.xlinear import check_relevance
    X, Y, C, R, usn, kw = rl.train_kwargs("induce_l1_R")
    bad = smat.csr_matrix(R).copy()
    b = int(bad.indptr[11])
    bad.indices[b] = sorted(set(range(rl.LABELS)) - set(bad.indices[b:int(bad.indptr[12])]))[0]
    bad.sort_indices()
    with pytest.raises(ValueError) as host:
        check_relevance(Y, bad)
    for rel in (dict(rel_mode="induce", rel_norm="l1"), dict(rel_mode="ranker-only", rel_norm="no-norm"), dict(rel_mode="induce", mode="ranker", ranker_level=1)):
        with pytest.raises(ValueError) as device:
            XLinearModel.train_ext(X, Y, C=C, R=bad, **dict(kw, **rel))
        assert str(device.value) == str(host.value) and str(host.value).startswith("Invalid relevance matrix: Y.")
    neg = smat.csr_matrix(R).copy()
    neg.data[5] = -1.0
    with pytest.raises(ValueError, match="Invalid relevance matrix: got value < 0"):
        XLinearModel.train_ext(X, Y, C=C, R=neg, **dict(kw, rel_norm="no-norm"))
