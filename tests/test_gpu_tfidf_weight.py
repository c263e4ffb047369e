"""GPU half of the tf-idf weighting tests (-m gpu; cases: tests/tfidf_weight_cases.py, CPU half: tests/test_tfidf_weight_cpu.py): the two kernels
of pecos_amd/csrc/xrl_features.hip.

* tfidf_weight_kernel through the raw-count entry (xrl_queries_tfidf_device) on row_lengths, epsilon_edges and value_edges, in place and into
  a separate buffer, in batches of 1, 3, 4 and 5 rows (four rows share a block) and all at once, against the numpy mirror bit for bit -- the
  mirror itself is held against the compiled reference and a scalar restatement in the CPU half;
* both routes of c_tfidf_predict (host weighting up to 4 documents, the device beyond) and Tfidf.predict_device with either tokenizer
  against the compiled reference's own output (oracle/_ref) on count_sweep, row_lengths and the ensembles, bit for bit;
* the sublinear_tf transform for EVERY count 1 .. 2^24 against numpy's fp64 log;
* the refusals of the raw entry; concat_csr_kernel with the bound of its normalised block derived from its reduction shape.
"""
import numpy as np
import pytest

import tfidf_weight_cases as wc

pytestmark = pytest.mark.gpu

SENT = np.float32(-12345.5)


@pytest.fixture(scope="module")
def xmodel(tmp_path_factory):
    """Any loaded XLinearModel: the producers take the device and the stream from it."""
    import xrl_synth
    from pecos_amd import XLinearModel, clib
    clib.set_device(0)
    d = str(tmp_path_factory.mktemp("k5_model"))
    xrl_synth.make_model(d, 500, 800, [150, 90, 25], seed=21, shape=[4, 28, 800])
    return XLinearModel.load(d)


@pytest.fixture(scope="module")
def ref(oracle_mod, tmp_path_factory):
    """{case name: (folder, the reference's X)} of every text case, computed once (host code of oracle/_ref in a child process; oracle_mod
    builds oracle/_ref where the reference's sources are)."""
    if not wc.reference_available():
        pytest.skip("oracle/_ref not built")
    return wc.reference_predict(wc.all_text_cases(), tmp_path_factory.mktemp("tfidf_weight_ref"))


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).cuda()


def _batches(rows):
    yield 0, rows
    for bs in (1, 3, 4, 5):
        for a in range(0, rows, bs):
            yield a, min(a + bs, rows)


def _raw_groups():
    return {"row_lengths": lambda: [wc.raw_of_text(c) for _, c in wc.row_lengths()], "epsilon_edges": lambda: wc.epsilon_edges()[0], "value_edges": wc.value_edges}


# ------------------------------------------------------------------------------------------------------------------ 1: the raw-count entry
@pytest.mark.parametrize("group", ["row_lengths", "epsilon_edges", "value_edges"])
def test_raw_counts_entry_vs_mirror(group, xmodel):
    import torch
    from pecos_amd import clib
    h = xmodel.model.model_chain
    for case in _raw_groups()[group]():
        C = case.counts
        rows, D, nnz = C.shape[0], C.shape[1], int(C.nnz)
        want = wc.mirror(case)
        assert np.array_equal(want.indptr, C.indptr) and np.array_equal(want.indices, C.indices)
        crow, col, cnt0 = _dev(C.indptr, np.int64), _dev(C.indices, np.int32), _dev(C.data, np.float32)
        idf = _dev(case.idf, np.float32) if case.idf is not None else None
        args = (case.binary, case.sublinear_tf, 1 if case.norm == "l1" else 2)
        for a, b in _batches(rows):
            lo, hi = int(C.indptr[a]), int(C.indptr[b])
            for dest in ("in place", "out"):
                cnt = cnt0.clone()
                out = torch.full((nnz,), float(SENT), dtype=torch.float32, device="cuda") if dest == "out" else cnt
                torch.cuda.synchronize()
                q = clib.queries_tfidf_device(h, b - a, D, crow.data_ptr() + 8 * a, col.data_ptr(), cnt.data_ptr(), nnz, idf.data_ptr() if idf is not None else None,
                                              *args, out_addr=out.data_ptr())
                clib.queries_free(q)
                got = out.cpu().numpy()
                what = f"{case.name} rows [{a}, {b}) {dest}"
                wc.same_values(got[lo:hi], want.data[lo:hi], what)
                untouched = C.data if dest == "in place" else np.full(nnz, SENT, dtype=np.float32)
                assert np.array_equal(wc.bits(got[:lo]), wc.bits(untouched[:lo])) and np.array_equal(wc.bits(got[hi:]), wc.bits(untouched[hi:])), f"{what}: other rows were written"
                if dest == "out":
                    assert np.array_equal(wc.bits(cnt.cpu().numpy()), wc.bits(C.data)), f"{what}: the counts were changed"
        # the handle's own buffer, read back through the handle
        q = clib.queries_tfidf_device(h, rows, D, crow.data_ptr(), col.data_ptr(), cnt0.data_ptr(), nnz, idf.data_ptr() if idf is not None else None, *args)
        with clib.freeing(q):
            got = clib.queries_download(q)
        assert np.array_equal(got.indptr, C.indptr) and np.array_equal(got.indices, C.indices), case.name
        wc.same_values(got.data, want.data, f"{case.name} handle")


# ------------------------------------------------------------------------------------------------------------------ 2: both routes vs the reference
def _text_cases(group):
    return {"count_sweep": lambda: wc.count_sweep()[0], "row_lengths": lambda: [c for _, c in wc.row_lengths()], "ensembles": wc.ensembles}[group]()


def _same_rows(got, X, a, b, what):
    lo, hi = int(X.indptr[a]), int(X.indptr[b])
    assert got.shape == (b - a, X.shape[1]), what
    assert np.array_equal(got.indptr, X.indptr[a:b + 1] - lo) and np.array_equal(got.indices, X.indices[lo:hi]), f"{what}: pattern differs"
    wc.same_values(got.data, X.data[lo:hi], what)


def _windows(rows, n):
    """Windows of exactly n documents that cover every row."""
    if rows < n:
        return []
    starts = list(range(0, rows - n + 1, n))
    if starts[-1] + n < rows:
        starts.append(rows - n)
    return [(s, s + n) for s in starts]


@pytest.mark.parametrize("group", ["count_sweep", "row_lengths", "ensembles"])
def test_c_tfidf_predict_both_routes_vs_reference(group, ref, monkeypatch):
    # calls of 1 and 4 documents are weighted on the host (tfidf_weight_host), calls of 5 and more on the device; XRL_TFIDF_HOST_DOCS=0 sends
    # every call to the device (count_sweep has three documents only)
    from pecos_amd.features import Tfidf
    for case in _text_cases(group):
        folder, X = ref[case.name]
        vec = Tfidf.load(folder)
        rows = X.shape[0]
        for n in (1, 4, 5):
            for a, b in _windows(rows, n):
                _same_rows(vec.predict(case.docs[a:b], threads=2), X, a, b, f"{case.name} c_tfidf_predict docs [{a}, {b})")
        _same_rows(vec.predict(case.docs), X, 0, rows, f"{case.name} c_tfidf_predict all")
        monkeypatch.setenv("XRL_TFIDF_HOST_DOCS", "0")
        try:
            _same_rows(vec.predict(case.docs), X, 0, rows, f"{case.name} c_tfidf_predict all, device weighting")
            _same_rows(vec.predict(case.docs[-1:]), X, rows - 1, rows, f"{case.name} c_tfidf_predict last document, device weighting")
        finally:
            monkeypatch.delenv("XRL_TFIDF_HOST_DOCS")


@pytest.mark.parametrize("group", ["count_sweep", "row_lengths", "ensembles"])
def test_predict_device_x_vs_reference(group, ref, xmodel):
    # X left in HBM: the host tokenizer's counts (the row pointer of an ensemble gathered on the host, h_seg) and the device tokenizer's
    # (gathered on the device, launch_seg_to_row_ptr) under the same weighting tail
    from pecos_amd import clib
    from pecos_amd.features import Tfidf
    for case in _text_cases(group):
        folder, X = ref[case.name]
        vec = Tfidf.load(folder)
        for tokenizer in ("device", "host"):
            q = vec.predict_device(xmodel, case.docs, threads=2, tokenizer=tokenizer)
            with clib.freeing(q):
                got = clib.queries_download(q)
            _same_rows(got, X, 0, X.shape[0], f"{case.name} predict_device tokenizer={tokenizer}")


# ------------------------------------------------------------------------------------------------------------------ 3: every count
SWEEP_MISMATCHES = 0          # measured on an MI355X: the device's fp64 log gives numpy's (= glibc's) fp32 result for every count


@pytest.mark.parametrize("norm", ["l1", "l2"])
def test_sublinear_transform_every_count(norm, xmodel):
    # all integer counts 1 .. 2^24 (term counts are accumulated in fp32 by += 1: they cannot pass 2^24), 262 144 rows of 64 entries, every
    # idf = 2^-40: the row sums stay below FLT_EPSILON (64 x 17.7 x 2^-40 < 1.1e-9), the denominator is 1, the output is tf x 2^-40 exactly
    import torch
    from pecos_amd import clib
    h = xmodel.model.model_chain
    rows, L = 1 << 18, 64
    nnz = rows * L
    c = np.arange(1, nnz + 1, dtype=np.float32)
    assert c[-1] == 2.0 ** 24 and np.array_equal(c.astype(np.int64), np.arange(1, nnz + 1))
    want = wc.sweep_expected(c)
    assert 64 * float(want.max()) < float(wc.EPS) * 0.01
    crow = torch.arange(0, nnz + 1, L, dtype=torch.int64, device="cuda")
    col = (torch.arange(nnz, dtype=torch.int32, device="cuda") % L).contiguous()
    cnt = torch.from_numpy(c).cuda()
    idf = torch.full((L,), wc.TINY_IDF, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    q = clib.queries_tfidf_device(h, rows, L, crow.data_ptr(), col.data_ptr(), cnt.data_ptr(), nnz, idf.data_ptr(), False, True, 1 if norm == "l1" else 2,
                                  out_addr=cnt.data_ptr())
    clib.queries_free(q)
    got = cnt.cpu().numpy()
    bad = np.flatnonzero(wc.bits(got) != wc.bits(want))
    ulps = np.abs(wc.bits(got)[bad].astype(np.int64) - wc.bits(want)[bad].astype(np.int64))
    print(f"\nTFIDF-SWEEP {norm}: {len(bad)} of {nnz} counts differ from (float)(log((double)c) + 1.0) x 2^-40; first counts {c[bad[:10]].astype(np.int64).tolist()}, "
          f"largest distance {int(ulps.max()) if len(bad) else 0} ulp")
    assert len(bad) == SWEEP_MISMATCHES, c[bad[:10]]


# ------------------------------------------------------------------------------------------------------------------ 4: refusals
def test_raw_counts_entry_refusals(xmodel):
    import torch
    from pecos_amd import clib
    h = xmodel.model.model_chain
    D = 40
    crow = _dev([0, 2, 3], np.int64)
    cnt = _dev([1, 2, 3], np.float32)
    idf = _dev(np.linspace(1, 2, D), np.float32)
    want = wc.mirror(wc.RawCase("ok", wc.count_csr([[(3, 1), (D - 1, 2)], [(0, 3)]], D), np.linspace(1, 2, D).astype(np.float32), False, False, "l2"))

    def call(cols, with_idf=True, rows=2):
        col = _dev(np.array(cols, dtype=np.uint32).view(np.int32), np.int32)
        torch.cuda.synchronize()
        q = clib.queries_tfidf_device(h, rows, D, crow.data_ptr(), col.data_ptr(), cnt.data_ptr(), 3, idf.data_ptr() if with_idf else None, False, False, 2)
        with clib.freeing(q):
            return clib.queries_download(q) if rows else None

    message = r"xrl_queries_tfidf_device: a column id outside \[0, cols\)"
    wc.same_values(call([3, D - 1, 0]).data, want.data, "cols - 1 is accepted")
    for bad in (D, 0xFFFFFFFF):
        for at in (0, 1, 2):
            cols = [3, D - 1, 0]
            cols[at] = bad
            with pytest.raises(RuntimeError, match=message):
                call(cols)
            wc.same_values(call([3, D - 1, 0]).data, want.data, "a call after a refused one")
        # without idf the reference never looks the id up (idx_idf.at() is called under use_idf only): accepted
        got = call([3, bad, 0], with_idf=False)
        wc.same_values(got.data, wc.mirror(wc.RawCase("noidf", wc.count_csr([[(3, 1), (D - 1, 2)], [(0, 3)]], D), None, False, False, "l2")).data, "no idf")
        assert got.indices.astype(np.uint32).tolist() == [3, bad, 0]
    assert call([3, D, 0], rows=0) is None                       # 0 rows: accepted, nothing is read


# ------------------------------------------------------------------------------------------------------------------ 5: concat_csr_kernel
U = 2.0 ** -24          # unit roundoff of float32


def concat_norm_bound(dense_cols):
    """Relative bound of the normalised block x / sqrt(sum x^2) against the same in fp64, from the kernel's reduction shape.  Every square is
    rounded once (1 + d, |d| <= U; a fused multiply-add would only round less); lane l adds its n = ceil(dense_cols / 64) squares
    sequentially (n - 1 roundings after the first term enters a zero accumulator exactly: counted as n), the lanes meet in six exchange
    steps (6 more).  All terms are >= 0, so the sum carries a relative error of at most g = (n + 7) U / (1 - (n + 7) U).  The square root
    halves it (sqrt(1 + g) <= 1 + g / 2) and rounds once (U), the division rounds once (U):  |got - want| <= (g / 2 + 2 U) (1 + g) |want|.
    Holds where no square underflows: the cases keep a row's entries within a factor of 4 of each other, and a row that is divided has a
    norm of 10 eps or more, so its squares stay above 1e-17."""
    n = -(-dense_cols // 64)
    g = (n + 7) * U / (1 - (n + 7) * U)
    return (g / 2 + 2 * U) * (1 + g)


TEN_EPS = np.float32(10) * wc.EPS


KINDS = (1e15, 1e-15, 3e-6, 1.0, "exactly 10 eps", "below 10 eps")     # what a row of the embedding block holds: a scale, or one entry at the threshold
SPARSE_LENS = (0, 3, 0, 50, 7, 5)


@pytest.mark.parametrize("dense_cols", [1, 63, 64, 65, 768])
@pytest.mark.parametrize("rows", [1, 4, 5])
def test_concat_csr(rows, dense_cols, xmodel):
    # every rotation of KINDS / SPARSE_LENS over the rows, so that each row count meets every kind of block, and empty and non-empty sparse rows
    import torch
    from pecos_amd import clib
    h = xmodel.model.model_chain
    rng = np.random.default_rng(100 * rows + dense_cols)
    D = 50
    for start in range(len(KINDS)):
        kinds = [KINDS[(start + r) % len(KINDS)] for r in range(rows)]
        lens = [SPARSE_LENS[(start + r) % len(SPARSE_LENS)] for r in range(rows)]
        sparse = wc.count_csr([[(int(f), float(v)) for f, v in zip(np.sort(rng.choice(D, size=n, replace=False)), rng.standard_normal(n))] for n in lens], D)
        emb = np.zeros((rows, dense_cols), dtype=np.float32)
        edge = {}
        for r, kind in enumerate(kinds):
            if isinstance(kind, float):                  # (a row of entries ~1e-15 has a norm far below 10 eps: left as it is)
                emb[r] = (kind * rng.uniform(0.5, 2.0, dense_cols) * rng.choice([-1.0, 1.0], dense_cols)).astype(np.float32)
                assert np.all(np.abs(emb[r]) > 1e-16) and np.isfinite(np.sum(emb[r].astype(np.float64) ** 2))
                continue
            # a norm of exactly 10 FLT_EPSILON (divided) or the next float below (left as it is): one non-zero entry, so the kernel's sum is that
            # entry's rounded square whatever its order; float32 numpy restates the two operations
            x0 = TEN_EPS if kind == "exactly 10 eps" else wc.below(TEN_EPS)
            emb[r, int(rng.integers(dense_cols))] = -x0 if r % 2 else x0
            nrm = np.float32(np.sqrt(np.float32(x0 * x0)))
            assert (nrm == TEN_EPS) if kind == "exactly 10 eps" else (nrm < TEN_EPS)
            edge[r] = bool(nrm >= TEN_EPS)
        crow, col, val, temb = _dev(sparse.indptr, np.int64), _dev(sparse.indices, np.int32), _dev(sparse.data, np.float32), _dev(emb, np.float32)
        torch.cuda.synchronize()
        for normalize in (False, True):
            q = clib.queries_concat_device(h, rows, D, crow.data_ptr(), col.data_ptr() if sparse.nnz else temb.data_ptr(), val.data_ptr() if sparse.nnz else temb.data_ptr(),
                                           int(sparse.nnz), dense_cols, temb.data_ptr(), normalize_emb=normalize)
            with clib.freeing(q):
                got = clib.queries_download(q)
            what = f"concat rows {rows} dense_cols {dense_cols} rotation {start} normalize {normalize}"
            assert got.shape == (rows, D + dense_cols), what
            assert np.array_equal(got.indptr, sparse.indptr + np.arange(rows + 1) * dense_cols), what
            for r in range(rows):
                a, b = int(got.indptr[r]), int(got.indptr[r + 1])
                n = int(sparse.indptr[r + 1] - sparse.indptr[r])
                sa = int(sparse.indptr[r])
                assert np.array_equal(got.indices[a:a + n], sparse.indices[sa:sa + n]) and np.array_equal(got.indices[a + n:b], D + np.arange(dense_cols)), f"{what} row {r}"
                assert np.array_equal(wc.bits(got.data[a:a + n]), wc.bits(sparse.data[sa:sa + n])), f"{what} row {r}: the sparse part"
                block = got.data[a + n:b]
                nrm64 = float(np.sqrt(np.sum(emb[r].astype(np.float64) ** 2)))
                assert r in edge or abs(nrm64 / float(TEN_EPS) - 1) > 0.1          # (an ordinary row is far from the threshold on either side)
                if not normalize or edge.get(r) is False or (r not in edge and nrm64 < float(TEN_EPS)):
                    assert np.array_equal(wc.bits(block), wc.bits(emb[r])), f"{what} row {r} ({kinds[r]}): the block must be left as it is"
                elif edge.get(r):
                    assert np.array_equal(wc.bits(block), wc.bits((emb[r] / TEN_EPS).astype(np.float32))), f"{what} row {r}: norm exactly 10 eps is divided"
                else:
                    x = emb[r].astype(np.float64)
                    want = x / np.sqrt(np.sum(x * x))
                    err = np.abs(block.astype(np.float64) - want)
                    assert np.all(err <= concat_norm_bound(dense_cols) * np.abs(want)), f"{what} row {r} ({kinds[r]}): {np.max(err / np.abs(want)):.3e} > {concat_norm_bound(dense_cols):.3e}"
