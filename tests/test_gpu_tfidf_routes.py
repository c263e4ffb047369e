"""Every entry point that turns text into the tf-idf X, on one small corpus: they share one counting step and one weighting tail, so their
results are the same CSR bit for bit -- indptr, feature ids and fp32 values -- whichever tokenizer, stream and status argument they take.
The ensemble folder has three base vectorizers (the segment pointer -> row pointer step and the ensemble's norm run), the single one none."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as smat

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tfidf_models")
# an empty document, one of unknown tokens only, one repeated (rows 0 and 4), runs of spaces, non-ASCII text
DOCS = ["w6 w2 w12 w4 w4 w0 w7 w0", "", "zzz unknown tokens only", "w1  w2   w3 ", "w6 w2 w12 w4 w4 w0 w7 w0", "w0 w53 naïve w1 日本 w25 w0"]


@pytest.fixture(scope="module")
def xmodel(tmp_path_factory):
    """Any loaded XLinearModel: the calls that take a model handle read its device and stream."""
    import xrl_synth
    from pecos_amd import XLinearModel, clib
    clib.set_device(0)
    d = str(tmp_path_factory.mktemp("routes_model"))
    xrl_synth.make_model(d, 500, 800, [150, 90, 25], seed=21, shape=[4, 28, 800])
    return XLinearModel.load(d)


def _same(a, b, what):
    assert a.shape == b.shape, what
    assert np.array_equal(a.indptr, b.indptr), f"{what}: row lengths differ"
    assert np.array_equal(a.indices, b.indices), f"{what}: feature ids differ"
    assert np.array_equal(a.data.view(np.uint32), b.data.view(np.uint32)), f"{what}: values differ"


def _handle_csr(q):
    from pecos_amd import clib
    with clib.freeing(q):
        return clib.queries_download(q)


@pytest.mark.parametrize("caller_stream", [False, True], ids=["no_stream", "caller_stream"])
@pytest.mark.parametrize("name", ["ensemble_l1", "word_default"])
def test_every_route_gives_the_same_x(xmodel, monkeypatch, name, caller_stream):
    import torch
    from pecos_amd import clib
    from pecos_amd.features import Tfidf, tfidf_counts_device, tfidf_transform_device
    vec = Tfidf.load(os.path.join(GOLDEN, name, "model"))
    mc = xmodel.model.model_chain
    n = len(DOCS)
    stream = torch.cuda.Stream().cuda_stream if caller_stream else None

    monkeypatch.setenv("XRL_TFIDF_HOST_DOCS", "0")
    want = vec.predict(DOCS, threads=2)                               # c_tfidf_predict, weighted on the device
    monkeypatch.delenv("XRL_TFIDF_HOST_DOCS")
    assert want.shape == (n, vec.nr_features) and want[1].nnz == 0 and want[0].nnz > 0
    _same(want[0], want[4], "the repeated document")
    _same(smat.vstack([vec.predict(DOCS[:4], threads=2), vec.predict(DOCS[4:], threads=2)], format="csr"), want, "c_tfidf_predict, host weighting")

    _same(_handle_csr(clib.tfidf_predict_device(vec.model, mc, DOCS, threads=2)), want, "xrl_tfidf_predict_device")
    arr, lens, nr_doc = clib._corpus_arrays(DOCS)
    for tokenizer in (0, 1):
        q = clib.clib_float32.xrl_tfidf_predict_device_tok(vec.model, mc, arr, lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), nr_doc, tokenizer, 2)
        clib._check()
        _same(_handle_csr(q), want, f"xrl_tfidf_predict_device_tok, tokenizer {tokenizer}")

    buf, off, ln = clib.corpus_packed(DOCS)
    text = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
    off_t, len_t = torch.from_numpy(off.view(np.int64).copy()).cuda(), torch.from_numpy(ln.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    q = clib.tfidf_predict_device_text(vec.model, mc, text.data_ptr(), off_t.data_ptr(), len_t.data_ptr(), n, stream=stream)
    _same(_handle_csr(q), want, "xrl_tfidf_predict_device_text")
    _same(tfidf_transform_device(vec, text, off_t, len_t, stream=stream).download(), want, "xrl_tfidf_transform_device, no status")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _same(tfidf_transform_device(vec, text, off_t, len_t, status=status, stream=stream).download(), want, "xrl_tfidf_transform_device, status")
    assert status.cpu().tolist() == [0] * n

    counts = clib.tfidf_counts(vec.model, DOCS, threads=2)
    _same(_handle_csr(tfidf_counts_device(vec, xmodel, text, off_t, len_t, stream=stream)), counts, "xrl_tfidf_counts_device")
    status.fill_(-1)
    torch.cuda.synchronize()
    _same(_handle_csr(tfidf_counts_device(vec, xmodel, text, off_t, len_t, status=status, stream=stream)), counts, "xrl_tfidf_counts_device, status")
    assert status.cpu().tolist() == [0] * n
