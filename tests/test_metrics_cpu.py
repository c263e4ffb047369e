"""The device metrics (K8, xrl_metrics_device) without a GPU: the numpy restatement of tests/metrics_cases.py against the reference's
Metrics.generate -- live where oracle/_ref/refpy is built, and on the fixtures recorded from it --, the entry point's binding and refusals
(all made before a GPU is required), Metrics / from_sums, and evaluate_shard's collective algebra under gloo with stand-ins."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest

import metrics_cases as mc
from conftest import REPO

REFPY = os.path.join(REPO, "oracle", "_ref", "refpy")


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def check_against_reference(c, prec, recall, what):
    """prec bit-identical; recall bit-identical for rows <= R, else within the derived bound (metrics_cases.recall_bound)."""
    rows = c["idx"].shape[0]
    p, r = mc.from_sums(*mc.metric_sums(c), rows)
    assert np.array_equal(bits(p), bits(prec)), f"{what}: prec differs from the reference"
    if rows <= mc.rows_per_block(rows):
        assert np.array_equal(bits(r), bits(recall)), f"{what}: recall differs from the reference"
    else:
        err = float(np.max(np.abs(r - recall)))
        print(f"{what}: rows {rows} > R {mc.rows_per_block(rows)}: max |recall - reference| = {err:.3e}, bound {mc.recall_bound(rows):.3e}")
        assert err <= mc.recall_bound(rows), (what, err)
    # and in the reference's own order (one block) the restatement IS the reference
    p1, r1 = mc.from_sums(*mc.metric_sums(c, block=max(rows, 1)), rows)
    assert np.array_equal(bits(p1), bits(prec)) and np.array_equal(bits(r1), bits(recall)), f"{what}: row-order restatement differs"


@pytest.mark.parametrize("name", mc.GOLDEN)
def test_restatement_equals_the_recorded_reference(name):
    c, prec, recall = mc.golden(name)
    assert mc.same_inputs(c, mc.case(name)), f"{name}: the generator no longer makes the recorded inputs"
    assert len(prec) == c["topk"] and prec.dtype == np.float64 and recall.dtype == np.float64
    check_against_reference(c, prec, recall, name)


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_restatement_equals_the_reference_live(name):
    if not os.path.isdir(REFPY):
        pytest.skip("oracle/_ref/refpy is not built")
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import make_golden_metrics as gen
    if REFPY not in sys.path:
        sys.path.insert(0, REFPY)
    from pecos.utils import smat_util
    c = mc.case(name)
    h = gen.compact(c) if c["n_cols"] > 1 << 31 else c
    m = smat_util.Metrics.generate(mc.true_csr(h), mc.pred_csr(h), topk=c["topk"])
    check_against_reference(c, np.asarray(m.prec), np.asarray(m.recall), name)


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_vectorised_restatement_equals_the_row_loop(name):
    c = mc.case(name)
    rows = c["idx"].shape[0]
    m, r = mc.metric_sums(c, block=max(rows, 1))
    m2, r2 = mc.metric_sums_by_row(c)
    assert np.array_equal(m, m2) and np.array_equal(bits(r), bits(r2))
    assert np.array_equal(mc.metric_sums(c)[0], m2)                     # the integers do not depend on the blocks


def test_cases_hold_what_the_gpu_tests_rely_on():
    o = mc.case("order")
    stored = dict(o)                                                     # a kernel that trusted the stored order: rank = position
    stored["val"] = -np.tile(np.arange(4, dtype=np.float32), (o["idx"].shape[0], 1))
    want, lazy = mc.cum_matched(o)[:, 0], mc.cum_matched(stored)[:, 0]
    assert (want[0], lazy[0]) == (1, 0) and (want[1], lazy[1]) == (0, 1), (want, lazy)     # inside / outside top-1 under the two orders
    assert want.tolist() == [1, 0, 0, 1, 0, 1, 1], want                  # NaN last, -0.0 == +0.0, +inf first, zeros are entries
    assert mc.cum_matched(mc.case("order4"))[4].tolist() == [0, 1, 1, 2]  # +inf (2), 0 (4: true), -inf (1), NaN (3: true)
    e = mc.case("edges")
    lens = np.diff(e["tptr"].astype(np.int64)).tolist()
    assert lens[:7] == list(mc.TRUE_LENGTHS) and (e["idx"] == 0).any() and (e["idx"] == mc.TOP).any() and (e["tidx"] == mc.TOP).any()
    assert mc.rows_per_block(262144) == 64 and mc.rows_per_block(262145) == 128 and mc.rows_per_block(0xFFFFFFFF) == 1 << 20
    for name in mc.CASES:
        c = mc.case(name)
        rows, stride = c["idx"].shape
        if rows >= 3 and name.startswith("r"):
            assert c["cnt"][0] == 0 and c["cnt"][rows // 2] == 0 and c["cnt"][-1] == 0
            assert (c["cnt"] > stride).any() or stride == 1 or rows < 8, name
    assert any(np.isnan(mc.case(n)["val"]).any() for n in mc.CASES) and mc.metric_sums(mc.case("r129_s10_k10"))[0][-1] > 0


# ------------------------------------------------------------------------------------------------------------------ the entry point
def test_entry_point_is_exported_and_bound():
    import pecos_amd
    from pecos_amd import clib, features
    fn = clib.clib_float32.xrl_metrics_device
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
    assert callable(clib.metrics_device) and callable(features.metrics_device) and callable(features.metrics_sums_device)
    assert pecos_amd.Metrics is features.Metrics and pecos_amd.metrics_device is features.metrics_device
    hdr = open(os.path.join(REPO, "include", "xrl_abi.h")).read()
    assert "int xrl_metrics_device(int device, uint32_t rows," in hdr


def _call(rows=1, null=None, stride=10, topk=10):
    """xrl_metrics_device on made-up, never dereferenced addresses: every check under test comes before the first use of the GPU."""
    from pecos_amd import clib
    lib = clib.clib_float32
    a = {k: ctypes.c_void_p(None if k == null else 0x1000 * (i + 1)) for i, k in enumerate(("idx", "val", "cnt", "tptr", "tidx", "matched", "recall"))}
    rc = lib.xrl_metrics_device(0, rows, a["idx"], a["val"], a["cnt"], stride, a["tptr"], a["tidx"], topk, a["matched"], a["recall"], None, 1)
    err = lib.xrl_last_error()
    lib.xrl_clear_error()
    return rc, (err or b"").decode()


@pytest.mark.parametrize("kw, message", [
    (dict(null="idx"), "null argument"), (dict(null="val"), "null argument"), (dict(null="cnt"), "null argument"),
    (dict(null="tptr"), "null argument"), (dict(null="tidx"), "null argument"), (dict(null="matched"), "null argument"),
    (dict(null="recall"), "null argument"),
    (dict(stride=0), "stride must be 1..1024, got 0"), (dict(stride=1025), "stride must be 1..1024, got 1025"),
    (dict(topk=0), "topk must be 1..1024, got 0"), (dict(topk=1025), "topk must be 1..1024, got 1025"),
    (dict(rows=0, topk=1025), "topk must be 1..1024, got 1025"), (dict(rows=0, null="matched"), "null argument"),
])
def test_argument_errors_come_before_the_gpu(kw, message):
    rc, err = _call(**kw)
    assert rc == -1 and err.startswith("xrl_metrics_device: ") and message in err, (rc, err)


def test_valid_arguments_without_a_gpu():
    from pecos_amd import clib
    if clib.device_count() == 0:                                         # (with a GPU the made-up addresses would be filled: tests/test_gpu_metrics.py)
        assert _call(rows=0) == (0, "")                                 # nothing to fill without a GPU: a successful no-op
        assert _call(stride=1024, topk=1024, rows=0) == (0, "")
        rc, err = _call()                                                # the checks passed: what is missing is the device
        assert rc == -1 and "no HIP device visible" in err, err


def test_python_bounds_raise_value_error():
    from pecos_amd import clib
    for kw, msg in ((dict(stride=1025, topk=10), "stride must be 1..1024, got 1025"), (dict(stride=10, topk=0), "topk must be 1..1024, got 0")):
        with pytest.raises(ValueError, match="xrl_metrics_device: " + msg.replace(".", r"\.")):
            clib.metrics_device(0, 1, 0x1000, 0x2000, 0x3000, kw["stride"], 0x4000, 0x5000, kw["topk"], 0x6000, 0x7000)


# ------------------------------------------------------------------------------------------------------------------ Metrics
def test_metrics_str_and_from_sums():
    from pecos_amd.features import Metrics
    c, prec, recall = mc.golden("r63_s10_k10")
    m = Metrics(prec=prec, recall=recall)
    assert str(m) == open(os.path.join(mc.GOLDEN_DIR, "metrics_str.txt")).read()
    assert str(m).startswith("prec   = ") and "\nrecall = " in str(m) and m._fields == ("prec", "recall")
    sm, sr = mc.metric_sums(c)
    import torch
    as_i64 = torch.from_numpy(sm.copy()).view(torch.int64).numpy()       # what metrics_sums_device hands back: int64 holding the u64 bits
    for matched in (sm, as_i64):
        got = Metrics.from_sums(matched, sr, c["idx"].shape[0])
        assert np.array_equal(bits(got.prec), bits(prec)) and np.array_equal(bits(got.recall), bits(recall))
    # additive over row batches: the integer sums of two halves add up to the whole's
    rows = c["idx"].shape[0]
    a, b = _window(c, 0, 30), _window(c, 30, rows)
    assert np.array_equal(mc.metric_sums(a)[0] + mc.metric_sums(b)[0], sm)


def _window(c, lo, hi):
    d = dict(c)
    d["idx"], d["val"], d["cnt"], d["tptr"] = c["idx"][lo:hi], c["val"][lo:hi], c["cnt"][lo:hi], c["tptr"][lo:hi + 1]
    return d


# ------------------------------------------------------------------------------------------------------------------ the collective
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import torch.distributed as dist
    import metrics_cases as cases
    from pecos_amd.distributed import ShardedXLinear
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    c = cases.case("r129_s10_k10")
    rows, topk = c["idx"].shape[0], 7

    class Stub:
        nr_pred_cols = c["n_cols"]

    def predict_fn(Xs, beam, only_topk, pp):                             # X stands in for itself: column 0 holds the global row number
        r = Xs[:, 0].astype(np.int64)
        return tuple(torch.from_numpy(np.ascontiguousarray(a[r])) for a in (c["idx"].view(np.int32), c["val"], c["cnt"].view(np.int32)))

    seen = []

    def metrics_fn(result, Y_local, k):                                  # the restatement on this rank's rows, as CPU tensors
        lo = int(Y_local[0]) if len(Y_local) else 0
        w = _window(c, lo, lo + len(Y_local))
        assert np.array_equal(result[0].numpy().view(np.uint32), w["idx"]) and result[2].shape[0] == len(Y_local)
        m, s = cases.metric_sums(w, topk=k)
        seen.append(len(Y_local))
        return torch.from_numpy(m.view(np.int64).copy()), torch.from_numpy(s.copy())

    sh = ShardedXLinear(Stub(), predict_shard_fn=predict_fn, metrics_shard_fn=metrics_fn)
    want_p, want_r = cases.from_sums(*cases.metric_sums(c, topk=topk), rows)
    for b in ([0, 40, rows], [0, 100, rows], [0, 0, rows], [0, rows, rows]):          # uneven shards, and an empty shard on either rank
        bb = np.asarray(b, dtype=np.int64)
        lo, hi = int(bb[rank]), int(bb[rank + 1])
        X_local = np.arange(lo, hi, dtype=np.float64).reshape(-1, 1)
        got = sh.evaluate_shard(X_local, np.arange(lo, hi), bb, topk=topk)
        assert seen[-1] == hi - lo
        assert np.array_equal(got.prec, want_p), (b, got.prec, want_p)
        err = float(np.max(np.abs(got.recall - want_r)))
        assert err <= cases.recall_bound(rows), (b, err)
    with pytest.raises(ValueError):
        sh.evaluate_shard(np.zeros((3, 1)), np.arange(3), np.asarray([0, 1, 2]), topk=topk)
    open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_evaluate_shard_world2_gloo(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert os.path.exists(tmp_path / "ok0") and os.path.exists(tmp_path / "ok1")
