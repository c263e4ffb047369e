"""HNSW search on the device (K17) where finite inputs give distances that leave fp32's range: +inf, -inf and NaN distances (which carry the
host's default NaN 0xFFC00000), NaNs in both queues, ties at the infinities, subnormal distances, -0.0 and stored zeros.  Every case of
hnsw_rule.range_edge_cases() goes through test_gpu_hnsw.check() -- ids, order, distance bits, untouched tails, the traced counters against the
statement, the live reference where it can run -- and against the recording tests/golden/hnsw/range_edges.npz.  Bits only: no tolerance."""
import os

import numpy as np
import pytest

import hnsw_rule as hr
from test_gpu_hnsw import PF, PI, check

pytestmark = pytest.mark.gpu

CASES = hr.range_edge_cases()
REC = hr.range_edge_recording(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hnsw", "range_edges.npz"), CASES)


def recorded(name, efS, topk, idx, dist, what=""):
    """idx / dist started as zeros (the recording's fill)."""
    assert np.array_equal(idx, REC[(name, efS, topk)][0]), (name, efS, topk, what, "ids or order differ from the recording")
    assert np.array_equal(dist.view(np.uint32), REC[(name, efS, topk)][1]), (name, efS, topk, what, "distance bits differ from the recording")


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_entry_points_lds_and_hbm_heaps(tmp_path, name):
    """xrl_hnsw_predict_csr_f32 / _drm_f32 by the case's data type, at every recorded setting (the LDS form of the topk heap), then with
    efS = CAP + 1 (the HBM form).  With efS at or above the node count every visited node is admitted, so the HBM run is also held against
    the recording of (num_node, num_node) where the case has one."""
    ix, Q, settings = CASES[name]
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    m = hr.Ours(folder)
    for efS, topk in settings:
        check(folder, ix, Q, efS, topk, m=m, form="lds", what=(name, efS, topk))
        idx, dist, err = m.predict(Q, efS, topk)
        assert err is None, err
        recorded(name, efS, topk, idx, dist)
    n = ix.num_node
    check(folder, ix, Q, hr.caps()["CAP"] + 1, n, m=m, form="hbm", what=(name, "efS = CAP + 1"))
    if (n, n) in settings:
        idx, dist, err = m.predict(Q, hr.caps()["CAP"] + 1, n)
        assert err is None, err
        recorded(name, n, n, idx, dist, "efS = CAP + 1")
    m.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_resident_form(tmp_path, name):
    import torch
    import pecos_amd
    ix, Q, settings = CASES[name]
    m = pecos_amd.HNSW.load(hr.write_folder(ix, str(tmp_path / "m")))
    dev = "cuda:0"
    if ix.data_type == "drm":
        X = torch.from_numpy(Q).to(dev)
    else:
        X = (torch.from_numpy(Q.indptr.astype(np.int64)).to(dev), torch.from_numpy(Q.indices.astype(np.int32)).to(dev), torch.from_numpy(Q.data).to(dev))
    for efS, topk in settings + [(hr.caps()["CAP"] + 1, ix.num_node)]:
        idx, dist, cnt = pecos_amd.hnsw_predict_device(m, X, efS=efS, topk=topk)
        idx, dist, cnt = idx.cpu().numpy().view(np.uint32), dist.cpu().numpy(), cnt.cpu().numpy()
        want = hr.statement(ix, Q, efS, topk)
        assert np.array_equal(idx, want[0]), (name, efS, topk, "ids or order differ from the statement")
        assert np.array_equal(dist.view(np.uint32), want[1].view(np.uint32)), (name, efS, topk, "distance bits differ from the statement")
        assert np.array_equal(cnt, want[2].astype(np.int32)), (name, efS, topk)
        if (name, efS, topk) in REC:
            recorded(name, efS, topk, idx, dist, "resident")


NAN_IN_THE_QUEUES = [n for n in sorted(CASES) if n.startswith("nan_walk") or n in ("seed_csr_ip_init0", "seed_drm_ip_init3", "seed_csr_l2_init3", "inf_ties_drm_ip")]


def rows_that_rerun_holding_nans(ix, Q, efS, topk, cap):
    """Rows whose cand heap grows past `cap` (they run again) and whose answer holds a NaN."""
    rows = 0
    Qr = Q.tocsr() if ix.data_type == "csr" else Q
    for r in range(Q.shape[0]):
        t = {}
        with np.errstate(all="ignore"):
            got = hr.search_one(ix, ix.row(Qr, r), efS, topk, t)
        rows += int(t["max_cand"] > cap and any(np.isnan(d) for d, _ in got))
    return rows


@pytest.mark.parametrize("name", NAN_IN_THE_QUEUES)
def test_a_small_cand_capacity_reruns_queries_that_hold_nans(tmp_path, monkeypatch, name):
    ix, Q, settings = CASES[name]
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    monkeypatch.setenv("XRL_HNSW_CAND_CAP", "2")
    efS, topk = max(settings)
    assert rows_that_rerun_holding_nans(ix, Q, efS, topk, 2) > 0
    c = check(folder, ix, Q, efS, topk, what=(name, "cand capacity 2"))
    assert c["rerun"] > 0 and c["max_cand"] > 2


@pytest.mark.parametrize("name", ["nan_walk_csr_ip_init0", "nan_walk_drm_ip_init4", "nan_walk_csr_l2_init0"])
def test_searchers_reused_across_calls_that_rerun(tmp_path, monkeypatch, name):
    """One searchers handle (its cand capacity is fixed when it is made), two slots for four queries, calls that rerun queries holding NaNs
    in both heap forms and back: every call starts from a clean visited set and leaves no NaN behind in the scratch that matters."""
    ix, Q, settings = CASES[name]
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    monkeypatch.setenv("XRL_HNSW_CAND_CAP", "2")
    m = hr.Ours(folder)
    s = m.searchers(2)
    assert s
    reruns = 0
    for efS, topk in settings + [(hr.caps()["CAP"] + 1, 24)] + settings[:2]:
        c = check(folder, ix, Q, efS, topk, m=m, searchers=s, what=(name, efS, topk))
        reruns += int(c["rerun"] > 0)
        idx, dist, err = m.predict(Q, efS, topk, searchers=s, fill_idx=PI, fill_val=PF)
        assert err is None, err
        if (name, efS, topk) in REC:
            n = hr.statement(ix, Q, efS, topk)[2]
            for r in range(Q.shape[0]):                                 # (the recording's fill is 0; past a row's count the call leaves PI / PF)
                assert np.array_equal(idx[r, :n[r]], REC[(name, efS, topk)][0][r, :n[r]]) and np.array_equal(dist[r, :n[r]].view(np.uint32), REC[(name, efS, topk)][1][r, :n[r]])
                assert (idx[r, n[r]:] == PI).all() and (dist[r, n[r]:] == PF).all()
    assert reruns >= 2
    m.free_searchers(s)
    m.close()
