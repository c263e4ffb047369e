"""GPU (-m gpu): the bound-pruned K1G route (dense X against a dense-format layer, csrc/xrl_predict.cpp launch_k1g_layer) runs its SECOND stage.
The golden model s_eurlex ([4, 32, 900]: leaf parents of 28-29 children, one dense tile each) under l3-hinge with beam_size = 40: every one of the 32
leaf parents is in the beam, the first stage scores the children of the J = 64 // 29 = 2 best, k0b_remaining / k1_sort_items_rest / k1g_dense_x_rest /
k2_topk_rest the other slots of the queries whose top-k the first stage could not prove final.  The result equals the reference's bit for bit and the
same handle's under prune = 0.  That a later slot is NEEDED is asserted from the reference alone, before the GPU is consulted: a row's top-k holds a
label whose parent scores strictly below the J-th best parent of the row's beam, i.e. sits at beam rank >= J whatever the order among ties (with
only_topk = 20 about half of the rows, row 0 among them; the others saturate the hinge and are final after the first stage)."""
import json
import os
import shutil

import numpy as np
import pytest
import scipy.sparse as smat

from conftest import GOLDEN, assert_same_topk, load_X

pytestmark = pytest.mark.gpu

KW = dict(beam_size=40, only_topk=20, post_processor="l3-hinge")
ROWS = (1, 63, 65, 257)
LEAF = 2
REST = {("k0b_remaining", LEAF), ("k1_sort_items_rest", LEAF), ("k1g_dense_x_rest", LEAF), ("k2_topk_rest", LEAF)}
DEFAULTS = dict(k1g_min_items=16, prune=1, adaptive=1)


def _reference(folder, oracle_mod):
    return oracle_mod.RefModel(folder, "BINARY_SEARCH_CHUNKED") if oracle_mod.ref_available() else oracle_mod.OracleModel.load(folder)


def first_stage_slots(C, beam_in):
    """The library's rule (k1g_first_slots): the beam slots whose children fill about one candidate register of 64, never the whole beam."""
    return max(1, min(beam_in - 1, 64 // int(np.diff(C.indptr).max())))


def rows_beyond_first_stage(folder, X, want, tmp, oracle_mod):
    """From the reference alone: the rows whose top-k holds a label of a parent that scores strictly below the J-th best parent of the row's beam."""
    C = smat.load_npz(os.path.join(folder, "ranker", f"{LEAF}.model", "C.npz")).tocsc()
    parent_of = np.empty(C.shape[0], np.int64)
    parent_of[C.indices] = np.repeat(np.arange(C.shape[1]), np.diff(C.indptr))
    beam_in = min(KW["beam_size"], C.shape[1])
    J = first_stage_slots(C, beam_in)
    assert J < beam_in
    top = os.path.join(tmp, "top")            # the tree above the leaf layer: its prediction is the beam the leaf layer takes in
    for d in range(LEAF):
        shutil.copytree(os.path.join(folder, "ranker", f"{d}.model"), os.path.join(top, "ranker", f"{d}.model"))
    shutil.copy(os.path.join(folder, "param.json"), os.path.join(top, "param.json"))
    par = json.load(open(os.path.join(folder, "ranker", "param.json")))
    C1 = smat.load_npz(os.path.join(folder, "ranker", f"{LEAF - 1}.model", "C.npz"))
    par.update(depth=LEAF, nr_codes=C1.shape[1], nr_labels=C1.shape[0])
    json.dump(par, open(os.path.join(top, "ranker", "param.json"), "w"))
    beam = _reference(top, oracle_mod).predict(X, **dict(KW, only_topk=KW["beam_size"]))
    later = np.zeros(X.shape[0], bool)
    for r in range(X.shape[0]):
        idx, val = beam.indices[beam.indptr[r]:beam.indptr[r + 1]], beam.data[beam.indptr[r]:beam.indptr[r + 1]]
        if len(val) <= J:
            continue
        jth = np.sort(val)[::-1][J - 1]
        score = dict(zip(idx.tolist(), val.tolist()))
        later[r] = any(score[p] < jth for p in parent_of[want.indices[want.indptr[r]:want.indptr[r + 1]]].tolist())
    return later


def _same_rows(got, want, n, what):
    cnt = np.tile(np.diff(want.indptr), -(-n // want.shape[0]))[:n]
    data, idx = np.tile(want.data, -(-n // want.shape[0])), np.tile(want.indices, -(-n // want.shape[0]))
    exp = smat.csr_matrix((data[:cnt.sum()], idx[:cnt.sum()], np.concatenate([[0], np.cumsum(cnt)])), shape=(n, want.shape[1]))
    assert_same_topk(got, exp, exact_scores=True, what=what)


def test_second_stage_runs_and_matches(tmp_path, oracle_mod):
    folder = os.path.join(GOLDEN, "synth", "s_eurlex")
    X = load_X(os.path.join(GOLDEN, "synth", "s_eurlex__X.npz"), "dense")
    want = _reference(folder, oracle_mod).predict(X, **KW)          # raw CSR: the score-sorted order inside the rows
    later = rows_beyond_first_stage(folder, X, want, str(tmp_path), oracle_mod)
    # (row 0 too: it is the whole batch of the 1-row case; about half of the 64 rows, so every larger batch holds finished and unfinished queries)
    assert later[0] and 0.25 < later.mean() < 0.75, f"rows that need a beam slot beyond the first stage: {later.sum()} of {len(later)}, row 0: {later[0]}"

    from pecos_amd import XLinearModel, clib
    assert clib.device_count() > 0, "no GPU visible"
    m = XLinearModel.load(folder)
    h = m.model.model_chain
    try:
        for n in ROWS:
            Xn = np.ascontiguousarray(np.tile(X, (-(-n // X.shape[0]), 1))[:n])
            for k, v in dict(k1g_min_items=1, prune=1, adaptive=0).items():
                clib.set_option(h, k, v)
            clib.profile_reset(h); clib.profile_enable(h, True)
            got = m.predict(Xn, **KW)
            prof = {(r["name"], int(r["layer"])) for r in clib.profile_get(h)}
            clib.profile_enable(h, False)
            assert ("k1g_dense_x", LEAF) in prof and REST <= prof, (n, sorted(prof))
            _same_rows(got, want, n, f"rows {n}: pruned K1G vs reference")
            clib.set_option(h, "prune", 0)
            clib.profile_reset(h); clib.profile_enable(h, True)
            base = m.predict(Xn, **KW)
            prof = {(r["name"], int(r["layer"])) for r in clib.profile_get(h)}
            clib.profile_enable(h, False)
            assert ("k1g_dense_x", LEAF) in prof and not (REST & prof), (n, sorted(prof))
            assert_same_topk(got, base, exact_scores=True, what=f"rows {n}: prune=1 vs prune=0")
    finally:
        for k, v in DEFAULTS.items():
            clib.set_option(h, k, v)
