"""GPU (-m gpu): every form of the per-query top-k at its boundaries, against ONE order (tests/topk_order.py).

The models of tests/topk_models.py make a query's candidate row equal to a row of the case table, so the expected answer is topk() of that row:
counts, label ids, order and fp32 score bits, NaN scores included, nothing within a tolerance.  Flat models walk the candidate-row length across
every NS bucket of the wave form, the wave -> reg hand-over and the reg kernel's 256-candidate fetch groups, with k on either side of 64 (reg / wave
-> lds), of the lds kernel's 64-wide shift loop and of n; one model of 20 482 labels crosses the lds -> big hand-over; a two-layer model reaches
n < cand_stride and the position -> (beam slot, child) -> label mapping.  Every case runs under each row of CONFIGS.  noop layers are never
bound-pruned, so on those models prune=1 and leaf_fuse=1 run K0 -> K1 -> K2 like prune=0; the stages of the bound pruning (rank-limited k2_topk_wave,
k2_topk_mid, k2_topk_list) and K1T's selecting epilogue are reached by one more model under l3-hinge (PRUNED_CONFIGS), whose expected rows are the
restatement's UNSORTED scores ranked by topk(), and whose profile must show the staged launches.  Before a stand-alone K2 case is
compared the profile must show the k2_topk launch on that layer and xrl_debug_k2_form must name the form the table expects for its
(k, cand_stride).  Results land in sentinel-filled caller buffers through xrl_predict_device: entries beyond a row's count stay untouched."""
from collections import namedtuple

import numpy as np
import pytest

import device_views as V
import topk_models as M
import topk_order as T

pytestmark = pytest.mark.gpu

BSC = "BINARY_SEARCH_CHUNKED"
# standalone: the layer's top-k is a k2_topk launch of its own (asserted); max_k: the configuration is only defined up to this k
# must / must_not: kernel names the profile has to show / must not show on the last layer
Config = namedtuple("Config", "name opts layout standalone max_k must must_not", defaults=((), ()))
CONFIGS = [Config("tile format prune=0", dict(dense_layers=0, prune=0, leaf_fuse=0, adaptive=0), BSC, True, None),
           Config("tile format prune=1", dict(dense_layers=0, prune=1, leaf_fuse=0, adaptive=0), BSC, True, None),
           Config("k2_big_min_k=1", dict(dense_layers=0, k2_big_min_k=1, adaptive=0), BSC, True, None),
           Config("dense_layers=1", dict(dense_layers=1), BSC, False, None),
           Config("leaf_fuse=1", dict(dense_layers=0, prune=1, leaf_fuse=1, adaptive=0), BSC, False, 20),
           Config("CSC (K1C)", {}, "CSC", True, None)]
# the same model under a COMBINING post-processor (topk_models.pruned_cases): here prune=1 really stages the layer -- a rank-limited k2_topk_wave, the
# middle stage for beams of >= 16 parents (added in run_case), k2_topk_list on the unfinished queries -- and leaf_fuse=1 hands the first stage to K1T
PRUNED_CONFIGS = [Config("l3-hinge prune=0", dict(dense_layers=0, prune=0, leaf_fuse=0, adaptive=0), BSC, True, None, ("k2_topk",), ("k2_topk_rest", "k2_topk_mid")),
                  Config("l3-hinge prune=1 leaf_fuse=0", dict(dense_layers=0, prune=1, leaf_fuse=0, adaptive=0), BSC, False, None,
                         ("k0_prolongate", "k2_topk", "k0b_remaining", "k2_topk_rest"), ()),
                  Config("l3-hinge prune=1 leaf_fuse=1", dict(dense_layers=0, prune=1, leaf_fuse=1, adaptive=0), BSC, False, 20,
                         ("k1_sparse", "k0b_remaining", "k2_topk_rest"), ("k0_prolongate", "k2_topk"))]
OPTION_DEFAULTS = dict(dense_layers=1, prune=1, leaf_fuse=1, adaptive=1, k2_big_min_k=0)
SENT_BITS = int(np.float32(V.SENT_VAL).view(np.uint32))


@pytest.fixture(scope="module")
def clib():
    from pecos_amd import clib
    assert clib.device_count() > 0, "no GPU visible"
    return clib


class _Buffers:
    """Sentinel result buffers per (rows, stride), refilled before every predict."""

    def __init__(self):
        self.made = {}

    def get(self, n, stride):
        if (n, stride) not in self.made:
            self.made[(n, stride)] = V.sentinel_out(n, stride, elem_offsets=(1, 3, 2))
        (wi, pi), (wv, pv), (wc, pc) = out = self.made[(n, stride)]
        wi.fill_(V.SENT_IDX); wv.fill_(V.SENT_VAL); wc.fill_(V.SENT_IDX)
        return out


def _expected_arrays(case, k, stride):
    """What the three buffers must hold: the winners' labels and score bits, the sentinel beyond every row's count."""
    n = len(case.cand)
    idx = np.full((n, stride), V.SENT_IDX, np.int64); bits = np.full((n, stride), SENT_BITS, np.int64); cnt = np.zeros(n, np.int64)
    for r, (lab, b) in enumerate(M.expected(case, k)):
        idx[r, : len(lab)] = lab; bits[r, : len(lab)] = b; cnt[r] = len(lab)
    return idx, bits, cnt


def _name(case, r):
    return "no candidates" if case.rows[r] is None else case.rows[r].name


def _compare(out, want, case, what):
    import torch
    (wi, pi), (wv, pv), (wc, pc) = out
    torch.cuda.synchronize()
    idx = pi.cpu().numpy().view(np.uint32).astype(np.int64)
    bits = pv.cpu().numpy().view(np.uint32).astype(np.int64)
    cnt = pc.cpu().numpy().view(np.uint32).astype(np.int64)
    widx, wbits, wcnt = want
    for r in np.flatnonzero(cnt != wcnt)[:1]:
        raise AssertionError(f"{what}: row {r} ({_name(case, r)}, n = {len(case.cand[r])}): count {cnt[r]}, expected {wcnt[r]}")
    bad = (idx != widx) | (bits != wbits)
    if bad.any():
        r = int(np.flatnonzero(bad.any(axis=1))[0]); c = int(np.flatnonzero(bad[r])[0])
        where = "beyond the row's count (sentinel overwritten)" if c >= wcnt[r] else f"rank {c}"
        raise AssertionError(f"{what}: row {r} ({_name(case, r)}, n = {len(case.cand[r])}) {where}: label {idx[r, c]} score 0x{bits[r, c]:08X}, "
                             f"expected label {widx[r, c]} score 0x{wbits[r, c]:08X}; {int(bad.any(axis=1).sum())} of {len(wcnt)} rows differ: "
                             f"{sorted({_name(case, int(q)) for q in np.flatnonzero(bad.any(axis=1))})[:12]}")
    V.assert_bands_intact(wi, pi, np.int32(V.SENT_IDX), what + " labels")
    V.assert_bands_intact(wv, pv, np.float32(V.SENT_VAL), what + " scores")
    V.assert_bands_intact(wc, pc, np.int32(V.SENT_IDX), what + " counts")


def _profiled(clib, h, fn):
    clib.profile_reset(h); clib.profile_enable(h, True)
    try:
        fn()
        return {(p["name"], int(p["layer"])) for p in clib.profile_get(h) if p["launches"] > 0}
    finally:
        clib.profile_enable(h, False)


def run_case(clib, case, ks, configs, dense_x=False, bufs=None, pp="noop"):
    """Every k under every configuration; returns {(configuration, k): (form of the stand-alone launch or None, kernel names on the last layer)}."""
    from pecos_amd import XLinearModel
    bufs = bufs or _Buffers()
    n = len(case.cand)
    Xq = np.ascontiguousarray(case.X.toarray()) if dense_x else case.X
    want = {k: _expected_arrays(case, k, k + 3) for k in ks}
    reached = {}
    for layout in dict.fromkeys(c.layout for c in configs):
        m = XLinearModel.load(case.folder, weight_matrix_type=layout)
        h = m.model.model_chain
        last = clib.xlinear_get_int_attr(h, "depth") - 1
        q = clib.queries_upload(h, Xq)
        try:
            for cfg in (c for c in configs if c.layout == layout):
                for o, v in cfg.opts.items():
                    clib.set_option(h, o, v)
                try:
                    for k in ks:
                        if cfg.max_k is not None and k > cfg.max_k:
                            continue
                        what = f"{cfg.name} k={k} beam={case.beam} cand_stride={case.cand_stride} dense X={dense_x}"
                        out = bufs.get(n, k + 3)
                        (_, pi), (_, pv), (_, pc) = out
                        prof = _profiled(clib, h, lambda: clib.predict_device(h, q, case.beam, pp, k, V.addr(pi), V.addr(pv), V.addr(pc), k + 3, sync=True))
                        on_last = sorted(nm for nm, l in prof if l == last or nm.startswith("k1q_fused"))
                        form = None
                        if cfg.standalone:
                            assert ("k2_topk", last) in prof, f"{what}: no k2_topk launch on the last layer: {sorted(prof)}"
                            form = clib.debug_k2_form(k, case.cand_stride, cfg.opts.get("k2_big_min_k", 0))
                            assert form == T.expected_form(k, case.cand_stride, cfg.opts.get("k2_big_min_k", 0)), f"{what}: the library dispatches to {form}"
                        elif cfg.name == "dense_layers=1":        # K1Q's epilogue, or the hand-over to K0 -> K1 -> K2 with the table's form: never both, never neither
                            k1q = any(nm.startswith("k1q") for nm in on_last)
                            assert k1q != ("k2_topk" in on_last), f"{what}: {on_last}"
                            if not k1q:
                                form = clib.debug_k2_form(k, case.cand_stride)
                                assert form == T.expected_form(k, case.cand_stride), f"{what}: the library dispatches to {form}"
                        staged = bool(cfg.opts.get("prune")) and pp != "noop"
                        for nm in cfg.must + (("k2_topk_mid",) if staged and case.beam >= 16 else ()):
                            assert nm in on_last, f"{what}: no {nm} launch on the last layer: {on_last}"
                        for nm in cfg.must_not + (() if staged and case.beam >= 16 else ("k2_topk_mid",)):
                            assert nm not in on_last, f"{what}: a {nm} launch on the last layer: {on_last}"
                        reached[(cfg.name, k)] = (form, on_last)
                        _compare(out, want[k], case, what)
                finally:
                    for o in cfg.opts:
                        clib.set_option(h, o, OPTION_DEFAULTS[o])
        finally:
            clib.queries_free(q)
    return reached


def _report(tag, reached):
    forms = sorted({f for f, _ in reached.values() if f is not None})
    other = sorted({(c, tuple(names)) for (c, _), (f, names) in reached.items() if f is None})
    print(f"\nTOPK-FORMS {tag}: {len(reached)} predicts; stand-alone forms {forms}; other configurations ran {other}")


@pytest.mark.parametrize("L", T.FLAT_L)
def test_flat_rows_through_every_form(L, tmp_path, clib):
    rows = T.scenario_rows(L)
    for s in rows:
        T.check_precondition(s)
    bufs = _Buffers()
    case = M.flat_case(str(tmp_path / "m"), L, rows)
    assert case.cand_stride == L and all(len(c) == L for c in case.cand)
    reached = run_case(clib, case, T.K_VALUES, CONFIGS, bufs=bufs)
    # the stand-alone form is the table's for this (k, L): wave bucket, reg beyond 2048 candidates, lds beyond k = 64
    for k in T.K_VALUES:
        assert reached[("tile format prune=0", k)][0] == T.expected_form(k, L)
        assert reached[("k2_big_min_k=1", k)][0] == ("big", 0)
        assert (L <= 1024 and k <= 64) or "k2_topk" in reached[("dense_layers=1", k)][1]
        if L <= 1024 and k <= 64:      # K1Q holds up to 16 candidate registers per lane and a beam of up to 64: there its epilogue ranks the row
            names = reached[("dense_layers=1", k)][1]
            assert any(nm.startswith("k1q") for nm in names) and "k2_topk" not in names, f"dense_layers=1 k={k}: K1Q's epilogue did not serve the layer: {names}"
    fin = M.flat_case(str(tmp_path / "f"), L, M.finite_rows(rows))
    run_case(clib, fin, T.K_VALUES, [c for c in CONFIGS if c.max_k is None], dense_x=True, bufs=bufs)
    _report(f"flat L={L}", reached)


def test_lds_to_big_handover(tmp_path, clib):
    rows = M.big_rows()
    for s in rows:
        T.check_precondition(s)
    case = M.flat_case(str(tmp_path / "m"), T.BIG_L, rows)
    reached = run_case(clib, case, T.BIG_K, [c for c in CONFIGS if c.max_k is None])
    assert reached[("tile format prune=0", 20480)][0] == ("lds", 0) and reached[("tile format prune=0", 20481)][0] == ("big", 0)
    _report(f"flat L={T.BIG_L}", reached)


def test_two_layers_ragged_rows_and_label_mapping(tmp_path, clib):
    bufs = _Buffers()
    for finite_only in (False, True):
        cases = M.two_layer_cases(str(tmp_path / f"m{int(finite_only)}"), finite_only=finite_only)
        for beam, case in cases.items():
            for s in case.rows:
                if s is not None:
                    T.check_precondition(s)
            assert max(len(c) for c in case.cand) <= case.cand_stride
            cfgs = [c for c in CONFIGS if c.max_k is None] if finite_only else CONFIGS
            reached = run_case(clib, case, M.TWO_LAYER_K, cfgs, dense_x=finite_only, bufs=bufs)
            _report(f"two layers beam={beam} dense X={finite_only}", reached)
        assert len({len(c) for c in cases[3].cand}) >= 4 and all(len(c) < cases[3].cand_stride for c in cases[3].cand)
        assert any(len(c) == 0 for c in cases[1].cand)


def test_bound_pruned_stages_and_fused_epilogue(tmp_path, clib, oracle_mod):
    cases = M.pruned_cases(str(tmp_path / "m"), oracle_mod)
    bufs = _Buffers()
    for beam, case in cases.items():
        M.check_pruned_precondition(case)
        reached = run_case(clib, case, M.PRUNED_K, PRUNED_CONFIGS, bufs=bufs, pp=M.PRUNED_PP)
        # the stages' own dispatch: a rank-limited first stage holds registers for the first slot's children, the last one walks the list
        assert clib.debug_k2_form(20, case.cand_stride, stage=2) == (("wave" if T.wave_bucket(case.cand_stride) == 16 else "list"), T.wave_bucket(case.cand_stride))
        _report(f"bound-pruned beam={beam}", reached)
