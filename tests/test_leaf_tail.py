"""GPU (-m gpu): the later stage of a bound-pruned tile-format layer of two stages runs from a LIST of the unfinished queries (library option
leaf_tail; csrc/xrl_k1t.hip and xrl_k2.hip append to it, k0b_remaining_list / k1_list_kernel / k2_topk_list walk it).  For every case the
result under leaf_tail = 1 (the default) and leaf_tail = 8 (K1 always on a fixed grid of 8 workgroups: the looped kernel) equals, bit for bit
(label ids, order, fp32 score bits, counts), the same handle's under leaf_tail = 0, under prune = 0, and the reference's.

Two trees ([2, 64, 2000]: leaf parents of one tile, K1T's epilogue writes the list; [2, 36, 6000]: parents of 167 children = two tiles, K2
writes it), three weight variants each: `saturated` (every transform is 1: every query is done after slot 0, the list is empty), `unsaturated`
(no transform saturates and the parents score alike: the reference alone shows >= 90 % of the rows with a label that is not a child of
their best parent, i.e. needing a later slot) and `mixed` (the children of every other leaf parent saturate: some of each).  What the reference says about a variant is asserted on the CPU side
before the GPU is consulted."""
import json
import os
import shutil

import numpy as np
import pytest
import scipy.sparse as smat

from conftest import assert_same_topk

pytestmark = pytest.mark.gpu

D = 1500
ROWS = (1, 3, 5, 63, 64, 65, 257, 1000)
TREES = {"one_tile": [2, 64, 2000], "two_tiles": [2, 36, 6000]}
KW = {2: dict(beam_size=2, only_topk=10), 6: dict(beam_size=6, only_topk=10), 10: dict(beam_size=10, only_topk=10), 20: dict(beam_size=20, only_topk=10)}
REST = {("k0b_remaining", 2), ("k1_sparse_rest", 2), ("k2_topk_rest", 2)}
LIST, GRID = ("rest_list", 2), ("rest_list_grid", 2)     # profile slots of the list-driven route alone: the list was reset / K1 ran its fixed-grid kernel
MID = {("k0b_remaining_mid", 2), ("k1_sparse_mid", 2), ("k2_topk_mid", 2)}


@pytest.fixture(scope="module")
def clib():
    from pecos_amd import clib
    assert clib.device_count() > 0, "no GPU visible"
    return clib


def _rescale(folder, variant):
    for d in range(3):
        f = os.path.join(folder, "ranker", f"{d}.model", "W.npz")
        W = smat.load_npz(f).tocsc().astype(np.float32)
        if variant == "saturated":
            W.data[:] = 2.0                              # z = 2 (sum x + 1) >= 1: l3-hinge gives exactly 1 everywhere
        elif d < 2:
            W.data[:] = (0.01 * W.data).astype(np.float32)   # the parents score alike: the leaf's transform decides
        else:
            W.data[:] = np.clip(0.3 * W.data, -0.6, 0.12).astype(np.float32)   # z <= 0.12 (sum x + 1) stays below the hinge's knee at 1
            if variant in ("mixed", "few_unfinished"):   # the children of every other leaf parent (few_unfinished: of 15 in 16) saturate: a query is done iff its best parent is one of those
                C = smat.load_npz(os.path.join(folder, "ranker", "2.model", "C.npz")).tocsc()
                sat = np.zeros(W.shape[1], bool)
                sat[C.indices] = np.repeat(np.arange(C.shape[1]) % (2 if variant == "mixed" else 16) != 1, np.diff(C.indptr))
                W.data[np.repeat(sat, np.diff(W.indptr))] = 2.0
        smat.save_npz(f, W, compressed=False)


class Case:
    """One model folder, its handle, its queries and the reference's answers (computed once, never changed)."""

    def __init__(self, tree, variant, tmp, oracle_mod):
        import xrl_synth
        from pecos_amd import XLinearModel
        self.tree, self.variant = tree, variant
        self.folder = os.path.join(tmp, f"{tree}_{variant}")
        seed = 301 + 7 * sorted(TREES).index(tree)
        shape = TREES[tree]
        xrl_synth.make_model(self.folder, D, shape[-1], [40, 40, 14], seed=seed, shape=shape, permute_leaf=True, only_topk=10)
        _rescale(self.folder, variant)
        self.X = xrl_synth.make_queries(1000, D, 12, seed=seed + 1, relabel_seed=seed)
        self.ref = oracle_mod.RefModel(self.folder, "BINARY_SEARCH_CHUNKED") if oracle_mod.ref_available() else oracle_mod.OracleModel.load(self.folder)
        self.want = {b: self.ref.predict(self.X, **KW[b]) for b in KW}
        C = smat.load_npz(os.path.join(self.folder, "ranker", "2.model", "C.npz")).tocsc()
        self.parent_of = np.empty(C.shape[0], np.int64)
        self.parent_of[C.indices] = np.repeat(np.arange(C.shape[1]), np.diff(C.indptr))
        # the best leaf parent of every row, from the reference on the tree's first two layers
        top = os.path.join(tmp, f"{tree}_{variant}_top")
        shutil.copytree(os.path.join(self.folder, "ranker", "0.model"), os.path.join(top, "ranker", "0.model"))
        shutil.copytree(os.path.join(self.folder, "ranker", "1.model"), os.path.join(top, "ranker", "1.model"))
        shutil.copy(os.path.join(self.folder, "param.json"), os.path.join(top, "param.json"))
        par = json.load(open(os.path.join(self.folder, "ranker", "param.json")))
        par.update(depth=2, nr_codes=shape[0], nr_labels=shape[1])
        json.dump(par, open(os.path.join(top, "ranker", "param.json"), "w"))
        rt = oracle_mod.RefModel(top, "BINARY_SEARCH_CHUNKED") if oracle_mod.ref_available() else oracle_mod.OracleModel.load(top)
        best = rt.predict(self.X, beam_size=2, only_topk=1)
        assert np.all(np.diff(best.indptr) == 1)
        self.best_parent = best.indices.astype(np.int64)
        check_reference_side(self)                        # on the CPU side, before the model goes to the device
        self.m = XLinearModel.load(self.folder)
        self.h = self.m.model.model_chain

    def needs_later_slot(self, beam):
        """Rows whose reference top-k holds a label that is not a child of the row's best parent: beam slot 0 alone cannot have been final."""
        w = self.want[beam]
        return np.array([np.any(self.parent_of[w.indices[w.indptr[r]:w.indptr[r + 1]]] != self.best_parent[r]) for r in range(w.shape[0])])


@pytest.fixture(scope="module")
def cases(tmp_path_factory, oracle_mod):
    tmp, made = str(tmp_path_factory.mktemp("leaf_tail")), {}

    def get(tree, variant):
        if (tree, variant) not in made:
            made[(tree, variant)] = Case(tree, variant, tmp, oracle_mod)
        return made[(tree, variant)]
    return get


DEFAULTS = dict(dense_layers=1, adaptive=1, leaf_tail=1, leaf_fuse=1, prune=1, prune_mid=1, sort_rest=1, sort_rest_min=32768, max_batch_rows=0, overlap_min_rows=0)


def predict(c, clib, X, beam, profile=False, **opts):
    """Every layer on the tile pipeline, always staged unless the case says otherwise; options back to their defaults afterwards."""
    for k, v in dict(dict(dense_layers=0, adaptive=0), **opts).items():
        clib.set_option(c.h, k, v)
    try:
        if not profile:
            return c.m.predict(X, **KW[beam])
        clib.profile_reset(c.h); clib.profile_enable(c.h, True)
        out = c.m.predict(X, **KW[beam])
        prof = clib.profile_get(c.h)
        clib.profile_enable(c.h, False)
        return out, {(r["name"], int(r["layer"])) for r in prof}
    finally:
        for k, v in DEFAULTS.items():
            clib.set_option(c.h, k, v)


def same(a, b, what):
    assert_same_topk(a, b, exact_scores=True, what=what)


def rows_of(w, n):
    return smat.csr_matrix((w.data[:w.indptr[n]], w.indices[:w.indptr[n]], w.indptr[:n + 1]), shape=(n, w.shape[1]))


def check_reference_side(c):
    """What the reference ALONE says about the variant (no GPU involved)."""
    for beam in (2, 6, 10):
        w, later = c.want[beam], c.needs_later_slot(beam)
        if c.variant == "saturated":
            assert np.all(w.data == np.float32(1.0)) and not later.any(), "saturated: every row must be settled by its best parent"
        elif c.variant == "unsaturated":
            assert np.all(w.data < np.float32(1.0)), "unsaturated: a transform saturated"
            assert later.mean() >= 0.9, f"unsaturated: only {later.mean():.3f} of the rows need a later slot (beam {beam})"
        elif c.variant == "mixed":
            assert 0.1 < later.mean() < 0.9, f"mixed: {later.mean():.3f} of the rows need a later slot (beam {beam})"
        else:   # few_unfinished: some rows, and clearly fewer than the eighth of the slots up to which K1 takes its fixed grid by default
            assert 0.01 < later.mean() < 0.1, f"few_unfinished: {later.mean():.3f} of the rows need a later slot (beam {beam})"


@pytest.mark.parametrize("variant", ["saturated", "unsaturated", "mixed"])
@pytest.mark.parametrize("tree", sorted(TREES))
def test_row_counts_and_beams(tree, variant, cases, clib):
    c = cases(tree, variant)
    for n in ROWS:
        X = c.X[:n]
        for beam in (2, 10):
            what = f"{tree} {variant} rows {n} beam {beam}"
            want = rows_of(c.want[beam], n)
            base = predict(c, clib, X, beam, leaf_tail=0)
            same(base, want, what + ": leaf_tail=0 vs reference")
            for lt in (1, 8):
                got = predict(c, clib, X, beam, leaf_tail=lt)
                same(got, base, what + f": leaf_tail={lt} vs 0")
                same(got, want, what + f": leaf_tail={lt} vs reference")
            if beam == 10:
                same(predict(c, clib, X, beam, prune=0), base, what + ": prune=0 vs leaf_tail=0")


@pytest.mark.parametrize("tree", sorted(TREES))
def test_which_path_ran(tree, cases, clib):
    # the list-driven launches keep the profile names of the ones they replace; a beam of 20 has a middle stage and keeps the batch-sized path
    c = cases(tree, "mixed")
    X = c.X[:257]
    for beam in (2, 6, 10):      # (two tiles, beam 6: 1002 candidates = 16 registers -- the k2_topk_rest that keeps its batch-sized grid)
        for lt in (0, 1, 8):
            got, prof = predict(c, clib, X, beam, profile=True, leaf_tail=lt)
            assert REST <= prof and not (MID & prof), (tree, beam, lt, sorted(prof))
            assert (LIST in prof) == (lt != 0) and (GRID in prof) == (lt == 8), (tree, beam, lt, sorted(prof))
            assert (("k2_topk", 2) in prof) == (tree == "two_tiles"), (tree, beam, lt, sorted(prof))   # one tile: K1T selects (and lists) itself
            same(got, rows_of(c.want[beam], 257), f"{tree} beam {beam} leaf_tail={lt} profiled")
    if tree == "two_tiles":
        return                                            # (20 parents x 167 children: past the register top-k, the layer is not bound-pruned)
    for lt in (0, 1):
        got, prof = predict(c, clib, X, 20, profile=True, leaf_tail=lt)
        assert MID <= prof and REST <= prof and LIST not in prof and GRID not in prof, (tree, lt, sorted(prof))
        same(got, rows_of(c.want[20], 257), f"{tree} beam 20 leaf_tail={lt}")
    # without the middle stage the same beam is a two-stage layer: list-driven
    base = predict(c, clib, X, 20, leaf_tail=0, prune_mid=0)
    for lt in (1, 8):
        got, prof = predict(c, clib, X, 20, profile=True, leaf_tail=lt, prune_mid=0)
        assert REST <= prof and not (MID & prof) and LIST in prof and (GRID in prof) == (lt == 8), (tree, lt, sorted(prof))
        same(got, base, f"{tree} beam 20 prune_mid=0 leaf_tail={lt} vs 0")
        same(got, rows_of(c.want[20], 257), f"{tree} beam 20 prune_mid=0 leaf_tail={lt} vs reference")


def test_fixed_grid_k1_falls_back_where_it_is_not_compiled(cases, clib):
    # the sigmoid family (post-processor class 1) has no k1_list_kernel: the list-driven route, K1 on the worst-case grid
    c = cases("one_tile", "mixed")
    X = c.X[:257]
    for extra, kw in ((dict(), dict(post_processor="sigmoid")),):
        outs = {}
        for lt in (0, 8):
            for k, v in dict(dense_layers=0, adaptive=0, leaf_tail=lt, **extra).items():
                clib.set_option(c.h, k, v)
            clib.profile_reset(c.h); clib.profile_enable(c.h, True)
            outs[lt] = c.m.predict(X, **dict(KW[10], **kw))
            prof = {(r["name"], int(r["layer"])) for r in clib.profile_get(c.h)}
            clib.profile_enable(c.h, False)
            for k, v in dict(DEFAULTS, k1_group=0).items():
                clib.set_option(c.h, k, v)
            assert REST <= prof and (LIST in prof) == (lt == 8) and GRID not in prof, (extra, kw, lt, sorted(prof))
        same(outs[8], outs[0], f"{extra} {kw}: leaf_tail 8 vs 0")


def test_default_threshold_picks_the_fixed_grid(cases, clib):
    # 240 000 rows x 9 later slots >= 2^21 item slots, under 10 % of the rows unfinished: once the pruning feedback has seen a later stage's item count,
    # the default (leaf_tail = 1) runs K1 on its fixed grid of 6144 workgroups; the first predict (count unknown) and leaf_tail = 0 do not
    c = cases("one_tile", "few_unfinished")
    X = smat.vstack([c.X] * 240, format="csr")
    w = c.want[10]
    n = np.diff(w.indptr)
    want = smat.csr_matrix((np.tile(w.data, 240), np.tile(w.indices, 240), np.concatenate([[0], np.cumsum(np.tile(n, 240))])), shape=(X.shape[0], w.shape[1]))
    for lt in (1, 0):
        clib.set_option(c.h, "adaptive", 0)               # (resets the feedback's state)
        for i in range(3):
            got, prof = predict(c, clib, X, 10, profile=True, leaf_tail=lt, adaptive=1)
            assert REST <= prof and (LIST in prof) == (lt == 1), (lt, i, sorted(prof))
            assert (GRID in prof) == (lt == 1 and i > 0), (lt, i, sorted(prof))
            same(got, want, f"240 000 rows leaf_tail={lt} predict #{i + 1}")


@pytest.mark.parametrize("variant", ["unsaturated", "mixed"])
@pytest.mark.parametrize("tree", sorted(TREES))
def test_options_batches_lanes(tree, variant, cases, clib):
    c = cases(tree, variant)
    X, want = c.X[:257], rows_of(c.want[10], 257)
    for lt in (1, 8):
        for lf in (0, 1, 2):
            same(predict(c, clib, X, 10, leaf_tail=lt, leaf_fuse=lf), want, f"{tree} {variant} leaf_tail={lt} leaf_fuse={lf}")
        # the later stage on tile-sorted items (always, without the feedback's count) and in query order
        got, prof = predict(c, clib, X, 10, profile=True, leaf_tail=lt, sort_rest_min=0)
        assert ("k1_sort_items_rest", 2) in prof, sorted(prof)
        same(got, want, f"{tree} {variant} leaf_tail={lt} sorted")
        got, prof = predict(c, clib, X, 10, profile=True, leaf_tail=lt, sort_rest=0)
        assert ("k1_sort_items_rest", 2) not in prof, sorted(prof)
        same(got, want, f"{tree} {variant} leaf_tail={lt} query order")
        # several row batches re-use a lane's list and count; two lanes own one each
        for mb in (64, 100):
            same(predict(c, clib, X, 10, leaf_tail=lt, max_batch_rows=mb), want, f"{tree} {variant} leaf_tail={lt} max_batch_rows={mb}")
            same(predict(c, clib, X, 10, leaf_tail=lt, max_batch_rows=mb, overlap_min_rows=1), want, f"{tree} {variant} leaf_tail={lt} two lanes, max_batch_rows={mb}")
        same(predict(c, clib, X, 10, leaf_tail=lt, overlap_min_rows=1), want, f"{tree} {variant} leaf_tail={lt} two lanes")


@pytest.mark.parametrize("tree", sorted(TREES))
def test_repeated_predicts_with_feedback(tree, cases, clib):
    # the pruning feedback on: the item count a predict finds was written by an earlier one (or not yet); it may pick the sort, either K1 form, or
    # one unstaged pass -- never another result
    for variant in ("unsaturated", "mixed", "saturated"):
        c = cases(tree, variant)
        want = c.want[10]
        for lt in (1, 8, 0):
            clib.set_option(c.h, "adaptive", 0)           # (resets the feedback's state)
            for i in range(5):
                same(predict(c, clib, c.X, 10, leaf_tail=lt, adaptive=1, sort_rest_min=(0, 1 << 30)[i & 1]), want, f"{tree} {variant} leaf_tail={lt} predict #{i + 1}")


@pytest.mark.parametrize("tree", sorted(TREES))
def test_nonfinite_x_in_an_unfinished_query(tree, cases, clib):
    c = cases(tree, "unsaturated")
    X = c.X[:130].copy()
    unfinished = np.nonzero(c.needs_later_slot(10)[:130])[0]
    for r, bad in zip(unfinished[[0, 1, 2, -1]], (np.inf, np.nan, -np.inf, np.inf)):
        X.data[X.indptr[r]] = bad
    base = predict(c, clib, X, 10, prune=0)
    for lt in (0, 1, 8):
        got = predict(c, clib, X, 10, leaf_tail=lt)
        assert np.array_equal(got.indptr, base.indptr) and np.array_equal(got.indices, base.indices), (tree, lt)
        assert np.array_equal(got.data.view(np.uint32), base.data.view(np.uint32)), (tree, lt)      # NaN scores included
    keep = np.setdiff1d(np.arange(130), unfinished[[0, 1, 2, -1]])
    want = c.want[10]
    for r in keep[:: 7]:
        assert np.array_equal(base.indices[base.indptr[r]:base.indptr[r + 1]], want.indices[want.indptr[r]:want.indptr[r + 1]]), (tree, r)
