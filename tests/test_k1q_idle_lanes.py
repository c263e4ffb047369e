"""GPU (-m gpu): K1Q lanes WITHOUT a candidate -- the padding columns of a parent with fewer children than its dense tile is wide, the slots of a
beam shorter than the candidate registers -- switch their weight loads off (csrc/xrl_k1q_impl.h, k1q_candidate) instead of requesting column 0 of
the layer.  Nothing they accumulate is ever read, so every result (label ids, order, fp32 score bits, counts) must equal the reference's: staged,
unstaged with presence words (prune = 0), fused and single-layer launches, sparse and dense X, finite and non-finite x.

Trees (D = 600, about 14 features per query): `pad62` [4, 12, 744]: 62 children in 64-column tiles, ten registers at beam 10; `pad5` [3, 20, 100]:
5 children in 8-column tiles and beams of 2-3 parents in a register of 8 slots; `pad31` [2, 64, 2000]: 31-32 children in 32-column tiles."""
import numpy as np
import pytest

from conftest import assert_same_topk

pytestmark = pytest.mark.gpu

D = 600
TREES = {"pad62": [4, 12, 744], "pad5": [3, 20, 100], "pad31": [2, 64, 2000]}
DEFAULTS = dict(prune=1, adaptive=1, dense_layers=1, k1q_fuse=3, k1g_min_items=16, presence=1)


@pytest.fixture(scope="module")
def clib():
    from pecos_amd import clib
    assert clib.device_count() > 0, "no GPU visible"
    return clib


@pytest.fixture(scope="module")
def cases(tmp_path_factory, oracle_mod):
    import xrl_synth
    from pecos_amd import XLinearModel
    tmp, made = tmp_path_factory.mktemp("k1q_idle_lanes"), {}

    def get(tree):
        if tree not in made:
            folder, seed = str(tmp / tree), 511 + 3 * sorted(TREES).index(tree)
            xrl_synth.make_model(folder, D, TREES[tree][-1], [60, 40, 16], seed=seed, shape=TREES[tree], permute_leaf=True, only_topk=10)
            X = xrl_synth.make_queries(300, D, 14, seed=seed + 1, relabel_seed=seed)
            ref = oracle_mod.RefModel(folder, "BINARY_SEARCH_CHUNKED") if oracle_mod.ref_available() else oracle_mod.OracleModel.load(folder)
            made[tree] = (XLinearModel.load(folder), ref, X)
        return made[tree]
    return get


def run(m, clib, X, kw, **opts):
    h = m.model.model_chain
    for k, v in dict(dict(adaptive=0), **opts).items():
        clib.set_option(h, k, v)
    try:
        return m.predict(X, **kw)
    finally:
        for k, v in DEFAULTS.items():
            clib.set_option(h, k, v)


OPTS = (dict(), dict(prune=0), dict(prune=0, presence=2), dict(k1q_fuse=0), dict(k1q_fuse=0, prune=0), dict(dense_layers=2))


@pytest.mark.parametrize("tree", sorted(TREES))
def test_equal_to_the_reference(tree, cases, clib):
    m, ref, X = cases(tree)
    for kw in (dict(beam_size=10, only_topk=10), dict(beam_size=3, only_topk=5), dict(beam_size=2, only_topk=10), dict(beam_size=10, only_topk=10, post_processor="sigmoid")):
        want = ref.predict(X, **kw)
        # the sigmoid family goes through an expf that is not the reference's last bit everywhere (the suite compares it within 1e-5 relative):
        # there the bit-for-bit partner is the same library's tile-format pipeline, which has no K1Q lanes at all
        exact = "post_processor" not in kw
        tile = None if exact else run(m, clib, X, kw, prune=0, dense_layers=0)
        for n in (1, 65, 300):
            for o in OPTS:
                got = run(m, clib, X[:n], kw, **o)
                assert_same_topk(got, want[:n], exact_scores=exact, what=f"{tree} {kw} rows {n} {o} vs reference")
                if tile is not None:
                    assert_same_topk(got, tile[:n], exact_scores=True, what=f"{tree} {kw} rows {n} {o} vs the tile-format kernels")


@pytest.mark.parametrize("tree", sorted(TREES))
def test_nonfinite_x_and_dense_x(tree, cases, clib):
    m, ref, X = cases(tree)
    kw = dict(beam_size=10, only_topk=10)
    Xb = X[:130].copy()
    for r, bad in zip((0, 7, 64, 129), (np.inf, np.nan, 3e38, -np.inf)):
        Xb.data[Xb.indptr[r]] = bad
    base = run(m, clib, Xb, kw, prune=0, dense_layers=0)          # the tile-format kernels: no idle K1Q lanes involved
    for o in OPTS:
        got = run(m, clib, Xb, kw, **o)
        assert np.array_equal(got.indptr, base.indptr) and np.array_equal(got.indices, base.indices), (tree, o)
        assert np.array_equal(got.data.view(np.uint32), base.data.view(np.uint32)), (tree, o)      # NaN scores included
    Xd = np.ascontiguousarray(X[:40].toarray())
    want = ref.predict(Xd, **kw)
    for o in (dict(k1g_min_items=0), dict(k1g_min_items=0, prune=0), dict(k1g_min_items=0, k1q_fuse=0)):
        assert_same_topk(run(m, clib, Xd, kw, **o), want, exact_scores=True, what=f"{tree} dense X {o}")
