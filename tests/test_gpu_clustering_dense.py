"""Clustering of a dense matrix resident in HBM (K11D): run_clustering_device on a CUDA tensor against the numpy statement of the rule on
the CSR of all rows * cols entries -- codes, the bits of the scores and the iterations per level, exactly."""
import functools

import numpy as np
import pytest

import clustering_rule as cr

pytestmark = pytest.mark.gpu

ALGOS = [cr.SKMEANS, cr.KMEANS]
SAMPLED = dict(max_rate=0.8, min_rate=0.5, warmup=0.5)


@functools.lru_cache(maxsize=None)
def problem(rows, cols, depth, algo, seed=0, max_iter=20, sampled=False):
    """(D, the statement's keywords, the statement's answer), computed once per case."""
    D = np.random.RandomState(1000 * rows + cols).standard_normal((rows, cols)).astype(np.float32)
    kw = dict(algo=algo, seed=seed, max_iter=max_iter, **(SAMPLED if sampled else {}))
    return D, kw, cr.statement(cr.as_full_csr(D), depth, **kw)


def device_kw(kw):
    return dict(partition_algo=kw["algo"], seed=kw["seed"], kmeans_max_iter=kw["max_iter"], max_sample_rate=kw.get("max_rate", 1.0),
                min_sample_rate=kw.get("min_rate", 1.0), warmup_ratio=kw.get("warmup", 1.0))


def check(codes, scores, t, depth):
    from pecos_amd import clib
    assert np.array_equal(codes.cpu().numpy().view(np.uint32), t["codes"]), "codes differ from the statement"
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), t["scores"].view(np.uint32)), "scores differ from the statement"
    forms = clib.debug_cluster_forms()
    assert forms["iters"] == [max(k for nid, k in t["iters"].items() if nid.bit_length() - 1 == d) for d in range(depth)]
    assert (forms["lane_runs"], forms["wave_runs"]) == (0, 0)
    return clib.debug_cluster_dense_forms()


SHAPES = ([(130, c, 3) for c in (1, 63, 64, 65, 129, 768)] + [(4, c, 2) for c in (1, 63, 64, 65, 129, 768)] +      # feature-tile edges
          [(257, 65, 1), (257, 65, 5), (257, 65, 7), (64, 65, 5), (65, 65, 5)])                                     # element tiles, node sizes
OPTIONS = [(200, 129, 6, cr.SKMEANS, 0, k, False) for k in (0, 1, 2)] + [(200, 129, 6, a, 0, 20, True) for a in ALGOS] + \
          [(200, 129, 6, cr.KMEANS, s, 20, False) for s in (1, 2)]


@pytest.mark.parametrize("case", [s + (a,) for s in SHAPES for a in ALGOS] + OPTIONS, ids=lambda c: "-".join(str(v) for v in c))
def test_tensor_form_against_the_statement(case):
    import pecos_amd
    import torch
    D, kw, t = problem(*case)
    rows, cols, depth = case[:3]
    codes, scores = pecos_amd.run_clustering_device(torch.from_numpy(D).cuda(), depth, return_scores=True, **device_kw(kw))
    dense = check(codes, scores, t, depth)
    if kw["max_iter"] > 1:
        assert dense["centre_chains"] > 0
    if (rows, depth) == (257, 1):
        assert dense["one_node_tiles"] > 0 and dense["mixed_tiles"] == 0
    if (rows, depth) == (257, 7):
        assert dense["mixed_tiles"] > 0


def test_window_of_a_wider_tensor_on_a_side_stream():
    """row_stride = cols + 3, an odd element offset, NaN in the padding and around the window: the packed copy's answer, operand unchanged."""
    import pecos_amd
    import torch
    rows, cols, depth = 130, 129, 3
    D, kw, t = problem(rows, cols, depth, cr.SKMEANS)
    flat = torch.full((1 + (rows + 2) * (cols + 3),), float("nan"), dtype=torch.float32, device="cuda")
    window = flat[1:].view(rows + 2, cols + 3)[1:rows + 1, :cols]
    window.copy_(torch.from_numpy(D))
    assert window.storage_offset() % 2 == 1 and window.stride() == (cols + 3, 1)
    before = flat.view(torch.int32).clone()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    codes, scores = pecos_amd.run_clustering_device(window, depth, return_scores=True, stream=side.cuda_stream, **device_kw(kw))
    torch.cuda.synchronize()
    check(codes, scores, t, depth)
    assert torch.equal(flat.view(torch.int32), before)


def test_three_doors_give_one_answer():
    import pecos_amd
    import torch
    rows, cols, depth = 130, 129, 3
    D, kw, t = problem(rows, cols, depth, cr.SKMEANS)
    host, err = cr.run_library(cr.OURS, D, depth, **kw)
    assert err is None, err
    tensor = pecos_amd.run_clustering_device(torch.from_numpy(D).cuda(), depth, **device_kw(kw)).cpu().numpy().view(np.uint32)
    csr = pecos_amd.run_clustering_device(cr.as_full_csr(D), depth, **device_kw(kw)).cpu().numpy().view(np.uint32)
    assert np.array_equal(host, tensor) and np.array_equal(tensor, csr) and np.array_equal(csr, t["codes"])
