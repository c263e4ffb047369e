"""HNSW search (K17) without a GPU: the numpy statement of the rule against the recording under tests/golden/hnsw/ and against the compiled
reference when oracle/_ref is there (dense comparisons only where the host has avx512f: the dense rule is that clone's), the wrong
variants shown to differ, the heap restatement, the folder reader and writer, every refusal that needs no GPU, and the Python surface.
The cases of hnsw_rule.range_edge_cases() -- finite inputs whose distances overflow fp32 or are NaN -- agree three ways: statement, live
reference, the recording golden/hnsw/range_edges.npz; a test shows each case to hold what it is named for, and the comparisons written
as negations of their opposites (and a positive NaN) are shown to differ."""
import ctypes
import json
import os

import numpy as np
import pytest
import scipy.sparse as smat

import hnsw_rule as hr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hnsw")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
SETTINGS = [tuple(s) for s in MANIFEST["settings"]]
needs_reference = pytest.mark.skipif(not hr.have_reference(), reason="oracle/_ref/libpecos_float32.so is not built")


def gate(kind):
    """The live reference answers for dense data by its CPU clone; only the avx512f one is the rule."""
    if not hr.have_reference():
        pytest.skip("oracle/_ref/libpecos_float32.so is not built")
    if kind == "drm" and not hr.host_has_avx512f():
        pytest.skip("dense comparison with the live reference needs avx512f on this host (the recording is the yardstick)")


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def golden_queries(name):
    folder = os.path.join(GOLDEN, name)
    if MANIFEST["cases"][name]["data_type"] == "drm":
        return folder, np.load(os.path.join(folder, "queries.npy"))
    return folder, smat.load_npz(os.path.join(folder, "queries.npz")).tocsr()


def all_pairs_index(items, metric):
    """Every item is returned with topk = num_node, so the answer reads the distance statement."""
    return hr.Index(items, hr.full_graph(items.shape[0]), metric=metric)


# ------------------------------------------------------------------------------------------------ the statement against the recording
def test_recording_host_had_avx512f():
    assert "avx512f" in MANIFEST["cpu_flags"]


@pytest.mark.parametrize("name", sorted(MANIFEST["cases"]))
def test_statement_matches_the_recording(name):
    folder, Q = golden_queries(name)
    ix = hr.read_folder(folder)
    exp = np.load(os.path.join(folder, "expected.npz"))
    for efS, topk in SETTINGS:
        idx, dist, _, _ = hr.statement(ix, Q, efS, topk)
        assert np.array_equal(idx, exp["idx_%d_%d" % (efS, topk)]), (name, efS, topk)
        assert np.array_equal(dist.view(np.uint32), exp["bits_%d_%d" % (efS, topk)]), (name, efS, topk)


@pytest.mark.parametrize("name", sorted(MANIFEST["cases"]))
def test_live_reference_matches_the_recording(name):
    gate(MANIFEST["cases"][name]["data_type"])
    folder, Q = golden_queries(name)
    exp = np.load(os.path.join(folder, "expected.npz"))
    for efS, topk in SETTINGS:
        idx, dist = hr.run_reference(folder, Q, efS, topk)
        assert np.array_equal(idx, exp["idx_%d_%d" % (efS, topk)]) and np.array_equal(dist.view(np.uint32), exp["bits_%d_%d" % (efS, topk)])
        idx4, dist4 = hr.run_reference(folder, Q, efS, topk, threads=4)     # 1 and 4 searchers: the same ids and bits
        assert same((idx, dist), (idx4, dist4))


# ------------------------------------------------------------------------------------------------ the distance statements
DENSE_LENS = list(range(0, 71)) + [127, 128, 129, 130]


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_dense_distance_statement_against_the_live_reference(tmp_path, metric):
    gate("drm")
    for ln in DENSE_LENS:
        items, Q = hr.dense_items(6, ln, 1000 + ln), hr.dense_items(3, ln, 2000 + ln)
        ix = all_pairs_index(items, metric)
        folder = hr.write_folder(ix, str(tmp_path / ("d%d" % ln)))
        assert same(hr.run_reference(folder, Q, 6, 6), hr.statement(ix, Q, 6, 6)[:2]), ln


SPARSE_LENS = list(range(0, 10)) + [63, 64, 65]


def sparse_length_cases():
    items = hr.sparse_items(len(SPARSE_LENS), 80, 0, 5, lengths=SPARSE_LENS)
    Q = hr.sparse_items(len(SPARSE_LENS), 80, 0, 6, lengths=SPARSE_LENS)
    return items, Q


def one_common_id_cases():
    """Rows of 9 ids; the query shares exactly one id with the item: its first, its last, and one at position 3 of the item and 4 of the query
    (the two sides of a 4-block boundary); and a query that shares none."""
    item = smat.csr_matrix((np.arange(1, 10, dtype=np.float32), (np.zeros(9, int), np.arange(10, 100, 10))), shape=(1, 200))
    rows = []
    for common, below in ((10, 0), (90, 8), (40, 4)):
        ids = sorted([common] + [1 + 2 * k for k in range(below)] + [101 + 2 * k for k in range(8 - below)])
        rows.append(ids)
    rows.append([1 + 2 * k for k in range(9)])
    Q = smat.lil_matrix((4, 200), dtype=np.float32)
    for r, ids in enumerate(rows):
        for k, c in enumerate(ids):
            Q[r, c] = 0.5 + k
    items = smat.vstack([item, item * 2.0]).tocsr().astype(np.float32)
    return items, Q.tocsr()


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("case", ["lengths", "one_common_id"])
def test_sparse_distance_statement_against_the_live_reference(tmp_path, metric, case):
    gate("csr")
    items, Q = sparse_length_cases() if case == "lengths" else one_common_id_cases()
    ix = all_pairs_index(items, metric)
    folder = hr.write_folder(ix, str(tmp_path / "s"))
    n = items.shape[0]
    got, want = hr.run_reference(folder, Q, n, n), hr.statement(ix, Q, n, n)
    assert same(got, want[:2])
    if case == "one_common_id":                      # the query that shares no id: every distance is exactly 1 (ip) or 0 (l2)
        assert set(want[1][3].tolist()) == ({0.0} if metric == "l2" else {1.0})


def test_sparse_l2_is_minus_two_dot():
    qi, qv = np.array([1, 5, 9]), np.array([0.5, 2.0, 3.0], np.float32)
    ii, iv = np.array([5, 9, 11]), np.array([1.5, -1.0, 4.0], np.float32)
    dot = np.float32(np.float32(0.0) + np.float32(3.0)) + np.float32(-3.0)
    assert hr.sparse_dist(qi, qv, ii, iv, True) == np.float32(-2.0 * dot)
    assert hr.sparse_dist(qi, qv, ii, iv, False) == np.float32(1.0 - dot)


# ------------------------------------------------------------------------------------------------ the wrong variants differ
def test_wrong_dense_variants_differ():
    """len 35 = 2 fused 16-blocks + 3 fused tail elements; len 24 = one 16-block (whose fused step onto +0 is a rounded product, so only
    the order of the additions shows there) and two unfused groups of 4."""
    for ln in (24, 35, 67):
        q, V = hr.dense_items(1, ln, 31)[0], hr.dense_items(200, ln, 32)
        for l2 in (False, True):
            rule = hr.dense_dist(q, V, l2).view(np.uint32)
            if ln >= 32:
                assert not np.array_equal(rule, hr.dense_dist(q, V, l2, "unfused_main").view(np.uint32)), ("unfused_main", ln, l2)
            assert not np.array_equal(rule, hr.dense_dist(q, V, l2, "sequential").view(np.uint32)), ("sequential", ln, l2)


def duplicates_index(n=12, metric="ip"):
    items = np.tile(hr.dense_items(1, 5, 3), (n, 1))
    return hr.Index(items, hr.full_graph(n), metric=metric), hr.dense_items(2, 5, 4)


def test_heaps_that_break_ties_by_node_id_differ():
    ix, Q = duplicates_index()
    a = hr.statement(ix, Q, 12, 12)
    b = hr.statement(ix, Q, 12, 12, ties="id")
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and not np.array_equal(a[0], b[0])


def per_step_case():
    """Level 1: node 0 lists [1, 2], node 1 lists [3]; distances to the query: 0 -> 4, 1 -> 3, 2 -> 2, 3 -> 2.5.  A pass over node 0's list ends at
    node 2 (the first j of the strict minimum); moving at once to node 1 and fetching ITS list ends at node 3."""
    items = np.array([[4.0], [3.0], [2.0], [2.5]], dtype=np.float32)
    ix = hr.Index(items, [[], [], [], []], {(0, 1): [1, 2], (1, 1): [3], (2, 1): [], (3, 1): []}, maxM=2, maxM0=4, max_level=1, init_node=0, metric="l2")
    return ix, np.zeros((1, 1), dtype=np.float32)


def test_per_step_upper_level_update_differs():
    ix, Q = per_step_case()
    assert hr.statement(ix, Q, 1, 1)[0][0, 0] == 2
    assert hr.statement(ix, Q, 1, 1, upper="step")[0][0, 0] == 3


@needs_reference
def test_per_pass_upper_level_update_is_the_references(tmp_path):
    gate("drm")
    ix, Q = per_step_case()
    folder = hr.write_folder(ix, str(tmp_path / "u"))
    assert hr.run_reference(folder, Q, 1, 1)[0][0, 0] == 2


# ------------------------------------------------------------------------------------------------ distances that leave fp32's range
EDGE_CASES = hr.range_edge_cases()
EDGE_REC = hr.range_edge_recording(os.path.join(GOLDEN, "range_edges.npz"), EDGE_CASES)
_edge_statements = {}


def edge_statement(name, efS, topk):
    """Computed once per (case, setting) and shared; nothing writes to it."""
    if (name, efS, topk) not in _edge_statements:
        ix, Q, _ = EDGE_CASES[name]
        _edge_statements[(name, efS, topk)] = hr.statement(ix, Q, efS, topk)
    return _edge_statements[(name, efS, topk)]


def test_range_edge_cases_stay_small_and_finite():
    assert {(ix.data_type, ix.metric) for ix, _, _ in EDGE_CASES.values()} == {(k, m) for k in ("csr", "drm") for m in ("ip", "l2")}
    for name, (ix, Q, settings) in EDGE_CASES.items():
        assert ix.num_node <= 64 and Q.shape[0] <= 8 and ix.feat_dim <= 40 and settings, name
        for A in (ix.items, Q):
            assert np.isfinite(A.data if smat.issparse(A) else A).all(), name


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_range_edges_statement_matches_the_recording(name):
    for efS, topk in EDGE_CASES[name][2]:
        idx, dist, _, _ = edge_statement(name, efS, topk)
        assert np.array_equal(idx, EDGE_REC[(name, efS, topk)][0]), (name, efS, topk)
        assert np.array_equal(dist.view(np.uint32), EDGE_REC[(name, efS, topk)][1]), (name, efS, topk)


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_range_edges_live_reference_matches_the_recording(tmp_path, name):
    ix, Q, settings = EDGE_CASES[name]
    gate(ix.data_type)
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    assert hr.check_folder(folder)[1] is None                       # finite inputs: the loader serves them
    for efS, topk in settings:
        for threads in (1, 4):                                       # the reference repeats itself, with 1 and with 4 searchers
            idx, dist = hr.run_reference(folder, Q, efS, topk, threads=threads)
            assert np.array_equal(idx, EDGE_REC[(name, efS, topk)][0]) and np.array_equal(dist.view(np.uint32), EDGE_REC[(name, efS, topk)][1]), (name, efS, topk, threads)


@pytest.mark.parametrize("name", sorted(n for n in EDGE_CASES if (EDGE_CASES[n][0].num_node,) * 2 in EDGE_CASES[n][2]))
def test_range_edges_efS_above_the_node_count_admits_every_visited_node(name):
    """What lets the GPU tests hold the HBM heap form (efS = CAP + 1) against the recording of (num_node, num_node)."""
    ix, Q, _ = EDGE_CASES[name]
    n = ix.num_node
    a, b = edge_statement(name, n, n), hr.statement(ix, Q, hr.caps()["CAP"] + 1, n)
    assert same(a, b) and {k: a[3][k] for k in hr.COUNTERS[:5]} == {k: b[3][k] for k in hr.COUNTERS[:5]}


def bits_of(name):
    return np.concatenate([edge_statement(name, e, t)[1].view(np.uint32).reshape(-1) for e, t in EDGE_CASES[name][2]])


def rows_of(name):
    for e, t in EDGE_CASES[name][2]:
        idx, dist, count, _ = edge_statement(name, e, t)
        for r in range(dist.shape[0]):
            yield dist[r, :count[r]]


def nan_inside(row):
    """A NaN with a number before it and a number after it: sort_heap leaves NaNs where its comparisons drop them."""
    k = np.flatnonzero(np.isnan(row))
    return len(k) > 0 and any((~np.isnan(row[:i])).any() and (~np.isnan(row[i + 1:])).any() for i in k)


NAN, PINF, NINF, MAXF = 0xFFC00000, 0x7F800000, 0xFF800000, 0x7F7FFFFF


def is_subnormal(bits):
    return ((bits & 0x7F800000) == 0) & ((bits & 0x007FFFFF) != 0)


def test_range_edge_cases_cover_what_they_claim():
    for name in EDGE_CASES:
        ix = EDGE_CASES[name][0]
        b = bits_of(name)
        nans = b[(b & 0x7FFFFFFF) > 0x7F800000]
        assert (nans == NAN).all(), (name, "every NaN of the rule is the host's default NaN")
        if (ix.data_type, ix.metric) == ("drm", "l2"):                # sums of squares: no NaN and no -inf
            assert PINF in b and NINF not in b and len(nans) == 0, name
        elif name != "stages_ip_len3":                                # (length 3 is the fused tail alone: both infinities, never a NaN)
            assert len(nans) and PINF in b and NINF in b, name
        if name.startswith(("seed", "nan_walk", "sparse_dot", "stages_ip_len23")) and (ix.data_type, ix.metric) != ("drm", "l2"):
            assert any(nan_inside(row) for row in rows_of(name)), (name, "a NaN strictly inside a sorted row")
    assert PINF in bits_of("stages_ip_len3") and NINF in bits_of("stages_ip_len3") and not np.isnan(bits_of("stages_ip_len3").view(np.float32)).any()
    # the issue's row: seed, dense ip, query 0
    row = edge_statement("seed_drm_ip_init0", 9, 9)[1][0]
    assert np.array_equal(row.view(np.uint32), np.array([-np.inf, -10, np.nan, np.nan, np.nan, 1, 2.5, np.inf, np.nan], np.float32).view(np.uint32) | (np.isnan(row) * np.uint32(0x80000000)))
    # FLT_MAX reached exactly and not passed; 1 - FLT_MAX is -FLT_MAX; sparse l2 doubles it past the range
    assert MAXF in bits_of("stages_l2_len39") and (MAXF | 0x80000000) in bits_of("sparse_dot_ip")
    assert all((MAXF | 0x80000000) in bits_of("stages_ip_len%d" % ln) for ln in hr.STAGE_POSITIONS)
    # subnormal outputs: l2 only
    for name in ["sparse_dot_l2"] + ["stages_l2_len%d" % ln for ln in hr.STAGE_POSITIONS]:
        assert is_subnormal(bits_of(name)).any(), name
    assert not is_subnormal(bits_of("sparse_dot_ip")).any()
    # the vector on which the fused and the unfused reading of the 16-lane loop differ: BIG and -BIG in accumulator lane 0
    v = hr._dense([{0: hr.BIG, 16: -hr.BIG}], 39)
    q = np.full(39, 2.0, np.float32)
    ix = EDGE_CASES["stages_ip_len39"][0]
    assert any(np.array_equal(v[0].view(np.uint32), it.view(np.uint32)) for it in ix.items) and np.array_equal(EDGE_CASES["stages_ip_len39"][1][0], q)
    with np.errstate(all="ignore"):
        assert hr.dense_dist(q, v, False).view(np.uint32)[0] == NINF and hr.dense_dist(q, v, False, "unfused_main").view(np.uint32)[0] == NAN
    # -0.0 and zeros that are stored
    sp = EDGE_CASES["sparse_dot_ip"]
    for A in (sp[0].items, sp[1]):
        assert (A.data.view(np.uint32) == 0x80000000).any() and (A.data.view(np.uint32) == 0).any()
    assert (EDGE_CASES["stages_ip_len23"][0].items.view(np.uint32) == 0x80000000).any()
    # NaN where the traversal decides
    for name in (n for n in EDGE_CASES if n.startswith("nan_walk")):
        ix, Q, settings = EDGE_CASES[name]
        assert ix.max_level >= 1
        t = {s: edge_statement(name, *s)[3] for s in settings}
        assert all(tr["nan_upper"] > 0 and (tr["nan_break"] > 0 or s == (1, 1)) for s, tr in t.items()), name
        assert all((tr["nan_entry"] > 0) == name.endswith("init0") for tr in t.values()), name
        assert t[(4, 4)]["nan_admit"] > 0 and t[(24, 24)]["nan_admit"] == 0 and t[(12, 5)]["nan_popdown"] > 0, name
        if name.endswith("init0"):                                    # query 0 enters at a NaN and never moves on the upper levels
            got = edge_statement(name, 1, 1)
            assert got[0][0, 0] == 0 and got[1].view(np.uint32)[0, 0] == NAN
    # ties larger than efS at both infinities
    for name in (n for n in EDGE_CASES if n.startswith("inf_ties")):
        ix, Q, _ = EDGE_CASES[name]
        full = edge_statement(name, 30, 30)[1].view(np.uint32)
        if (ix.data_type, ix.metric) == ("drm", "l2"):
            assert ((full == PINF).sum(axis=1) >= 12).any(), name
        else:
            assert (((full == PINF).sum(axis=1) == 12) & ((full == NINF).sum(axis=1) == 12)).any(), name
            assert (edge_statement(name, 5, 5)[1].view(np.uint32) == NINF).all(axis=1).any(), name


@pytest.mark.parametrize("variant", hr.NAN_VARIANTS)
def test_wrong_nan_variants_differ(variant):
    """The three comparisons written as the negation of their opposites, and NaN distances with the positive default NaN."""
    differ = [name for name, (ix, Q, settings) in EDGE_CASES.items() if name.startswith(("nan_walk", "seed_csr"))
              for efS, topk in settings if not same(edge_statement(name, efS, topk), hr.statement(ix, Q, efS, topk, nan=variant))]
    assert differ, variant
    if variant != "positive_nan":                                     # a comparison: ids or finite distances move, not only NaN bits
        name = "nan_walk_csr_ip_init0"
        ix, Q, _ = EDGE_CASES[name]
        assert not np.array_equal(edge_statement(name, 4, 4)[0], hr.statement(ix, Q, 4, 4, nan=variant)[0])


def test_fma32_at_the_range_edges():
    """One rounding, also where the sum is infinite and where a product overflows only once it is rounded."""
    f = np.float32
    B, M, inf = hr.BIG, hr.FLT_MAX, f(np.inf)
    with np.errstate(all="ignore"):
        cases = [((B, f(2), -inf), -inf), ((B, f(2), inf), inf), ((B, f(2), -B), B), ((B, f(2), f(0)), inf), ((-B, f(2), B), -B),
                 ((f(2.0 ** 52), f(2.0 ** 52), M), inf), ((f(2.0 ** 51), f(2.0 ** 51), M), M), ((f(2.0 ** 64), f(2.0 ** 64), -M), f(2.0 ** 104)),
                 ((inf, inf, f(1)), inf), ((f(1e-20), f(1e-20), f(0)), f(np.float64(f(1e-20)) ** 2)), ((f(2), f(3), hr.HOST_NAN), hr.HOST_NAN)]
        for (a, b, c), want in cases:
            got = hr.fma32(np.array([a]), np.array([b]), np.array([c]))
            assert got.dtype == np.float32 and got.view(np.uint32)[0] == np.array([want], np.float32).view(np.uint32)[0], (a, b, c, got, want)


# ------------------------------------------------------------------------------------------------ the heaps
def test_heap_restatement_against_the_recorded_pop_orders():
    rec = np.load(os.path.join(GOLDEN, "heap_orders.npz"))
    for kind, n, values in hr.heap_lists():
        ix, Q = hr.star_index(values)
        assert np.array_equal(hr.statement(ix, Q, n, n)[0][0], rec["%s_%d" % (kind, n)]), (kind, n)
        # the same order from the heap functions alone: push in j order, then sort_heap
        h = []
        for i, v in enumerate(values):
            h.append((np.float32(1.0 - np.float64(v)), i))
            hr.push_heap(h, "max")
        hr.sort_heap(h)
        assert [i for _, i in h] == rec["%s_%d" % (kind, n)].tolist(), (kind, n)


@needs_reference
def test_live_reference_pop_orders_match_the_recording(tmp_path):
    rec = np.load(os.path.join(GOLDEN, "heap_orders.npz"))
    for kind, n, values in hr.heap_lists():
        if n % 7 and n not in (1, 2, 3, 64, 65):
            continue
        ix, Q = hr.star_index(values)
        folder = hr.write_folder(ix, str(tmp_path / ("%s%d" % (kind, n))))
        assert np.array_equal(hr.run_reference(folder, Q, n, n)[0][0], rec["%s_%d" % (kind, n)]), (kind, n)


def test_min_heap_pop_order_is_not_by_id():
    order = hr.heap_pop_order([0.5] * 9, "min")
    assert sorted(order) == list(range(9)) and order != list(range(9))


# ------------------------------------------------------------------------------------------------ reader and writer
@pytest.mark.parametrize("name", sorted(MANIFEST["cases"]))
def test_writer_reproduces_what_the_reader_read(tmp_path, name):
    folder, Q = golden_queries(name)
    ix = hr.read_folder(folder)
    again = hr.read_folder(hr.write_folder(ix, str(tmp_path / "w")))
    assert (again.num_node, again.feat_dim, again.maxM, again.maxM0, again.max_level, again.init_node, again.l1_levels) == \
           (ix.num_node, ix.feat_dim, ix.maxM, ix.maxM0, ix.max_level, ix.init_node, ix.l1_levels)
    assert all(np.array_equal(a, b) for a, b in zip(again.l0, ix.l0)) and again.l1.keys() == ix.l1.keys()
    assert all(np.array_equal(again.l1[k], ix.l1[k]) for k in ix.l1)
    if ix.data_type == "drm":
        assert np.array_equal(again.items.view(np.uint32), ix.items.view(np.uint32))
    else:
        assert np.array_equal(again.items.indptr, ix.items.indptr) and np.array_equal(again.items.indices, ix.items.indices)
        assert np.array_equal(again.items.data.view(np.uint32), ix.items.data.view(np.uint32))


@pytest.mark.parametrize("name", sorted(MANIFEST["cases"]))
def test_reference_loads_what_the_writer_wrote(tmp_path, name):
    gate(MANIFEST["cases"][name]["data_type"])
    folder, Q = golden_queries(name)
    written = hr.write_folder(hr.read_folder(folder), str(tmp_path / "w"))
    assert same(hr.run_reference(written, Q, 20, 10), hr.run_reference(folder, Q, 20, 10))


@pytest.mark.parametrize("name", sorted(MANIFEST["cases"]))
def test_library_reads_the_folder_as_the_reader_does(name):
    folder, _ = golden_queries(name)
    ix = hr.read_folder(folder)
    info, err = hr.check_folder(folder)
    assert err is None
    c = MANIFEST["cases"][name]
    assert info[:9].tolist() == [ix.num_node, ix.feat_dim, ix.maxM, ix.maxM0, ix.efC, ix.max_level, ix.init_node, int(c["data_type"] == "drm"), int(c["metric_type"] == "l2")]
    assert info[9] > 0


# ------------------------------------------------------------------------------------------------ refusals that need no GPU
def small_index(kind="drm", metric="ip"):
    items = hr.dense_items(8, 4, 1) if kind == "drm" else hr.sparse_items(8, 10, 3, 1)
    l0, l1, lv, init = hr.random_graph(8, 3, 2, levels=1, maxM=2)
    return hr.Index(items, l0, l1, maxM=2, maxM0=4, max_level=lv, init_node=init, metric=metric)


def refused(tmp_path, ix, words, **kw):
    folder = hr.write_folder(ix, str(tmp_path / "bad"), **kw)
    info, err = hr.check_folder(folder)
    assert err is not None and err.startswith("xrl_hnsw_load: ") and words in err, err
    m = hr.Ours(folder)                                   # the load itself refuses the same way, before a GPU is required
    assert m.h is None and m.error == err


def test_refused_unknown_type_in_the_references_words(tmp_path):
    refused(tmp_path, small_index(), "Inconsistent HNSW_T: hnsw_t_cur = ", hnsw_t="pecos::ann::HNSWProductQuantizer4Bits<float, pecos::ann::FeatVecDenseL2Simd<float>>")


def test_refused_other_version_in_the_references_words(tmp_path):
    refused(tmp_path, small_index(), "Unable to load memory-mapped file with version = v1.0", version="v1.0")


def test_refused_missing_version(tmp_path):
    refused(tmp_path, small_index(), "Unable to load memory-mapped file with version = not found", version=None)


def test_refused_neighbour_id_out_of_range(tmp_path):
    ix = small_index()
    ix.l0[3] = np.array([1, 8], dtype=np.uint32)
    refused(tmp_path, ix, "node 3, level 0: neighbour id 8 is not below num_node = 8")


def test_refused_upper_level_neighbour_id_out_of_range(tmp_path):
    ix = small_index()
    ix.l1[(0, 1)] = np.array([9], dtype=np.uint32)
    refused(tmp_path, ix, "node 0, level 1: neighbour id 9 is not below num_node = 8")


def test_refused_degree_above_maxM0(tmp_path):
    def patch(parts):
        parts["buf"][0:4] = (5).to_bytes(4, "little")
    refused(tmp_path, small_index(), "node 0, level 0: degree 5 is above maxM0 = 4", patch=patch)


def test_refused_degree_above_maxM(tmp_path):
    def patch(parts):
        parts["l1"][2, 0, 0] = 3
    refused(tmp_path, small_index(), "node 2, level 1: degree 3 is above maxM = 2", patch=patch)


def test_refused_node_listed_twice(tmp_path):
    ix = small_index()
    ix.l0[5] = np.array([2, 4, 2], dtype=np.uint32)
    refused(tmp_path, ix, "node 5, level 0: node 2 is listed twice in one neighbourhood")


def test_refused_init_node_out_of_range(tmp_path):
    def patch(parts):
        parts["init_node"] = 8
    refused(tmp_path, small_index(), "init_node = 8 is not below num_node = 8", patch=patch)


def test_refused_sparse_ids_not_ascending(tmp_path):
    ix = small_index("csr")
    ix.items.indices[0:2] = ix.items.indices[0:2][::-1].copy()
    ix.items.has_sorted_indices = True
    refused(tmp_path, ix, "node 0: a sparse item's ids are not strictly ascending")


def test_refused_sparse_id_reaches_feat_dim(tmp_path):
    ix = small_index("csr")
    ix.items.indices[2] = 10
    refused(tmp_path, ix, "node 0: a sparse item's id 10 reaches feat_dim = 10")


@pytest.mark.parametrize("kind", ["drm", "csr"])
def test_refused_non_finite_stored_value(tmp_path, kind):
    ix = small_index(kind)
    if kind == "drm":
        ix.items[6, 1] = np.inf
    else:
        ix.items.data[ix.items.indptr[6]] = np.nan
    refused(tmp_path, ix, "node 6: a stored value is not finite")


def test_refused_sparse_records_that_leave_the_buffer(tmp_path):
    """mem_start_of_node is read from the file: past the buffer, near 2^64 (a sum with it would wrap), going down, a record too short for its
    neighbourhood, and an item whose length reaches past its record."""
    def start_at(i, value):
        def patch(parts):
            parts["start"] = parts["start"].copy()
            parts["start"][i] = value
        return patch
    ix = small_index("csr")
    size = int(hr.node_records(ix)[0][-1])
    refused(tmp_path, ix, "node 2: its record leaves the buffer", patch=start_at(3, size + 4))
    refused(tmp_path, ix, "node 2: its record leaves the buffer", patch=start_at(3, 2 ** 64 - 8))
    refused(tmp_path, ix, "node 0: its record leaves the buffer", patch=start_at(0, 2 ** 64 - 8))        # at + its neighbourhood would wrap to a small sum
    refused(tmp_path, ix, "node 2: its record leaves the buffer", patch=start_at(3, int(hr.node_records(ix)[0][2]) - 4))
    refused(tmp_path, ix, "node 7: its record leaves the buffer", patch=start_at(8, size + 8))
    refused(tmp_path, ix, "node 2: its record leaves the buffer", patch=start_at(3, int(hr.node_records(ix)[0][2]) + 8))

    def long_item(parts):
        at = int(parts["start"][4]) + 4 * (1 + parts["maxM0"])
        parts["buf"][at:at + 4] = (1000).to_bytes(4, "little")
    refused(tmp_path, ix, "node 4: its sparse item leaves its record", patch=long_item)

    def huge_item(parts):
        at = int(parts["start"][4]) + 4 * (1 + parts["maxM0"])
        parts["buf"][at:at + 4] = (2 ** 32 - 1).to_bytes(4, "little")
    refused(tmp_path, ix, "node 4: its sparse item leaves its record", patch=huge_item)


def test_refused_dense_records_of_another_size(tmp_path):
    def patch(parts):
        parts["node_mem"] += 4
    refused(tmp_path, small_index("drm"), "the dense node records do not have the size of maxM0 and feat_dim", patch=patch)

    def short(parts):
        parts["buf"] = parts["buf"][:-4]
    refused(tmp_path, small_index("drm"), "the dense node records do not have the size of maxM0 and feat_dim", patch=short)


def test_refused_missing_folder(tmp_path):
    info, err = hr.check_folder(str(tmp_path / "nothing"))
    assert "Unable to open config file at " in err


def test_null_handles_are_refused_by_name():
    lib = hr.ours()
    X = np.zeros((1, 4), dtype=np.float32)
    idx, dist = np.full((1, 3), 7, np.uint32), np.full((1, 3), -1.0, np.float32)
    view = hr.DrmView(1, 4, X.ctypes.data)
    assert lib.xrl_hnsw_predict_drm_f32(None, ctypes.byref(view), idx.ctypes.data, dist.ctypes.data, 10, 3, 1, None) == -1
    assert hr.last_error(lib) == "xrl_hnsw_predict_drm_f32: null index handle"
    assert (idx == 7).all() and (dist == -1.0).all()
    assert lib.xrl_hnsw_searchers_create(None, 2) is None and "null index handle" in hr.last_error(lib)
    assert lib.xrl_hnsw_info(None, None, 0) == -1 and "null index handle" in hr.last_error(lib)
    lib.xrl_hnsw_destruct(None)
    lib.xrl_hnsw_searchers_destruct(None)


def test_caps_are_reported():
    c = hr.caps()
    assert c["CAP"] >= 64 and c["cand_cap"] >= 64 and 8 * (c["CAP"] + 1) <= 160 * 1024


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_surface_and_its_messages(tmp_path):
    import pecos_amd
    from pecos_amd import HNSW
    assert HNSW.PredParams().to_dict() == {"efS": 100, "topk": 10, "threads": 1}
    assert HNSW.TrainParams().to_dict() == {"M": 32, "efC": 100, "threads": -1, "max_level_upper_bound": -1, "metric_type": "ip"}
    assert HNSW.PredParams.from_dict({"efS": 7, "__meta__": {}}).efS == 7
    with pytest.raises(NotImplementedError, match="HNSW.train"):
        HNSW.train(np.zeros((2, 2), dtype=np.float32))
    with pytest.raises(NotImplementedError, match="HNSW.save"):
        HNSW(None, 1, 1, "drm", "ip").save(str(tmp_path))
    with pytest.raises(NotImplementedError, match="PairwiseANN"):
        pecos_amd.PairwiseANN.train(None, None)
    with pytest.raises(NotImplementedError, match="product-quantised"):
        pecos_amd.HNSWProductQuantizer4Bits.load(str(tmp_path))
    folder = hr.write_folder(small_index(), str(tmp_path / "m"))
    param = json.load(open(os.path.join(folder, "param.json")))
    json.dump(dict(param, model="Other"), open(os.path.join(folder, "param.json"), "w"))
    with pytest.raises(ValueError, match="param\\[model\\] != cls.__name__"):
        HNSW.load(folder)
    json.dump({k: v for k, v in param.items() if k != "metric_type"}, open(os.path.join(folder, "param.json"), "w"))
    with pytest.raises(ValueError, match="param.json did not have data_type or metric_type!"):
        HNSW.load(folder)
    json.dump(param, open(os.path.join(folder, "param.json"), "w"))
    os.rename(os.path.join(folder, "c_model"), os.path.join(folder, "elsewhere"))
    with pytest.raises(ValueError, match="c_model_dir did not exist"):
        HNSW.load(folder)
    m = HNSW(None, 8, 4, "drm", "ip", {"efS": 5, "topk": 2, "threads": 1})
    assert (m.data_type, m.metric_type, m.get_pred_params().efS) == ("drm", "ip", 5)
    with pytest.raises(ValueError, match="data_type=csr is NOT consistent with self.data_type=drm"):
        m.predict(smat.csr_matrix(np.ones((1, 4), dtype=np.float32)))
    with pytest.raises(ValueError, match="pX.cols=3 is NOT consistent with self.feat_dim=4"):
        m.predict(np.ones((1, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="type\\(X\\)=.* is NOT supported!"):
        m.predict([[1.0]])
    with pytest.raises(ValueError, match="self.model_ptr must exist"):
        m.searchers_create(1)


def test_bad_folder_through_the_python_class(tmp_path):
    from pecos_amd import HNSW
    ix = small_index()
    ix.l0[5] = np.array([2, 4, 2], dtype=np.uint32)
    folder = hr.write_folder(ix, str(tmp_path / "m"))
    with pytest.raises(RuntimeError, match="listed twice in one neighbourhood"):
        HNSW.load(folder)
