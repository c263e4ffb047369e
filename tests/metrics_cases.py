"""What the metrics tests (test_metrics_cpu.py, test_gpu_metrics.py), the fixture generator (golden/make_golden_metrics.py) and
scripts/metrics_probe.py share: a numpy statement of what K8 (xrl_metrics_device) computes, and the seeded case generators.

THE RULE (smat_util.Metrics.generate, pecos/utils/smat_util.py:968-997, stated on the fixed-stride form).  Per row, the T = min(count, stride)
entries are ordered by value descending -- -0.0 tied with +0.0, every NaN last -- and ties by label ascending; the stored order does not
matter.  matched[p] = the label of rank p occurs in the true row; cum[p] = matched entries of rank <= p for p < topk, positions past the
row carrying cum[T-1]; a row with T == 0 adds nothing.  Sums over the rows: matched_sum[p] += cum[p] (integers) and recall_sum[p] +=
float64(cum[p]) / float64(max(n_true, 1)), n_true the true row's stored length.  The fp64 sum runs in BLOCKS: with R(rows) =
64 * max(1, ceil(rows / 262144)), block w = rows [w R, (w+1) R) is added in ascending row order from 0.0, then the blocks in ascending w from
0.0.  For rows <= R that is the reference's own row-order sum.

A case is a dict: idx u32 [rows, stride], val f32 [rows, stride], cnt u32 [rows] (entries past the count are filler with teeth: a TRUE label
of the row with score +inf), tptr u64 [rows + 1], tidx u32 (ascending inside rows), topk, n_cols."""
import functools
import os

import numpy as np
import scipy.sparse as smat

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics")
f32 = np.float32
TOP = 0xFFFFFFFE                 # the largest label id a uint32 CSR with 2^32 - 1 columns can hold
NEG_NAN = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
TRUE_LENGTHS = (0, 1, 2, 63, 64, 65, 1000)


def rows_per_block(rows):
    return 64 * max(1, -(-int(rows) // 262144))


def recall_bound(rows):
    """|recall - reference's recall| when the blocks differ from the row order: both sides add at most `rows` non-negative fp64 terms of at
    most 1, each side's error at most (rows - 1) 2^-53 of the sum (<= rows), then one division by rows: (2 rows + 2) 2^-53 absolute."""
    return (2 * int(rows) + 2) * 2.0 ** -53


# ------------------------------------------------------------------------------------------------------------------ the restatement
def ranked_matches(case):
    """bool [rows, stride]: entry of RANK p of every row matches (False past the row)."""
    idx, val, cnt = case["idx"], case["val"], case["cnt"]
    rows, stride = idx.shape
    T = np.minimum(cnt.astype(np.int64), stride)
    live = np.arange(stride)[None, :] < T[:, None]
    nan = np.isnan(val)
    neg = np.where(nan, f32(0), -val)                                    # (-0.0 == +0.0 under the sort's comparison)
    row = np.repeat(np.arange(rows, dtype=np.int64), stride)
    order = np.lexsort((idx.ravel(), neg.ravel(), nan.ravel(), ~live.ravel(), row))       # last key first: row, live, NaN last, value, label
    lab = idx.ravel()[order].reshape(rows, stride)
    tptr = case["tptr"].astype(np.int64)
    trow = np.repeat(np.arange(rows, dtype=np.uint64), np.diff(tptr))
    tkey = (trow << np.uint64(32)) | case["tidx"][tptr[0]:tptr[-1]].astype(np.uint64)
    pkey = (np.arange(rows, dtype=np.uint64)[:, None] << np.uint64(32)) | lab.astype(np.uint64)
    return np.isin(pkey, tkey) & live                                    # (sorted rows: the live entries are the first T)


def cum_matched(case, topk=None):
    """uint64 [rows, topk]: cum[p] of every row, carried past the row's end (all zero for a row without entries)."""
    topk = int(case["topk"] if topk is None else topk)
    m = ranked_matches(case)
    stride = m.shape[1]
    cum = np.cumsum(m, axis=1, dtype=np.uint64)
    if topk <= stride:
        return cum[:, :topk]
    return np.concatenate([cum, np.repeat(cum[:, -1:], topk - stride, axis=1)], axis=1)


def metric_sums(case, topk=None, block=None):
    """(matched uint64 [topk], recall_sum float64 [topk]) in the blocked order; block = rows per block (default R(rows); `rows` or more: the
    reference's row order)."""
    cum = cum_matched(case, topk)
    rows, topk = cum.shape
    n_true = np.maximum(np.diff(case["tptr"].astype(np.int64)), 1)
    q = cum.astype(np.float64) / n_true.astype(np.float64)[:, None]
    R = int(block or rows_per_block(rows))
    nb = -(-rows // R) if rows else 0
    pad = np.zeros((nb * R, topk))
    pad[:rows] = q                                                       # (+0.0 terms leave a non-negative sum as it is)
    pad = pad.reshape(nb, R, topk)
    part = np.zeros((nb, topk))
    for r in range(min(R, rows)):                                        # row order inside every block ...
        part += pad[:, r, :]
    total = np.zeros(topk)
    for w in range(nb):                                                  # ... then the blocks in order
        total += part[w]
    return cum.sum(axis=0, dtype=np.uint64), total


def metric_sums_by_row(case, topk=None):
    """The same sums by the definition, one row at a time in row order (the reference's order): the check of the vectorised form above."""
    topk = int(case["topk"] if topk is None else topk)
    idx, val, cnt, tptr, tidx = case["idx"], case["val"], case["cnt"], case["tptr"], case["tidx"]
    matched, recall = np.zeros(topk, dtype=np.uint64), np.zeros(topk, dtype=np.float64)
    for r in range(idx.shape[0]):
        T = min(int(cnt[r]), idx.shape[1])
        if T == 0:
            continue
        lab, v = idx[r, :T], val[r, :T]
        nan = np.isnan(v)
        order = np.lexsort((lab, np.where(nan, f32(0), -v), nan))
        truth = tidx[int(tptr[r]):int(tptr[r + 1])]
        cum = np.cumsum(np.isin(lab[order][:topk], truth), dtype=np.uint64)
        cum = np.concatenate([cum, np.full(topk - len(cum), cum[-1], dtype=np.uint64)])
        matched += cum
        recall += cum.astype(np.float64) / float(max(len(truth), 1))
    return matched, recall


def from_sums(matched, recall_sum, rows):
    """(prec, recall) by the reference's last two lines."""
    return matched.astype(np.uint64) / int(rows) / np.arange(1, len(matched) + 1), recall_sum / int(rows)


# ------------------------------------------------------------------------------------------------------------------ CSR forms for the host
def pred_csr(case, n_cols=None):
    """The result as scipy CSR with exactly the stored entries in the stored order (explicit zeros kept), labels as they are."""
    idx, val, cnt = case["idx"], case["val"], case["cnt"]
    rows, stride = idx.shape
    T = np.minimum(cnt.astype(np.int64), stride)
    mask = np.arange(stride)[None, :] < T[:, None]
    m = smat.csr_matrix((rows, int(n_cols or case["n_cols"])), dtype=np.float32)
    m.indptr, m.indices, m.data = np.concatenate([[0], np.cumsum(T)]).astype(np.int64), idx[mask].astype(np.int64), val[mask].astype(np.float32)
    return m


def true_csr(case, n_cols=None):
    rows = case["idx"].shape[0]
    tptr = case["tptr"].astype(np.int64)
    m = smat.csr_matrix((rows, int(n_cols or case["n_cols"])), dtype=np.float32)
    m.indptr, m.indices = tptr - tptr[0], case["tidx"][tptr[0]:tptr[-1]].astype(np.int64)
    m.data = np.ones(len(m.indices), dtype=np.float32)
    return m


# ------------------------------------------------------------------------------------------------------------------ the generators
def _finish(rows, stride, topk, n_cols, pred, truth):
    """pred: per row (labels, scores, stored count); truth: per row an ascending label array."""
    idx = np.zeros((rows, stride), np.uint32); val = np.zeros((rows, stride), np.float32); cnt = np.zeros(rows, np.uint32)
    for r, (lab, sc, c) in enumerate(pred):
        n = len(lab)
        assert n <= stride and len(set(int(x) for x in lab)) == n and (c == n or (n == stride and c > n)), (r, n, c)
        idx[r, :n], val[r, :n], cnt[r] = lab, sc, c
        t = truth[r]
        idx[r, n:] = t[len(t) // 2] if len(t) else 7                     # filler with teeth: a true label, best score
        val[r, n:] = np.inf
    for t in truth:
        assert np.all(np.diff(t.astype(np.int64)) >= 0)
    tptr = np.concatenate([[0], np.cumsum([len(t) for t in truth])]).astype(np.uint64)
    tidx = np.concatenate([t for t in truth] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return dict(idx=idx, val=val, cnt=cnt, tptr=tptr, tidx=tidx, topk=int(topk), n_cols=int(n_cols))


def _scores(rng, n, special):
    """Integer-valued scores from a small range (ties are the rule), exact zeros of both signs; `special`: NaNs of both signs and +-inf too."""
    v = rng.integers(-2, 4, size=n).astype(np.float32)
    v[(v == 0) & (rng.random(n) < 0.5)] = f32(-0.0)
    if special and n:
        for x in (np.nan, NEG_NAN, np.inf, -np.inf):
            v[rng.integers(0, n, size=max(1, n // 16))] = x
    return v


def random_case(rows, stride, topk, seed, wide=False):
    """Seeded rows: counts 0 .. stride and above it, 0 in the first, a middle and the last row; stored order random in odd rows, best first by
    position (predict's) in even rows; true rows of the TRUE_LENGTHS in turn, sharing labels with the row's predictions."""
    rng = np.random.default_rng(seed)
    n_pool = 3 * stride + 1100
    if wide:
        pool = np.unique(np.concatenate([[0, TOP], rng.integers(1, TOP, size=n_pool + 8, dtype=np.int64)]))[:n_pool].astype(np.int64)
        pool[-1] = TOP
        n_cols = 0xFFFFFFFF
    else:
        pool, n_cols = np.arange(n_pool, dtype=np.int64), n_pool
    pred, truth = [], []
    for r in range(rows):
        if rows >= 3 and r in (0, rows // 2, rows - 1):
            n, c = 0, 0
        else:
            n = int(rng.integers(0, stride + 1)) if r % 3 else stride
            c = n + int(rng.integers(1, 4)) if (n == stride and r % 2) else n          # counts above the stride
        lab = rng.choice(pool, size=n, replace=False)
        sc = _scores(rng, n, special=(r % 4 == 1))
        if r % 2 == 0 and n:
            o = np.argsort(-np.where(np.isnan(sc), -np.inf, sc), kind="stable")
            lab, sc = lab[o], sc[o]
        L = TRUE_LENGTHS[r % len(TRUE_LENGTHS)]
        own = lab[rng.random(n) < 0.4][:L]
        rest = rng.choice(pool, size=L, replace=False)
        t = np.sort(np.concatenate([own, rest])[:L])                     # (a label drawn twice stays twice: len(truth) counts it)
        pred.append((lab, sc, c)); truth.append(t.astype(np.uint32))
    return _finish(rows, stride, topk, n_cols, pred, truth)


def order_case():
    """Hand-written rows on which the order decides.  topk = 1 sees only the best entry."""
    nan, inf = f32(np.nan), f32(np.inf)
    u = lambda *a: np.array(a, dtype=np.uint32)                                          # noqa: E731
    v = lambda *a: np.array(a, dtype=np.float32)                                         # noqa: E731
    pred = [
        (u(9, 3), v(1, 1), 2),                         # tie: label order puts the matching 3 first, the stored order the 9
        (u(9, 3), v(1, 1), 2),                         # the converse: the matching 9 leads only in the stored order
        (u(4, 8, 6), v(nan, 2, NEG_NAN), 3),           # NaNs of both signs go last, 6 after 4
        (u(5, 2), v(-0.0, 0.0), 2),                    # -0.0 ties with +0.0: label 2 leads
        (u(1, 2, 3, 4), v(-inf, inf, nan, 0), 4),      # +inf first, then 0, -inf, NaN
        (u(7, 5), v(0, 0), 2),                         # exact zeros are entries
        (u(2, 1), v(3, 5), 2),                         # a row stored worst first
    ]
    truth = [u(3), u(9), u(6), u(2), u(3, 4), u(5, 7), u(1)]
    return _finish(len(pred), 4, 1, 16, pred, truth)


def order_case_topk4():
    c = dict(order_case())
    c["topk"] = 4
    return c


def edges_case():
    """The binary search at its edges: true rows of every TRUE_LENGTH; predicted labels equal to the first and the last true label, just outside
    both, inside, and the ids 0 and 2^32 - 2."""
    rng = np.random.default_rng(77)
    pred, truth = [], []
    for k, L in enumerate(TRUE_LENGTHS + (1000, 2)):
        if k == len(TRUE_LENGTHS):                     # a true row that itself starts at 0 and ends at 2^32 - 2
            t = np.unique(np.concatenate([[0, TOP], rng.integers(1, TOP, size=L, dtype=np.int64)]))
        elif k == len(TRUE_LENGTHS) + 1:               # a label twice in the true row: n_true counts both
            t = np.array([40, 40], dtype=np.int64)
        else:
            t = np.unique(rng.integers(100, TOP - 100, size=4 * L + 4, dtype=np.int64))[: L]
            t = np.sort(rng.permutation(t))
        assert len(t) >= L
        want = [0, TOP]
        if len(t):
            mid = int(t[len(t) // 2])
            want += [int(t[0]), int(t[-1]), int(t[0]) - 1, int(t[-1]) + 1, mid, mid + 1, mid - 1]
        lab = np.array(sorted({x for x in want if 0 <= x <= TOP}), dtype=np.int64)
        lab = rng.permutation(lab)
        sc = np.linspace(1, 2, len(lab)).astype(np.float32)              # distinct scores: every position of cum is pinned
        pred.append((lab, sc, len(lab))); truth.append(t.astype(np.uint32))
    return _finish(len(pred), 10, 10, 0xFFFFFFFF, pred, truth)


def big_case(rows=262145, seed=5):
    """More rows than 262144 (R becomes 128) at stride 2, built without a python loop: labels from 0 .. 7, scores from {0, 1} (ties), counts
    0 .. 3, true rows of 0 .. 3 labels from 0 .. 7."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 8, size=rows)
    idx = np.stack([a, (a + rng.integers(1, 8, size=rows)) % 8], axis=1).astype(np.uint32)
    val = rng.integers(0, 2, size=(rows, 2)).astype(np.float32)
    cnt = rng.integers(0, 4, size=rows).astype(np.uint32)
    cnt[[0, rows // 2, rows - 1]] = 0
    n_true = rng.integers(0, 4, size=rows)
    tptr = np.concatenate([[0], np.cumsum(n_true)]).astype(np.uint64)
    first = rng.integers(0, 5, size=rows)
    tidx = (np.repeat(first, n_true) + (np.arange(int(tptr[-1])) - np.repeat(tptr[:-1].astype(np.int64), n_true))).astype(np.uint32)
    return dict(idx=idx, val=val, cnt=cnt, tptr=tptr, tidx=tidx, topk=3, n_cols=8)


# name -> (maker, arguments).  rows 1 / 63 / 64 / 65 / 129 = the partial boundaries at R = 64; strides and topk on both sides of 64-entry slots,
# topk below, at and above the stride (the carry)
CASES = {
    "order": (order_case, ()),
    "order4": (order_case_topk4, ()),
    "edges": (edges_case, ()),
    "r1_s1_k1": (random_case, (1, 1, 1, 11)),
    "r63_s10_k10": (random_case, (63, 10, 10, 12)),
    "r64_s10_k63": (random_case, (64, 10, 63, 13)),
    "r65_s63_k64": (random_case, (65, 63, 64, 14)),
    "r129_s10_k10": (random_case, (129, 10, 10, 15)),
    "r129_s64_k65": (random_case, (129, 64, 65, 16)),
    "r65_s65_k10": (random_case, (65, 65, 10, 17)),
    "r64_s128_k1": (random_case, (64, 128, 1, 18)),
    "r5_s1024_k1024": (random_case, (5, 1024, 1024, 19)),
    "r65_s1_k1024": (random_case, (65, 1, 1024, 20)),
    "r9_s1024_k63_wide": (random_case, (9, 1024, 63, 21, True)),
    "r129_s65_k64_wide": (random_case, (129, 65, 64, 22, True)),
}
# the cases recorded under tests/golden/metrics/ with the reference's prec / recall
GOLDEN = ("order", "order4", "edges", "r1_s1_k1", "r63_s10_k10", "r64_s10_k63", "r65_s63_k64", "r129_s10_k10", "r129_s64_k65", "r5_s1024_k1024",
          "r129_s65_k64_wide")


@functools.lru_cache(maxsize=None)
def case(name):
    maker, args = CASES[name]
    c = maker(*args)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)                                      # shared among tests: left unchanged
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    return metric_sums(case(name))


def golden(name):
    """The recorded fixture: (case, prec, recall) -- the inputs as stored, the reference's outputs."""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    c = dict(idx=z["idx"], val=z["val"], cnt=z["cnt"], tptr=z["tptr"], tidx=z["tidx"], topk=int(z["topk"]), n_cols=int(z["n_cols"]))
    return c, z["prec"], z["recall"]


def same_inputs(a, b):
    return all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k], b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k])
               for k in ("idx", "val", "cnt", "tptr", "tidx")) and a["topk"] == b["topk"]
