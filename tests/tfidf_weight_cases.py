"""TEST INFRASTRUCTURE for the tf-idf weighting (K5, tfidf_weight_kernel in pecos_amd/csrc/xrl_features.hip; the host form in
xrl_tfidf_abi.cpp; the numpy mirror pecos_amd.features.tfidf_weight; oracle/tfidf_oracle.py): case generators only, shared by the CPU half
(tests/test_tfidf_weight_cpu.py) and the GPU half (tests/test_gpu_tfidf_weight.py).  Every generator states what it assumes on the
REFERENCE side alone -- in numpy float32 / float64, never from the code under test -- and asserts it.

Text cases are vectorizer folders in the reference's file format (tests/tfidf_cases.py::write_base / write_ensemble; word tokenizer, unigram
features, token i of base b = feature i of base b) with documents that are " ".join of every word repeated its count: the term counts are
chosen exactly.  Raw cases are count CSRs for xrl_queries_tfidf_device, holding values no text can produce.
"""
import collections
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import scipy.sparse as smat

import tfidf_cases as tc

F32 = np.float32
F64 = np.float64
EPS = F32(np.finfo(F32).eps)                       # FLT_EPSILON, 2^-23
TINY_IDF = 2.0 ** -40                              # count_sweep's idf: a power of two, so tf x idf is exact and every row's norm stays below EPS
REF_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "oracle", "_ref"))
REFPY = os.path.join(REF_ROOT, "refpy")


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def below(x):
    return np.nextafter(F32(x), F32(0))


def tf_double_log(c):
    """tfidf.hpp:801 as the reference's translation unit computes it: the DOUBLE log of <cmath>, the add in fp64, one rounding to fp32."""
    return (np.log(np.asarray(c, dtype=F32).astype(F64)) + 1.0).astype(F32)


def tf_float_log(c):
    """The form this project computed before: logf, widened, + 1.0, rounded."""
    return (np.log(np.asarray(c, dtype=F32)).astype(F64) + 1.0).astype(F32)


def seq_sum(terms):
    """The reference's denominator: float32, accumulated in stored order (np.add.accumulate is strictly sequential)."""
    terms = np.asarray(terms, dtype=F32)
    return F32(np.add.accumulate(terms, dtype=F32)[-1]) if len(terms) else F32(0)


def norm_terms(v, norm):
    v = np.asarray(v, dtype=F32)
    return np.abs(v) if norm == "l1" else (v * v).astype(F32)


def same_values(got, want, what=""):
    """Bit equality where the expected value is a number, NaN-ness where it is NaN."""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN at other places"
    bad = np.flatnonzero((bits(got) != bits(want)) & ~nan)
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} values differ, first at {bad[:5].tolist()}: {got[bad[:5]]!r} != {want[bad[:5]]!r}"


# ----------------------------------------------------------------------------------------------------------------------------- text cases
BaseSpec = collections.namedtuple("BaseSpec", "idf binary use_idf sublinear_tf norm")        # idf: float32 [features of this base]


def _word(b, i):
    return f"{'abcdefgh'[b]}{i:x}"


class TextCase:
    """docs[r] holds count rows[r][b][j][1] of word rows[r][b][j][0] of base b.  ens_norm None: a plain base folder (no meta.json)."""

    def __init__(self, name, bases, ens_norm, rows):
        self.name, self.bases, self.ens_norm = name, list(bases), ens_norm
        assert ens_norm is not None or len(self.bases) == 1
        self.offsets = np.concatenate([[0], np.cumsum([len(B.idf) for B in self.bases])]).astype(np.int64)
        self.nr_features = int(self.offsets[-1])
        indptr, idx, val, docs = [0], [], [], []
        for row in rows:
            assert len(row) == len(self.bases)
            words = []
            for b, seg in enumerate(row):
                assert [f for f, _ in seg] == sorted({f for f, _ in seg}) and all(0 <= f < len(self.bases[b].idf) and c >= 1 for f, c in seg)
                idx += [int(self.offsets[b]) + f for f, _ in seg]
                val += [c for _, c in seg]
                words += [_word(b, f) for f, c in seg for _ in range(c)]
            indptr.append(len(idx))
            docs.append(" ".join(words))
        self.docs = docs
        self.counts = smat.csr_matrix((np.asarray(val, dtype=F32), np.asarray(idx, dtype=np.int64), np.asarray(indptr, dtype=np.int64)),
                                      shape=(len(rows), self.nr_features))

    def write(self, folder):
        args = []
        for b, B in enumerate(self.bases):
            n = len(B.idf)
            args.append(dict(tok_type=10, vocab=[(i, _word(b, i).encode()) for i in range(n)], features=[(i, float(B.idf[i]), (i,)) for i in range(n)],
                             binary=B.binary, use_idf=B.use_idf, sublinear_tf=B.sublinear_tf, norm_p=B.norm))
        if self.ens_norm is None:
            return tc.write_base(folder, **args[0])
        return tc.write_ensemble(folder, args, norm_p=self.ens_norm)

    def weigh(self, weight):
        """X by `weight` (the signature of pecos_amd.features.tfidf_weight): every base's segment with its parameters, then -- an ensemble of
        several bases, or of one whose norm differs (tfidf.hpp:1405-1430) -- the whole rows once more with no weighting."""
        C = self.counts
        out = np.zeros(C.nnz, dtype=F32)
        for b, B in enumerate(self.bases):
            lo, hi = self.offsets[b], self.offsets[b + 1]
            m = (C.indices >= lo) & (C.indices < hi)
            ptr = np.concatenate([[0], np.cumsum(m)])[C.indptr]
            seg = smat.csr_matrix((C.data[m], C.indices[m] - lo, ptr), shape=(C.shape[0], hi - lo))
            out[m] = weight(seg, idf=B.idf if B.use_idf else None, binary=B.binary, sublinear_tf=B.sublinear_tf, norm=B.norm).data
        X = smat.csr_matrix((out, C.indices.copy(), C.indptr.copy()), shape=C.shape)
        if self.ens_norm is not None and (len(self.bases) > 1 or {1: "l1", 2: "l2"}[self.ens_norm] != self.bases[0].norm):
            X = weight(X, norm={1: "l1", 2: "l2"}[self.ens_norm])
        return X


_cache = {}


def _cached(fn):
    def get():
        if fn.__name__ not in _cache:
            _cache[fn.__name__] = fn()
        return _cache[fn.__name__]
    get.__name__ = fn.__name__
    get.__doc__ = fn.__doc__
    return get


SWEEP_ROW = 193


@_cached
def count_sweep():
    """Every count 1 .. 512 and three dozen larger ones (<= 20 000) at which the two log forms give other fp32 bits, 193 to a document, under
    sublinear_tf with every idf = 2^-40 and both norms.  Preconditions: at least 10 of the counts tell the forms apart; every row's l1 (hence
    l2) sum stays below FLT_EPSILON, so the denominator is 1 and the expected X is tf x 2^-40 exactly -- the transform shows bit for bit.
    Returns ([TextCase l1, TextCase l2], counts in stored order, the counts that tell the forms apart)."""
    cand = np.arange(1, 20001)
    differ = cand[bits(tf_double_log(cand)) != bits(tf_float_log(cand))]
    assert (differ <= 512).sum() >= 10, differ[:20]
    big = differ[differ > 512]
    counts = np.concatenate([np.arange(1, 513), big[:: max(1, len(big) // 36)][:36]])
    telling = np.intersect1d(counts, differ)
    assert len(telling) >= 10 + 24
    rows = [[[(j, int(c)) for j, c in enumerate(counts[a:a + SWEEP_ROW])]] for a in range(0, len(counts), SWEEP_ROW)]
    idf = np.full(SWEEP_ROW, TINY_IDF, dtype=F32)
    assert float(idf[0]) == TINY_IDF and repr(float(idf[0])) == repr(TINY_IDF)
    for row in rows:
        l1 = float(np.sum(tf_double_log([c for _, c in row[0]]).astype(F64))) * TINY_IDF
        assert l1 * (1 + 1e-3) < float(EPS), l1
    cases = [TextCase(f"count_sweep_{norm}", [BaseSpec(idf, False, True, True, norm)], None, rows) for norm in ("l1", "l2")]
    return cases, counts, telling


def sweep_expected(counts):
    return (tf_double_log(counts) * F32(TINY_IDF)).astype(F32)


LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1025)
ROW_FEATURES = 1025
CONFIGS = [dict(norm=n, binary=b, sublinear_tf=s, use_idf=u) for n in ("l1", "l2") for b in (False, True) for s in (False, True) for u in (True, False)]


def order_sensitive(v, norm):
    """Whether the reference's sequential fp32 denominator gives output bits that neither numpy's pairwise fp32 sum nor the fp64 sum rounded
    once gives: a kernel that reduces by a tree, or per 64-entry step, fails on such a row."""
    t = norm_terms(v, norm)
    outs = []
    for d in (seq_sum(t), F32(np.sum(t, dtype=F32)), F32(np.sum(t.astype(F64)))):
        d = F32(np.sqrt(d)) if norm == "l2" else d
        outs.append(bits((np.asarray(v, dtype=F32) / d).astype(F32)))
    return bool(np.any(outs[0] != outs[1]) and np.any(outs[0] != outs[2]))


@_cached
def row_lengths():
    """One document of every length in LENGTHS (entries = distinct features out of 1025, idf spread over 1e-3 .. 1e3, counts 1 .. 60), under every
    combination of norm x binary x sublinear_tf x use_idf.  Precondition: every row of 65 entries or more is order-sensitive under the plain
    idf weighting with either norm (seeds are searched until it is).  Returns [(config, TextCase)]; all cases share documents and counts."""
    rng = np.random.default_rng(7)
    idf = (10.0 ** rng.uniform(-3, 3, ROW_FEATURES)).astype(F32)
    rows = []
    for L in LENGTHS:
        for seed in range(400):
            r = np.random.default_rng(1000 * L + seed)
            cols = np.sort(r.choice(ROW_FEATURES, size=L, replace=False))
            cnt = r.integers(1, 61, size=L)
            v = (cnt.astype(F32) * idf[cols]).astype(F32)
            if L < 65 or (order_sensitive(v, "l1") and order_sensitive(v, "l2")):
                break
        else:
            raise AssertionError(f"no order-sensitive row of {L} entries found")
        rows.append([[(int(f), int(c)) for f, c in zip(cols, cnt)]])
    assert max(c for row in rows for _, c in row[0]) >= 52       # (sublinear_tf meets counts at which the two log forms differ: 28 .. 52)
    return [(cfg, TextCase("rows_" + "_".join(f"{k[0]}{int(v) if isinstance(v, bool) else v}" for k, v in cfg.items()),
                           [BaseSpec(idf, cfg["binary"], cfg["use_idf"], cfg["sublinear_tf"], cfg["norm"])], None, rows)) for cfg in CONFIGS]


SEGMENTS = (0, 1, 63, 64, 65, 129)
SEG_FEATURES = 129


@_cached
def ensembles():
    """nb = 2 and nb = 3 base vectorizers with disjoint vocabularies (one text fills each base's segment independently), per-document segment
    lengths out of SEGMENTS (nb = 2: every pair; nb = 3: (0, 0, 0), the all-equal triples and 40 random ones), so whole rows cross 64 and 128
    elsewhere than their segments; bases: sublinear + l1, binary without idf, plain l2; ensemble norm_p 1 and 2.  And one-base ensembles
    whose norm_p differs from the base's (both ways round) and one where it is the same.  Counts 1 .. 40.  Returns [TextCase]."""
    rng = np.random.default_rng(11)
    idfs = [(10.0 ** rng.uniform(-1, 1, SEG_FEATURES)).astype(F32) for _ in range(3)]
    specs = [BaseSpec(idfs[0], False, True, True, "l1"), BaseSpec(idfs[1], True, False, False, "l2"), BaseSpec(idfs[2], False, True, False, "l2")]

    def segment(n):
        cols = np.sort(rng.choice(SEG_FEATURES, size=n, replace=False))
        return [(int(f), int(c)) for f, c in zip(cols, rng.integers(1, 41, size=n))]

    cases = []
    for nb in (2, 3):
        combos = list(itertools.product(SEGMENTS, repeat=nb))
        if nb == 3:
            pick = rng.choice(len(combos), size=40, replace=False)
            combos = [(n, n, n) for n in SEGMENTS] + [combos[int(i)] for i in pick]
        rows = [[segment(n) for n in combo] for combo in combos]
        lens = np.array([sum(c) for c in combos])
        assert (lens == 0).any() and ((lens > 64) & (lens < 128)).any() and (lens > 128).any()
        for ens in (1, 2):
            cases.append(TextCase(f"ens{nb}_norm{ens}", specs[:nb], ens, rows))
    rows1 = [[segment(n)] for n in SEGMENTS + (SEG_FEATURES - 1,)]
    cases.append(TextCase("ens1_l1_norm2", [specs[0]], 2, rows1))
    cases.append(TextCase("ens1_l2_norm1", [specs[2]], 1, rows1))
    cases.append(TextCase("ens1_l2_norm2", [specs[2]], 2, rows1))
    return cases


# ----------------------------------------------------------------------------------------------------------------------------- raw cases
RawCase = collections.namedtuple("RawCase", "name counts idf binary sublinear_tf norm")      # counts: scipy CSR float32; idf: float32 [cols] or None


def count_csr(rows, cols):
    rows = [sorted(r, key=lambda fc: fc[0]) for r in rows]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.array([f for r in rows for f, _ in r], dtype=np.int64)
    val = np.array([c for r in rows for _, c in r], dtype=F32)
    return smat.csr_matrix((val, idx, indptr), shape=(len(rows), cols))


EPS_COLS, EPS_NEG = 400, 200          # epsilon_edges: idf = +1 for columns below 200, -1 from there on (a product with +-1 is exact)


@_cached
def epsilon_edges():
    """Denominators exactly FLT_EPSILON (kept; l2: the sqrt is taken) and at nextafter below it (replaced by 1), both norms, with negative
    idf (the l1 sum needs its fabs: +a and -a would cancel to 0), rows of 65 entries whose first 64-entry step sums below epsilon while the row
    does not, the same with the large entry FIRST, rows that reach epsilon only through their last entry (64, 65, 128, 129 entries), and
    their neighbours that stay one ulp below.  The values ride in the counts.  Precondition: the sequential fp32 sum of every row, computed
    here, is exactly EPS or exactly nextafter(EPS, 0) as its label says.  Returns ([RawCase l1, RawCase l2], {norm: [label per row]})."""
    e = float(EPS)
    p = lambda k: 2.0 ** k                                                                    # noqa: E731
    l1 = [("kept", [(0, e)]), ("replaced", [(0, below(e))]), ("kept", [(EPS_NEG, e)]), ("replaced", [(EPS_NEG, below(e))]),
          ("kept", [(0, p(-24)), (EPS_NEG, p(-24))]), ("replaced", [(0, p(-24)), (EPS_NEG, p(-24) - p(-47))]),
          ("kept", [(j, p(-30)) for j in range(64)] + [(64, p(-24))]), ("replaced", [(j, p(-30)) for j in range(64)] + [(64, p(-24) - p(-47))]),
          ("kept", [(0, p(-24))] + [(j, p(-30)) for j in range(1, 65)]), ("replaced", [(0, p(-24) - p(-47))] + [(j, p(-30)) for j in range(1, 65)]),
          ("kept", [(j, p(-30)) for j in range(63)] + [(63, 65 * p(-30))]), ("replaced", [(j, p(-30)) for j in range(63)] + [(63, 65 * p(-30) - p(-47))]),
          ("kept", [(j, p(-31)) for j in range(128)] + [(128, p(-24))]), ("replaced", [(j, p(-31)) for j in range(128)] + [(128, p(-24) - p(-47))]),
          ("kept", [(EPS_NEG + j, p(-31)) for j in range(127)] + [(EPS_NEG + 127, p(-24) + p(-31))])]
    # l2: squares.  43 x (2^-15)^2 + 84 x (2^-16)^2 = 2^-24 in 127 entries (n entries whose squares are powers of 4 sum to a power of 4 only for n = 1 mod 3)
    pre127 = [(j, p(-15)) for j in range(43)] + [(j, p(-16)) for j in range(43, 127)]
    l2 = [("kept", [(0, p(-12)), (1, p(-12))]), ("replaced", [(0, p(-12)), (1, below(p(-12)))]),
          ("kept", [(EPS_NEG, p(-12)), (EPS_NEG + 1, p(-12))]), ("replaced", [(0, below(p(-12))), (EPS_NEG, p(-12))]),
          ("kept", [(j, p(-15)) for j in range(64)] + [(64, p(-12))]), ("replaced", [(j, p(-15)) for j in range(64)] + [(64, below(p(-12)))]),
          ("kept", [(0, p(-12))] + [(j, p(-15)) for j in range(1, 65)]), ("replaced", [(0, below(p(-12)))] + [(j, p(-15)) for j in range(1, 65)]),
          ("kept", pre127 + [(127, p(-12))]), ("replaced", pre127 + [(127, below(p(-12)))])]
    idf = np.where(np.arange(EPS_COLS) < EPS_NEG, 1.0, -1.0).astype(F32)
    cases, labels = [], {}
    for norm, rows in (("l1", l1), ("l2", l2)):
        for label, row in rows:
            v = np.array([c for _, c in row], dtype=F32) * idf[[f for f, _ in row]]
            d = seq_sum(norm_terms(v, norm))
            assert d == (EPS if label == "kept" else below(EPS)), (norm, label, len(row), d)
            if len(row) > 64:
                assert seq_sum(norm_terms(v[:64], norm)) < EPS                               # the first 64-entry step alone stays below
        assert any(len(row) == 65 for _, row in rows) and any(len(row) == 128 for _, row in rows)
        cases.append(RawCase(f"eps_{norm}", count_csr([row for _, row in rows], EPS_COLS), idf, False, False, norm))
        labels[norm] = [label for label, _ in rows]
    return cases, labels


FMAX = float(np.finfo(F32).max)
V_IDF = np.array([0.0, -0.0, 1e-42, -1e-42, 1e-25, 1e-30, 0.9 * FMAX, 0.8 * FMAX, np.inf, -np.inf, np.nan, 1.0, 2.5, -3.0, 1e-20, 0.125], dtype=F32)
Z, NZ, SUB, NSUB, T25, T30, BIG, BIG2, INF, NINF, NAN, ONE, TWO5, M3, T20, EIGHTH = range(16)


@_cached
def value_edges():
    """Values no text produces.  idf: +-0 (the sign survives the division), subnormal (the l1 sum stays below epsilon: replaced), products whose
    squares underflow to 0 (l2: replaced) or to subnormals, idf near FLT_MAX (the l2 sum, and an l1 sum of two, overflow to +inf: finite / inf =
    0), +-inf (inf / inf = NaN, the others 0) and NaN (the whole row NaN).  counts: 0 and negative under sublinear_tf (-inf, NaN), non-integer
    counts with and without it, and NaN / negative / 0 / inf counts under binary, which must be ignored.  Preconditions (float32 numpy, here):
    the sums that are said to overflow, underflow or stay below epsilon do.  Returns [RawCase]."""
    idf_rows = [[(Z, 3), (ONE, 2)], [(NZ, 3), (ONE, 2)], [(Z, 1), (NZ, 1)], [(SUB, 5), (NSUB, 3)], [(SUB, 1), (ONE, 1)], [(T25, 1), (T30, 7)],
                [(T25, 1), (T20, 1)], [(T20, 3), (ONE, 2)], [(BIG, 1), (ONE, 1)], [(BIG, 1), (BIG2, 1)], [(BIG, 3), (EIGHTH, 2)], [(INF, 1), (ONE, 2)],
                [(NINF, 2), (ONE, 2), (TWO5, 1)], [(NAN, 1), (ONE, 2)], [(Z, 1), (INF, 1)], [(ONE, 1)], [(TWO5, 7), (M3, 2), (EIGHTH, 60)], []]
    with np.errstate(all="ignore"):
        t = lambda r, norm: norm_terms(np.array([c for _, c in r], dtype=F32) * V_IDF[[f for f, _ in r]], norm)      # noqa: E731
        assert seq_sum(t(idf_rows[3], "l1")) < EPS and seq_sum(t(idf_rows[3], "l1")) > 0                 # subnormal sum
        assert seq_sum(t(idf_rows[5], "l2")) == 0 and seq_sum(t(idf_rows[5], "l1")) > 0                  # squares underflow to 0
        assert 0 < seq_sum(t(idf_rows[6], "l2")) < np.finfo(F32).tiny                                    # ... to a subnormal
        assert np.isinf(seq_sum(t(idf_rows[8], "l2"))) and np.isfinite(seq_sum(t(idf_rows[8], "l1")))    # the l2 sum overflows
        assert np.isinf(seq_sum(t(idf_rows[9], "l1")))                                                   # the l1 sum of two overflows
        assert np.isinf(F32(3) * V_IDF[BIG])                                                             # the product itself overflows
    cnt_rows = [[(ONE, 0.0), (TWO5, 3)], [(ONE, -2.0), (TWO5, 3)], [(ONE, -0.0)], [(ONE, 0.5), (TWO5, 1.5), (M3, 2.75), (EIGHTH, 30000.5)],
                [(ONE, 1e-3), (TWO5, 1e30)], [(ONE, np.inf), (TWO5, 2)], [(ONE, np.nan), (TWO5, 2)], [(ONE, 1e-45), (TWO5, 28)], [(EIGHTH, 28), (T20, 35), (ONE, 16777216)]]
    bin_rows = [[(ONE, np.nan), (TWO5, -5), (M3, 0.0), (EIGHTH, np.inf)], [(ONE, np.nan)], [(j, np.nan if j % 2 else -1.0) for j in (ONE, TWO5, M3, T20, EIGHTH)]]
    cols = len(V_IDF)
    cases = []
    for norm in ("l1", "l2"):
        cases.append(RawCase(f"idf_edges_{norm}", count_csr(idf_rows, cols), V_IDF, False, False, norm))
        cases.append(RawCase(f"count_edges_sublinear_{norm}", count_csr(cnt_rows, cols), V_IDF, False, True, norm))
        cases.append(RawCase(f"count_edges_plain_{norm}", count_csr(cnt_rows, cols), V_IDF, False, False, norm))
        cases.append(RawCase(f"count_edges_sublinear_noidf_{norm}", count_csr(cnt_rows, cols), None, False, True, norm))
        for sub in (False, True):
            cases.append(RawCase(f"binary_nan_sub{int(sub)}_{norm}", count_csr(bin_rows, cols), V_IDF, True, sub, norm))
        cases.append(RawCase(f"binary_nan_noidf_{norm}", count_csr(bin_rows, cols), None, True, False, norm))
    return cases


def raw_of_text(case):
    """A single-base text case as a raw case (its exact counts)."""
    B = case.bases[0]
    return RawCase(case.name, case.counts, B.idf if B.use_idf else None, B.binary, B.sublinear_tf, B.norm)


def mirror(case):
    """pecos_amd.features.tfidf_weight of a raw case (numpy warns about the edge values: silenced)."""
    from pecos_amd.features import tfidf_weight
    with np.errstate(all="ignore"):
        return tfidf_weight(case.counts, idf=case.idf, binary=case.binary, sublinear_tf=case.sublinear_tf, norm=case.norm)


# ----------------------------------------------------------------------------------------------------------------------------- the live reference
def reference_available():
    return os.path.isdir(REFPY) and os.path.exists(os.path.join(REF_ROOT, "libpecos_float32.so"))


def reference_predict(cases, workdir):
    """{case name: (folder, X)}: every case written as a vectorizer folder under workdir and predicted by the reference's own c_tfidf_load +
    c_tfidf_predict (oracle/_ref/refpy; host code only), all in ONE child process."""
    jobs = []
    for case in cases:
        folder = case.write(os.path.join(str(workdir), case.name))
        docs = os.path.join(str(workdir), case.name + ".docs.json")
        with open(docs, "w") as f:
            json.dump(case.docs, f)
        jobs.append({"folder": folder, "docs": docs, "out": os.path.join(str(workdir), case.name + ".ref.npz")})
    job_file = os.path.join(str(workdir), "jobs.json")
    with open(job_file, "w") as f:
        json.dump(jobs, f)
    code = (f"import sys, json, numpy as np; sys.path.insert(0, {REFPY!r})\n"
            "from pecos.utils.featurization.text.vectorizers import Tfidf\n"
            f"for j in json.load(open({job_file!r})):\n"
            "    X = Tfidf.load(j['folder']).predict(json.load(open(j['docs']))).tocsr()\n"
            "    np.savez(j['out'], indptr=X.indptr, indices=X.indices, data=X.data.astype(np.float32), shape=np.asarray(X.shape))\n")
    subprocess.check_call([sys.executable, "-c", code])
    out = {}
    for case, j in zip(cases, jobs):
        z = np.load(j["out"])
        out[case.name] = (j["folder"], smat.csr_matrix((z["data"], z["indices"], z["indptr"]), shape=tuple(int(v) for v in z["shape"])))
    return out


def all_text_cases():
    return count_sweep()[0] + [c for _, c in row_lengths()] + ensembles()
