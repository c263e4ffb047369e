"""What the tests of the ensemble methods (test_ensemble_methods_cpu.py, test_gpu_ensemble_methods.py) and their fixture generator
(golden/make_golden_ensemble_methods.py) share: the fixtures' loader, a plain numpy RESTATEMENT of the rules of
xrl_ensemble_methods_device (include/xrl_abi.h), and the one derivation of the value bounds.

Fixtures: tests/golden/ensemble_methods/<case>.npz (rows with empty segments and an empty row: "sigmoid_average", "round_robin" and the
cuts "<method>_top<k>") and <case>_full.npz (no empty segment, so the reference's softmax runs: "softmax_average").  Array layout as
tests/ensemble_cases.py; inputs are stored in sorted_csr order (score descending, NaN last, ties by ascending label); `exp_ulp` is the
largest distance, in fp32 ulps, between numpy's float32 exp and the float64 exp rounded to fp32 over every exponent argument of the file.

THE BOUNDS.  u = 2^-24 (half an ulp, relative).  Two implementations differ only in their exponentials, by at most E ulps = 2Eu relative
each, and in the order of the softmax denominator's sum.  Every operand below is >= 0, so nothing cancels, and a difference of two
COMPUTED values is at most the difference of the exact ones plus one half-ulp per side and operation.  First order, relative:
  sigmoid   t = 1 + e:   2Eu (e / (1 + e) <= 1) + 2u;   s = 1 / t:   + 2u                                    -> (2E + 4) u per term
  softmax   e_j: 2Eu.  denominator D = sum of n terms: 2Eu + `den` u, where den = (n - 1) + 1 when one side adds in fp32 in an order of its
            own (numpy's sum: at most n - 1 half-ulps) and the other rounds an fp64 sum once, and den = 2 when both round the same fp64
            sum once.  e_j / D: 2Eu + (2E + den) u + 2u                                                       -> (4E + den + 2) u per term
  the sum of M terms in model order: M - 1 additions, 2u each -> + 2 (M - 1) u; that is the bound on a SUM (sum_bound);
  the division by M: + 2u (value_bound).
A factor 1 + 2^-10 covers the second-order terms, and 2^-126 absolute the results below the normal range (where an ulp is absolute).
The GPU tests use E = 1: the device's fp64 exp and libm's differ by at most one fp32 ulp after rounding.  The CPU tests use the
fixture's exp_ulp.  The generator accepts a seed only if any two sums of a row that are not bit-equal differ by more than
4 x sum_bound(max(exp_ulp, 1)) -- at least twice the CPU bound, and enough that the device's order is the reference's too -- so no row
is ever excluded from a comparison."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ensemble_methods")
CASES = ("a", "b", "c", "d", "e")
TOPKS = (1, 3, 100)
CUT_METHODS = ("average", "rank_average", "round_robin")
METHODS = ("average", "rank_average", "sigmoid_average", "softmax_average", "round_robin")
f32 = np.float32
U = 2.0 ** -24


class MCase:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        self.name = name
        self.n_models, self.n_cols, self.exp_ulp = int(z["n_models"]), int(z["n_cols"]), int(z["exp_ulp"])
        self.idx = [z[f"idx{m}"] for m in range(self.n_models)]
        self.val = [z[f"val{m}"] for m in range(self.n_models)]
        self.cnt = [z[f"cnt{m}"] for m in range(self.n_models)]
        self.rows = self.idx[0].shape[0]
        self.out = {k[:-7]: (z[k].astype(np.int64), z[k[:-7] + "_indices"].astype(np.uint32), z[k[:-7] + "_data"]) for k in z.files
                    if k.endswith("_indptr")}

    def expected(self, name):
        """(indptr, labels, values) of a recorded output; the float64 of round_robin cast to fp32 like the device casts it."""
        ip, ix, dv = self.out[name]
        return ip, ix, dv.astype(np.float32)


def exp_f32(x):
    """exp taken in float64 and rounded to fp32."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(np.asarray(x, dtype=np.float32).astype(np.float64)).astype(np.float32)


def segment_lengths(idx, cnt):
    return [np.minimum(c.astype(np.int64), i.shape[1]) for i, c in zip(idx, cnt)]


def softmax_segment(x, first_j):
    """One segment (fp32 scores x, the first at entry first_j of the row's list): the kernel's order of the fp64 sum."""
    with np.errstate(over="ignore", invalid="ignore"):
        x_max = f32(np.nan) if np.isnan(x).any() else x.max()
        e = exp_f32(x - x_max)
        s = [0.0] * 64
        for t, ej in enumerate(e):                                       # a lane adds its entries in ascending j
            s[(first_j + t) % 64] = s[(first_j + t) % 64] + float(ej)
        s = np.array(s, dtype=np.float64)
        for d in (1, 2, 4, 8, 16, 32):                                   # the six exchange steps
            s = s + s[np.arange(64) ^ d]
        return e / f32(s[0])


def _value_order(v):
    """Sort key of an fp32 value under sorted_csr: descending, -0.0 tied with +0.0, NaN last."""
    v = float(v)
    return (1, 0.0) if v != v else (0, -v if v != 0 else 0.0)


def restate(idx, val, cnt, method, only_topk=0):
    """The rules of xrl_ensemble_methods_device on fixed-stride host arrays -> (indptr int64, labels uint32, values float32)."""
    M = len(idx)
    n = segment_lengths(idx, cnt)
    rows = idx[0].shape[0]
    mm = max(int(x.max()) if rows else 0 for x in n)
    base = 1.0 / (M + 1.0)
    indptr, labels, values = [0], [], []
    for r in range(rows):
        merged = {}                                                      # label -> accumulator, in list order = model order
        first_j = 0
        for m in range(M):
            k = int(n[m][r])
            x = val[m][r, :k].astype(np.float32)
            with np.errstate(over="ignore", invalid="ignore"):
                if method == "sigmoid_average":
                    x = f32(1) / (f32(1) + exp_f32(-x))
                elif method == "softmax_average" and k:
                    x = softmax_segment(x, first_j)
                for p in range(k):
                    lab = int(idx[m][r, p])
                    if method == "rank_average":
                        merged[lab] = merged.get(lab, 0) + (mm - p)
                    elif method == "round_robin":
                        rel = float(mm - p) + float(M - m) * base
                        merged[lab] = max(merged.get(lab, rel), rel)
                    else:
                        merged[lab] = f32(merged[lab] + x[p]) if lab in merged else x[p]
            first_j += k
        out = []
        for lab, acc in merged.items():
            if method in ("rank_average", "round_robin"):
                out.append(((0, -float(acc)), lab, f32(float(acc) / float(M))))
            elif not (M >= 2 and acc == 0):                              # an exactly zero sum is not stored (NaN stays)
                with np.errstate(invalid="ignore"):
                    out.append((_value_order(acc), lab, f32(acc / f32(M))))
        if only_topk:
            out = [(_value_order(v), lab, v) for _, lab, v in out]
        out.sort(key=lambda t: (t[0], t[1]))
        if only_topk:
            out = out[:only_topk]
        labels += [t[1] for t in out]
        values += [t[2] for t in out]
        indptr.append(len(labels))
    return np.array(indptr, np.int64), np.array(labels, np.uint32), np.array(values, np.float32)


def per_term(method, E, den):
    return (2 * E + 4) if method == "sigmoid_average" else (4 * E + den + 2)


def sum_bound(method, M, E, den=2):
    """Relative bound on the difference of two computed SUMS (see the header); den: the denominator's term, softmax only."""
    return (per_term(method, E, den) + 2 * (M - 1)) * U * (1 + 2.0 ** -10)


def value_bound(method, M, E, den=2):
    return (per_term(method, E, den) + 2 * (M - 1) + 2) * U * (1 + 2.0 ** -10)


def longest_segment_per_entry(indptr, idx, cnt):
    """For every output entry, the longest segment of its row (the n of the softmax denominator against numpy's fp32 sum)."""
    n = np.max(np.stack(segment_lengths(idx, cnt)), axis=0)
    return np.repeat(n, np.diff(indptr))


def close_rows(got, want, rel, what=""):
    """Row lengths and labels in order identical; NaN where NaN is; values within rel * |want| + 2^-126 (rel: scalar or per entry)."""
    (gp, gi, gv), (wp, wi, wv) = got, want
    assert np.array_equal(gp, wp), f"{what}: row lengths differ"
    assert np.array_equal(gi, wi), f"{what}: labels or their order differ"
    gv, wv = np.asarray(gv, np.float64), np.asarray(wv, np.float64)
    nan = np.isnan(wv)
    assert np.array_equal(np.isnan(gv), nan), f"{what}: NaN positions differ"
    err = np.abs(gv - wv)[~nan]
    lim = (np.broadcast_to(rel, wv.shape)[~nan] * np.abs(wv[~nan])) + 2.0 ** -126
    worst = float((err / lim).max()) if err.size else 0.0
    print(f"{what}: largest error / bound = {worst:.3f} over {err.size} values")
    assert (err <= lim).all(), f"{what}: value beyond the bound ({worst:.2f} x)"
