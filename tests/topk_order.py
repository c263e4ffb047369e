"""The ONE order of the per-query top-k, in numpy, and the rows that tell its forms apart.

Every form of the top-k (k2_topk_wave / _list / _reg / _lds, the segmented sort of xrl_topk_big.hip, the epilogues of K1Q and K1T) ranks a query's
candidate row by (score_key descending, candidate position ascending), score_key being xrl_device.h's map of fp32 bit patterns to unsigned keys:
-0.0 ties with +0.0, a positive NaN ranks above +inf by its payload, a negative NaN below -inf.  Where the reference defines an order (no NaN) this
is the comparator of its sorted_csr; with NaN scores the reference's std::sort is undefined and the order is the library's own.

topk() is the statement the GPU tests hold every form against; SCENARIOS-style rows (scenario_rows) are fp32 score vectors written as BIT PATTERNS,
each with a precondition that is asserted wherever the row is used.  tests/test_topk_order_cpu.py holds topk() against the C restatement and the
compiled reference on the NaN-free rows; tests/test_gpu_topk_forms.py runs the rows through models whose candidate rows ARE these vectors."""
from collections import namedtuple

import numpy as np

POS_NAN, NEG_NAN = 0x7FC00000, 0xFFC00000          # one payload per sign: NaNs of a sign tie, position orders them
POS_INF, NEG_INF = 0x7F800000, 0xFF800000
POS_MAX, NEG_MAX = 0x7F7FFFFF, 0xFF7FFFFF          # +-FLT_MAX
NEG_ZERO = 0x80000000
UNSTORED = None

K_VALUES = (1, 2, 63, 64, 65, 127, 128, 129, 192, 193)
FLAT_L = (1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 832, 833, 1024, 1025, 1536, 1537, 2048, 2049, 2303, 2304, 2305)
BIG_L, BIG_K = 20482, (20480, 20481)
K2_MAX_K = 20480                                     # k2_max_k(): 160 KB of LDS / 8 bytes per entry
WAVE_NS = (1, 2, 4, 8, 13, 16, 24, 32)


def score_key(bits):
    """xrl_device.h score_key on uint32 bit patterns (array or scalar) -> uint32 keys; 0 is never returned (it marks "no candidate")."""
    b = np.asarray(bits, dtype=np.uint32).copy()
    b[b == np.uint32(0x80000000)] = 0
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[k == 0] = 1
    return k


def topk(row_bits, k):
    """(positions, score bits) of the first min(k, n) candidates of a row under (key descending, position ascending)."""
    row = np.asarray(row_bits, dtype=np.uint32)
    key = score_key(row).astype(np.int64)
    order = np.lexsort((np.arange(len(row)), -key))[: min(int(k), len(row))]
    return order.astype(np.int64), row[order]


def candidate_row(weight_bits, stored):
    """What a query with the single entry (f, 1.0) scores against weight row f, `0 + 1 * w` in fp32: the weight's own bits, except that a stored
    -0.0 and an unstored cell both give +0.0 (quiet NaNs keep sign and payload; the CPU tests show the reference's arithmetic does the same)."""
    w = np.where(np.asarray(stored, bool), np.asarray(weight_bits, np.uint32), np.uint32(0)).astype(np.uint32)
    w[w == np.uint32(NEG_ZERO)] = 0
    return w


def is_nan(bits):
    b = np.asarray(bits, np.uint32)
    return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


# ------------------------------------------------------------------------------------------------------------------ the rows
# name; k the row was built around (0: none); weight bits and the stored mask (uint32[n], bool[n]); nan_free / inf_free: dense X may carry the row
# (a one-hot dense query multiplies every OTHER row's weights by 0, harmless only where those are finite); check(cand, k): the precondition
Scenario = namedtuple("Scenario", "name k bits stored nan_free inf_free check")


def _ordinal_bits(o):
    """Odd ordinals ..., -3, -1, 1, 3, ... -> floats one ulp step apart around +-0.5, strictly increasing with the ordinal."""
    o = np.asarray(o, np.int64)
    mag = (np.uint32(0x3F000000) + np.abs(o).astype(np.uint32)).astype(np.uint32)
    return np.where(o < 0, mag | np.uint32(0x80000000), mag).astype(np.uint32)


def _descending(n):
    return _ordinal_bits(2 * (n - 1 - 2 * np.arange(n, dtype=np.int64)) + 1)


def _strict(sign):
    def check(cand, k):
        key = score_key(cand).astype(np.int64)
        assert (np.diff(key) * sign > 0).all(), "the row is not strictly monotonic"
        assert len(cand) < 2 or ((cand >> 31) == 0).any() and ((cand >> 31) == 1).any(), "the row does not cross zero"
    return check


def _all_tied(cand, k):
    assert len(np.unique(score_key(cand))) == 1, "the keys are not all equal"


def _zeros_check(cand, k):
    _all_tied(cand, k)
    assert (cand == 0).all(), "a zero score kept a sign"


def _tie_check(cand, k):
    key = np.sort(score_key(cand))[::-1]
    assert len(key) > k and key[k - 1] == key[k], "the k-th and the (k+1)-th candidate do not tie"
    tied = np.flatnonzero(score_key(cand) == key[k])
    above = np.flatnonzero(score_key(cand) > key[k])
    assert len(above) == (k - 1) // 2 and tied.max() > tied[k - len(above) - 1], "no tied candidate is left out by position"
    assert len(above) == 0 or above.max() > tied.min(), "no better candidate arrives after the first tied one"


def _subnormal_check(cand, k):
    mag = cand & np.uint32(0x7FFFFFFF)
    sub = (mag > 0) & (mag < np.uint32(0x00800000))
    n = len(cand)
    assert (sub & (cand >> 31 == 0)).any() or n < 1, "no positive subnormal"
    assert n < 2 or (sub & (cand >> 31 == 1)).any(), "no negative subnormal"
    assert n < 3 or (cand == 0).any(), "no zero between them"
    flushed = np.where(sub, np.uint32(0), cand)
    assert n < 2 or not np.array_equal(topk(cand, n)[0], topk(flushed, n)[0]), "a flushing compare would rank the row the same way"


def _range_check(cand, k):
    for b in (POS_INF, NEG_INF, POS_MAX, NEG_MAX)[: len(cand)]:
        assert (cand == np.uint32(b)).any(), f"0x{b:08X} is missing"


def _nan_check(cand, k):
    for b in (POS_NAN, NEG_NAN):
        assert (cand[:k] == np.uint32(b)).any() and (cand[k:] == np.uint32(b)).any(), f"no 0x{b:08X} on both sides of position {k}"
    assert (is_nan(cand) == ((cand == np.uint32(POS_NAN)) | (cand == np.uint32(NEG_NAN)))).all(), "a NaN of another payload"


def _cycle(pattern, n):
    """n cells of the pattern (UNSTORED = no weight) -> (bits, stored)."""
    cells = [pattern[i % len(pattern)] for i in range(n)]
    return (np.array([0 if c is UNSTORED else c for c in cells], np.uint32), np.array([c is not UNSTORED for c in cells], bool))


def _tie_run(n, k):
    """Fewer than k candidates above T = 0.5, more than k at or above it: tied and better candidates alternate at evenly spread positions (the
    better ones ascending, so each of them goes to the front of the list), worse ones fill the gaps."""
    above = (k - 1) // 2
    tied = min(k - above + 2, n - above)
    assert above + tied > k
    special = above + tied
    at = (np.arange(special, dtype=np.int64) * n) // special
    bits = (np.uint32(0x3EFFFFFF) - np.arange(n, dtype=np.uint32)).astype(np.uint32)          # worse: distinct, descending
    kinds = ["ta"[j % 2] if j < 2 * min(above, tied) else ("t" if tied > above else "a") for j in range(special)]
    bits[at] = [0x3F000000 if c == "t" else 0 for c in kinds]
    up = at[[c == "a" for c in kinds]]
    bits[up] = np.uint32(0x3F000001) + np.arange(len(up), dtype=np.uint32)
    return bits


def _with_nans(base, before, after):
    bits = base.copy()
    for (p_pos, p_neg) in (before, after):
        bits[p_pos], bits[p_neg] = POS_NAN, NEG_NAN
    return bits


def _zigzag(n):
    d = _descending(n)
    out = d.copy()
    out[0::2] = d[: (n + 1) // 2]
    out[1::2] = d[(n + 1) // 2:][::-1]
    return out


def nan_rows(n, k):
    """The three NaN placements of a row built around k (needs 2 <= k <= n - 2): both signs before the list fills and right after; right before it fills
    and in the middle of what follows, on a descending row (nothing else enters a full list); early and at the LAST positions, on a zigzag row."""
    assert 2 <= k <= n - 2
    mid = k + (n - k - 2) // 2
    full = np.ones(n, bool)
    return [Scenario(f"nan_before_fill_k{k}", k, _with_nans(_descending(n)[::-1].copy(), (0, 1), (k + 1, k)), full, False, False, _nan_check),
            Scenario(f"nan_after_fill_k{k}", k, _with_nans(_descending(n), (k - 1, k - 2), (mid, mid + 1)), full, False, False, _nan_check),
            Scenario(f"nan_last_k{k}", k, _with_nans(_zigzag(n), (k // 2, 0), (n - 1, n - 2)), full, False, False, _nan_check)]


def tie_run_row(n, k):
    return Scenario(f"tie_run_k{k}", k, _tie_run(n, k), np.ones(n, bool), True, True, _tie_check)


def scenario_rows(n, ks=K_VALUES):
    """The table for candidate rows of n scores: the rows that do not depend on k, then for every k of `ks` that leaves room the run of ties
    straddling rank k (n >= k + 1) and the three NaN rows (2 <= k <= n - 2)."""
    full = np.ones(n, bool)
    rows = [Scenario("descending", 0, _descending(n), full, True, True, _strict(-1)),
            Scenario("ascending", 0, _descending(n)[::-1].copy(), full, True, True, _strict(+1)),
            Scenario("all_equal", 0, np.full(n, 0xC0490FDB, np.uint32), full, True, True, _all_tied),
            Scenario("zeros", 0, *_cycle((0, NEG_ZERO, UNSTORED, NEG_ZERO, 0), n), True, True, _zeros_check),
            Scenario("subnormals", 0, *_cycle((0x00000001, 0x80000001, UNSTORED, 0x007FFFFF, 0x807FFFFF, NEG_ZERO, 0x00000002, 0x80000002,
                                               0x00800000, 0x80800000, 0), n), True, True, _subnormal_check),
            Scenario("inf_fltmax", 0, *_cycle((POS_INF, NEG_INF, POS_MAX, NEG_MAX, 0x3F800000, UNSTORED, 0xBF800000, POS_MAX, POS_INF, NEG_INF, NEG_MAX), n),
                     True, False, _range_check)]
    for k in ks:
        if n >= k + 1:
            rows.append(tie_run_row(n, k))
        if 2 <= k <= n - 2:
            rows.extend(nan_rows(n, k))
    return rows


def check_precondition(s):
    s.check(candidate_row(s.bits, s.stored), s.k)


def cand_bound(chunk_sizes, beam):
    """Floats a layer reserves per query for a beam of `beam` parents: its `beam` largest chunks (Layer::cand_bound), at least 1."""
    return max(1, int(np.sort(np.asarray(chunk_sizes, np.int64))[::-1][: int(beam)].sum()))


def wave_bucket(cand_stride):
    ns = (cand_stride + 63) // 64
    return next(b for b in WAVE_NS if ns <= b)


def expected_form(k, cand_stride, big_min_k=0):
    """(form, NS) a whole-row top-k launch must take: the table of the issue, restated independently of the library's dispatch function."""
    if k > K2_MAX_K or (big_min_k > 0 and k >= big_min_k):
        return "big", 0
    if k <= 64:
        return ("wave", wave_bucket(cand_stride)) if cand_stride <= 2048 else ("reg", 0)
    return "lds", 0
