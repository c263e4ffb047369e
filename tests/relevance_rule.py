"""Cost-sensitive and user-negative training (K12 under l1 / max, K14's relevance check, the chain builders, XLinearModel.train_ext):
the numpy statements of rules R1a and R1b with every rounding explicit, two wrong variants of l1, the check rule, the chain rules in
scipy over the numpy statement of the sparse product, the case generators and the problem of the recorded fixture."""
import os

import numpy as np
import scipy.sparse as smat

import matching_rule as mr
import ranker_training_rule as rr
import sparse_matmul_rule as smr

F32, F64, U32 = np.float32, np.float64, np.uint32
QUIET = 0x00400000
DEFAULT_NAN = 0xFFC00000               # what an x86 host leaves for inf / inf
NORMS = ("l1", "l2", "max")
NORM_TYPES = (None, "no-norm", "l1", "l2", "max")
KEYSETS = {"k0": (0,), "k02": (0, 2), "k1": (1,), "none": ()}
FIXTURE = os.path.join(rr.REPO, "tests", "golden", "relevance_chains_ref.npz")


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


# ------------------------------------------------------------------------------------------------ R1a, R1b
def _row_l1(v, variant=None):
    """One row under R1a: s = the fp64 chain from +0 of fabs((double)v) in stored order; every entry (float)((double)v / s).
    variant "f32sum": the chain in fp32; "f32div": v / (float)s in fp32 -- both wrong."""
    with np.errstate(all="ignore"):
        if variant == "f32sum":
            s = F64(np.add.accumulate(np.abs(v), dtype=F32)[-1])
        else:
            s = np.add.accumulate(np.abs(v.astype(F64)), dtype=F64)[-1]             # (accumulate adds one after the other: no pairwise tree)
    nan = np.isnan(v)
    if nan.any():                                           # the first NaN, its sign cleared by fabs, rides the chain and the division
        row = (bits(v[nan][:1])[0] & U32(0x7FFFFFFF)) | U32(QUIET)
        return np.where(nan, bits(v) | U32(QUIET), row).astype(U32).view(F32)
    if s == 0.0:
        return v.copy()
    with np.errstate(all="ignore"):
        out = (v / F32(s)).astype(F32) if variant == "f32div" else (v.astype(F64) / s).astype(F32)
    out_bits = bits(out).copy()
    out_bits[np.isnan(out)] = DEFAULT_NAN                   # inf / inf
    return out_bits.view(F32)


def _row_max(v):
    """One row under R1b: n = the fp32 maximum of |v| (NaN if any entry is one); every entry v / n in fp32.  A row with a NaN: a NaN
    entry keeps its bits, quieted; the payload of the others is not part of the contract (0x7FC00000 here)."""
    nan = np.isnan(v)
    if nan.any():
        return np.where(nan, bits(v) | U32(QUIET), U32(0x7FC00000)).astype(U32).view(F32)
    n = np.abs(v).max()
    if n == 0:
        return v.copy()
    with np.errstate(all="ignore"):
        out = (v / F32(n)).astype(F32)
    out_bits = bits(out).copy()
    out_bits[np.isnan(out)] = DEFAULT_NAN
    return out_bits.view(F32)


def normalize(A, norm, variant=None):
    """sklearn.preprocessing.normalize(A, norm=norm) on a float32 CSR read as stored, by the rules: a new CSR of the same pattern."""
    out = smat.csr_matrix(A.shape, dtype=F32)
    out.indptr, out.indices, out.data = A.indptr.copy(), A.indices.copy(), np.asarray(A.data, F32).copy()
    for r in range(A.shape[0]):
        b, e = int(A.indptr[r]), int(A.indptr[r + 1])
        if e > b:
            v = out.data[b:e].copy()
            out.data[b:e] = _row_l1(v, variant) if norm == "l1" else _row_max(v) if norm == "max" else _row_l2_direct(v)
    return out


def _row_l2_direct(v):
    """R1: s = the fp64 chain of the rounded fp32 squares, n = sqrt(s), every entry (float)((double)v / n); NaN and inf as R1 states."""
    with np.errstate(all="ignore"):
        s = np.add.accumulate((v * v).astype(F32).astype(F64), dtype=F64)[-1]
        nan = np.isnan(v)
        if nan.any():
            row = bits(v[nan][:1])[0] | U32(QUIET)
            return np.where(nan, bits(v) | U32(QUIET), row).astype(U32).view(F32)
        if s == 0.0:
            return v.copy()
        out = (v.astype(F64) / np.sqrt(s)).astype(F32)
    out_bits = bits(out).copy()
    out_bits[np.isnan(out)] = DEFAULT_NAN
    return out_bits.view(F32)


def same_normalized(got, want, norm, nan_rows_exact=None):
    """Row pointer, ids and value bits; in a row of ``want`` that holds a NaN the entries must be NaNs, and carry the same bits unless the
    norm is max (R1b: the payload follows numpy's reduction order on the host)."""
    if not mr.same_pattern(got, want):
        return False
    g, w = bits(got.data), bits(want.data)
    wn = np.isnan(np.asarray(want.data, F32))
    if not np.array_equal(np.isnan(np.asarray(got.data, F32)), wn):
        return False
    exact = (norm != "max") if nan_rows_exact is None else nan_rows_exact
    in_nan_row = np.zeros(len(w), bool)
    for r in range(want.shape[0]):
        b, e = int(want.indptr[r]), int(want.indptr[r + 1])
        if wn[b:e].all() and e > b and norm == "max":
            in_nan_row[b:e] = True
    keep = ~in_nan_row if not exact else np.ones(len(w), bool)
    return np.array_equal(g[keep], w[keep])


# the rows that tell the wrong variants of l1 from R1a, found once by search_l1_rows() and kept as bit patterns
L1_F32SUM_ROW = np.array([0x3F180BF0, 0x3F3E612F, 0x3F247A08, 0x3F17241E, 0x3EF66B8E], dtype=U32)
L1_F32DIV_ROW = np.array([0x3F2E69FC, 0x3EFCD716, 0x3F671083, 0x3F77A0BE, 0x3EE3E3CD], dtype=U32)


def search_l1_rows(seed=0, tries=100000, n=5):
    """A row on which the fp32 sum gives another result than R1a, and one on which v / (float)s does (how the two rows above were found)."""
    rs = np.random.RandomState(seed)
    found = {}
    for _ in range(tries):
        v = rs.uniform(0.1, 1.0, n).astype(F32)
        want = bits(_row_l1(v))
        for variant in ("f32sum", "f32div"):
            if variant not in found and not np.array_equal(bits(_row_l1(v, variant)), want):
                found[variant] = bits(v).copy()
        if len(found) == 2:
            break
    return found


def rows_case(lengths, seed=0, cols=1200, scale=1.0, signs=True):
    """One row per length: distinct ascending column ids, values away from zero of either sign."""
    rs = np.random.RandomState(seed)
    rows = []
    for n in lengths:
        ids = np.sort(rs.choice(cols, n, replace=False))
        v = rs.uniform(0.05, 1.0, n) * scale * (rs.choice([-1.0, 1.0], n) if signs else 1.0)
        rows.append((ids, v))
    return mr.raw_csr((len(lengths), cols), rows)


LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 1000)
FLT_MAX = float(np.finfo(F32).max)
SNAN = np.array([0x7FA00123], dtype=U32).view(F32)[0]
NEG_QNAN = np.array([0xFFC00456], dtype=U32).view(F32)[0]


def _spread(values, n, seed):
    """n entries of ordinary values with ``values`` written over the last slots (so a 65-entry row keeps its last one in the 65th)."""
    rs = np.random.RandomState(seed)
    v = rs.uniform(0.05, 1.0, n).astype(F32)
    v[n - len(values):] = values
    return np.arange(n), v


def norm_cases():
    """name -> float32 CSR, rows ascending and without repeated ids (what every norm serves)."""
    out = {"lengths": rows_case(LENGTHS), "negative": rows_case((5, 70), seed=2, signs=False)}
    out["negative"].data *= -1
    sr, dr = L1_F32SUM_ROW.view(F32), L1_F32DIV_ROW.view(F32)
    out["order_rows"] = mr.raw_csr((4, 200), [(np.arange(len(sr)), sr), (np.arange(len(dr)), dr), (np.arange(130), np.resize(sr, 130)), (np.arange(130), np.resize(dr, 130))])
    out["zero_rows"] = mr.raw_csr((3, 100), [(np.arange(3), [0.0, -0.0, 0.0]), (np.arange(70), np.zeros(70)), ([4], [0.0])])
    out["max_last_of_65"] = mr.raw_csr((2, 100), [_spread([7.5], 65, 1), _spread([-7.5], 65, 2)])
    out["tie"] = mr.raw_csr((2, 100), [([1, 5, 9], [2.0, -2.0, 1.0]), _spread([-3.0, 3.0], 66, 3)])
    out["subnormal"] = mr.raw_csr((2, 100), [([0, 1, 2], [1e-45, 3e-42, -5e-40]), _spread([1e-45, 3e-42], 70, 4)])
    out["subnormal"].data[3:71] *= F32(1e-38)
    out["near_flt_max"] = mr.raw_csr((2, 100), [([0, 1, 2], [FLT_MAX, -FLT_MAX, FLT_MAX * 0.5]), (np.arange(70), np.full(70, FLT_MAX * 0.9))])
    inf = np.inf
    out["inf"] = mr.raw_csr((4, 100), [([0, 1, 2], [inf, 1.0, -2.0]), ([0, 1], [-inf, inf]), _spread([-inf], 65, 5), _spread([inf, 3.0], 80, 6)])
    nan = np.nan
    out["nan"] = mr.raw_csr((5, 100), [([0, 1, 2], [1.0, nan, -2.0]), ([0, 1, 2], [NEG_QNAN, SNAN, 3.0]), _spread([SNAN], 65, 7), _spread([NEG_QNAN, 3.0, nan], 90, 8),
                                       ([3, 4], [inf, nan])])
    out["no_rows"] = smat.csr_matrix((0, 9), dtype=F32)
    out["no_entries"] = smat.csr_matrix((4, 9), dtype=F32)
    return out


def duplicate_ids_case():
    """A row that stores one column twice (sklearn's max sums the two before its maximum) and an unsorted row."""
    return mr.raw_csr((3, 50), [([1, 2, 3], [1.0, 2.0, 3.0]), ([4, 9, 9, 12], [1.0, 2.0, 2.5, -3.0]), ([7, 3], [1.0, 2.0])])


# ------------------------------------------------------------------------------------------------ the check
def check_rule(Y, R):
    """(code, row) as xrl_smat_check_relevance_device states them, over two CSRs read as stored."""
    yp, rp = np.asarray(Y.indptr, np.int64), np.asarray(R.indptr, np.int64)
    diff = np.nonzero(yp != rp)[0]
    if len(diff):
        return 1, max(int(diff[0]), 1) - 1
    for code, bad in ((2, np.asarray(Y.indices) != np.asarray(R.indices)), (3, np.asarray(R.data, F32) < 0)):
        at = np.nonzero(bad)[0]
        if len(at):
            return code, int(np.searchsorted(yp, at[0], side="right") - 1)
    return 0, 0


# ------------------------------------------------------------------------------------------------ the chains
def product(A, B):
    """A * B by the numpy statement of the sparse product (eliminate_zeros = 0, sorted_indices = 1), as a CSR."""
    ptr, idx, val = smr.logical(smr.rule(smr.from_scipy(smat.csr_matrix(A, dtype=F32)), smr.from_scipy(smat.csr_matrix(B, dtype=F32)), False, True))
    out = smat.csr_matrix((A.shape[0], B.shape[1]), dtype=F32)
    out.indptr, out.indices, out.data = np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(val, F32)
    return out


def relevance_chain_rule(R_dict, chain, norm_type=None, induce=True):
    """cluster_util.py:257-281 over CSRs; a list of len(chain) CSRs or None (nothing given: all None)."""
    L = len(chain)
    if R_dict is None or all(R_dict[k] is None for k in R_dict):
        return [None] * L
    levels = [None if R_dict.get(0) is None else smat.csr_matrix(R_dict[0], dtype=F32)]
    for i in range(1, L + 1):
        if R_dict.get(i) is not None:
            levels.append(smat.csr_matrix(R_dict[i], dtype=F32))
        elif levels[i - 1] is not None and induce:
            levels.append(product(levels[i - 1], chain[-i]))
        else:
            levels.append(None)
    levels.reverse()
    if norm_type not in (None, "no-norm"):
        levels = [None if m is None else normalize(m, norm_type) for m in levels]
    return levels[1:]


def matching_chain_rule(M_dict, chain):
    """cluster_util.py:219-238 up to the values: a list of len(chain) CSRs of ones with ascending rows, or None (nothing given)."""
    L = len(chain)
    if M_dict is None or all(M_dict[k] is None for k in M_dict):
        return [None] * L
    n = [v.shape[0] for v in M_dict.values() if v is not None][0]
    level = mr.union([smat.csr_matrix(M_dict[0], dtype=F32)]) if M_dict.get(0) is not None else smat.csr_matrix((n, chain[-1].shape[0]), dtype=F32)
    levels = []
    for i in range(1, L + 1):
        parts = [product(level, chain[-i])] + ([smat.csr_matrix(M_dict[i], dtype=F32)] if M_dict.get(i) is not None else [])
        level = mr.union(parts)
        levels.append(level)
    levels.reverse()
    return levels


def canonical_csr(M):
    """Any sparse matrix as a float32 CSR with ascending rows (no entry summed or dropped)."""
    M = smat.csr_matrix(M, dtype=F32)
    M.sort_indices()
    return M


# ------------------------------------------------------------------------------------------------ the recorded problem
N, LABELS, FEATURES, CODES, NR_SPLITS = 200, 48, 64, 16, 4
TRAIN_KW = dict(threshold=0.05, max_iter=30, solver_type="L2R_L2LOSS_SVC_DUAL")


def fixture_problem():
    """X (200 x 64), Y (200 x 48), the bottom clustering C (48 x 16) -- under nr_splits 4 the chain 1 <- 4 <- 16 <- 48 --, a relevance R
    over Y's pattern, and the partial chains R_dict / M_dict per key set."""
    X, Y, C, _ = rr.problem(N, FEATURES, LABELS, CODES, 6, 12, 41)
    Y = canonical_csr(Y)
    rs = np.random.RandomState(43)
    R = Y.copy()
    R.data = rs.uniform(0.1, 2.0, Y.nnz).astype(F32)
    return X, Y, smat.csc_matrix(C, dtype=F32), R


def random_level(cols, per_row, seed, values=True):
    rs = np.random.RandomState(seed)
    ids = np.concatenate([np.sort(rs.choice(cols, min(per_row, cols), replace=False)) for _ in range(N)])
    k = min(per_row, cols)
    v = rs.uniform(0.1, 2.0, len(ids)).astype(F32) if values else np.ones(len(ids), F32)
    return smat.csr_matrix((v, ids, np.arange(N + 1) * k), shape=(N, cols), dtype=F32)


def partial_dict(keys, kind):
    """The partial chain of a key set: level 0 over the labels (R itself for a relevance chain), level 1 over 16 codes, level 2 over 4."""
    _, _, _, R = fixture_problem()
    cols = {0: LABELS, 1: CODES, 2: CODES // NR_SPLITS}
    if kind == "R":
        return {k: (R if k == 0 else random_level(cols[k], 3, 50 + k)) for k in keys}
    return {k: random_level(cols[k], 2, 60 + k, values=False) for k in keys}


# train_ext configurations of the fixture: name -> (keywords of XLinearModel.train, with R, with user_supplied_negatives)
TRAIN_CONFIGS = {
    "induce_l1": (dict(rel_mode="induce", rel_norm="l1"), False, False), "induce_l1_R": (dict(rel_mode="induce", rel_norm="l1"), True, False),
    "induce_max": (dict(rel_mode="induce", rel_norm="max"), False, False), "induce_max_R": (dict(rel_mode="induce", rel_norm="max"), True, False),
    "induce_nonorm": (dict(rel_mode="induce", rel_norm="no-norm"), False, False), "induce_nonorm_R": (dict(rel_mode="induce", rel_norm="no-norm"), True, False),
    "ranker_only": (dict(rel_mode="ranker-only", rel_norm="l1"), True, False),
    "usn": (dict(negative_sampling_scheme="usn"), False, True), "tfn_usn": (dict(negative_sampling_scheme="tfn+usn"), False, True),
    "matcher_1": (dict(mode="matcher", ranker_level=1), False, False), "matcher_2": (dict(mode="matcher", ranker_level=2), False, False),
    "ranker_1": (dict(mode="ranker", ranker_level=1), False, False), "ranker_2": (dict(mode="ranker", ranker_level=2), False, False),
    "combined": (dict(rel_mode="induce", rel_norm="l1", negative_sampling_scheme="tfn+man", post_processor="l3-hinge", beam_size=3), True, False),
}


def train_kwargs(name):
    kw, with_R, with_usn = TRAIN_CONFIGS[name]
    X, Y, C, R = fixture_problem()
    full = dict(nr_splits=NR_SPLITS, min_codes=NR_SPLITS, **TRAIN_KW)
    full.update(kw)
    return X, smat.csc_matrix(Y), C, (R if with_R else None), (partial_dict((0,), "M") if with_usn else None), full
