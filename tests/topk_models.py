"""Models whose candidate rows ARE the rows of tests/topk_order.py, written directly in the reference's folder layout (bias -1.0: no bias row;
post-processor noop), shared by tests/test_topk_order_cpu.py and tests/test_gpu_topk_forms.py.

flat_case: depth 1, W is D x L and row f is scenario f; query r is the single entry (f_r, 1.0), so its candidate row is W[f_r, :] and n = cand_stride = L.
two_layer_case: seven parents with chunks of 1, 63, 64, 65, 300, 0 and 700 children under a permuted leaf; layer 0 weighs the parents a query selects
with exactly 1.0 (they all score 1.0 and enter the beam in id order), the leaf row of the query is its scenario laid along the candidate positions of
that beam -- n differs from query to query and stays below cand_stride, and a position maps back to a label through (beam slot, child, perm)."""
import json
import os
from collections import namedtuple

import numpy as np
import scipy.sparse as smat

import topk_order as T

# X: one stored 1.0 per row; cand[r]: the candidate row of query r (uint32 bits); label[r]: candidate position -> label id; rows[r]: its Scenario (or None);
# beam: beam_size of the predict; cand_stride: floats the last layer reserves per query
Case = namedtuple("Case", "folder X cand label rows beam cand_stride nr_labels")
CHUNKS = (1, 63, 64, 65, 300, 0, 700)
TWO_LAYER_K = (1, 2, 20, 63, 64, 65, 129)


def _csc_from_cells(bits, stored):
    """D x L CSC holding exactly the stored cells of the two [D, L] arrays, explicit zeros, -0.0 and NaN bit patterns included."""
    st = np.ascontiguousarray(stored.T)
    indptr = np.zeros(st.shape[0] + 1, np.int64)
    np.cumsum(st.sum(axis=1), out=indptr[1:])
    indices = np.nonzero(st)[1].astype(np.int32)
    data = np.ascontiguousarray(bits.T)[st].astype(np.uint32).view(np.float32)
    return smat.csc_matrix((data, indices, indptr), shape=stored.shape)


def write_model(folder, layers, only_topk=10):
    """layers: [(W csc, C csc)] top-down."""
    os.makedirs(os.path.join(folder, "ranker"), exist_ok=True)
    for d, (W, C) in enumerate(layers):
        lf = os.path.join(folder, "ranker", f"{d}.model")
        os.makedirs(lf, exist_ok=True)
        smat.save_npz(os.path.join(lf, "W.npz"), W, compressed=False)
        smat.save_npz(os.path.join(lf, "C.npz"), C, compressed=False)
        json.dump({"model": "MLModel", "bias": -1.0, "pred_kwargs": {"only_topk": only_topk, "post_processor": "noop"}}, open(os.path.join(lf, "param.json"), "w"))
    json.dump({"model": "HierarchicalMLModel", "depth": len(layers)}, open(os.path.join(folder, "ranker", "param.json"), "w"))
    json.dump({"model": "XLinearModel"}, open(os.path.join(folder, "param.json"), "w"))
    return folder


def one_hot(D):
    return smat.csr_matrix((np.ones(D, np.float32), np.arange(D, dtype=np.int32), np.arange(D + 1, dtype=np.int64)), shape=(D, D))


def flat_case(folder, L, rows):
    D = len(rows)
    bits = np.stack([s.bits for s in rows]); stored = np.stack([s.stored for s in rows])
    C = smat.csc_matrix(np.ones((L, 1), np.float32))
    write_model(folder, [(_csc_from_cells(bits, stored), C)])
    ident = np.arange(L, dtype=np.int64)
    return Case(folder, one_hot(D), [T.candidate_row(s.bits, s.stored) for s in rows], [ident] * D, list(rows), 1, T.cand_bound([L], 1), L)


def big_rows():
    """The three rows of the 20 482-label model, built around k = 20 480: ascending (an insertion sort of 20 480 entries by one wavefront in the lds
    form), the run of ties straddling rank k, NaNs early and at the last positions."""
    n, k = T.BIG_L, T.BIG_K[0]
    asc = T.scenario_rows(n, ())[1]
    assert asc.name == "ascending"
    return [asc, T.tie_run_row(n, k), T.nan_rows(n, k)[2]]


def finite_rows(rows):
    return [s for s in rows if s.nan_free and s.inf_free]


# ---------------------------------------------------------------------------------------------------------------- two layers
PARENT_SETS = {1: ((0,), (3,), (6,), (5,), (4,)),                       # (5,): the empty parent alone, a query without candidates
               3: ((0, 1, 2), (2, 3, 4), (4, 5, 6), (1, 3, 5), (0, 5, 6)),
               7: (tuple(range(7)),)}
DECOY = 0x7F000000          # a huge finite weight on the children of the parents a query did NOT select: a mapping that reaches them shows at rank 0


def two_layer_cases(folder, finite_only=False, seed=11):
    """One model, one Case per beam size (1, 3, 7): the queries of a case select parent sets of that size."""
    rng = np.random.default_rng(seed)
    n_leaf = sum(CHUNKS)
    perm = rng.permutation(n_leaf)
    start = np.concatenate([[0], np.cumsum(CHUNKS)])
    kids = [perm[start[p]: start[p + 1]] for p in range(len(CHUNKS))]
    C0 = smat.csc_matrix(np.ones((len(CHUNKS), 1), np.float32))
    C1 = smat.csc_matrix((np.ones(n_leaf, np.float32), perm.astype(np.int32), start.astype(np.int64)), shape=(n_leaf, len(CHUNKS)))
    queries = []                                                       # (beam, parent set, label of every position, Scenario or None)
    for beam, sets in PARENT_SETS.items():
        for ps in sets:
            label = np.concatenate([kids[p] for p in ps]).astype(np.int64)
            table = T.scenario_rows(len(label), TWO_LAYER_K) if len(label) else [None]
            for s in table:
                if s is None or not finite_only or (s.nan_free and s.inf_free):
                    queries.append((beam, ps, label, s))
    D = len(queries)
    w0 = np.zeros((D, len(CHUNKS)), np.uint32); s0 = np.zeros((D, len(CHUNKS)), bool)
    w1 = np.zeros((D, n_leaf), np.uint32); s1 = np.zeros((D, n_leaf), bool)
    for f, (beam, ps, label, s) in enumerate(queries):
        w0[f, list(ps)] = 0x3F800000; s0[f, list(ps)] = True
        if f % 2:
            others = np.setdiff1d(np.arange(n_leaf), label)
            w1[f, others] = DECOY; s1[f, others] = True
        if s is not None:
            w1[f, label] = s.bits; s1[f, label] = s.stored
    write_model(folder, [(_csc_from_cells(w0, s0), C0), (_csc_from_cells(w1, s1), C1)])
    X = one_hot(D)
    cases = {}
    for beam in PARENT_SETS:
        fs = [f for f, q in enumerate(queries) if q[0] == beam]
        cases[beam] = Case(folder, X[fs], [T.candidate_row(queries[f][3].bits, queries[f][3].stored) if queries[f][3] is not None else np.zeros(0, np.uint32) for f in fs],
                           [queries[f][2] for f in fs], [queries[f][3] for f in fs], beam, T.cand_bound(CHUNKS, beam), n_leaf)
    return cases


def expected(case, k):
    """Per query: (label ids best first, score bits) of its first min(k, n) candidates under topk_order.topk."""
    out = []
    for cand, label in zip(case.cand, case.label):
        pos, bits = T.topk(cand, k)
        out.append((label[pos], bits))
    return out


def expected_csr(case, k):
    exp = expected(case, k)
    indptr = np.concatenate([[0], np.cumsum([len(l) for l, _ in exp])]).astype(np.int64)
    idx = np.concatenate([l for l, _ in exp]) if exp else np.zeros(0, np.int64)
    bits = np.concatenate([b for _, b in exp]) if exp else np.zeros(0, np.uint32)
    return smat.csr_matrix((bits.astype(np.uint32).view(np.float32), idx, indptr), shape=(len(exp), case.nr_labels))


# ---------------------------------------------------------------------------------------------------------------- bound-pruned layers
# noop layers are never bound-pruned, so the rank-limited first stage, the middle stage, the list form of the last stage and K1T's selecting
# epilogue need a COMBINING post-processor.  Then a candidate's score is no longer its weight: the expected row is what the restatement's unsorted
# route (predict_on_selected_outputs: no sort anywhere) scores for the beam's children, ranked by topk_order.topk.
PRUNED_PP = "l3-hinge"
PRUNED_CHUNKS = (64, 1, 63, 65, 128, 127, 100, 32) + (64,) * 12          # every parent is one tile (<= 128 children): what K1T's epilogue asks for
_TWELVE = tuple(range(8, 20))
PRUNED_BEAMS = {2: ((0, 1), (0, 2), (0, 3), (1, 2), (4, 5)),               # n = 65, 127, 129, 64, 255
                3: ((0, 8, 9), (0, 8, 3), (4, 5, 6)),                       # 192, 193, 355
                13: (_TWELVE + (0,),), 14: (_TWELVE + (0, 1),),             # 832, 833
                16: (_TWELVE + (0, 1, 2, 3),), 18: (_TWELVE + (0, 1, 2, 3, 7, 4),)}   # 961, 1121: beams of >= 16 parents take the middle stage
PRUNED_K = (1, 2, 20, 63, 64)


def pruned_cases(folder, oracle_mod, seed=12):
    """One two-layer l3-hinge model, one Case per beam size.  Query f lists its parents best first: weight 1.0 on the first, then either far
    lower ones (f even: the first parent's children settle the query, the first stage is final) or nearly equal ones (f odd: it is not);
    the other parents weigh -3.  Its leaf row lays a finite row of the table along the candidate positions of that beam."""
    rng = np.random.default_rng(seed)
    P, n_leaf = len(PRUNED_CHUNKS), sum(PRUNED_CHUNKS)
    perm = rng.permutation(n_leaf)
    start = np.concatenate([[0], np.cumsum(PRUNED_CHUNKS)])
    kids = [perm[start[p]: start[p + 1]] for p in range(P)]
    C0 = smat.csc_matrix(np.ones((P, 1), np.float32))
    C1 = smat.csc_matrix((np.ones(n_leaf, np.float32), perm.astype(np.int32), start.astype(np.int64)), shape=(n_leaf, P))
    queries = []
    for beam, lists in PRUNED_BEAMS.items():
        for ps in lists:
            label = np.concatenate([kids[p] for p in ps]).astype(np.int64)
            for s in finite_rows(T.scenario_rows(len(label), PRUNED_K)):
                if s.name != "subnormals":
                    queries += [(beam, ps, label, s)] * 2
    D = len(queries)
    w0 = np.full((D, P), np.float32(-3.0).view(np.uint32), np.uint32); s0 = np.ones((D, P), bool)
    w1 = np.zeros((D, n_leaf), np.uint32); s1 = np.zeros((D, n_leaf), bool)
    for f, (beam, ps, label, s) in enumerate(queries):
        lower = (0.9 if f % 2 else -1.0) - 0.01 * np.arange(1, len(ps), dtype=np.float32)
        w0[f, list(ps)] = np.concatenate([[1.0], lower]).astype(np.float32).view(np.uint32)
        w1[f, label] = s.bits; s1[f, label] = s.stored
    write_model(folder, [(_csc_from_cells(w0, s0), C0), (_csc_from_cells(w1, s1), C1)])
    for lf in (os.path.join(folder, "ranker", f"{d}.model", "param.json") for d in range(2)):
        json.dump({"model": "MLModel", "bias": -1.0, "pred_kwargs": {"only_topk": 10, "post_processor": PRUNED_PP}}, open(lf, "w"))
    # what the reference's arithmetic scores, without any sort: the parents, then the children of the beam
    X = one_hot(D)
    layers = oracle_mod.load_model_folder(folder)
    top = oracle_mod.OracleModel(layers[:1]).predict_on_selected_outputs(X, smat.csr_matrix(np.ones((D, P), np.float32)), PRUNED_PP)
    S = smat.lil_matrix((D, n_leaf), dtype=np.float32)
    for f, q in enumerate(queries):
        S[f, q[2]] = 1.0
    leaf = oracle_mod.OracleModel(layers).predict_on_selected_outputs(X, S.tocsr(), PRUNED_PP)
    cand = []
    for f, (beam, ps, label, s) in enumerate(queries):
        pbits = np.zeros(P, np.uint32)
        pbits[top.indices[top.indptr[f]: top.indptr[f + 1]]] = top.data[top.indptr[f]: top.indptr[f + 1]].astype(np.float32).view(np.uint32)
        assert T.topk(pbits, beam)[0].tolist() == list(ps), "the beam is not the listed parents in the listed order"
        bits = np.zeros(n_leaf, np.uint32)
        bits[leaf.indices[leaf.indptr[f]: leaf.indptr[f + 1]]] = leaf.data[leaf.indptr[f]: leaf.indptr[f + 1]].astype(np.float32).view(np.uint32)
        cand.append(bits[label])
    cases = {}
    for beam in PRUNED_BEAMS:
        fs = [f for f, q in enumerate(queries) if q[0] == beam]
        cases[beam] = Case(folder, X[fs], [cand[f] for f in fs], [queries[f][2] for f in fs], [queries[f][3] for f in fs], beam, T.cand_bound(PRUNED_CHUNKS, beam), n_leaf)
    return cases


def check_pruned_precondition(case):
    """The rows are scores now, not weights, and a child's score carries its parent's: equal weights tie inside one beam slot only.  What must
    still hold: at every k below the first slot's 64 children some row has its k-th and (k+1)-th score tied, and a row is not one value throughout
    unless its weights were."""
    tied = {k: 0 for k in PRUNED_K}
    for cand, s in zip(case.cand, case.rows):
        key = np.sort(T.score_key(cand))[::-1]
        for k in PRUNED_K:
            tied[k] += int(len(key) > k and key[k - 1] == key[k])
        if s.name in ("all_equal", "zeros"):
            assert len(set(key.tolist())) <= case.beam, f"{s.name}: the children of one parent do not tie"
        else:
            assert len(set(key.tolist())) > 1, f"{s.name}: every score is the same"
    assert all(tied[k] >= 2 for k in PRUNED_K if k < 64), f"rows whose k-th and (k+1)-th score tie, per k: {tied}"
