"""Output constraint (XLinearModel.set_output_constraint on the device), the half that needs no GPU: the numpy statement of the reference's
pruning rule (tests/constraint_view.py) is pinned against the compiled reference and against the reference's own Python method, the
preconditions the GPU tests rely on are asserted on the reference's output, and the Python plumbing is checked with a recording stand-in
for the library."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as smat

import constraint_view as cv
from conftest import GOLDEN, REPO, load_X

SYNTH = ("s_eurlex", "s_pruned", "s_deep", "s_flat", "s_wide", "s_nobias", "s_contig")
LAYOUTS = ("BINARY_SEARCH_CHUNKED", "HASH_CHUNKED", "CSC")
KW = dict(beam_size=10, only_topk=10)
REFPY = os.path.join(REPO, "oracle", "_ref", "refpy")


def bits(P):
    return np.asarray(P.data, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape[0] == b.shape[0] and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(bits(a), bits(b))


def rows_changed(a, b):
    n = 0
    for r in range(a.shape[0]):
        sa, sb = slice(a.indptr[r], a.indptr[r + 1]), slice(b.indptr[r], b.indptr[r + 1])
        n += not (np.array_equal(a.indices[sa], b.indices[sb]) and np.array_equal(bits(a)[sa], bits(b)[sb]))
    return n


def by_label(P):
    """Rows as {label: score bits}: for results whose order inside a row is not the thing compared."""
    v = bits(P)
    return [dict(zip(P.indices[P.indptr[r]: P.indptr[r + 1]].tolist(), v[P.indptr[r]: P.indptr[r + 1]].tolist())) for r in range(P.shape[0])]


@pytest.fixture(scope="module")
def goldens(oracle_mod):
    out = {}
    for name in SYNTH:
        folder = os.path.join(GOLDEN, "synth", name)
        layers = oracle_mod.load_model_folder(folder)
        out[name] = dict(folder=folder, layers=layers, X=load_X(os.path.join(GOLDEN, "synth", name + "__X.npz")),
                         sets=cv.kept_sets(layers[-1]["C"].shape[0], in_tree=layers[-1]["C"].indices))
    return out


@pytest.mark.parametrize("name", SYNTH)
def test_numpy_rule_is_the_compiled_references_answer(name, goldens, oracle_mod, tmp_path):
    """OracleModel on the pruned LAYERS == RefModel on the rewritten FOLDER, bit for bit, in the three layouts; and the preconditions of the
    GPU tests hold on the reference's output."""
    if not oracle_mod.ref_available():
        pytest.skip("oracle/_ref not built")
    g = goldens[name]
    X = g["X"]
    plain = oracle_mod.RefModel(g["folder"]).predict(X, **KW)
    for sname, labels in g["sets"].items():
        folder = cv.prune_folder(g["folder"], str(tmp_path / sname), labels)
        pruned, _ = cv.prune_layers(g["layers"], labels)
        for layout in LAYOUTS:
            want = oracle_mod.RefModel(folder, layout).predict(X, **KW)
            what = f"{name} {sname} {layout}"
            assert set(want.indices.tolist()) <= set(int(v) for v in labels), what + ": the reference returned a label outside the kept set"
            if layout != "CSC":
                assert same_bits(oracle_mod.OracleModel(pruned, layout).predict(X, **KW), want), what
            else:
                # (the restatement has no whole-model CSC arithmetic: it re-scores the reference's pattern through its CSC route, per label)
                S = smat.csr_matrix((np.ones_like(want.data), want.indices, want.indptr), shape=want.shape)
                assert by_label(oracle_mod.OracleModel(pruned).predict_on_selected_outputs(X, S)) == by_label(want), what
        ref = oracle_mod.RefModel(folder).predict(X, **KW)
        n, changed = X.shape[0], rows_changed(ref, plain)
        if sname in cv.CHANGING_SETS:
            assert changed >= 0.9 * n, f"{name} {sname}: only {changed} of {n} rows differ from the unconstrained answer"
        if sname in cv.SPARSE_SETS:
            assert (np.diff(ref.indptr) < KW["only_topk"]).all(), f"{name} {sname}: a row still has k results"


def _s_deep_with_an_emptied_parent(layers, victim):
    """s_deep with one parent of a middle layer emptied: node `victim` of layer 2 loses its children (column `victim` of layer 3's C)."""
    out = [dict(L) for L in layers]
    C = cv._stored_csc(layers[3]["C"])
    keep = np.ones(C.nnz, dtype=bool)
    keep[C.indptr[victim]: C.indptr[victim + 1]] = False
    per_col = np.diff(C.indptr).copy(); per_col[victim] = 0
    out[3]["C"] = smat.csc_matrix((C.data[keep], C.indices[keep], np.concatenate([[0], np.cumsum(per_col)]).astype(C.indptr.dtype)), shape=C.shape)
    return out, victim


def test_early_stop_keeps_an_already_empty_parent(goldens, oracle_mod):
    g = goldens["s_deep"]
    X = g["X"]
    # the victim: the node of layer 2 that most rows rank first there (so that the beam search meets it)
    trace = oracle_mod.OracleModel(g["layers"]).predict_arrays(X, beam_size=1, only_topk=10, trace=True)[3]
    victim = int(np.bincount(trace[0][2, :, 0]).argmax())
    layers, victim = _s_deep_with_an_emptied_parent(g["layers"], victim)
    # a kept set that keeps every node of layer 3 (one leaf under each of its 128 nodes that still has children ... which is all of them:
    # the victim is a node of layer 2), but not every leaf
    C4 = cv._stored_csc(layers[4]["C"])
    labels = np.array([C4.indices[C4.indptr[p]] for p in range(C4.shape[1]) if C4.indptr[p + 1] > C4.indptr[p]])
    assert len(labels) == layers[3]["C"].shape[0] < layers[4]["C"].shape[0]
    pruned, stopped = cv.prune_layers(layers, labels)
    assert stopped == 3, "the rule stops at the layer whose every node is kept"
    C3 = cv._stored_csc(pruned[3]["C"])
    assert C3.indptr[victim + 1] == C3.indptr[victim], "the emptied parent is still empty"
    C2 = cv._stored_csc(pruned[2]["C"])
    assert victim in C2.indices.tolist() and C2.nnz == layers[2]["C"].nnz, "... and stays in the layer above: C of layer 2 is as loaded"
    no_stop, _ = cv.prune_layers(layers, labels, early_stop=False)
    assert victim not in cv._stored_csc(no_stop[2]["C"]).indices.tolist(), "without the stop the rule would delete it"
    # the answers: with the stop a beam slot can go to the dead node (it scores like any other, then yields no candidates); without it the
    # slot goes to the next best node.  Whether a row shows the difference depends on the beam; assert it with the narrowest one.
    diff = 0
    for beam in (1, 2, 10):
        a = oracle_mod.OracleModel(pruned).predict(X, beam_size=beam, only_topk=10)
        b = oracle_mod.OracleModel(no_stop).predict(X, beam_size=beam, only_topk=10)
        diff += rows_changed(a, b)
    assert diff >= 1, "no beam width shows the difference between the rule with and without its stop on this tree"


@pytest.mark.parametrize("name", ("s_eurlex", "s_pruned", "s_deep", "s_contig"))
def test_numpy_rule_is_the_references_own_method(name, goldens):
    """The reference's HierarchicalMLModel.set_output_constraint on a non-predict-only load: C entry for entry."""
    if not os.path.isdir(os.path.join(REFPY, "pecos")):
        pytest.skip("oracle/_ref/refpy (the reference's python package) is not built")
    if REFPY not in sys.path:
        sys.path.insert(0, REFPY)
    from pecos.xmc.xlinear.model import XLinearModel as RefXLM
    g = goldens[name]
    for sname, labels in g["sets"].items():
        m = RefXLM.load(g["folder"], is_predict_only=False)
        m.set_output_constraint([int(v) for v in labels])
        pruned, _ = cv.prune_layers(g["layers"], labels)
        for l, (ml, L) in enumerate(zip(m.model.model_chain, pruned)):
            # (the reference's Python load sorts every column of C; the entries are compared, column by column, in sorted order)
            A, B = smat.csc_matrix(ml.C).copy(), cv._stored_csc(L["C"]).copy()
            A.sort_indices(); B.sort_indices()
            what = f"{name} {sname} layer {l}"
            assert A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices), what
            assert np.array_equal(A.data.astype(np.float32), B.data.astype(np.float32)), what


# ------------------------------------------------------------------------------------------------------------------ python plumbing
class _RecordingClib:
    """Stands in for pecos_amd.xlinear.clib: records the constraint calls."""

    def __init__(self):
        self.calls = []

    def set_output_constraint(self, h, labels):
        self.calls.append(("set", h, sorted(np.asarray(labels).tolist())))

    def clear_output_constraint(self, h):
        self.calls.append(("clear", h))

    def xlinear_destruct_model(self, h):
        pass


@pytest.fixture()
def recording(monkeypatch):
    import pecos_amd.xlinear as xl
    rec = _RecordingClib()
    monkeypatch.setattr(xl, "clib", rec)
    return rec


def _model(handle):
    from pecos_amd.xlinear import HierarchicalMLModel, XLinearModel
    return XLinearModel(HierarchicalMLModel(handle, pred_params={"model_chain": []}))


def test_xlinear_set_output_constraint_plumbing(recording):
    m = _model(11)
    m.set_output_constraint([3, 1, 3, 2])
    m.set_output_constraint(np.array([7, 5], dtype=np.int64))
    m.set_output_constraint(v for v in (9,))
    m.set_output_constraint(None)
    assert recording.calls == [("set", 11, [1, 2, 3]), ("set", 11, [5, 7]), ("set", 11, [9]), ("clear", 11)]
    with pytest.raises(TypeError, match="can not convert labels_to_keep as set variable type!"):
        m.set_output_constraint(5)
    with pytest.raises(ValueError):
        m.set_output_constraint([-1])
    assert len(recording.calls) == 4


def test_text2text_set_output_constraint_plumbing(recording):
    from pecos_amd.features import Text2Text
    t = Text2Text(None, [(_model(21), {}), (_model(22), {})], ["apple", "pear", "plum", "fig"])
    t.set_output_constraint(["plum", "no such item", "apple", "plum"])
    assert recording.calls == [("set", 21, [0, 2]), ("set", 22, [0, 2])]
    t.set_output_constraint(None)
    assert recording.calls[2:] == [("clear", 21), ("clear", 22)]
    with pytest.raises(TypeError):
        t.set_output_constraint(5)


def test_header_table_and_docs_name_the_entry_points():
    from pecos_amd.core import corelib
    names = ("xrl_set_output_constraint", "xrl_set_output_constraint_device", "xrl_clear_output_constraint", "xrl_output_constraint_info")
    header = open(os.path.join(REPO, "include", "xrl_abi.h")).read()
    for n in names:
        assert n in corelib.SIGNATURES and n + "(" in header, n
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "set_output_constraint" in open(os.path.join(REPO, doc)).read(), doc
