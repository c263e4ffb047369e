"""Selected outputs on the device (xrl_predict_selected_device, K7), the half that needs no GPU: the closed form of the reference's walk that
the plan kernel computes (tests/select_plan.py) against the oracle's predict_on_selected_outputs, the entry point's argument checks, its
binding, and the compiled kernels' resources."""
import ctypes
import os
import re

import numpy as np
import pytest

import select_plan as sp
from conftest import GOLDEN, load_X

SYNTH = ("s_eurlex", "s_contig", "s_deep", "s_nobias", "s_flat", "s_wide", "s_pruned")


@pytest.mark.parametrize("name", SYNTH)
def test_numpy_plan_equals_the_oracle_order(name, oracle_mod):
    folder = os.path.join(GOLDEN, "synth", name)
    layers = oracle_mod.load_model_folder(folder)
    om = oracle_mod.OracleModel(layers)
    tree = sp.tree_arrays(layers)
    nr_labels = layers[-1]["W"].shape[1]
    pool = sp.rooted_labels(tree)                       # every label, except on the pruned tree
    assert (len(pool) < nr_labels) == (name == "s_pruned")
    rows = sp.random_rows(pool, seed=len(name))
    assert [len(r) for r in rows] == [min(n, len(pool)) for n in sp.ROW_LENGTHS]
    X = load_X(os.path.join(GOLDEN, "synth", name + "__X.npz"))
    assert X.shape[0] >= len(rows)
    S = sp.rows_to_csr(rows, nr_labels)
    want = om.predict_on_selected_outputs(X[: len(rows)], S)
    deepest_crank = 0
    for r, lab in enumerate(rows):
        code, nodes, ppos = sp.plan_row(tree, lab, nr_labels)
        assert code == sp.OK
        got = nodes[-1]
        assert np.array_equal(got, want.indices[want.indptr[r]: want.indptr[r + 1]].astype(np.uint32)), f"{name} row {r} ({len(lab)} labels): order"
        for l in range(1, len(tree)):                   # every node's parent sits where ppos says
            assert np.array_equal(tree[l][0][nodes[l]], nodes[l - 1][ppos[l]]), f"{name} row {r} layer {l}: ppos"
        deepest_crank = max([deepest_crank] + [int(tree[l][1][nodes[l]].max()) for l in range(len(tree)) if len(nodes[l])])
    if name in ("s_flat", "s_wide"):
        assert deepest_crank >= 64                      # positions inside a parent's column beyond one wavefront


def test_numpy_plan_flags_bad_rows(oracle_mod):
    layers = oracle_mod.load_model_folder(os.path.join(GOLDEN, "synth", "s_pruned"))
    tree = sp.tree_arrays(layers)
    nr_labels = layers[-1]["W"].shape[1]
    pool = sp.rooted_labels(tree)
    orphans = np.setdiff1d(np.arange(nr_labels, dtype=np.uint32), pool)
    assert len(orphans)
    assert sp.plan_row(tree, [pool[0], pool[1], pool[0]], nr_labels)[0] == sp.TWICE
    assert sp.plan_row(tree, [pool[0], nr_labels], nr_labels)[0] == sp.OUT_OF_RANGE
    assert sp.plan_row(tree, [pool[0], orphans[0]], nr_labels)[0] == sp.NO_PARENT
    assert sp.plan_row(tree, [], nr_labels)[0] == sp.OK


# ------------------------------------------------------------------------------------------------------------------ the entry point
def test_entry_point_is_exported_and_bound():
    from pecos_amd import clib, features
    fn = clib.clib_float32.xrl_predict_selected_device
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
    assert callable(clib.predict_selected_device) and callable(features.predict_selected_from_torch)
    assert "ensemble_device" in features.predict_selected_from_torch.__doc__ and "predict_from_torch" in features.predict_selected_from_torch.__doc__


def _call(model=0, queries=0x2000, sel=0x3000, out=(0x4000, 0x5000, 0x6000), sel_stride=8, out_stride=8):
    """xrl_predict_selected_device on made-up, never dereferenced addresses: what is under test comes before any use of them."""
    from pecos_amd import clib
    lib = clib.clib_float32
    rc = lib.xrl_predict_selected_device(ctypes.c_void_p(model), ctypes.c_void_p(queries), None, ctypes.c_void_p(sel), None, sel_stride,
                                         ctypes.c_void_p(out[0]), ctypes.c_void_p(out[1]), ctypes.c_void_p(out[2]), out_stride, None, None, 1)
    err = lib.xrl_last_error()
    lib.xrl_clear_error()
    return rc, (err or b"").decode()


def test_null_handle_is_refused_without_a_gpu():
    rc, err = _call(model=0)
    assert rc == -1 and err.startswith("xrl_predict_selected_device: ") and "null argument" in err, (rc, err)


def test_k7_resources(tmp_path):
    # every instantiation of the plan kernel: no scratch, no spills, 16 bytes of wavefront-private LDS per entry (4 wavefronts per workgroup, 2 at 16 entries per lane)
    from test_kernel_resources import demangle, kernel_notes
    notes = kernel_notes(tmp_path)
    nice = demangle(sorted(notes))
    k7 = {nice[k]: v for k, v in notes.items() if "k7_select_plan_kernel<" in nice[k]}
    seen = set()
    for name, d in k7.items():
        ns = int(re.search(r"k7_select_plan_kernel<(\d+)>", name).group(1))
        seen.add(ns)
        assert d["scratch"] == 0 and d["vgpr_spill"] == 0, (name, d)
        assert d["lds"] == ns * 64 * 16 * (2 if ns == 16 else 4) and d["lds"] <= 32768, (name, d)
    assert seen == {1, 2, 4, 8, 16}, sorted(seen)
    k4 = [v for k, v in notes.items() if "k4_selected_dev_kernel<" in nice[k]]
    assert len(k4) == 2 and all(d["scratch"] == 0 for d in k4)
