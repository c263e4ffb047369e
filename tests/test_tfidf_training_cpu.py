"""TF-IDF training (K15), the part that needs no GPU: the statement of the rule (tests/tfidf_training_rule.py) against the recorded and
the live compiled reference, the idf expression pinned by the reference's in-memory predict bits, the two wrong variants, the float
rounding of the df-ratio products, every refusal the arguments alone decide, the Python config handling, and the exported symbols."""
import copy
import ctypes
import json
import math
import os
import sys
import tempfile

import numpy as np
import pytest

import tfidf_training_rule as tr

F32 = np.float32
CASES = tr.cases()
HAVE_REF = os.path.exists(tr.REF)
need_ref = pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/libpecos_float32.so (the compiled reference) is not built")


@pytest.fixture(scope="module")
def golden():
    return np.load(tr.GOLDEN)


def predict_statement(model, p, docs, idf_fn=tr.idf_of, nr_doc=None):
    """tfidf.hpp:775-822 for one base without binary / sublinear_tf: counts * idf, the norm summed in ascending feature order, all float32."""
    indptr, indices, data = [0], [], []
    for d in docs:
        ts = tr.tokens_of(d, p["tok_type"])
        if p["max_length"] > 0:
            ts = ts[:p["max_length"]]
        ids = [model["vocab"].get(t, -1) for t in ts]
        cnt = {}
        for n in range(p["min_ngram"], min(p["max_ngram"], len(ids)) + 1):
            for i in range(len(ids) - n + 1):
                f = model["ngrams"].get(tuple(ids[i:i + n]))
                if f is not None:
                    cnt[f] = cnt.get(f, 0) + 1
        feats = sorted(cnt)
        v = [F32(cnt[f]) * model["idf"][f] if p["use_idf"] else F32(cnt[f]) for f in feats]
        den = F32(0)
        for x in v:
            den = F32(den + (abs(x) if p["norm_p"] == 1 else F32(x * x)))
        den = F32(1) if abs(den) < np.finfo(F32).eps else (np.sqrt(den, dtype=F32) if p["norm_p"] == 2 else den)
        indices += feats
        data += [F32(x / den) for x in v]
        indptr.append(len(indices))
    return np.array(indptr), np.array(indices, dtype=np.int64), np.array(data, dtype=F32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_statement_equals_the_recorded_reference(name, golden):
    corpus, bases, norm_p = CASES[name]
    meta, parsed = tr.statement_as_parsed(corpus, bases, norm_p)
    assert [[len(b["vocab"]), len(b["ngrams"])] for b in parsed] == golden[name + "/sizes"].tolist()
    assert tr.digest(tr.canon_model(meta, parsed)) == str(golden[name + "/digest"])
    if len(bases) == 1 and not bases[0]["sublinear_tf"]:
        s = tr.statement(corpus, bases[0])
        indptr, indices, data = predict_statement(s, bases[0], tr.probe_of(bases))
        assert np.array_equal(indptr, golden[name + "/indptr"]) and np.array_equal(indices, golden[name + "/indices"])
        assert np.array_equal(data.view(np.uint32), golden[name + "/data_bits"]), "the idf expression is not the reference's"


@need_ref
@pytest.mark.parametrize("threads", [1, 8])
def test_statement_equals_the_live_reference(threads, golden):
    for name, (corpus, bases, norm_p) in CASES.items():
        m = tr.Trained(tr.REF, "c_", corpus, bases, norm_p, threads=threads)
        with tempfile.TemporaryDirectory() as d:
            assert m.save(d) is None
            meta, parsed = tr.parse_folder(d)
        indptr, indices, data = m.predict(tr.probe_of(bases))
        m.close()
        assert tr.canon_model(meta, parsed) == tr.canon_model(*tr.statement_as_parsed(corpus, bases, norm_p)), name
        assert np.array_equal(indptr, golden[name + "/indptr"]) and np.array_equal(indices, golden[name + "/indices"]), name
        assert np.array_equal(data.view(np.uint32), golden[name + "/data_bits"]), name


def test_idf_is_the_double_log_of_a_float_quotient(golden):
    # tfidf.hpp:955 `log(float / size_t)` resolves to the double log and is rounded to float once: over the cases some feature's idf differs
    # between the two readings, and the reference's predict bits (recorded from its in-memory model) agree with the double reading only
    differs = 0
    for name in ("word_uni", "word_23", "char_uni"):
        corpus, bases, _ = CASES[name]
        p = bases[0]
        a = tr.statement(corpus, p)
        b = dict(a, idf=np.array([tr.idf_of_float_log(len(corpus), c, p["smooth_idf"], p["add_one_idf"]) for c in a["df"]], dtype=F32))
        da = predict_statement(a, p, tr.probe_of(bases))[2]
        db = predict_statement(b, p, tr.probe_of(bases))[2]
        assert np.array_equal(da.view(np.uint32), golden[name + "/data_bits"])
        differs += int(not np.array_equal(a["idf"].view(np.uint32), b["idf"].view(np.uint32))) + 2 * int(not np.array_equal(da.view(np.uint32), db.view(np.uint32)))
    assert differs >= 2, "no case tells logf from log: the recording cannot pin the expression"


def test_wrong_variants_differ():
    corpus, bases, _ = CASES["word_uni"]
    good = tr.statement(corpus, bases[0])
    assert tr.statement(corpus, bases[0], token_key=tr.signed_byte_key)["vocab"] != good["vocab"], "signed-byte order must move the tokens with high bytes"
    corpus, bases, _ = CASES["repeats"]
    good, bad = tr.statement(corpus, bases[0]), tr.statement(corpus, bases[0], per_occurrence=True)
    assert not np.array_equal(good["df"], bad["df"]) or good["ngrams"] != bad["ngrams"]
    # probes of the issue: unsigned bytes, a prefix first
    v = tr.statement([b"zz \xc3\xa9x \xff a ab"], tr.base())["vocab"]
    assert v[b"a"] < v[b"ab"] < v[b"zz"] < v[b"\xc3\xa9x"] < v[b"\xff"]


def test_ratio_products_are_float_products():
    # max_df_ratio = 0.7f, 5 documents: the float product is 3.5 (rounds to 4), the double product of the same float ratio 3.4999999 (3)
    p = tr.base(max_df_ratio=0.7)
    assert tr.df_bounds(p, 5)[1] == 4
    assert tr.df_bounds(p, 5, product=lambda r, n: float(F32(r)) * n)[1] == 3
    corpus = [b"a b", b"a b", b"a b", b"a", b"c"]
    s = tr.statement(corpus, p)
    assert s["vocab"][b"a"] in [g[0] for g in s["ngrams"]], "df 4 is kept under the float product"
    if HAVE_REF:
        m = tr.Trained(tr.REF, "c_", corpus, [p], threads=1)
        with tempfile.TemporaryDirectory() as d:
            m.save(d)
            meta, parsed = tr.parse_folder(d)
        m.close()
        assert parsed[0]["ngrams"] == s["ngrams"]


def test_bound_and_trim_cases_have_the_shapes_they_claim():
    corpus, bases, _ = CASES["df_cnt_bounds"]
    s, everything = tr.statement(corpus, bases[0]), tr.statement(corpus, tr.base())
    assert sorted(everything["df"].tolist()) == list(range(1, 9)), "df 1 .. 8, one token each"
    assert sorted(s["df"].tolist()) == [3, 4, 5, 6], "min_df_cnt 3 and max_df_cnt 6 keep df 3 and 6, drop 2 and 7"
    corpus = tr.tie_docs()
    v = tr.statement(corpus, tr.base())["vocab"]
    name = {i: t for t, i in v.items()}
    kept = lambda mf, keep: [name[g[0]] for g, _ in sorted(tr.statement(corpus, tr.base(max_feature=mf, keep_frequent_feature=keep))["ngrams"].items(), key=lambda x: x[1])]
    assert kept(3, True) == [b"q3", b"r", b"s"] and kept(3, False) == [b"p", b"q1", b"q2"], "the df-2 tie straddles both cuts"
    for mf in (6, 9):
        assert kept(mf, True) == kept(mf, False) == [b"p", b"q1", b"q2", b"q3", b"r", b"s"]
    for name_, bits in (("char15_n15_60bits", 60), ("char17_n13_65bits", 65), ("char16_n16_64bits", 64), ("char_n25_125bits", 125), ("char16_n32_128bits", 128)):
        corpus, bases, _ = CASES[name_]
        s = tr.statement(corpus, bases[0])
        width = max(1, (len(s["vocab"]) - 1).bit_length())
        assert bases[0]["max_ngram"] * width == bits and len(s["ngrams"]) > 0, name_


# ---- refusals that need no GPU
def _refused(corpus, bases, norm_p=None, **kw):
    m = tr.Trained(tr.OURS, "xrl_", corpus, bases, norm_p, **kw)
    assert not m.h and m.error, "the call must be refused"
    return m.error


def test_refusals_before_a_gpu_is_required():
    docs = [b"a b", b"c"]
    assert "unknown tok_type: 7" in _refused(docs, [tr.base(tok_type=7)])
    assert "char_wb" in _refused(docs, [tr.base(tok_type=30)])
    assert "expect 0 < min_ngram <= max_ngram" in _refused(docs, [tr.base(ngram_range=(0, 1))])
    assert "expect 0 < min_ngram <= max_ngram" in _refused(docs, [tr.base(ngram_range=(3, 2))])
    for lo, hi in ((-0.1, 1.0), (0.5, 0.5), (0.0, 1.5)):
        assert "expect 0 <= min_df_ratio < max_df_ratio <= 1.0" in _refused(docs, [tr.base(min_df_ratio=lo, max_df_ratio=hi)])
    assert "norm_p" in _refused(docs, [tr.base(norm_p=3)])
    assert "norm_p" in _refused(docs, [tr.base()], norm_p=0)
    lib = tr.load(tr.OURS)
    fn = lib.xrl_tfidf_train
    fn.restype, fn.argtypes = ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int]
    arr, lens, keep = tr.corpus_arrays(docs)
    vp = tr.make_param([tr.base()])
    empty = tr.make_param([tr.base()])
    empty.num_base_vect = 0
    for args, word in (((None, lens.ctypes.data, 2, ctypes.addressof(vp), 1), "null corpus"), ((arr, None, 2, ctypes.addressof(vp), 1), "null corpus"),
                       ((arr, lens.ctypes.data, 2, None, 1), "null param"), ((arr, lens.ctypes.data, 0, ctypes.addressof(vp), 1), "nr_doc 0"),
                       ((arr, lens.ctypes.data, 1 << 32, ctypes.addressof(vp), 1), "too many documents"),
                       ((arr, lens.ctypes.data, 2, ctypes.addressof(empty), 1), "num_base_vect")):
        assert not fn(*args)
        err = tr.last_error(lib)
        assert err and err.startswith("xrl_tfidf_train: ") and word in err, (word, err)
    dv = lib.xrl_tfidf_train_device
    dv.restype, dv.argtypes = ctypes.c_void_p, [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    assert not dv(0, None, None, None, 2, ctypes.addressof(vp), None)
    assert tr.last_error(lib).startswith("xrl_tfidf_train_device: null text")
    assert not dv(0, 8, 8, 8, 0, ctypes.addressof(vp), None)
    assert "nr_doc 0" in tr.last_error(lib)
    lib.xrl_tfidf_save.restype, lib.xrl_tfidf_save.argtypes = None, [ctypes.c_void_p, ctypes.c_char_p]
    lib.xrl_tfidf_save(None, b"/nowhere")
    assert tr.last_error(lib).startswith("xrl_tfidf_save: null")
    lib.xrl_tfidf_export.restype = ctypes.c_int
    assert lib.xrl_tfidf_export(None, 0, None, None, None, None, None, None, None, None) == -1
    assert tr.last_error(lib).startswith("xrl_tfidf_export: null")


def test_new_symbols_are_exported_and_the_reference_names_are_not():
    lib = tr.load(tr.OURS)
    for name in ("xrl_tfidf_train", "xrl_tfidf_train_device", "xrl_tfidf_save", "xrl_tfidf_transform_device", "xrl_tfidf_export", "xrl_debug_tfidf_train_forms"):
        assert hasattr(lib, name), name
    assert not hasattr(lib, "c_tfidf_train") and not hasattr(lib, "c_tfidf_save")
    import pecos_amd
    for name in ("Tfidf", "Preprocessor", "tfidf_train_device", "tfidf_transform_device"):
        assert name in pecos_amd.__all__ and getattr(pecos_amd, name) is not None
    assert callable(pecos_amd.clib.tfidf_train) and callable(pecos_amd.clib.tfidf_save)


def test_a_folder_without_the_training_keys_is_saved_with_the_reference_defaults(tmp_path):
    # load -> save needs no GPU.  Keys the loader never needed may be absent: the saved folder then states Tfidf.train's defaults
    import json
    import tfidf_cases as tc
    from pecos_amd.features import Tfidf
    src = tc.write_base(str(tmp_path / "src"), 10, [(0, b"a"), (1, b"bb")], [(0, 1.5, (0,)), (1, 0.25, (0, 1))], ngram_range=(1, 2))
    cf = os.path.join(src, "vectorizer", "config.json")
    cfg = json.load(open(cf))
    dropped = ("max_feature", "min_df_ratio", "max_df_ratio", "min_df_cnt", "max_df_cnt", "smooth_idf", "add_one_idf", "keep_frequent_feature")
    for k in dropped:
        del cfg["kwargs"][k]
    json.dump(cfg, open(cf, "w"))
    h = tr.Trained.loaded(tr.OURS, src)
    assert h.error is None and h.h
    h.prefix = "xrl_"
    assert h.save(str(tmp_path / "dst")) is None
    h.close()
    meta, (b,) = tr.parse_folder(str(tmp_path / "dst"))
    assert meta["kwargs"] == {"num_base_vect": 1, "norm_p": 2}
    for k in dropped:
        assert b["config"]["kwargs"][k] == Tfidf.DEFAULTS[k], k
    assert b["config"]["kwargs"]["max_df_ratio"] == 1.0
    assert (b["vocab"], b["ngrams"], b["idf_text"]) == ({b"a": 0, b"bb": 1}, {(0,): 0, (0, 1): 1}, {0: "1.500000", 1: "0.250000"})


GOLDEN_MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tfidf_models")


@pytest.mark.parametrize("name", sorted(os.listdir(GOLDEN_MODELS)))
def test_a_loaded_folder_saves_to_the_reference_bytes_and_loads_back(name, tmp_path):
    # load -> save -> load needs no GPU.  The golden folders were written by the reference: the json files of the saved folder are theirs
    # byte for byte (key order, indentation, floats, no trailing newline), and both handles export the same content
    from pecos_amd import clib
    from pecos_amd.features import Tfidf
    src, dst = os.path.join(GOLDEN_MODELS, name, "model"), str(tmp_path / "saved")
    a = Tfidf.load(src)
    a.save(dst)
    b = Tfidf.load(dst)
    nb = json.load(open(os.path.join(src, "meta.json")))["kwargs"]["num_base_vect"]
    files = ["meta.json"] + [f"{i}.base/{part}/config.json" for i in range(nb) for part in ("tokenizer", "vectorizer")]
    for f in files:
        assert open(os.path.join(dst, f), "rb").read() == open(os.path.join(src, f), "rb").read(), f
    assert a.nr_features == b.nr_features
    for i in range(nb):
        (va, ga, ia), (vb, gb, ib) = clib.tfidf_export(a.model, i), clib.tfidf_export(b.model, i)
        assert va == vb and ga == gb and len(va) > 0 and len(ga) > 0, (name, i)
        assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32)), (name, i)
        # the content is the golden folder's own: every token of its vocab.txt with its index
        lines = open(os.path.join(src, f"{i}.base", "tokenizer", "vocab.txt"), "rb").read().split(b"\n")[1:]
        want = {t: int(k) for k, t in (ln.split(b"\t", 1) for ln in lines if b"\t" in ln) if t}
        assert va == want, (name, i)


# ---- the Python layer
CONFIGS = [
    {},
    {"ngram_range": (1, 3), "truncate_length": 64, "norm": "l1", "analyzer": "char", "max_df_ratio": 0.5, "min_df_cnt": 2},
    {"base_vect_configs": [{"ngram_range": (1, 2), "norm": "l2", "analyzer": "word"}, {"analyzer": "char_wb", "norm": "l1", "max_feature": 9}], "norm_p": 1},
    {"base_vect_configs": [{}]},
]


def _fields(vp):
    return [(vp.num_base_vect, vp.norm_p)] + [[(n, getattr(vp.base_param_ptr[i], n)) for n, _ in type(vp.base_param_ptr[i])._fields_] for i in range(vp.num_base_vect)]


def test_python_config_handling_is_the_references():
    from pecos_amd.core import TfidfVectorizerParam
    from pecos_amd.features import Tfidf
    refpy = os.path.join(tr.REPO, "oracle", "_ref", "refpy")
    have = os.path.isdir(os.path.join(refpy, "pecos"))
    if have and refpy not in sys.path:
        sys.path.insert(0, refpy)
    for cfg in CONFIGS:
        full = Tfidf._full_config(copy.deepcopy(cfg))
        ours = TfidfVectorizerParam.from_config(copy.deepcopy(full))
        assert ours.num_base_vect == len(cfg.get("base_vect_configs", [0]))
        if have:
            import pecos.core.base as pcb
            theirs_cfg = copy.deepcopy(full)
            if "base_vect_configs" in theirs_cfg:
                theirs = pcb.TfidfVectorizerParam([pcb.TfidfBaseVectorizerParam(c) for c in theirs_cfg["base_vect_configs"]], theirs_cfg["norm_p"])
            else:
                b = pcb.TfidfBaseVectorizerParam(theirs_cfg)
                theirs = pcb.TfidfVectorizerParam([b], b.norm_p)
            assert _fields(ours) == _fields(theirs), cfg
    with pytest.raises(ValueError, match="Unknown argument"):
        Tfidf._full_config({"ngram": (1, 2)})
    with pytest.raises(ValueError, match="Unknown argument"):
        Tfidf._full_config({"base_vect_configs": [{"nope": 1}]})
    with pytest.raises(NotImplementedError, match="corpus.txt"):
        Tfidf.train("corpus.txt", {})
    from pecos_amd import clib
    with pytest.raises(NotImplementedError, match="some/folder"):
        clib.tfidf_train("some/folder", {})


def test_reference_binding_links_train_and_save_after_the_rename():
    # the reference's link_tfidf_vectorizer (base.py:1648-1694) binds c_tfidf_train / c_tfidf_save: with the one rename to the xrl_
    # prefix its prototypes fit this library's entry points
    refpy = os.path.join(tr.REPO, "oracle", "_ref", "refpy")
    if not os.path.isdir(os.path.join(refpy, "pecos")):
        pytest.skip("oracle/_ref/refpy (the reference's python package) is not built")
    if refpy not in sys.path:
        sys.path.insert(0, refpy)
    import pecos.core.base as pcb
    ours = ctypes.CDLL(tr.OURS)
    taken = set()

    class Renamed:
        def __getattr__(self, name):
            real = {"c_tfidf_train": "xrl_tfidf_train", "c_tfidf_save": "xrl_tfidf_save"}.get(name, name)
            try:
                f = getattr(ours, real)
                taken.add(real)
            except AttributeError:
                f = getattr(pcb.clib.clib_float32, name)
            return f

    lib = pcb.corelib.__new__(pcb.corelib)
    lib.clib_float32 = Renamed()
    lib.link_tfidf_vectorizer()
    assert {"xrl_tfidf_train", "xrl_tfidf_save", "c_tfidf_load", "c_tfidf_predict"} <= taken
    assert ours.xrl_tfidf_train.restype is not None and len(ours.xrl_tfidf_train.argtypes) == 5
