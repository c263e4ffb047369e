"""Records tests/golden/tfidf_training_ref.npz from the COMPILED REFERENCE (oracle/_ref/libpecos_float32.so): for every case of
tests/tfidf_training_rule.py the folder its c_tfidf_train + c_tfidf_save wrote, parsed and digested (vocabulary, n-gram ids, idf text,
configs), and the raw CSR its in-memory trained model predicts on the case's probe corpus (value bits kept).

    python tests/golden/make_golden_tfidf_training.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import tfidf_training_rule as tr  # noqa: E402


def main():
    out = {}
    for name, (corpus, bases, norm_p) in tr.cases().items():
        m = tr.Trained(tr.REF, "c_", corpus, bases, norm_p, threads=1)
        with tempfile.TemporaryDirectory() as d:
            assert m.save(d) is None
            meta, parsed = tr.parse_folder(d)
        out[name + "/digest"] = np.array(tr.digest(tr.canon_model(meta, parsed)))
        out[name + "/sizes"] = np.array([[len(b["vocab"]), len(b["ngrams"])] for b in parsed], dtype=np.int64)
        indptr, indices, data = m.predict(tr.probe_of(bases))
        out[name + "/indptr"], out[name + "/indices"], out[name + "/data_bits"] = indptr.astype(np.int64), indices.astype(np.int64), data.view(np.uint32)
        m.close()
    # the end-to-end corpus: the X the reference's in-memory trained vectorizer gives for its own training documents
    docs, _ = tr.e2e_corpus()
    m = tr.Trained(tr.REF, "c_", docs, tr.E2E_BASES, threads=1)
    indptr, indices, data = m.predict(docs)
    out["e2e/indptr"], out["e2e/indices"], out["e2e/data_bits"] = indptr.astype(np.int64), indices.astype(np.int64), data.view(np.uint32)
    m.close()
    np.savez_compressed(tr.GOLDEN, **out)
    print(tr.GOLDEN, os.path.getsize(tr.GOLDEN), "bytes,", len(tr.cases()), "cases")


if __name__ == "__main__":
    main()
