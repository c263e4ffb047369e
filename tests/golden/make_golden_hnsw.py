"""Records tests/golden/hnsw/: four indexes trained by the compiled reference (csr / drm x ip / l2, at most 600 items, M = 8, threads = 1),
their queries, and the reference's ids and distance bits at (efS, topk) = (1, 1), (20, 10), (10, 20), (50, 50), plus the CPU flags of the
recording host.  Dense distances depend on the reference's CPU clone: without avx512f the dense fixtures are refused.
range_edges.npz holds what the reference returns for hnsw_rule.range_edge_cases() -- distances that overflow fp32 and NaNs in the queues --
as ids and distance bits only (the indexes are written from the generators by the tests); it is recorded on its own and leaves the rest alone.

    python tests/golden/make_golden_hnsw.py                  (needs oracle/_ref/libpecos_float32.so)
    python tests/golden/make_golden_hnsw.py range_edges      (range_edges.npz only)
"""
import json
import os
import shutil
import sys

import numpy as np
import scipy.sparse as smat

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hnsw_rule as hr  # noqa: E402

OUT = os.path.join(HERE, "hnsw")
SETTINGS = ((1, 1), (20, 10), (10, 20), (50, 50))
CASES = {"drm_ip": ("drm", "ip", 11), "drm_l2": ("drm", "l2", 12), "csr_ip": ("csr", "ip", 13), "csr_l2": ("csr", "l2", 14)}


def items_and_queries(kind, seed):
    if kind == "drm":
        X = hr.dense_items(500, 35, seed)
        X[40:44] = X[40]                                     # duplicates: the tie case of the heaps
        return X, hr.dense_items(24, 35, seed + 100)
    X = hr.sparse_items(600, 300, 9, seed).tolil()
    X[50] = X[51]
    return X.tocsr().astype(np.float32), hr.sparse_items(24, 300, 12, seed + 100)


def record_range_edges():
    """ids (u8: at most 64 nodes) and distance bits of every case and setting, in the layout of hr.range_edge_blocks; run twice and with 4
    searchers, and refused if the reference does not repeat itself."""
    import tempfile
    cases = hr.range_edge_cases()
    idx, bits, layout = [], [], []
    for name, efS, topk, at in hr.range_edge_blocks(cases):
        ix, Q, _ = cases[name]
        with tempfile.TemporaryDirectory() as d:
            hr.write_folder(ix, d)
            got = hr.run_reference(d, Q, efS, topk)
            for threads in (1, 4):
                again = hr.run_reference(d, Q, efS, topk, threads=threads)
                assert np.array_equal(got[0], again[0]) and np.array_equal(got[1].view(np.uint32), again[1].view(np.uint32)), (name, efS, topk, "the reference is not deterministic")
        assert got[0].max() < 256
        idx.append(got[0].astype(np.uint8).reshape(-1))
        bits.append(got[1].view(np.uint32).reshape(-1))
        layout.append("%s:%d:%d:%d" % (name, efS, topk, at.stop))
    path = os.path.join(OUT, "range_edges.npz")
    np.savez_compressed(path, idx=np.concatenate(idx), bits=np.concatenate(bits), layout=np.array(layout))
    assert os.path.getsize(path) <= 16 * 1024, os.path.getsize(path)
    print("recorded", path, os.path.getsize(path), "bytes")


def main():
    if not hr.have_reference():
        sys.exit("oracle/_ref/libpecos_float32.so is missing: build it first")
    flags = sorted({f for line in open("/proc/cpuinfo") if line.startswith("flags") for f in line.split(":", 1)[1].split()} & {"sse", "sse2", "avx", "avx2", "fma", "avx512f"})
    if "avx512f" not in flags:
        sys.exit("this host has no avx512f: the dense fixtures would record another clone of the reference's distance functions; refused")
    os.makedirs(OUT, exist_ok=True)
    if sys.argv[1:] == ["range_edges"]:
        return record_range_edges()
    manifest = {"cpu_flags": flags, "settings": [list(s) for s in SETTINGS], "cases": {}}
    for name, (kind, metric, seed) in CASES.items():
        folder = os.path.join(OUT, name)
        if os.path.exists(folder):
            shutil.rmtree(folder)
        X, Q = items_and_queries(kind, seed)
        hr.train_reference(X, folder, metric=metric, M=8, efC=100, threads=1)
        if kind == "drm":
            np.save(os.path.join(folder, "queries.npy"), Q)
        else:
            smat.save_npz(os.path.join(folder, "queries.npz"), Q)
        rec = {}
        for efS, topk in SETTINGS:
            idx, dist = hr.run_reference(folder, Q, efS, topk)
            rec["idx_%d_%d" % (efS, topk)] = idx
            rec["bits_%d_%d" % (efS, topk)] = dist.view(np.uint32)
        np.savez_compressed(os.path.join(folder, "expected.npz"), **rec)
        size = max(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(folder) for f in fs)
        assert size <= 512 * 1024, (name, size)
        manifest["cases"][name] = {"data_type": kind, "metric_type": metric, "num_item": int(X.shape[0]), "feat_dim": int(X.shape[1]), "queries": int(Q.shape[0])}
    # the pop orders of libstdc++'s heaps on all-equal and two-valued distance lists of 1 .. 70 entries (sparse ip: the same on any x86 host)
    orders = {}
    for kind, n, values in hr.heap_lists():
        ix, Q = hr.star_index(values)
        tmp = os.path.join(OUT, "_heap_tmp")
        hr.write_folder(ix, tmp)
        orders["%s_%d" % (kind, n)] = hr.run_reference(tmp, Q, n, n)[0][0]
        shutil.rmtree(tmp)
    np.savez_compressed(os.path.join(OUT, "heap_orders.npz"), **orders)
    json.dump(manifest, open(os.path.join(OUT, "manifest.json"), "w"), indent=1, sort_keys=True)
    record_range_edges()
    print("recorded", OUT)


if __name__ == "__main__":
    main()
