"""Records tests/golden/ranker_training_ref.npz from the compiled reference (oracle/_ref/libpecos_float32.so, threads = 1): the COO of
its c_xlinear_single_layer_train_csr_f32 on every case of tests/ranker_training_rule.cases() (and a digest of its canonical form at 8
threads), digests of the results too large to keep (the 20 000 x 2 000 problem, the jobs of 65 535 to 65 537 instances), and permutations of std::shuffle(..., std::mt19937(0)) recorded from a
program compiled here with the C++ standard library the reference is compiled with, and the per-layer W and C of the reference's
XLinearModel.train (oracle/_ref/refpy) on ranker_training_rule.e2e_problem().  Inputs and outputs only.
Run from the repository root where the reference is built."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ranker_training_rule as rr  # noqa: E402

SHUFFLE_SIZES = list(range(0, 71)) + [65535, 65536, 65537]

SHUFFLE_PROGRAM = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
int main(int argc, char** argv) {
    for (int k = 1; k < argc; ++k) {
        const uint64_t n = std::strtoull(argv[k], nullptr, 10);
        std::vector<uint64_t> a(n);
        for (uint64_t i = 0; i < n; ++i) a[i] = i;
        std::mt19937 g(0);
        std::shuffle(a.begin(), a.end(), g);
        for (uint64_t v : a) std::printf("%llu\n", (unsigned long long)v);
        std::printf("%lu\n", (unsigned long)g());
    }
    return 0;
}
"""


def record_shuffles():
    """{n: (permutation of 0 .. n-1, the generator's next raw word)}"""
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "shuffle.cpp"), os.path.join(d, "shuffle")
        open(src, "w").write(SHUFFLE_PROGRAM)
        subprocess.check_call(["g++", "-O1", "-o", exe, src])
        words = np.array(subprocess.check_output([exe] + [str(n) for n in SHUFFLE_SIZES]).split(), dtype=np.uint64)
    out, at = {}, 0
    for n in SHUFFLE_SIZES:
        out[n] = (words[at:at + n].astype(np.uint16 if n <= 65536 else np.uint32), int(words[at + n]))      # (the file stays small)
        at += n + 1
    assert at == len(words)
    return out


def record(path):
    out = {}
    for name, (X, Y, C, M, R, kw) in rr.cases().items():
        ref = rr.reference(X, Y, C, M, R, threads=1, **kw)
        out[f"case__{name}__rows"], out[f"case__{name}__cols"], out[f"case__{name}__vals"] = ref["rows"].astype(np.uint32), ref["cols"].astype(np.uint32), ref["vals"]
        out[f"digest8__{name}"] = np.array(rr.digest(rr.reference(X, Y, C, M, R, threads=8, **kw)))       # the same weights, another order
    X, Y, C, M, kw = rr.scale_problem()
    out["digest__scale"] = np.array(rr.digest(rr.reference(X, Y, C, M, None, threads=1, **kw)))
    for n in rr.BIG_JOBS:
        X, Y, kw = rr.big_job(n)
        out[f"digest__big{n}"] = np.array(rr.digest(rr.reference(X, Y, None, None, None, threads=1, **kw)))
    # the reference's XLinearModel.train, layer by layer
    sys.path.insert(0, os.path.join(rr.REPO, "oracle", "_ref", "refpy"))
    from pecos.xmc.xlinear.model import XLinearModel
    X, Y, C = rr.e2e_problem()
    chain = XLinearModel.train(X, Y, C=C, **rr.E2E_KW).model.model_chain
    out["e2e__depth"] = np.array([len(chain)])
    for d, layer in enumerate(chain):
        for tag, A in (("W", layer.W.tocsc()), ("C", layer.C.tocsc())):
            A.sort_indices()
            out[f"e2e__{d}__{tag}__shape"], out[f"e2e__{d}__{tag}__indptr"] = np.array(A.shape), A.indptr.astype(np.int64)
            out[f"e2e__{d}__{tag}__indices"], out[f"e2e__{d}__{tag}__data"] = A.indices.astype(np.int32), A.data.astype(np.float32)
    for n, (perm, nxt) in record_shuffles().items():
        out[f"shuffle__{n}__perm"], out[f"shuffle__{n}__next"] = perm, np.array([nxt], dtype=np.uint32)
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    record(os.path.join(HERE, "ranker_training_ref.npz"))
