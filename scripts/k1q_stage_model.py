"""CPU model of K1Q's bound-pruning stages: how many beam parents does a query need on a staged layer, and how many does a
given list of stage ends make the kernel evaluate?

    python scripts/k1q_stage_model.py [--config amazon-670k] [--rows 20000] [--beam B] [--topk 10] [--stages 4,10 --stages 3,4,10 ...]

A layer held in the dense row format scores the children of the best `e_0` beam parents first, asks whether k candidates already
reach the score of parent `e_0` (the exact bound: a child never beats its parent, a later candidate loses ties), and goes on to the
parents [e_0, e_1), ... only for the queries that fail the test.  "Parents needed" of a query is the shortest beam prefix that
passes that test (the beam's length when none does); with stage ends e_0 < e_1 < ... the kernel evaluates the first end that
reaches it.  Every (feature, parent) pair the kernel evaluates is one 64-byte request, so parents per query x features per
query is the layer's request count.

This is a MODEL, not parity: the bench's synthetic model and queries (xrl_synth, the bench's seeds), scores in fp64, the beam
search in numpy.  It prints, for every layer that K1Q would stage (children padded to Gp = a power of two <= 64 columns, more than
one candidate register of 64 at this beam), the histogram of parents needed and the parents per query for every list of stage
ends.  The default lists are today's rule and its neighbours for S = 64 / Gp parents in register 0:
    S, beam | S - S/4, S, beam | S - S/4, S, S + 2, beam | S/2, S - S/4, S, beam
(a stage end in --stages that is not below the beam is dropped; the beam itself is always the last end).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as smat

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xrl_synth  # noqa: E402


def transform(name, z):
    """The post-processor's transform in fp64 and whether it combines by adding (log forms) or multiplying."""
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z)), False
    if name == "log-sigmoid":
        return -np.log1p(np.exp(-z)), True
    if name.startswith("log-l") and name.endswith("-hinge"):
        return -np.maximum(0.0, 1.0 - z) ** int(name[5:-6]), True
    if name.startswith("l") and name.endswith("-hinge"):
        return np.exp(-np.maximum(0.0, 1.0 - z) ** int(name[1:-6])), False
    raise SystemExit(f"post-processor {name!r} has no bound (no staging)")


def k1q_geometry(C, beam_in):
    """(widest parent, Gp, candidate registers, staged by K1Q?) of a layer whose beam holds beam_in parents: children padded to a power of two
    <= 64 columns, 2 .. 16 registers of 64 candidates."""
    width = int(np.diff(C.indptr).max())
    gp = 1
    while gp < width:
        gp <<= 1
    regs = -(-beam_in * gp // 64)
    return width, gp, regs, (gp <= 64 and 1 < regs <= 16)


def load_layers(folder, beam):
    """The layers down to the last one K1Q would stage (W of the layers below it is never read: Amazon-670K's leaf is the largest to load)."""
    depth = json.load(open(os.path.join(folder, "ranker", "param.json")))["depth"]
    metas, last, beam_in = [], -1, 1
    for d in range(depth):
        lf = os.path.join(folder, "ranker", f"{d}.model")
        C = smat.load_npz(os.path.join(lf, "C.npz")).tocsc()
        if d > 0 and k1q_geometry(C, beam_in)[3]:
            last = d
        beam_in = min(beam, C.shape[0])
        metas.append((lf, C))
    layers = []
    for lf, C in metas[:last + 1]:
        par = json.load(open(os.path.join(lf, "param.json")))
        layers.append(dict(W=smat.load_npz(os.path.join(lf, "W.npz")).tocsc().astype(np.float64), C=C,
                           bias=float(par["bias"]), pp=par["pred_kwargs"]["post_processor"]))
    return layers, depth


def beam_layer(Xb, Ly, beam_idx, beam_val, beam_cnt, keep, first):
    """One layer of the beam search for every row: returns the new beam and, per row, the candidates in reference order
    (beam rank major, child order minor) as (scores, beam rank of the parent, validity)."""
    C, W = Ly["C"], Ly["W"]
    n, B = beam_idx.shape
    nch = np.diff(C.indptr)
    width = int(nch.max())
    par = np.where(np.arange(B)[None, :] < beam_cnt[:, None], beam_idx, 0)
    col = np.arange(width)[None, None, :]
    valid = (col < nch[par][:, :, None]) & (np.arange(B)[None, :, None] < beam_cnt[:, None, None])
    child = C.indices[np.minimum(C.indptr[par][:, :, None] + col, len(C.indices) - 1)]
    child = np.where(valid, child, 0)
    score = np.full(child.shape, -np.inf)
    for r0 in range(0, n, 2048):      # (X W for a block of rows as a dense array: 2048 x the layer's labels)
        r1 = min(n, r0 + 2048)
        Z = np.asarray((Xb[r0:r1] @ W).todense())
        t, adds = transform(Ly["pp"], np.take_along_axis(Z, child[r0:r1].reshape(r1 - r0, -1), axis=1).reshape(child[r0:r1].shape))
        if not first:
            t = t + beam_val[r0:r1, :, None] if adds else t * beam_val[r0:r1, :, None]
        score[r0:r1] = np.where(valid[r0:r1], t, -np.inf)
    flat, fchild = score.reshape(n, -1), child.reshape(n, -1)
    order = np.argsort(-flat, axis=1, kind="stable")[:, :keep]         # value descending, position ascending
    new_val = np.take_along_axis(flat, order, axis=1)
    new_idx = np.take_along_axis(fchild, order, axis=1)
    new_cnt = np.minimum(keep, valid.reshape(n, -1).sum(axis=1))
    return new_idx, new_val, new_cnt, score, valid


def parents_needed(score, valid, beam_val, beam_cnt, k, adds):
    """Shortest beam prefix p >= 1 whose candidates hold k scores >= the bound of parent p (its score; max(score, 0) under a
    multiplying combiner); the beam's length when no prefix short of it does."""
    n, B, _ = score.shape
    need = beam_cnt.copy()
    for p in range(B - 1, 0, -1):
        bound = beam_val[:, p] if adds else np.maximum(beam_val[:, p], 0.0)
        reach = ((score[:, :p, :] >= bound[:, None, None]) & valid[:, :p, :]).sum(axis=(1, 2))
        need = np.where((p < beam_cnt) & (reach >= k), p, need)
    return need


def evaluated(need, beam_cnt, ends):
    ev = np.zeros_like(need)
    done = np.zeros(len(need), bool)
    for e in ends:
        stop = ~done & (need <= e)
        ev = np.where(stop, np.minimum(e, beam_cnt), ev)
        done |= stop
    return np.where(done, ev, beam_cnt)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="amazon-670k", choices=sorted(xrl_synth.CONFIGS))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--beam", type=int, default=0, help="default: the config's")
    ap.add_argument("--topk", type=int, default=10, help="what the leaf keeps")
    ap.add_argument("--stages", action="append", default=[], help="comma-separated stage ends in beam slots, repeatable")
    ap.add_argument("--cache", default="/tmp/xrl_bench", help="where the model folder is generated (re-used when present)")
    args = ap.parse_args()

    folder = os.path.join(args.cache, f"{args.config}_{args.scale}")
    if not os.path.exists(os.path.join(folder, ".done")):
        t0 = time.time()
        ks, X, cfg = xrl_synth.make_config(args.config, folder, scale=args.scale)
        smat.save_npz(os.path.join(folder, "X.npz"), X, compressed=False) if smat.issparse(X) else np.save(os.path.join(folder, "X.npy"), X)
        json.dump({"ks": ks, "cfg": cfg}, open(os.path.join(folder, "meta.json"), "w"))
        open(os.path.join(folder, ".done"), "w").write("ok")
        print(f"generated {args.config} in {time.time() - t0:.0f} s", flush=True)
    if os.path.exists(os.path.join(folder, "X.npy")):
        X = smat.csr_matrix(np.load(os.path.join(folder, "X.npy"), mmap_mode="r")[:args.rows])
    else:
        X = smat.load_npz(os.path.join(folder, "X.npz")).tocsr()[:args.rows]
    X = X.astype(np.float64)
    beam = args.beam or xrl_synth.CONFIGS[args.config]["beam"]
    layers, depth = load_layers(folder, beam)
    n = X.shape[0]
    print(f"{args.config}: {n} rows, {X.nnz / n:.1f} features per row, beam {beam}, top-k {args.topk}, layers 0 .. {len(layers) - 1} of {depth} (down to the last one K1Q would stage)")

    beam_idx, beam_val, beam_cnt = np.zeros((n, 1), np.int64), np.ones((n, 1)), np.ones(n, np.int64)
    for l, Ly in enumerate(layers):
        W = Ly["W"]
        Xb = X
        if Ly["bias"] > 0:             # the bias column: W carries its row behind the features
            Xb = smat.hstack([X, smat.csr_matrix(np.full((n, 1), Ly["bias"]))], format="csr")
        if Xb.shape[1] != W.shape[0]:
            raise SystemExit(f"layer {l}: X has {Xb.shape[1]} columns, W {W.shape[0]} rows")
        keep = args.topk if l == depth - 1 else beam      # what the layer keeps: the beam, the top-k on the leaf
        B = beam_idx.shape[1]
        new_idx, new_val, new_cnt, score, valid = beam_layer(Xb, Ly, beam_idx, beam_val, beam_cnt, keep, first=(l == 0))
        width, gp, regs, staged = k1q_geometry(Ly["C"], B)
        if l > 0 and staged:
            S = 64 // gp
            adds = transform(Ly["pp"], np.zeros(1))[1]
            need = parents_needed(score, valid, beam_val, beam_cnt, keep, adds)
            hist = np.bincount(need, minlength=B + 1)[1:]
            print(f"layer {l}: {width} children per parent (Gp {gp}), S = {S} parents in register 0, {regs} registers; mean parents needed {need.mean():.2f}")
            print("  parents needed  " + " ".join(f"{p + 1:>6d}" for p in range(B)))
            print("  share of rows   " + " ".join(f"{100.0 * h / n:5.1f}%" for h in hist))
            lists = [[int(v) for v in s.split(",") if v] for s in args.stages] or [[S], [S - S // 4, S], [S - S // 4, S, S + 2], [S // 2, S - S // 4, S]]
            seen = set()
            for ends in lists:
                ends = sorted({e for e in ends if 0 < e < B}) + [B]
                if tuple(ends) in seen:
                    continue
                seen.add(tuple(ends))
                ev = evaluated(need, beam_cnt, ends)
                later = " ".join(f"{100.0 * np.mean(need > e):.1f}%" for e in ends[:-1])
                print(f"  stage ends {','.join(map(str, ends)):<12s} parents per query {ev.mean():.2f}   rows that run each later stage: {later}")
        beam_idx, beam_val, beam_cnt = new_idx, new_val, new_cnt


if __name__ == "__main__":
    main()
