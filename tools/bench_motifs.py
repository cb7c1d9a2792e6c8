#!/usr/bin/env python3
"""Times of motif mining on the MI355X: one cg_kmeans_step beside the torch restatement a user would
otherwise write (torch.cdist + argmin + index_add_), and codonlm_amd.motifs.mine end to end.

    python tools/bench_motifs.py                       # the four (d, k) points at n = 1 M, then mine
    python tools/bench_motifs.py --n 200000 --no-mine

Step: random fp32 points and centres, ``--reps`` calls between HIP events on the stream, ``--rounds``
rounds that alternate the native step and the torch restatement so that drift of the machine falls
on both; the median round in ms per call, and the spread.  ``assign`` is the native step without
the statistics (labels and dist2 only).  Mine: the reference's default scale (src/codonlm/
mine_motifs.py: 20 000 sequences of 256 tokens, window 9, stride 1, 100 clusters, a 2-layer d = 128
model with random weights), wall clock around a device synchronise, per stage.  Prints one JSON
line per measurement.  Not part of bench.py.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "genomics-lm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

POINTS = ((50, 10), (50, 100), (256, 10), (256, 100))


def _timed(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _stats(ms):
    ms = sorted(ms)
    return {"ms": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def bench_step(n, d, k, reps, rounds):
    import torch
    from codonlm_amd import _lib as L
    from codonlm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(d * 1000 + k)
    X = torch.randn(n, d, device="cuda", generator=g) * 1.5
    Cn = X[torch.randperm(n, device="cuda", generator=g)[:k]].clone()
    ws = torch.empty(int(L.lib.cg_kmeans_workspace(n, d, k)), dtype=torch.uint8, device="cuda")

    def native():
        return ops.kmeans_step(X, Cn, workspace=ws)

    def assign():
        return ops.kmeans_step(X, Cn, want_stats=False, want_inertia=False, workspace=ws)

    def restated():
        dist, lab = torch.cdist(X, Cn).min(1)
        sums = torch.zeros(k, d, device="cuda").index_add_(0, lab, X)
        return lab, dist, sums, torch.bincount(lab, minlength=k)

    r, t = native(), restated()
    same = float((r.labels.long() == t[0]).float().mean())
    for fn in (native, assign, restated):
        _timed(fn, 2)
    tn, ta, tt = [], [], []
    for i in range(rounds):
        order = ((native, tn), (assign, ta), (restated, tt))
        for fn, out in order if i % 2 == 0 else order[::-1]:
            out.append(_timed(fn, reps))
    res = {"what": "kmeans_step", "n": n, "d": d, "k": k, "reps": reps, "rounds": rounds, "native": _stats(tn),
           "assign": _stats(ta), "torch": _stats(tt), "labels_equal_share": round(same, 6),
           "x_gbytes": round(n * d * 4 / 1e9, 3), "gflop_xc": round(2.0 * n * d * k / 1e9, 2)}
    res["native_over_torch"] = round(res["native"]["ms"] / res["torch"]["ms"], 3)
    print(json.dumps(res), flush=True)
    return res


def bench_mine(n_seq, pca, dtype):
    import numpy as np
    import torch
    from codonlm_amd import TinyGPT
    from codonlm_amd import motifs as M
    torch.manual_seed(0)
    m = TinyGPT(68, 256, n_layer=2, n_head=4, n_embd=128, dropout=0.0, compute_dtype=dtype, device="cuda").eval()
    ids = np.random.default_rng(1).integers(4, 68, size=(n_seq, 256)).astype(np.int64)
    ids[:, 0] = 1

    def clock():
        torch.cuda.synchronize()
        return time.perf_counter()

    M.window_embeddings(m, ids[:512], 9, 1, exclude_ids=(0, 1, 2, 3))  # code objects and allocator warm
    t0 = clock()
    emb, meta = M.window_embeddings(m, ids, 9, 1, exclude_ids=(0, 1, 2, 3))
    t1 = clock()
    X = M.pca_project(emb, pca)[0].contiguous() if pca else emb
    t2 = clock()
    labels, centers, inertia, n_iter = M.kmeans(X, 100, seed=42)
    t3 = clock()
    res = {"what": "mine", "sequences": n_seq, "T": 256, "window": 9, "stride": 1, "dtype": dtype, "pca": pca,
           "windows": int(emb.shape[0]), "d": int(X.shape[1]), "clusters": 100, "n_iter": n_iter,
           "embed_s": round(t1 - t0, 3), "pca_s": round(t2 - t1, 3), "kmeans_s": round(t3 - t2, 3),
           "total_s": round(t3 - t0, 3), "inertia": inertia}
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sequences", type=int, default=20000)
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--no-mine", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_motifs needs the MI355X")
    if not args.no_step:
        for d, k in POINTS:
            bench_step(args.n, d, k, args.reps, args.rounds)
    if not args.no_mine:
        for pca in (0, 50):
            bench_mine(args.sequences, pca, args.dtype)


if __name__ == "__main__":
    main()
