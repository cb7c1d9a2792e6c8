#!/usr/bin/env python3
"""Times of the structural regression probes on the MI355X.

    python tools/bench_probe.py                 # the Gram kernel at the C4 batch, then the CLI end to end
    python tools/bench_probe.py --no-cli --rows 8192

Kernel: cg_gram_accum at rows = 32 x 1024 (a C4 batch), d = 512, m = 14, G = 5, for fp32 and bf16
hidden states, beside what one would write in torch without it -- per fold
``Z[rows of the fold].double().T @ Z[...].double()`` on the same rows, once with building
Z = [h | y | 1] and gathering the fold's rows inside the timed region (``torch``) and once with
both done beforehand (``torch_matmul``).  ``--reps`` calls between HIP events, ``--rounds`` rounds
that alternate the candidates; the median round in ms per call and the spread.  ``tflops`` counts
the 2 n P^2 operations of the full (not the half) Gram.

End to end: a run directory with a random-weight 12-layer d = 512 model of block_size 512 and 1000
sequences of 512 tokens is written to a temporary directory; ``probe_structural_regression
--sample_size 150 --no_cache`` on it (wall clock around a device synchronise, checkpoint loading
and file writing included, and the library call alone), beside the same 150 sequences done the
reference's way through this package's model: one forward per sequence, hidden states copied to
the host, targets in Python, and per fold one multi-target fp64 normal-equation solve in numpy on
the N x d matrix (a cheaper host solve than the reference's 84 single-target sklearn fits).
Prints one JSON line per measurement.  Not part of bench.py.
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "genomics-lm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


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


def bench_gram(rows, d, m, G, dtype, reps, rounds):
    import torch
    from codonlm_amd import ops
    from codonlm_amd.structure_probe import kfold_assign
    g = torch.Generator(device="cuda").manual_seed(rows + d)
    h = (torch.randn(rows, d, device="cuda", generator=g) * 1.5).to(torch.bfloat16 if dtype == "bf16" else torch.float32)
    y = torch.randn(rows, m, device="cuda", generator=g)
    grp = torch.from_numpy(kfold_assign(rows, G)).cuda()
    P = d + m + 1
    gram = torch.empty(G, P, P, dtype=torch.float64, device="cuda")
    ws = ops.gram_workspace(rows, d, m, G, "cuda")
    ones = torch.ones(rows, 1, dtype=torch.float64, device="cuda")
    lists = [torch.nonzero(grp == f).reshape(-1) for f in range(G)]
    Zpre = [torch.cat([h.double(), y.double(), ones], 1)[ix] for ix in lists]

    def native():
        return ops.gram_accum(h, y, grp, G, gram, workspace=ws)

    def restated():
        Z = torch.cat([h.double(), y.double(), ones], 1)
        return torch.stack([Z[ix].T @ Z[ix] for ix in lists])

    def matmul_only():
        return torch.stack([z.T @ z for z in Zpre])

    a, b = native().clone(), restated()
    rel = float(((a - b).abs() / (b.abs() + 1.0)).max())
    for fn in (native, restated, matmul_only):
        _timed(fn, 2)
    tn, tt, tm = [], [], []
    for i in range(rounds):
        order = ((native, tn), (restated, tt), (matmul_only, tm))
        for fn, out in order if i % 2 == 0 else order[::-1]:
            out.append(_timed(fn, reps))
    res = {"what": "gram_accum", "rows": rows, "d": d, "m": m, "G": G, "dtype": dtype, "reps": reps, "rounds": rounds,
           "native": _stats(tn), "torch": _stats(tt), "torch_matmul": _stats(tm), "max_rel_diff": rel,
           "gflop_full": round(2.0 * rows * P * P / 1e9, 2)}
    res["native_tflops"] = round(res["gflop_full"] / res["native"]["ms"], 2)
    res["torch_matmul_tflops"] = round(res["gflop_full"] / res["torch_matmul"]["ms"], 2)
    res["native_over_torch"] = round(res["native"]["ms"] / res["torch"]["ms"], 3)
    res["native_over_torch_matmul"] = round(res["native"]["ms"] / res["torch_matmul"]["ms"], 3)
    print(json.dumps(res), flush=True)
    return res


def _reference_way(model, ids, itos):
    """One forward per sequence, host copies, Python targets, numpy normal equations per fold."""
    import numpy as np
    import torch
    from codonlm_amd.structure_probe import NAMES, kfold_assign
    sys.path.insert(0, str(ROOT / "tests"))
    import probe_restatement as R
    Xs, Ys = [], []
    for row in ids:
        toks = [int(t) for t in row if 0 < t < len(itos)]
        if len(toks) < 10:
            continue
        x = torch.tensor([toks], device="cuda")
        for which, t in model.iter_hidden_states(x):
            if which == int(model.n_layer):
                hs = t[0].float().cpu().numpy()
        y, valid = R.shape_targets(np.asarray([toks]), itos)
        Xs.append(hs[valid.astype(bool)])
        Ys.append(y[valid.astype(bool)])
    X, Y = np.concatenate(Xs).astype(np.float64), np.concatenate(Ys).astype(np.float64)
    fold = kfold_assign(len(X))
    r2 = np.zeros((5, len(NAMES)))
    for f in range(6):
        tr = fold != f
        mu, yb = X[tr].mean(0), Y[tr].mean(0)
        Xc = X[tr] - mu
        W = np.linalg.solve(Xc.T @ Xc + np.eye(X.shape[1]), Xc.T @ (Y[tr] - yb))
        if f < 5:
            te = fold == f
            res = Y[te] - ((X[te] - mu) @ W + yb)
            tot = ((Y[te] - Y[te].mean(0)) ** 2).sum(0)
            r2[f] = 1.0 - (res ** 2).sum(0) / np.where(tot > 0, tot, 1.0)
    return len(X), r2.mean(0)


def bench_cli(n_seq, sample, dtype):
    import numpy as np
    import torch
    from codonlm_amd import TinyGPT
    from codonlm_amd import probe_structural_regression as C
    from codonlm_amd import structure_probe as SP
    from codonlm_amd.score_mutations import load_model, load_vocab

    def clock():
        torch.cuda.synchronize()
        return time.perf_counter()

    with tempfile.TemporaryDirectory() as tmp:
        rd = Path(tmp) / "runs" / "bench"
        (rd / "checkpoints").mkdir(parents=True)
        itos = SP.default_vocab()
        (rd / "itos.txt").write_text("\n".join(itos) + "\n")
        torch.manual_seed(0)
        m = TinyGPT(68, 512, n_layer=12, n_head=8, n_embd=512, dropout=0.0, device="cpu")
        cfg = {"vocab_size": 68, "block_size": 512, "n_layer": 12, "n_head": 8, "n_embd": 512, "dropout": 0.0,
               "tie_embeddings": True}
        torch.save({"model": m.state_dict(), "cfg": cfg}, rd / "checkpoints" / "best.pt")
        rng = np.random.default_rng(1)
        X = rng.integers(4, 68, size=(n_seq, 512)).astype(np.int32)
        X[:, 0] = 1
        for b in range(n_seq):
            n = int(rng.integers(200, 512))
            X[b, n - 1] = 2
            X[b, n:] = 0
        np.savez(Path(tmp) / "test.npz", X=X)
        argv = ["--run_dir", str(rd), "--test_npz", str(Path(tmp) / "test.npz"), "--sample_size", str(sample),
                "--no_cache", "--dtype", dtype]
        C.main(argv)  # code objects, allocator and file cache warm
        t0 = clock()
        metrics = C.main(argv)
        t1 = clock()
        model, _ = load_model(None, rd, dtype)
        ids = C.load_sequences(Path(tmp) / "test.npz", sample, 512)
        SP.probe(model, ids[:8])
        t2 = clock()
        lib_metrics, probes = SP.probe(model, ids)
        t3 = clock()
        _reference_way(model, ids[:4], load_vocab(None, rd))
        t4 = clock()
        n_ref, r2_ref = _reference_way(model, ids, load_vocab(None, rd))
        t5 = clock()
        res = {"what": "probe_structural_regression", "sequences": sample, "T": 512, "dtype": dtype,
               "rows": int(probes["n_rows"]), "cli_s": round(t1 - t0, 3), "probe_s": round(t3 - t2, 3),
               "reference_way_s": round(t5 - t4, 3), "reference_way_rows": n_ref,
               "avg_r2": metrics["regression_probe.avg_r2"], "reference_way_avg_r2": float(r2_ref.mean())}
        print(json.dumps(res), flush=True)
        return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=32 * 1024)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--sample_size", type=int, default=150)
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_probe needs the MI355X")
    if not args.no_kernel:
        for dtype in ("fp32", "bf16"):
            bench_gram(args.rows, args.d, 14, 5, dtype, args.reps, args.rounds)
    if not args.no_cli:
        bench_cli(args.sequences, args.sample_size, args.dtype)


if __name__ == "__main__":
    main()
