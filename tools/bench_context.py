#!/usr/bin/env python3
"""Timings of the context-diagnostic kernels against a torch restatement on the same device.

    python tools/bench_context.py [--tokens 10000000 100000000] [--V 68] [--T 1024] [--out result.json]

Per token count: cg_ngram_count, cg_ngram_nll and cg_diag_rows (ns per token, achieved bytes/s
against the read floor of 16 B/token for x and y plus 4 V B/token of logits), the integer-atomic
rate of the counting kernel (one 64-bit global add per token), and the torch restatement of each:
bincount counting, a gather-based nll, and softmax + a masked reduction per calibration bin.  Then the wall
time of a full context.diagnose at the reference's seven default windows on a synthetic model.
Warm-up launches first, then the median of ``--repeats`` event-timed runs.  Not wired into bench.py.
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "genomics-lm_amd"))

from codonlm_amd import context as X  # noqa: E402
from codonlm_amd import ops  # noqa: E402

DEV = "cuda"
SEP, PAD = 3, 0
DIAG_CHUNK = 10_000_000  # tokens of logits held at once (4 V bytes each)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)) * 1e-3


def tokens_on_device(n, T, V, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    tok = torch.randint(4, V, (n // T, T + 1), generator=g, device=DEV)
    tok[torch.rand(tok.shape, generator=g, device=DEV) < 0.06] = SEP
    return tok[:, :-1].contiguous(), tok[:, 1:].contiguous()


# ------------------------------------------------------------------ the torch restatement
def torch_count(x, y, V):
    B, T = x.shape
    keep = y != PAD
    reset = (x == SEP)
    reset[:, 0] = True
    p2 = torch.where(reset, torch.full_like(x, PAD), torch.roll(x, 1, 1))
    ctx = (p2 * V + x)[keep]
    t = y[keep]
    uni = torch.bincount(t, minlength=V)
    bi = torch.bincount(x[keep] * V + t, minlength=V * V)
    tri = torch.bincount(ctx * V + t, minlength=V ** 3)
    return uni, bi.view(V, V), tri.view(V, V, V)


def torch_nll(x, y, uni, bi, tri, V, alpha):
    keep = y != PAD
    reset = (x == SEP)
    reset[:, 0] = True
    p2 = torch.where(reset, torch.full_like(x, PAD), torch.roll(x, 1, 1))
    den0 = alpha * (V - 1)
    tb, tt = bi[:, 1:].sum(-1), tri[:, :, 1:].sum(-1)
    l_uni = -torch.log((uni[y].double() + alpha) / (uni[1:].sum().double() + den0))
    l_bi = -torch.log((bi[x, y].double() + alpha) / (tb[x].double() + den0))
    seen = tt[p2, x] > 0
    ct = torch.where(seen, tri[p2, x, y], bi[x, y]).double()
    ctot = torch.where(seen, tt[p2, x], tb[x]).double()
    l_tri = -torch.log((ct + alpha) / (ctot + den0))
    return torch.stack([(l * keep).sum() for l in (l_uni, l_bi, l_tri)]), keep.sum()


def torch_diag(logits, y, n_bins=15):
    """What cg_diag_rows accumulates, in torch ops on the same device: the calibration sums of every
    bin (count, confidence, hits; a masked reduction per bin, with no host read), the Brier sum and
    the nll sum of the PAD-free targets."""
    t = y.reshape(-1)
    live = t != PAD
    logp = torch.log_softmax(logits[live], -1)
    t = t[live]
    p = logp.exp()
    top, guess = p.max(-1)
    hit = (guess == t).to(p.dtype)
    edges = torch.linspace(0, 1, n_bins + 1, device=p.device)
    calib = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        inside = ((top > lo) & (top <= hi)).to(p.dtype)
        calib.append(torch.stack([inside.sum(), (inside * top).sum(), (inside * hit).sum()]))
    p_true = p.gather(1, t[:, None]).squeeze(1)
    brier = ((p * p).sum(-1) - 2.0 * p_true + 1.0).sum()
    nll = -logp.gather(1, t[:, None]).sum()
    return torch.stack(calib), brier, nll


# ------------------------------------------------------------------ one token count
def bench_tokens(n, T, V, warmup, repeats):
    x, y = tokens_on_device(n, T, V, seed=n % 1000)
    n = x.numel()
    out = {"tokens": n, "T": T, "V": V}
    tables = ops.NgramTables(V, DEV, PAD, (SEP,))
    s = timed(lambda: ops.ngram_count(tables, x, y), warmup, repeats)
    out["ngram_count"] = {"s": s, "ns_per_token": s / n * 1e9, "read_GBps": 16 * n / s / 1e9,
                          "global_int64_atomics_per_s": n / s}
    s = timed(lambda: torch_count(x, y, V), warmup, repeats)
    out["torch_count"] = {"s": s, "ns_per_token": s / n * 1e9}
    tables = ops.ngram_totals(ops.ngram_count(ops.NgramTables(V, DEV, PAD, (SEP,)), x, y))
    acc = torch.zeros(5, dtype=torch.float64, device=DEV)
    s = timed(lambda: ops.ngram_nll(tables, x, y, 0.01, acc=acc, want=("row_sums", "row_count")), warmup, repeats)
    out["ngram_nll"] = {"s": s, "ns_per_token": s / n * 1e9, "read_GBps": 16 * n / s / 1e9}
    s = timed(lambda: torch_nll(x, y, tables.uni, tables.bi, tables.tri, V, 0.01), warmup, repeats)
    out["torch_nll"] = {"s": s, "ns_per_token": s / n * 1e9}
    # the logits pass, in chunks of DIAG_CHUNK tokens over one logits buffer
    rows = min(n, DIAG_CHUNK) // T
    logits = torch.randn(rows * T, V, device=DEV) * 2.0
    cls = torch.from_numpy(np.r_[np.zeros(4, np.uint8), np.full(V - 4, 3, np.uint8)]).to(DEV)
    edges = torch.linspace(0, 1, 16).to(DEV)
    slices = torch.zeros(13, 2, dtype=torch.float64, device=DEV)
    calib = torch.zeros(15, 3, dtype=torch.float64, device=DEV)
    brier = torch.zeros(2, dtype=torch.float64, device=DEV)
    ws = ops.diag_workspace(rows, DEV)
    chunks = [(a, min(a + rows, x.shape[0])) for a in range(0, x.shape[0], rows)]

    def diag():
        for a, b in chunks:
            ops.diag_rows(logits[:(b - a) * T], x[a:b], y[a:b], V=V, sep_id=SEP, tok_class=cls, edges=edges, slices=slices,
                          calib=calib, brier_acc=brier, want=("row_nll", "row_count"), workspace=ws)

    def diag_torch():
        for a, b in chunks:
            torch_diag(logits[:(b - a) * T], y[a:b])
    s = timed(diag, warmup, repeats)
    out["diag_rows"] = {"s": s, "ns_per_token": s / n * 1e9, "read_GBps": (16 + 4 * V) * n / s / 1e9}
    s = timed(diag_torch, warmup, repeats)
    out["torch_diag"] = {"s": s, "ns_per_token": s / n * 1e9}
    for k, t in (("ngram_count", "torch_count"), ("ngram_nll", "torch_nll"), ("diag_rows", "torch_diag")):
        out[k]["speedup_vs_torch"] = out[t]["s"] / out[k]["s"]
    return out


def bench_diagnose(V):
    """Wall time of context.diagnose at the seven default windows: a 4-layer d = 256 model, block 256,
    10^7 training tokens and 2^20 test tokens in batches of 64."""
    from codonlm_amd import TinyGPT
    from codonlm_amd.data_loading import DeviceBatchLoader, DeviceCodonDataset
    T = 256
    itos = ["<PAD>", "<BOS_CDS>", "<EOS_CDS>", "<SEP>"] + [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
    torch.manual_seed(0)
    model = TinyGPT(V, T, n_layer=4, n_head=4, n_embd=256, dropout=0.0, sep_id=SEP, device=DEV).eval()
    with tempfile.TemporaryDirectory() as tmp:
        loaders = []
        for name, n, bs in (("train", 10_000_000, 1024), ("test", 1 << 20, 64)):
            x, y = tokens_on_device(n, T, V, seed=len(name))
            np.savez(Path(tmp) / f"{name}.npz", X=x.cpu().numpy().astype(np.int32), Y=y.cpu().numpy().astype(np.int32))
            ds = DeviceCodonDataset(Path(tmp) / f"{name}.npz", device=DEV)
            loaders.append(DeviceBatchLoader(ds, bs, shuffle=False, drop_remainder=False))
        wall = []
        for _ in range(2):  # the first run warms the allocator and the kernels
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            X.diagnose(model, loaders[0], loaders[1], itos[:V], log=lambda s: None)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
    return {"windows": X.DEFAULT_WINDOWS, "train_tokens": 10_000_000, "test_tokens": 1 << 20, "batch": 64,
            "first_s": wall[0], "second_s": wall[1]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--V", type=int, default=68)
    ap.add_argument("--T", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-diagnose", action="store_true")
    ap.add_argument("--out", type=Path)
    args = ap.parse_args(argv)
    result = {"device": torch.cuda.get_device_name(0), "runs": []}
    for n in args.tokens:
        result["runs"].append(bench_tokens(n, args.T, args.V, args.warmup, args.repeats))
        print(json.dumps(result["runs"][-1]), flush=True)
    if not args.no_diagnose:
        result["diagnose"] = bench_diagnose(args.V)
        print(json.dumps(result["diagnose"]), flush=True)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(json.dumps(result, indent=2) + "\n")
    return result


if __name__ == "__main__":
    main()
