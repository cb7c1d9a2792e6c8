#!/usr/bin/env python3
"""Throughput of batched on-device generation (codonlm_amd.generate.generate_batch) beside the
single-sequence path it extends (a loop of query_model.generate), on the C4 geometry with random
weights: 12 layers, 8 heads, d = 512, block 1024; an 8-token prompt, 256 new tokens per sequence
(the stop rules are off, so every sequence runs the full length).

    python tools/bench_generate.py                  # every point, one child process each
    python tools/bench_generate.py --point gen:bf16:64

Points: gen:<dtype>:<B> (the batched path), parent:<dtype> (query_model.generate, B = 1) and
attn:<dtype> (cg_attn_decode_ragged beside cg_attn_decode alone, B = 64, pos = 512).  Each point
runs in its own process under its own time limit and prints one JSON line; the driver stops at
the first point that fails.  Times are host clocks around work that ends in a device synchronise.
Not part of bench.py.
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "genomics-lm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GEOM = dict(n_layer=12, n_head=8, n_embd=512)
V, BLOCK, PROMPT, NEW, REPS = 68, 1024, 8, 256, 5
ITOS = ["<PAD>", "<BOS_CDS>", "<EOS_CDS>", "<SEP>"] + [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
STOI = {t: i for i, t in enumerate(ITOS)}


def _model(dtype):
    import torch
    from codonlm_amd import TinyGPT
    torch.manual_seed(0)
    m = TinyGPT(V, BLOCK, dropout=0.0, compute_dtype=dtype, device="cuda", **GEOM)
    m.eval()
    return m


def _stats(rates):
    rates = sorted(rates)
    return {"tokens_per_s": rates[len(rates) // 2], "min": rates[0], "max": rates[-1], "reps": len(rates)}


def point_gen(dtype, B):
    import torch
    from codonlm_amd.generate import generate_batch
    m = _model(dtype)
    ctx = [[1] + [4 + (7 * b + i) % 61 for i in range(PROMPT - 1)] for b in range(B)]
    rates = []
    for rep in range(REPS + 1):  # the first run warms every shape up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = generate_batch(m, ctx, STOI, ITOS, seed=rep, max_tokens=NEW, stop_on_eos=False, stop_on_bio_stop=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert all(rec["n_tokens"] == NEW for _, rec in res)
        if rep:
            rates.append(B * NEW / dt)
    return dict(point=f"gen:{dtype}:{B}", **_stats(rates))


def point_parent(dtype):
    import torch
    from codonlm_amd import query_model as Q
    m = _model(dtype)
    dev = torch.device("cuda")
    ctx = [1] + [4 + i % 61 for i in range(PROMPT - 1)]
    rates = []
    for rep in range(REPS + 1):
        torch.manual_seed(rep)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids = Q.generate(m, dev, ctx, max_new=NEW)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert len(ids) == PROMPT + NEW
        if rep:
            rates.append(NEW / dt)
    return dict(point=f"parent:{dtype}", **_stats(rates))


def point_attn(dtype):
    """One layer's decode attention alone at B = 64, pos = 512 (H = KV = 8, hd = 64): microseconds per
    launch, the median of REPS windows of 200 launches, old kernel and ragged kernel alternating."""
    import torch
    from codonlm_amd import ops
    B, H, hd, pos, tmax, n = 64, 8, 64, 512, BLOCK, 200
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(0)
    q = torch.randn(B, 3 * H * hd, generator=g).to(td).cuda()
    cache = torch.randn(B, tmax, 2 * H * hd, generator=g).to(td).cuda()
    posv = torch.full((B,), pos, dtype=torch.int32, device="cuda")
    y = torch.zeros(B, H * hd, dtype=td, device="cuda")
    runs = {"cg_attn_decode": lambda: ops.attn_decode(q, cache, pos, H, H, hd),
            "cg_attn_decode_ragged": lambda: ops.attn_decode_ragged(q, cache, posv, H, H, hd, out=y)}
    us = {k: [] for k in runs}
    for rep in range(REPS + 1):
        for name, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            if rep:
                us[name].append((time.perf_counter() - t0) / n * 1e6)
    out = {"point": f"attn:{dtype}"}
    for name, v in us.items():
        v.sort()
        out[name] = {"us_per_launch": v[len(v) // 2], "min": v[0], "max": v[-1]}
    return out


def run_point(spec):
    kind, *rest = spec.split(":")
    if kind == "gen":
        return point_gen(rest[0], int(rest[1]))
    if kind == "parent":
        return point_parent(rest[0])
    if kind == "attn":
        return point_attn(rest[0])
    raise SystemExit(f"unknown point {spec!r}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--point", help="run one point in this process")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per point")
    ap.add_argument("--out", help="also write the JSON lines to this file")
    args = ap.parse_args(argv)
    if args.point:
        print(json.dumps(run_point(args.point)), flush=True)
        return
    points = [f"{k}:{dt}" for dt in ("fp32", "bf16") for k in ("parent", "gen")]
    specs = []
    for p in points:
        specs += [f"{p}:{B}" for B in (1, 8, 64)] if p.startswith("gen") else [p]
    specs += ["attn:fp32", "attn:bf16"]
    lines = []
    for spec in specs:
        try:
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--point", spec], capture_output=True,
                               text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"{spec}: no result within {args.timeout} s; stopping", flush=True)
            raise SystemExit(124)
        if r.returncode != 0:
            print(f"{spec}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
            raise SystemExit(r.returncode if r.returncode > 0 else 1)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
