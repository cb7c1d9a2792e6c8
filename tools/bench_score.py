#!/usr/bin/env python3
"""Two figures of batched scoring, measured on the GPU (not part of bench.py):

  kernel  cg_score_rows alone at rows = 32768, V = 68 (one C4 microbatch of 32 x 1024 tokens),
          device events around REPS calls queued behind a long matrix product (so the host's
          enqueue cost is hidden and the interval is device time), beside its byte floor
          rows * ldl * 4 B;
          once with the outputs score_batch asks for, once with the accumulators only (evaluate)
  batch   codonlm_amd.score.score_batch tokens/s on the C4 geometry (12 layers, 8 heads, d = 512,
          block 1024, random weights, bf16): N sequences of 1025 tokens, 32 per forward, host clock
          around calls that end in their read-back; beside the bare eval forward of the same
          batches (what `bench.py --path forward` times)

    python tools/bench_score.py            # prints one JSON line per figure
"""
from __future__ import annotations

import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "genomics-lm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROWS, V, T, B, NSEQ, REPS = 32768, 68, 1024, 32, 128, 100


def kernel_figure():
    from codonlm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    z = torch.randn(ROWS, V, device="cuda", generator=g) * 4
    y = torch.randint(1, V, (ROWS,), device="cuda", generator=g)
    ws = ops.score_workspace(ROWS, z.device)
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    blocker = torch.randn(8192, 8192, device="cuda")
    out = {"what": "cg_score_rows", "rows": ROWS, "V": V, "ldl": V, "floor_bytes": ROWS * V * 4}
    for name, kw in (("score_batch_outputs", dict(want=("logp", "rank", "seq_logp", "seq_count"), T=T)),
                     ("evaluate_accumulators", dict(want=(), acc=acc, smoothing=0.05))):
        for _ in range(5):
            ops.score_rows(z, y, workspace=ws, **kw)
        times = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(4):  # tens of ms of device work: the calls below queue up behind it
                torch.mm(blocker, blocker)
            a.record()
            for _ in range(REPS):
                ops.score_rows(z, y, workspace=ws, **kw)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / REPS)  # us per call: its two launches, back to back
        us = statistics.median(times)
        out[name] = {"us_per_call": round(us, 2), "min_us": round(min(times), 2), "max_us": round(max(times), 2),
                     "floor_gbs_equiv": round(ROWS * V * 4 / us / 1e3, 1)}
    print(json.dumps(out), flush=True)


def batch_figure():
    from codonlm_amd import TinyGPT
    from codonlm_amd import score as S
    torch.manual_seed(0)
    m = TinyGPT(V, T, n_layer=12, n_head=8, n_embd=512, dropout=0.0, compute_dtype="bf16", device="cuda").eval()
    rng = np.random.default_rng(0)
    seqs = [[1] + rng.integers(4, V, size=T - 1).tolist() + [2] for _ in range(NSEQ)]
    tokens = NSEQ * T
    xs = [torch.from_numpy(np.array([s[:-1] for s in seqs[i:i + B]])).cuda() for i in range(0, NSEQ, B)]

    def forward_only():
        with torch.no_grad():
            for x in xs:
                logits, _ = m(x)
        torch.cuda.synchronize()

    def scored():
        S.score_batch(m, seqs, batch_size=B)

    res = {"what": "score_batch vs eval forward", "config": "c4 bf16", "sequences": NSEQ, "tokens": tokens, "batch": B}
    for name, fn in (("forward", forward_only), ("score_batch", scored), ("forward_again", forward_only)):
        fn()
        fn()
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        res[name] = {"tok_per_s": round(tokens / statistics.median(ts)), "best_tok_per_s": round(tokens / min(ts)),
                     "worst_tok_per_s": round(tokens / max(ts))}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_score.py measures on the GPU; none is visible")
    kernel_figure()
    batch_figure()
