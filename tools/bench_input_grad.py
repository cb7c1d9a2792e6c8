#!/usr/bin/env python3
"""Time of the input-gradient-only backward (Engine.input_grad, cg_model_input_grad) beside the
full backward (Engine.backward) after the same eval forward, on the C4 geometry with random
weights: 12 layers, 8 heads, d = 512, T = 1024, B = 32, bf16.

    python tools/bench_input_grad.py
    python tools/bench_input_grad.py --dtype fp32 --batch 8 --rounds 5

Both run from the loss seed (the fused cross-entropy's dlogits of the forward) on the same inputs.
Each round times ``--reps`` calls of one, then of the other, between HIP events on the stream; the
rounds alternate the two so that drift of the machine falls on both.  Prints one JSON line: the
median round of each in ms per call, the spread, and their ratio.  Not part of bench.py.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "genomics-lm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GEOM = dict(n_layer=12, n_head=8, n_embd=512)
V, BLOCK = 68, 1024


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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=BLOCK)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args(argv)
    import torch
    from codonlm_amd import TinyGPT
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_grad needs the MI355X")
    torch.manual_seed(0)
    m = TinyGPT(V, BLOCK, dropout=0.0, compute_dtype=args.dtype, device="cuda", **GEOM).eval()
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(4, V, (args.batch, args.seq + 1), generator=g).cuda()
    x, y = tok[:, :-1].contiguous(), tok[:, 1:].contiguous()
    eng = m.engine
    eng.forward(x, y, training=False)
    eng.set_head_grads(1.0)

    def full():
        eng.backward(accumulate=False)

    def input_only():
        eng.input_grad()

    for fn in (full, input_only):  # every shape of the timed window, once
        _timed(fn, 2)
    t_full, t_in = [], []
    for r in range(args.rounds):
        for fn, out in ((full, t_full), (input_only, t_in)) if r % 2 == 0 else ((input_only, t_in), (full, t_full)):
            out.append(_timed(fn, args.reps))
    res = {"geometry": dict(GEOM, V=V, T=args.seq, B=args.batch, dtype=args.dtype), "reps": args.reps,
           "rounds": args.rounds, "full_backward": _stats(t_full), "input_grad": _stats(t_in)}
    res["input_grad_over_full"] = round(res["input_grad"]["ms"] / res["full_backward"]["ms"], 4)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
