#!/usr/bin/env python3
"""Times of the termination-head correction steps on the MI355X at the C5 geometry (L10 H8 d384 T512,
5 termination classes, offset heads {2, 4, 8, 16, 32}, bf16 engine):

  1. full_step     a full training step: the trainer's objective (next + offsets + dense termination
                   loss), the whole backward, FusedAdamW;
  2. replay_fused  a replay microbatch through the new path: trunk-only forward, the fused
                   termination loss on sparse labels (31 labelled positions per row), accumulating backward;
  3. replay_dense  the same replay microbatch through the dense path: full forward, aux heads, torch
                   cross-entropy on the termination logits, backward through d_term_logits;
  4. frozen_step   a frozen-backbone step: the same objective with the fused termination loss, the
                   heads-only backward, FusedAdamW over the aux range.

    python tools/bench_replay.py [--batch 32] [--reps 10] [--rounds 5] [--dtype bf16]

``--reps`` calls between HIP events on the stream, ``--rounds`` rounds that alternate the order of the
four so that drift of the machine falls on all of them; the median round in ms per call, and the
spread.  Prints one JSON line.  Not part of bench.py.
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

OFFSETS = (2, 4, 8, 16, 32)
OFFSET_WEIGHTS = {k: 0.1 for k in OFFSETS}
T, WINDOW = 512, 30


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


def _model(dtype, frozen):
    import torch
    from codonlm_amd import TinyGPT
    from codonlm_amd.optim import FusedAdamW
    torch.manual_seed(0)
    m = TinyGPT(68, T, n_layer=10, n_head=8, n_embd=384, dropout=0.1, label_smoothing=0.05, termination_aux=True,
                termination_n_classes=5, multi_offset_targets=list(OFFSETS), compute_dtype=dtype, device="cuda")
    m.train()
    if frozen:
        for k, p in m.named_parameters():
            p.requires_grad_(k.startswith(("termination_head", "offset_projs")))
        m.zero_grad()
    return m, FusedAdamW(m, lr=3e-4, weight_decay=0.05, lr_embedding=1e-3)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="bf16")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_replay needs the MI355X")
    from codonlm_amd.replay import replay_labels
    from codonlm_amd.training import objectives as obj

    B = args.batch
    rng = np.random.default_rng(1)
    tok = rng.integers(4, 68, size=(B, T + 1))
    tok[:, 0] = 1
    tok[:, 200::97] = 2  # stop tokens so that the distance buckets are all populated
    x = torch.from_numpy(tok[:, :-1]).cuda()
    y = torch.from_numpy(tok[:, 1:]).cuda()
    rlab = np.full((B, T), -100, np.int64)
    for item in replay_labels(T, 5, WINDOW, (0, 3, 10, 30)):
        rlab[:, item["pos"]] = item["class"]
    rlabels = torch.from_numpy(rlab).cuda()
    cw = torch.tensor([2.0, 1.5, 1.0, 0.5, 0.25], device="cuda")
    full, opt_full = _model(args.dtype, frozen=False)
    frozen, opt_frozen = _model(args.dtype, frozen=True)

    def objective(m, fused):
        labels = obj.termination_distance_bucket_labels(y, stop_ids=(2,))
        if fused:
            _, loss, aux = m(x, y, return_aux=True, termination_labels=labels, termination_class_weights=cw)
            term = aux["termination_loss"]
        else:
            _, loss, aux = m(x, y, return_aux=True)
            term = obj.termination_aux_loss(aux["termination_logits"], labels, class_weights=cw)
        off, _, _ = obj.multi_offset_lm_loss(aux["offset_logits"], y, OFFSET_WEIGHTS, label_smoothing=0.05,
                                             return_counts=True)
        return loss + off + 0.1 * term

    def full_step():
        opt_full.zero_grad()
        objective(full, False).backward()
        opt_full.step()

    def frozen_step():
        opt_frozen.zero_grad()
        objective(frozen, True).backward()
        opt_frozen.step()

    def replay_fused():
        _, _, aux = full(x, return_aux=True, termination_labels=rlabels, termination_class_weights=cw, head=False)
        (0.1 * aux["termination_loss"]).backward()

    def replay_dense():
        _, _, aux = full(x, return_aux=True)
        (0.1 * obj.termination_aux_loss(aux["termination_logits"], rlabels, class_weights=cw)).backward()

    fns = (("full_step", full_step), ("replay_fused", replay_fused), ("replay_dense", replay_dense),
           ("frozen_step", frozen_step))
    for _, fn in fns:
        _timed(fn, 3)
    times = {name: [] for name, _ in fns}
    for i in range(args.rounds):
        for name, fn in fns if i % 2 == 0 else fns[::-1]:
            times[name].append(_timed(fn, args.reps))
    res = {"what": "replay_steps", "geometry": "C5 L10 H8 d384 T512", "batch": B, "dtype": args.dtype,
           "labelled_per_row": WINDOW + 1, "reps": args.reps, "rounds": args.rounds,
           **{name: _stats(v) for name, v in times.items()}}
    res["frozen_over_full"] = round(res["frozen_step"]["ms"] / res["full_step"]["ms"], 3)
    res["fused_over_dense"] = round(res["replay_fused"]["ms"] / res["replay_dense"]["ms"], 3)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
