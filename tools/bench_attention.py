#!/usr/bin/env python3
"""Timings of the fused attention statistics (cg_attn_stats) at the C4 geometry.

    python tools/bench_attention.py [--layers 12] [--batch 32] [--T 1024] [--sep 0.06] [--out result.json]

12 layers, 8 heads, d 512, T 1024, batch 32, bf16, random weights, tokens with 6 % separators.
Two figures, event-timed after two warm-ups, the median of 5 alternating rounds with [min, max]:
  1. cg_attn_stats for one layer with every output, and with head_acc only, beside its operation
     count (two QK^T passes over the visible (query, key) pairs) and its byte floor (q and k read
     once, the outputs and the received partials written once), and which of the two floors is
     the larger;
  2. the all-layer head statistics of one batch by the fused route, against the only route there was
     before it: Engine.attn_probs per layer (B H T^2 floats) plus torch reductions of the same 14
     statistics; the head means of the two routes are compared.
Not wired into bench.py.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "genomics-lm_amd"))

from codonlm_amd import _lib as L  # noqa: E402
from codonlm_amd import ops  # noqa: E402

DEV = "cuda"
SEP, PAD, V = 3, 0, 68
PEAK_BF16_FLOPS, PEAK_HBM_BPS = 2.5e15, 8.0e12


def alternating(fns, warmup=2, rounds=5):
    """{name: (median, min, max) seconds}: every round runs each function once, in order."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) * 1e-3)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}


def torch_head_sums(P, idx, cls, lo, keep):
    """fp64 (H, 14): the 14 statistics of cg_attn_stats from the materialised P (B, H, T, T), summed
    over the kept rows -- masked reductions of the full tensor, as a script reading it would."""
    B, H, T, _ = P.shape
    pos = torch.arange(T, device=P.device)
    dist = (pos[:, None] - pos[None, :])
    ent = -(torch.where(P > 0, P * torch.log(P.clamp_min(1e-38)), torch.zeros_like(P))).sum(-1)
    nvis = (pos[None, :] - lo + 1).to(torch.float32)
    norm = torch.where(nvis[:, None] > 1, ent / torch.log(nvis.clamp_min(2))[:, None], torch.zeros_like(ent))
    onehot = torch.nn.functional.one_hot(cls[idx].long().clamp_max(4), 5)[..., :4].to(P.dtype)      # (B, T, 4)
    mass = torch.matmul(P, onehot[:, None])                                                          # (B, H, T, 4)
    bins = [(P * ((dist >= a) & (dist <= b))).sum(-1) for a, b in ((0, 0), (1, 3), (4, 15), (16, 63), (64, T))]
    md = (P * dist).sum(-1)
    mx = P.amax(-1)
    first = P.gather(-1, lo[:, None, :, None].expand(B, H, T, 1))[..., 0]
    rows = torch.stack([ent, norm, *mass.unbind(-1), *bins, md, mx, first], -1)
    return (rows.double() * keep[:, None, :, None]).sum((0, 2))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--T", type=int, default=1024)
    ap.add_argument("--sep", type=float, default=0.06, help="fraction of separator tokens (0: the full causal triangle)")
    ap.add_argument("--out", type=Path)
    args = ap.parse_args(argv)
    from codonlm_amd import TinyGPT
    B, T, Ln, H, d = args.batch, args.T, args.layers, 8, 512
    hd = d // H
    torch.manual_seed(0)
    model = TinyGPT(V, T, n_layer=Ln, n_head=H, n_embd=d, dropout=0.0, sep_id=SEP, compute_dtype="bf16",
                    device=DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randint(4, V, (B, T), generator=g, device=DEV)
    x[torch.rand(x.shape, generator=g, device=DEV) < args.sep] = SEP
    cls = torch.tensor([0] * 4 + [3] * (V - 4), dtype=torch.uint8, device=DEV)
    cls[4 + 14], cls[4 + 48], cls[4 + 50], cls[4 + 56] = 1, 2, 2, 2          # ATG, TAA, TAG, TGA
    eng = model.engine
    with torch.no_grad():
        eng.forward(x, None, training=False, head=False)
    ws = ops.attn_stats_workspace(B, T, H, DEV)
    acc = torch.zeros(Ln, H, L.AS_NSTAT, dtype=torch.float64, device=DEV)
    n_rows = torch.zeros(1, dtype=torch.float64, device=DEV)
    r = eng.attn_stats(0, pad_id=PAD, tok_class=cls, workspace=ws)
    pairs = float(r.nvis.double().sum().item()) * H
    lo = (torch.arange(T, device=DEV)[None, :] - r.nvis + 1).long()
    keep = (x != PAD)
    flops = 2 * 2.0 * hd * pairs
    nqt = (T + 127) // 128
    floor_all = B * T * 2 * H * hd * 2 + B * H * T * (L.AS_NSTAT + 1 + 2 * nqt) * 4
    floor_acc = B * T * 2 * H * hd * 2
    res = {"device": torch.cuda.get_device_name(0), "B": B, "T": T, "layers": Ln, "H": H, "hd": hd, "sep": args.sep,
           "visible_pairs": pairs, "qk_flops_two_passes": flops}

    one = alternating({
        "all_outputs": lambda: eng.attn_stats(0, pad_id=PAD, tok_class=cls, head_acc=acc[0], n_rows=n_rows, workspace=ws),
        "head_acc_only": lambda: eng.attn_stats(0, pad_id=PAD, tok_class=cls, want=(), head_acc=acc[0], workspace=ws)})
    for k, floor in (("all_outputs", floor_all), ("head_acc_only", floor_acc)):
        s = one[k][0]
        t_flop, t_byte = flops / PEAK_BF16_FLOPS, floor / PEAK_HBM_BPS
        res[k] = {"s": s, "min_s": one[k][1], "max_s": one[k][2], "TFLOPs": flops / s / 1e12, "byte_floor": floor,
                  "floor_GBps": floor / s / 1e9, "flop_floor_s": t_flop, "byte_floor_s": t_byte,
                  "larger_floor": "bytes" if t_byte > t_flop else "flops"}
    print(json.dumps({k: res[k] for k in ("all_outputs", "head_acc_only")}), flush=True)

    def fused():
        acc.zero_()
        for layer in range(Ln):
            eng.attn_stats(layer, pad_id=PAD, tok_class=cls, want=(), head_acc=acc[layer], workspace=ws)
        return acc

    def materialised():
        return torch.stack([torch_head_sums(eng.attn_probs(layer), x, cls, lo, keep) for layer in range(Ln)])

    both = alternating({"fused": fused, "attn_probs_torch": materialised})
    a, b = fused().clone(), materialised()
    n = float(keep.sum().item())
    diff = ((a - b).abs() / n).amax((0, 1)).cpu().numpy()
    res["all_layers"] = {k: {"s": v[0], "min_s": v[1], "max_s": v[2]} for k, v in both.items()}
    res["all_layers"]["ratio"] = both["attn_probs_torch"][0] / both["fused"][0]
    res["all_layers"]["max_abs_diff_of_head_means"] = dict(zip(L.AS_STATS, (float(v) for v in diff)))
    print(json.dumps(res["all_layers"]), flush=True)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(json.dumps(res, indent=2) + "\n")
    return res


if __name__ == "__main__":
    main()
