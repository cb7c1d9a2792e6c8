#!/usr/bin/env python3
"""Attention head statistics of a run on the MI355X (the numbers behind the reference's
scripts/conference_attention.py and scripts/analyze_attention.py; no plotting).

    python -m codonlm_amd.analyze_attention --run_dir runs/<ID>
    python -m codonlm_amd.analyze_attention --run_dir runs/<ID> --npz val.npz --n_seqs 512 --maps 4

The sequences are the rows of ``X`` in ``--npz`` or, without it, of ``val_inputs`` in the run's
``artifacts.npz``; ``--n_seqs`` takes the first N.  Every non-PAD position of every sequence counts:
the statistics come from the fused cg_attn_stats pass (attention.head_stats), which writes no
attention tensor.  Writes
  ``<run>/tables/attention_heads.csv``     one line per layer and head with every mean statistic,
  ``<run>/attention/head_stats.npz``       ``sums`` (L, H, 14), ``n_rows``, ``means``, ``stats`` (the
                                           names) and ``reference_row0`` (L, H, 3): the reference's
                                           entropy / start / stop triple of the first sequence,
  ``<run>/attention/attention_report.md``  the specialist tables,
and with ``--maps K`` ``<run>/attention/attn_maps.npz`` with ``attn`` (L, K, H, T, T) fp32 and
``val_inputs`` of the first K sequences cropped to ``--max_tokens``: the layout the reference's
plotting scripts load.
"""
from __future__ import annotations

import argparse
import csv
from pathlib import Path
from typing import List

import numpy as np

from . import attention as A
from .context import markdown_table


def load_inputs(run_dir: Path, npz, n_seqs) -> np.ndarray:
    """int64 [N][T]: ``X`` of --npz, or ``val_inputs`` of the run's artifacts.npz; the first n_seqs rows."""
    path, key = (Path(npz), "X") if npz is not None else (run_dir / "artifacts.npz", "val_inputs")
    if not path.exists():
        raise FileNotFoundError(f"{path.name} missing: {path}")
    with np.load(path, allow_pickle=False) as data:
        if key not in data.files:
            raise ValueError(f"{path} holds no '{key}' array")
        x = np.asarray(data[key])
    if x.ndim != 2 or x.size == 0:
        raise ValueError(f"'{key}' of {path} must be a non-empty (N, T) array")
    return x[:n_seqs].astype(np.int64) if n_seqs is not None else x.astype(np.int64)


def csv_rows(stats: A.HeadStats) -> List[list]:
    """Header and one row per (layer, head): the mean of every statistic as ``%.6f``."""
    means = stats.means
    rows = [["layer", "head"] + list(A.STATS)]
    for l in range(means.shape[0]):
        for h in range(means.shape[1]):
            rows.append([l, h] + [f"{float(v):.6f}" for v in means[l, h]])
    return rows


def report_markdown(stats: A.HeadStats, k: int = 8) -> str:
    """The specialist tables: one section per ranking of attention.specialists."""
    lines = ["# Attention Head Analysis", "",
             f"{stats.sums.shape[0]} layers x {stats.sums.shape[1]} heads, {stats.n_rows} query positions.", ""]
    stat_of = {name: stat for name, stat, _ in A.SPECIALIST_KINDS}
    for name, ranked in A.specialists(stats, k).items():
        lines += [f"## {name} (mean {stat_of[name]})", ""]
        lines += markdown_table(("Rank", "Layer", "Head", "Value"), "| ---: | ---: | ---: | ---: |",
                                ((str(i + 1), str(l), str(h), f"{v:.6f}") for i, (l, h, v) in enumerate(ranked)))
        lines.append("")
    return "\n".join(lines[:-1]) + "\n"


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Per-head attention statistics of a run.")
    ap.add_argument("--run_dir", required=True, help="run directory: checkpoints/best.pt, itos.txt, artifacts.npz")
    ap.add_argument("--npz", default=None, help="file with the token array X (default: artifacts.npz val_inputs)")
    ap.add_argument("--n_seqs", type=int, default=None, help="use the first N sequences (default: all)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--window", type=int, default=None, help="attention window (default: the full context)")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="fp32")
    ap.add_argument("--maps", type=int, default=0, help="also save the attention maps of the first K sequences")
    ap.add_argument("--max_tokens", type=int, default=60, help="crop of the saved maps")
    return ap


def check_args(args) -> None:
    """The argument checks that need no device."""
    if args.n_seqs is not None and args.n_seqs < 1:
        raise ValueError("--n_seqs must be at least 1")
    if args.batch < 1:
        raise ValueError("--batch must be at least 1")
    if args.window is not None and args.window < 1:
        raise ValueError("--window must be at least 1")
    if args.maps < 0:
        raise ValueError("--maps cannot be negative")
    if args.max_tokens < 1:
        raise ValueError("--max_tokens must be at least 1")


def write_outputs(run_dir: Path, stats: A.HeadStats, triple: np.ndarray) -> dict:
    out = {"csv": run_dir / "tables" / "attention_heads.csv", "npz": run_dir / "attention" / "head_stats.npz",
           "report": run_dir / "attention" / "attention_report.md"}
    for p in out.values():
        p.parent.mkdir(parents=True, exist_ok=True)
    with out["csv"].open("w", newline="") as f:
        csv.writer(f).writerows(csv_rows(stats))
    np.savez(out["npz"], sums=stats.sums, n_rows=np.int64(stats.n_rows), means=stats.means,
             stats=np.array(A.STATS), reference_row0=triple)
    out["report"].write_text(report_markdown(stats))
    return out


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    check_args(args)
    from .score_mutations import load_model, load_vocab
    run_dir = Path(args.run_dir)
    x = load_inputs(run_dir, args.npz, args.n_seqs)
    model, _ = load_model(None, run_dir, args.dtype)
    itos = load_vocab(None, run_dir)
    if x.shape[1] > int(model.block_size):
        raise ValueError(f"sequences of {x.shape[1]} tokens exceed block_size {int(model.block_size)}")
    stats = A.head_stats(model, x, itos, window=args.window, batch=args.batch)
    out = write_outputs(run_dir, stats, A.reference_head_stats(model, x[0], itos))
    if args.maps:
        k = min(args.maps, x.shape[0])
        maps = A.attention_maps(model, x[:k], max_tokens=args.max_tokens)
        out["maps"] = run_dir / "attention" / "attn_maps.npz"
        np.savez(out["maps"], attn=maps, val_inputs=x[:k, :maps.shape[-1]])
    for name, p in out.items():
        print(f"[attention] wrote {name} to {p}")
    return out


if __name__ == "__main__":
    main()
