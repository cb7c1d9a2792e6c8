#!/usr/bin/env python3
"""DNAshape structural regression probes of a run on the MI355X (mirrors
scripts/probe_structural_regression.py).

    python -m codonlm_amd.probe_structural_regression --run_dir runs/<ID> --test_npz test.npz
    python -m codonlm_amd.probe_structural_regression --run_id <ID> --test_npz test.npz \
        --sample_size 0 --layers all

The reference's flags (``--run_id | --run_dir``, ``--ckpt``, ``--test_npz``, ``--sample_size``,
``--no_cache``), sequence choice (``random.Random(42)`` shuffle of the dataset's indices, the first
``sample_size`` in that order) and metric keys (``regression_probe.<name>.r2`` / ``.corr``,
``regression_probe.avg_r2`` / ``.avg_corr``, merged into ``<run>/scores/metrics.json``).  Added:
``--sample_size 0`` (every sequence, in dataset order), ``--layers`` (``-1``, a comma list or
``all``; several layers add ``regression_probe.layer<l>.`` keys, and the plain keys then hold the
last block or, when it is not among them, are not written), ``--batch_size``, ``--dtype``.
Fixed-window files (``X`` [N][T]) and dynamic ones (``X`` flat with ``lengths``) are accepted;
sequences are trimmed to the model's block_size.

The fitted probes go to ``<run>/checkpoints/structural_regression_probes.npz`` (``coef``,
``intercept``, ``names``, ``layers``, ``alpha``, ``n_rows``) and are loaded from there, and only
scored, unless ``--no_cache`` is given or they were fitted for other layers.  The reference's
``structural_regression_probes.pt`` (pickled sklearn objects) is neither read nor written.
"""
from __future__ import annotations

import argparse
import random
from pathlib import Path

import numpy as np

from . import structure_probe as SP

PROBE_FILE = "structural_regression_probes.npz"


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Ridge probes from hidden states to DNAshape targets, 5-fold CV.")
    ap.add_argument("--run_id", help="run under runs/")
    ap.add_argument("--run_dir", help="run directory: checkpoints/<ckpt> and itos.txt")
    ap.add_argument("--ckpt", default="best.pt")
    ap.add_argument("--test_npz", default="data/processed/stage2.5_master_pack_v2/test_bs512.npz")
    ap.add_argument("--sample_size", type=int, default=150, help="sequences to probe (0 = all, in dataset order)")
    ap.add_argument("--no_cache", action="store_true", help="do not load fitted probes from disk")
    ap.add_argument("--layers", default="-1", help="block index (-1 = last), a comma list, or 'all'")
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    return ap


def parse_layers(text: str):
    """'all', or the list of ints of a comma list."""
    text = text.strip()
    if text == "all":
        return "all"
    try:
        out = [int(p) for p in text.split(",")]
    except ValueError:
        raise ValueError(f"--layers: '{text}' is neither 'all' nor a comma list of block indices") from None
    return out


def check_args(args) -> None:
    """The argument checks that need no device."""
    if not args.run_id and not args.run_dir:
        raise ValueError("one of --run_id / --run_dir is needed")
    if args.sample_size < 0:
        raise ValueError("--sample_size cannot be negative")
    if args.batch_size < 1:
        raise ValueError("--batch_size must be at least 1")
    parse_layers(args.layers)


def select_indices(n: int, sample_size: int):
    """The reference's choice: indices 0..n-1 shuffled by random.Random(42), the first sample_size;
    sample_size 0: all of them in dataset order."""
    if sample_size == 0:
        return list(range(n))
    idxs = list(range(n))
    random.Random(42).shuffle(idxs)
    return idxs[:min(sample_size, n)]


def load_sequences(path, sample_size: int, block_size: int, pad_id: int = 0) -> np.ndarray:
    """int64 [S][T] of the selected sequences, trimmed to block_size and right-padded with PAD; a
    file with ``lengths`` holds the sequences back to back in ``X``."""
    path = Path(path)
    if not path.exists():
        raise FileNotFoundError(f"Test dataset not found at {path}")
    with np.load(path, allow_pickle=False) as data:
        X = np.asarray(data["X"])
        lengths = np.asarray(data["lengths"]) if "lengths" in data.files else None
    if lengths is None:
        if X.ndim != 2:
            raise ValueError(f"'X' of {path} must be (N, T) when there is no 'lengths'")
        sel = select_indices(len(X), sample_size)
        return np.ascontiguousarray(X[sel, :block_size].astype(np.int64)).reshape(len(sel), -1)
    ends = np.cumsum(lengths)
    starts = ends - lengths
    sel = select_indices(len(lengths), sample_size)
    T = int(min(block_size, max([int(lengths[i]) for i in sel], default=0)))
    out = np.full((len(sel), T), pad_id, dtype=np.int64)
    for r, i in enumerate(sel):
        n = min(int(lengths[i]), T)
        out[r, :n] = X.reshape(-1)[starts[i]:starts[i] + n]
    return out


def load_probes(path: Path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in ("coef", "intercept", "names", "layers", "alpha", "n_rows")}


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    check_args(args)
    from .evaluate_test import merge_metrics
    from .score_mutations import load_model, load_vocab
    run_dir = Path(args.run_dir) if args.run_dir else Path("runs") / args.run_id
    print(f"[*] Probing run: {args.run_id or run_dir.name}")
    ckpt = None if args.ckpt == "best.pt" else run_dir / "checkpoints" / args.ckpt
    model, _ = load_model(ckpt, run_dir, args.dtype)
    itos = load_vocab(ckpt, run_dir)
    ids = load_sequences(args.test_npz, args.sample_size, int(model.block_size))
    layers = SP.layer_list(model, parse_layers(args.layers))
    probe_path = run_dir / "checkpoints" / PROBE_FILE
    cached = None
    if not args.no_cache and probe_path.exists():
        cached = load_probes(probe_path)
        if [int(l) for l in cached["layers"]] != layers or cached["coef"].shape[2] != int(model.n_embd):
            print(f"[!] {probe_path} was fitted for other layers; fitting anew")
            cached = None
        else:
            print(f"[+] Found saved structural regression probes at {probe_path}. Loading...")
    print(f"[*] Probing {len(ids)} test sequences, layers {layers}...")
    metrics, probes = SP.probe(model, ids, layers, batch_size=args.batch_size, cached=cached, itos=itos)
    tag = "Cached Probe" if cached is not None else "Training Probe"
    for name in SP.NAMES:
        if f"regression_probe.{name}.r2" in metrics:
            print(f"[{tag}] {name} -> R^2: {metrics[f'regression_probe.{name}.r2']:.4f} | "
                  f"Pearson: {metrics[f'regression_probe.{name}.corr']:.4f}")
    if cached is None:
        probe_path.parent.mkdir(parents=True, exist_ok=True)
        np.savez(probe_path, **probes)
        print(f"[*] Saved structural regression probes to {probe_path}")
    for key in sorted(k for k in metrics if k.endswith("avg_r2")):
        pre = key[:-len("avg_r2")]
        print(f"[{pre.rstrip('.')}] Overall R^2 Score: {metrics[key]:.4f} | Avg Pearson: "
              f"{metrics[pre + 'avg_corr']:.4f} ({int(probes['n_rows'])} codon positions)")
    merge_metrics(run_dir / "scores" / "metrics.json", metrics)
    print(f"[+] Wrote regression probe metrics to {run_dir / 'scores' / 'metrics.json'}")
    return metrics


if __name__ == "__main__":
    main()
