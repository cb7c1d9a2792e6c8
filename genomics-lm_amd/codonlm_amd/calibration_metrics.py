#!/usr/bin/env python3
"""Calibration metrics (ECE, Brier) of a checkpoint on a split, on the MI355X (mirrors
scripts/calibration_metrics.py).

    python -m codonlm_amd.calibration_metrics --ckpt runs/<RUN_ID>/checkpoints/best.pt \
        --npz val_bs512.npz --out runs/<RUN_ID>/scores/metrics.json

PAD (0) targets are ignored; ECE uses 15 bins on the max-probability predictions; the multiclass
Brier score is the mean of sum_k (p_k - y_k)^2.  ``ece_val`` and ``brier_val`` follow the reference:
per batch of 32 windows, weighted by the batch's token count.  ``ece_global`` bins all tokens at
once.  The keys are merged into whatever ``--out`` already holds.
"""
from __future__ import annotations

import argparse
from pathlib import Path

from . import context as X


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="ECE and Brier score of a checkpoint on a split.")
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--npz", required=True, help="NPZ with X,Y (val or test split)")
    ap.add_argument("--out", required=True, help="metrics.json to merge into")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--n-bins", type=int, default=15)
    ap.add_argument("--device", choices=("cuda",), default="cuda")
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    return ap


def check_args(args) -> None:
    if args.batch_size < 1:
        raise ValueError("--batch-size must be at least 1")
    if not 1 <= args.n_bins <= X.L.DIAG_MAX_BINS:
        raise ValueError(f"--n-bins must be in 1..{X.L.DIAG_MAX_BINS}")


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    check_args(args)
    from .checkpoints import load_codon_checkpoint
    from .data_loading import DeviceBatchLoader, DeviceCodonDataset
    from .evaluate_test import merge_metrics
    from .query_model import build_model_from_state

    ckpt = Path(args.ckpt)
    state_dict, cfg, _ = load_codon_checkpoint(ckpt.parent, ckpt_name=ckpt.name)
    model = build_model_from_state(state_dict, cfg, compute_dtype=args.dtype)
    ds = DeviceCodonDataset(args.npz, device=model.flat_parameters().device)
    loader = DeviceBatchLoader(ds, args.batch_size, shuffle=False, drop_remainder=False)
    result = X.calibration(model, loader, n_bins=args.n_bins)
    metrics = {k: result[k] for k in ("ece_val", "brier_val", "ece_global") if k in result}
    merge_metrics(Path(args.out), metrics)
    print(f"[calibration] merged {metrics} into {args.out}")
    return metrics


if __name__ == "__main__":
    main()
