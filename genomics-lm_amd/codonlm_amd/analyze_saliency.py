#!/usr/bin/env python3
"""Gradient x input saliency of one sequence on the MI355X (mirrors scripts/analyze_saliency.py).

    python -m codonlm_amd.analyze_saliency --run_dir runs/<ID>
    python -m codonlm_amd.analyze_saliency --run_dir runs/<ID> --dna cds.fasta --map deps.npy

Without ``--dna`` the sequence is the first row of ``val_inputs`` in the run's ``artifacts.npz``
(targets: the first row of ``val_targets``, or the inputs rolled left by one when the run kept
none), as in the reference; with ``--dna`` it is that CDS (BOS, codons, EOS; inputs ids[:-1],
targets ids[1:]).  Writes ``<run>/tables/saliency.csv`` -- ``position,token,saliency`` with
``%.6f`` values, the reference's file: the gradient of the model's loss at the token-embedding
output times that embedding, summed over its dimensions.  The forward and the input-only backward
run on the native engine (cg_model_input_grad); no autograd graph is built.  Added: ``--dna``,
``--dtype`` and ``--map``, which also saves the [n][n] dependency map of the sequence
(attribution.dependency_map) as a .npy file.
"""
from __future__ import annotations

import argparse
import csv
from pathlib import Path
from typing import List, Sequence

import numpy as np

from . import attribution as A
from . import score as S
from .score_mutations import load_model, load_vocab, read_dna


def run_sequence(run_dir: Path):
    """(inputs, targets) int64 [T] each: row 0 of the run's validation artifacts."""
    path = run_dir / "artifacts.npz"
    if not path.exists():
        raise FileNotFoundError(f"artifacts.npz missing under {run_dir}")
    with np.load(path, allow_pickle=False) as data:
        art = {k: data[k] for k in data.files}
    val_inputs, val_targets = art.get("val_inputs"), art.get("val_targets")
    if val_inputs is None or val_inputs.size == 0:
        raise ValueError("validation inputs missing from artifacts.npz")
    if val_targets is None or val_targets.size == 0:
        val_targets = np.roll(val_inputs, -1, axis=1)
    return val_inputs[0].astype(np.int64), val_targets[0].astype(np.int64)


def csv_rows(inputs: Sequence[int], itos: Sequence[str], values: np.ndarray) -> List[list]:
    """Header and one row per input position: index, token name (``tok_<id>`` past the
    vocabulary), ``%.6f`` value."""
    rows = [["position", "token", "saliency"]]
    for i, (tok, v) in enumerate(zip(inputs, values)):
        tok = int(tok)
        rows.append([i, itos[tok] if tok < len(itos) else f"tok_{tok}", f"{float(v):.6f}"])
    return rows


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Gradient x input saliency of one sequence.")
    ap.add_argument("--run_dir", required=True, help="run directory: checkpoints/best.pt, itos.txt, artifacts.npz")
    ap.add_argument("--dna", default=None, help="DNA string (ACGT...) or path to file (raw or FASTA) "
                                                "instead of the run's first validation row")
    ap.add_argument("--map", default=None, help="also write the sequence's dependency map here (.npy)")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    return ap


def main(argv=None) -> Path:
    args = build_parser().parse_args(argv)
    run_dir = Path(args.run_dir)
    model, _ = load_model(None, run_dir, args.dtype)
    itos = load_vocab(None, run_dir)
    if args.dna is not None:
        ids = np.asarray(S.dna_to_ids(read_dna(args.dna), {t: i for i, t in enumerate(itos)}), dtype=np.int64)
        x, y = ids[:-1], ids[1:]
    else:
        x, y = run_sequence(run_dir)
        ids = np.concatenate([x, y[-1:]])
    sal = A.loss_saliency(model, x, y)["gxt"]
    out = run_dir / "tables" / "saliency.csv"
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w", newline="") as f:
        csv.writer(f).writerows(csv_rows(x, itos, sal))
    print(f"[saliency] wrote saliency scores to {out}")
    if args.map:
        mp = Path(args.map)
        mp.parent.mkdir(parents=True, exist_ok=True)
        with mp.open("wb") as f:  # (np.save on a name would append .npy to another suffix)
            np.save(f, A.dependency_map(model, ids))
        print(f"[saliency] wrote dependency map to {mp}")
    return out


if __name__ == "__main__":
    main()
