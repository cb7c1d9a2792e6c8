#!/usr/bin/env python3
"""Mutation map of one CDS on the MI355X (mirrors src/codonlm/score_mutations.py).

    python -m codonlm_amd.score_mutations --ckpt runs/<ID>/checkpoints/best.pt --dna ATGAAACCCTAA
    python -m codonlm_amd.score_mutations --run_dir runs/<ID> --dna cds.fasta --out scores.tsv

For every codon position of the CDS, the log-probability of each of the 64 codons there minus
that of the wild-type codon, given the tokens before it.  Same flags, tokenisation (upper-case,
U -> T, unknown codons dropped, BOS / EOS added), sliding-window rule for inputs longer than
block_size, TSV layout (``pos  wt  <64 codons>``, ``%.4f``, ``-inf`` for a codon the model's
vocabulary lacks) and default output path (``outputs/scores[/$RUN_ID]/<stem>__<ckpt>.tsv``) as the
reference.  Added: ``--run_dir`` (its best.pt and itos.txt) and ``--dtype``.  The forward runs on
the native engine and the 64 deltas of every position come from one cg_score_rows pass; no
heatmap is drawn.
"""
from __future__ import annotations

import argparse
import csv
import os
from pathlib import Path
from typing import List, Mapping, Sequence

import numpy as np
import torch

from . import score as S


def read_dna(arg: str) -> str:
    """``arg`` itself when it is a short ACGTU string (score_mutations.py :74-78), else the file it
    names: raw DNA, or FASTA whose header lines are skipped."""
    if len(arg) <= 80 and all(c in "ACGTUacgtu" for c in arg):
        return arg
    lines = Path(arg).read_text().splitlines()
    return "".join(ln.strip() for ln in lines if not ln.startswith(">")).strip()


def load_vocab(ckpt: Path | None, run_dir: Path | None) -> List[str]:
    """itos.txt of the run (beside the checkpoint, or one level up), else the fixed codon
    vocabulary of the tokenizer."""
    places = []
    if run_dir is not None:
        places.append(run_dir / "itos.txt")
    if ckpt is not None:
        places += [ckpt.parent / "itos.txt", ckpt.parent.parent / "itos.txt"]
    for p in places:
        if p.exists():
            return [ln.strip() for ln in p.read_text().splitlines() if ln.strip()]
    return list(S.DEFAULT_VOCAB)


def load_model(ckpt: Path | None, run_dir: Path | None, dtype: str):
    """(model, checkpoint path): --ckpt is one file, --run_dir the run's best.pt."""
    from .checkpoints import load_codon_checkpoint
    from .query_model import build_model_from_state
    if ckpt is not None:
        state = torch.load(ckpt, map_location="cpu", weights_only=True)
        if isinstance(state, Mapping) and "model" in state:
            sd, cfg = state["model"], dict(state.get("cfg", {}))
        else:
            sd, cfg = state, {}
        path = ckpt
    else:
        sd, cfg, path = load_codon_checkpoint(run_dir)
    return build_model_from_state(sd, cfg, compute_dtype=dtype), Path(path)


def tsv_rows(ids: Sequence[int], itos: Sequence[str], deltas: np.ndarray) -> List[list]:
    """Header and one row per position 1..len(ids)-2: pos, wild-type token, 64 values ``%.4f``
    (``-inf`` prints as such)."""
    rows = [["pos", "wt"] + S.CODONS]
    for pos in range(1, len(ids) - 1):
        wt = itos[ids[pos]] if 0 <= ids[pos] < len(itos) else f"<{ids[pos]}>"
        rows.append([pos, wt] + [f"{float(v):.4f}" for v in deltas[pos - 1]])
    return rows


def write_tsv(path: Path, rows: List[list]) -> None:
    path.parent.mkdir(parents=True, exist_ok=True)
    with path.open("w", newline="") as f:
        csv.writer(f, delimiter="\t").writerows(rows)


def default_output(dna_arg: str, ckpt_path: Path) -> Path:
    base = Path("outputs/scores")
    run_id = os.environ.get("RUN_ID", "").strip()
    if run_id:
        base = base / run_id
    return base / f"{Path(dna_arg).stem}__{ckpt_path.stem}.tsv"


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Per-position delta log-prob of all 64 codons for one CDS.")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt", help="checkpoint file (best.pt)")
    src.add_argument("--run_dir", help="run directory holding checkpoints/best.pt and itos.txt")
    ap.add_argument("--dna", required=True, help="DNA string (ACGT...) or path to file (raw or FASTA)")
    ap.add_argument("--out", default=None, help="Write TSV here (default: auto path)")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    return ap


def main(argv=None) -> Path:
    args = build_parser().parse_args(argv)
    ckpt = Path(args.ckpt) if args.ckpt else None
    run_dir = Path(args.run_dir) if args.run_dir else None
    model, ckpt_path = load_model(ckpt, run_dir, args.dtype)
    itos = load_vocab(ckpt, run_dir)
    stoi = {t: i for i, t in enumerate(itos)}
    ids = S.dna_to_ids(read_dna(args.dna), stoi)
    deltas = S.mutation_map(model, ids, S.codon_ids(stoi))
    out = Path(args.out) if args.out else default_output(args.dna, ckpt_path)
    write_tsv(out, tsv_rows(ids, itos, deltas))
    print(f"[save] {out}")
    return out


if __name__ == "__main__":
    main()
