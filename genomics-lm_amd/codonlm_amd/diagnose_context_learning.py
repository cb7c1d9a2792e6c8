#!/usr/bin/env python3
"""Does a checkpoint use context beyond token composition?  (mirrors
scripts/diagnose_context_learning.py)

    python -m codonlm_amd.diagnose_context_learning --run-dir runs/<RUN_ID> --train train.npz \
        --test test.npz --manifest manifest.json --output-prefix out/context

Same flags, JSON keys and markdown layout as the reference.  The vocabulary comes from ``--itos`` or
``<run-dir>/itos.txt`` (provenance.read_itos_strict); the report's ``vocabulary`` block holds its
size and sha256, as the trainer's ``cfg["vocabulary"]`` does.  ``--device`` accepts the GPU only.
"""
from __future__ import annotations

import argparse
import csv
import json
from pathlib import Path

import numpy as np

from . import context as X


ARTIFACT_ROLES = {"test": "test_tokens", "validation": "val_tokens"}  # --split -> manifest artifact


def packing_window_flags(path, n_windows: int) -> np.ndarray:
    """bool [n_windows]: the packed windows that the packing metadata (TSV with window_index,
    continues_from_previous, continues_to_next) marks as holding a chunk continued on either side."""
    flags = np.zeros(n_windows, dtype=bool)
    if path is None:
        return flags
    with Path(path).open(newline="") as handle:
        records = [(int(r["window_index"]), "1" in (r["continues_from_previous"], r["continues_to_next"]))
                   for r in csv.DictReader(handle, delimiter="\t")]
    outside = [i for i, _ in records if not 0 <= i < n_windows]
    if outside:
        raise ValueError(f"packing metadata window index out of range: {outside[0]}")
    flags[[i for i, continued in records if continued]] = True
    return flags


def evaluation_artifact_role(split: str) -> str:
    if split not in ARTIFACT_ROLES:
        raise ValueError(f"unsupported evaluation split: {split}")
    return ARTIFACT_ROLES[split]


def markdown(report: dict) -> str:
    """The reference's report layout: four sections, three tables and the paired-gate sentence."""
    gate = report["paired_codonlm_vs_trigram"]
    sections = [
        ("# Context Learning Diagnostic", []),
        ("## Context Ablation", X.markdown_table(
            ("Input attention window", "NLL", "PPL"), "| ---: | ---: | ---: |",
            ((name, f"{r['nll']:.6f}", f"{r['perplexity']:.3f}") for name, r in report["context_ablation"].items()))),
        ("## Segment-Aware Markov Baselines", X.markdown_table(
            ("Model", "NLL", "PPL"), "| --- | ---: | ---: |",
            ((name, f"{r['cross_entropy_nats']:.6f}", f"{r['perplexity']:.3f}")
             for name, r in report["markov"]["results"].items()))),
        ("## Paired Gate", ["CodonLM minus trigram: `%.6f` nats/token (95%% packed-window bootstrap CI `[%.6f, %.6f]`)."
                            % (gate["codonlm_minus_trigram_nats_per_token"], gate["ci95"][0], gate["ci95"][1])]),
        ("## Loss Decomposition", X.markdown_table(
            ("Slice", "Tokens", "NLL", "PPL"), "| --- | ---: | ---: | ---: |",
            ((name, str(r["tokens"]), f"{r['nll']:.6f}", f"{r['perplexity']:.3f}")
             for name, r in report["loss_decomposition"].items()))),
    ]
    lines = []
    for title, body in sections:
        lines += [title, ""] + (body + [""] if body else [])
    return "\n".join(lines[:-1]) + "\n"


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Context-learning diagnostic of a run on the MI355X.")
    parser.add_argument("--run-dir", type=Path, required=True)
    parser.add_argument("--checkpoint-name", default="best.pt")
    parser.add_argument("--train", type=Path, required=True)
    parser.add_argument("--test", type=Path, required=True)
    parser.add_argument("--split", choices=("test", "validation"), default="test",
                        help="Manifest role of the evaluation input (default: test).")
    parser.add_argument("--manifest", type=Path, required=True)
    parser.add_argument("--itos", type=Path)
    parser.add_argument("--packing-tsv", type=Path)
    parser.add_argument("--context-windows", default=X.DEFAULT_WINDOWS)
    parser.add_argument("--batch-size", type=int, default=4)
    parser.add_argument("--device", choices=("cuda",), default="cuda")
    parser.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    parser.add_argument("--alpha", type=float, default=0.01)
    parser.add_argument("--bootstrap-samples", type=int, default=2000)
    parser.add_argument("--mask-audit-windows", type=int, default=32)
    parser.add_argument("--seed", type=int, default=1337)
    parser.add_argument("--output-prefix", type=Path, required=True)
    return parser


def check_args(args) -> list:
    """The argument checks that need no device; returns the parsed windows."""
    windows = X.parse_windows(args.context_windows)
    if None not in windows:
        raise ValueError("context windows must include 'full' for decomposition")
    if args.alpha <= 0:
        raise ValueError("alpha must be positive")
    return windows


def diagnose(args, windows) -> dict:
    from .checkpoints import load_codon_checkpoint
    from .data_loading import DeviceBatchLoader, DeviceCodonDataset
    from .provenance import artifact_provenance, bind_checkpoint_dataset, bind_dataset_manifest, read_itos_strict
    from .query_model import build_model_from_state

    train_path = args.train.expanduser().resolve()
    test_path = args.test.expanduser().resolve()
    _, manifest_provenance = bind_dataset_manifest(
        args.manifest, expected_artifacts={"train_tokens": train_path,
                                           evaluation_artifact_role(args.split): test_path})
    itos = read_itos_strict(args.itos if args.itos is not None else args.run_dir / "itos.txt")
    state_dict, cfg, checkpoint_path = load_codon_checkpoint(args.run_dir, ckpt_name=args.checkpoint_name)
    checkpoint_dataset = bind_checkpoint_dataset(cfg, manifest_provenance)
    model = build_model_from_state(state_dict, cfg, compute_dtype=args.dtype)
    dev = model.flat_parameters().device
    test = DeviceCodonDataset(test_path, device=dev)
    if test.is_dynamic:
        raise ValueError("packing-aware context diagnostics currently require fixed windows")
    train = DeviceCodonDataset(train_path, device=dev)
    flags = packing_window_flags(args.packing_tsv, len(test))
    provenance = {"evaluation_split": args.split, "checkpoint": artifact_provenance(checkpoint_path),
                  "checkpoint_dataset": checkpoint_dataset, "dataset_manifest": manifest_provenance,
                  "packing_metadata": artifact_provenance(args.packing_tsv) if args.packing_tsv else None}
    return X.diagnose(model, DeviceBatchLoader(train, 1024, shuffle=False, drop_remainder=False),
                      DeviceBatchLoader(test, args.batch_size, shuffle=False, drop_remainder=False), itos,
                      windows=windows, alpha=args.alpha, row_flags=flags, bootstrap_samples=args.bootstrap_samples,
                      seed=args.seed, mask_audit_windows=args.mask_audit_windows, provenance=provenance,
                      log=lambda s: print(s, flush=True))


def write_report(report: dict, prefix: Path) -> str:
    text = markdown(report)
    prefix.parent.mkdir(parents=True, exist_ok=True)
    prefix.with_suffix(".json").write_text(json.dumps(report, indent=2, sort_keys=True) + "\n")
    prefix.with_suffix(".md").write_text(text)
    return text


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    windows = check_args(args)
    report = diagnose(args, windows)
    print(write_report(report, args.output_prefix))
    return report


if __name__ == "__main__":
    main()
