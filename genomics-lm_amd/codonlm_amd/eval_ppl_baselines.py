#!/usr/bin/env python3
"""Uniform and count-based next-token baselines of a split, fitted and evaluated on the MI355X
(mirrors scripts/eval_ppl_baselines.py).  No model is needed: only the library and a device.

    python -m codonlm_amd.eval_ppl_baselines --train train.npz --test test.npz --itos itos.txt

Same flags, JSON keys and markdown layout as the reference.  The vocabulary comes from ``--itos``, or
``--run-dir``'s ``itos.txt`` (provenance.read_itos_strict); the report's ``vocabulary`` block holds its
size and sha256.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

from . import context as X


def artifact_hashes(path: Path) -> dict:
    from .provenance import file_sha256
    files = [path] + [path.with_name(path.stem + suffix) for suffix in ("_X.npy", "_Y.npy", "_lengths.npy")]
    return {str(f.resolve()): file_sha256(f) for f in files if f.exists()}


def markdown(report: dict) -> str:
    """One table, a row per baseline, every figure to six decimals (the reference's layout)."""
    columns = {"Cross-entropy (nats)": "cross_entropy_nats", "Perplexity": "perplexity", "Bits/codon": "bits_per_codon",
               "Improvement over best simple (nats)": "cross_entropy_improvement_over_best_simple"}
    rows = ([name] + [f"{metrics[key]:.6f}" for key in columns.values()] for name, metrics in report["results"].items())
    return "\n".join(X.markdown_table(["Model", *columns], "|---|---:|---:|---:|---:|", rows)) + "\n"


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Segment-aware n-gram baselines of a split on the MI355X.")
    parser.add_argument("--train", "--train_npz", dest="train", required=True)
    parser.add_argument("--test", "--test_npz", dest="test", required=True)
    parser.add_argument("--split", choices=("test", "validation"), default="test",
                        help="Manifest role of the evaluation input (default: test).")
    parser.add_argument("--itos", help="Vocabulary artifact; defaults to <run-dir>/itos.txt")
    parser.add_argument("--run-dir", type=Path, help="Run directory holding itos.txt")
    parser.add_argument("--manifest", type=Path, help="Dataset manifest to hash into provenance")
    parser.add_argument("--config", type=Path, help="Evaluation/run config to hash into provenance")
    parser.add_argument("--alpha", type=float, default=0.01)
    parser.add_argument("--batch-size", type=int, default=1024)
    parser.add_argument("--device", choices=("cuda",), default="cuda")
    parser.add_argument("--output-prefix", type=Path)
    return parser


def check_args(args) -> Path:
    """The argument checks that need no device; returns the vocabulary path."""
    if args.alpha <= 0:
        raise ValueError("alpha must be positive")
    if args.itos is None and args.run_dir is None:
        raise ValueError("provide --itos or --run-dir (the vocabulary is read from itos.txt)")
    return Path(args.itos) if args.itos is not None else args.run_dir / "itos.txt"


def evaluate(args, itos_path: Path) -> dict:
    import torch

    from .data_loading import DeviceBatchLoader, DeviceCodonDataset
    from .provenance import bind_dataset_manifest, file_sha256, read_itos_strict

    train, test = Path(args.train), Path(args.test)
    manifest_provenance = {"status": "legacy_unverified"}
    if args.manifest is not None:
        role = "val_tokens" if args.split == "validation" else "test_tokens"
        _, manifest_provenance = bind_dataset_manifest(args.manifest, expected_artifacts={"train_tokens": train, role: test},
                                                       require_scientific=False)
    itos = read_itos_strict(itos_path)
    reset_ids = [i for i, token in enumerate(itos) if token == "<SEP>"]
    dev = torch.device("cuda", torch.cuda.current_device())
    loaders = [DeviceBatchLoader(DeviceCodonDataset(p, device=dev), args.batch_size, shuffle=False,
                                 drop_remainder=False) for p in (train, test)]
    tables = X.fit_ngrams(loaders[0], len(itos), reset_ids)
    results, tokens, best = X.evaluate_ngrams(loaders[1], tables, args.alpha)
    # the reference's report keys, grouped: inputs and their hashes, the model family, the figures
    hashed_inputs = {"manifest": args.manifest, "config": args.config}
    report = {"schema_version": 1, "evaluation_split": args.split}
    report.update({name: str(path.resolve()) for name, path in (("train", train), ("test", test))})
    report["dataset_sha256"] = artifact_hashes(train) | artifact_hashes(test)
    report["input_provenance"] = {name: {"path": str(path.resolve()), "sha256": file_sha256(path)}
                                  for name, path in hashed_inputs.items() if path is not None}
    report["dataset_manifest"] = manifest_provenance
    report["vocabulary"] = X.vocabulary_block(itos)
    report["smoothing"] = {"method": "additive", "alpha": args.alpha}
    report["context_boundary"] = {"method": "reset_history_after_tokens", "token_ids": sorted(reset_ids),
                                  "tokens": [itos[i] for i in sorted(reset_ids)]}
    report.update(evaluated_tokens=tokens, best_simple_baseline=best, results=results)
    return report


def write_report(report: dict, prefix: Path) -> str:
    text = markdown(report)
    prefix.parent.mkdir(parents=True, exist_ok=True)
    prefix.with_suffix(".json").write_text(json.dumps(report, indent=2, sort_keys=True) + "\n")
    prefix.with_suffix(".md").write_text(text)
    return text


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    itos_path = check_args(args)
    report = evaluate(args, itos_path)
    test = Path(args.test)
    text = write_report(report, args.output_prefix or test.with_name(test.stem + "_ppl_baselines"))
    print(f"Baseline Perplexity Comparison ({report['evaluated_tokens']} tokens)\n{text}")
    return report


if __name__ == "__main__":
    main()
