#!/usr/bin/env python3
"""Test / validation cross-entropy and perplexity of a trained run on the MI355X (mirrors
scripts/evaluate_test.py).

    python -m codonlm_amd.evaluate_test --run_dir outputs/checkpoints/<RUN_ID>
    python -m codonlm_amd.evaluate_test --run_id <RUN_ID> --split validation --dtype bf16

Same flags, dataset discovery, argument checks and ``<run_dir>/scores/metrics.json`` keys as the
reference: ``{prefix}_loss``, ``_nll``, ``_ppl``, ``_objective_loss``, ``_label_smoothing``,
``_evaluated_tokens``, ``_offset_{k}_{name}``, the ``{prefix}_evaluation_provenance`` block and
``timestamp``, merged into whatever the file already holds.  The dataset lives on the device
(DeviceCodonDataset / DeviceBatchLoader) and all sums are device accumulators read once
(score.evaluate).  Relative dataset paths resolve against the working directory.
``--derived_provenance`` is not supported (provenance.py binds no derived datasets).
"""
from __future__ import annotations

import argparse
import json
from datetime import datetime, timezone
from pathlib import Path
from typing import Optional

from . import score as S


def find_test_npz(run_id: str, cfg: dict, root: Path, data_dir: Optional[Path]) -> Path:
    """--data_dir, else the config's test_npz, else the combined manifest of the run, else the
    default layout (evaluate_test.py :52-73)."""
    name = f"test_bs{cfg['block_size']}.npz"
    if data_dir is not None:
        return data_dir / name
    listed = cfg.get("test_npz")
    if listed:
        if isinstance(listed, list):
            listed = listed[0]
        p = Path(listed)
        return p if p.is_absolute() else root / p
    manifest = root / "data/processed/combined" / run_id / "manifest.json"
    if manifest.exists():
        p = Path(json.loads(manifest.read_text()).get("test", ""))
        return p if p.is_absolute() else root / p
    return root / "data/processed" / name


def find_validation_npz(cfg: dict, root: Path) -> Path:
    listed = cfg.get("val_npz")
    if isinstance(listed, list) and listed:
        listed = listed[0]
    if not listed:
        raise ValueError("validation evaluation requires val_npz in the run config")
    p = Path(listed)
    return p if p.is_absolute() else root / p


def resolve_run(run_id: Optional[str], run_dir: Optional[str]):
    """(run_id, run directory): --run_dir wins; a checkpoints/ or scores/ directory means its parent."""
    if run_dir is not None:
        rd = Path(run_dir)
        if not rd.exists():
            raise FileNotFoundError(f"run_dir not found: {rd}")
        if rd.name in ("checkpoints", "scores"):
            rd = rd.parent
        return rd.name, rd
    if run_id is not None:
        return run_id, Path("runs") / run_id
    raise ValueError("provide either --run_id or --run_dir")


def merge_metrics(path: Path, updates: dict) -> dict:
    """Read ``path`` (a JSON object, if it exists), overlay ``updates``, write it back."""
    merged = {}
    if path.exists():
        try:
            old = json.loads(path.read_text())
            if isinstance(old, dict):
                merged = old
        except json.JSONDecodeError:
            pass
    merged.update(updates)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(merged, indent=2) + "\n")
    return merged


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Evaluate test or validation NLL / perplexity of a run.")
    ap.add_argument("--run_dir", help="outputs/checkpoints/<RUN_ID>")
    ap.add_argument("--run_id", help="Run id (alternative to --run_dir)")
    ap.add_argument("--split", choices=("test", "validation"), default="test",
                    help="Frozen dataset split to evaluate (default: test).")
    ap.add_argument("--data_dir", help="override test NPZ directory (contains test_bs*.npz)")
    ap.add_argument("--test_npz", type=Path, help="explicit test or control dataset")
    ap.add_argument("--manifest", type=Path, help="Frozen dataset manifest; required for corrected checkpoints.")
    ap.add_argument("--derived_provenance", type=Path, help="(not supported on this path)")
    ap.add_argument("--checkpoint-name", default="best.pt",
                    help="Checkpoint filename under the run directory (default: best.pt).")
    ap.add_argument("--metric-prefix", default=None, help="Metrics key prefix; defaults to the selected split name.")
    ap.add_argument("--batch_size", type=int, default=None, help="evaluation batch size")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    return ap


def check_args(args) -> str:
    """The reference's argument checks (:210-216); returns the metric prefix."""
    prefix = args.metric_prefix or args.split
    if not prefix.replace("_", "").isalnum():
        raise ValueError("--metric-prefix must contain only letters, numbers, and underscores")
    if args.split == "validation" and args.test_npz is not None:
        raise ValueError("--test_npz cannot be used with --split validation")
    if args.derived_provenance is not None:
        raise ValueError("--derived_provenance is not supported: codonlm_amd.provenance binds no derived datasets; "
                         "evaluate the frozen split with --manifest instead")
    return prefix


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    prefix = check_args(args)
    from .checkpoints import load_codon_checkpoint
    from .data_loading import DeviceBatchLoader, DeviceCodonDataset
    from .provenance import artifact_provenance, bind_checkpoint_dataset, bind_dataset_manifest
    from .query_model import build_model_from_state

    run_id, run_dir = resolve_run(args.run_id, args.run_dir)
    root = Path.cwd()
    state_dict, cfg, checkpoint_path = load_codon_checkpoint(run_dir, ckpt_name=args.checkpoint_name)
    model = build_model_from_state(state_dict, cfg, compute_dtype=args.dtype)

    if args.split == "validation":
        npz, role = find_validation_npz(cfg, root), "val_tokens"
    else:
        npz = args.test_npz or find_test_npz(run_id, cfg, root, Path(args.data_dir) if args.data_dir else None)
        role = "test_tokens"
    npz = Path(npz).expanduser().resolve()
    manifest_provenance = None
    if args.manifest is not None:
        _, manifest_provenance = bind_dataset_manifest(args.manifest, expected_artifacts={role: npz})
    checkpoint_dataset = bind_checkpoint_dataset(cfg, manifest_provenance)

    ds = DeviceCodonDataset(npz, device=model.flat_parameters().device)
    batch_size = args.batch_size if args.batch_size is not None else int(cfg.get("eval_batch_size", 64))
    loader = DeviceBatchLoader(ds, batch_size, shuffle=False, drop_remainder=False)
    label_smoothing = float(cfg.get("label_smoothing", 0.0))
    offsets = tuple(int(k) for k in cfg.get("multi_offset_targets", None) or [])
    nll, ppl, objective, tokens, offset_metrics = S.evaluate(model, loader, label_smoothing=label_smoothing,
                                                             offset_targets=offsets)
    print(f"[{args.split}] nll={nll:.4f} ppl={ppl:.2f} objective={objective:.4f} "
          f"label_smoothing={label_smoothing:.4f}")
    for k, v in sorted(offset_metrics.items()):
        print(f"[{args.split}] offset=+{k} nll={v['nll']:.4f} ppl={v['ppl']:.2f} "
              f"unprojected_nll={v['unprojected_nll']:.4f} "
              f"relative_improvement={100.0 * v['relative_nll_improvement']:.2f}%")

    updates = {f"{prefix}_loss": float(nll), f"{prefix}_nll": float(nll), f"{prefix}_ppl": float(ppl),
               f"{prefix}_objective_loss": float(objective), f"{prefix}_label_smoothing": label_smoothing,
               f"{prefix}_evaluated_tokens": int(tokens)}
    for k, values in offset_metrics.items():
        for name, value in values.items():
            updates[f"{prefix}_offset_{k}_{name}"] = value
    updates[f"{prefix}_evaluation_provenance"] = {
        "schema_version": 2,
        "loss_definition": {"nll": "unsmoothed_cross_entropy", "perplexity": "exp(unsmoothed_cross_entropy)",
                            "objective": "cross_entropy_with_configured_label_smoothing"},
        "dataset_manifest": manifest_provenance or {"status": "legacy_unverified"},
        "checkpoint_dataset": checkpoint_dataset,
        "checkpoint": artifact_provenance(checkpoint_path),
        role: artifact_provenance(npz),
        "derived_dataset": None,
    }
    updates["timestamp"] = datetime.now(timezone.utc).isoformat()
    metrics_path = run_dir / "scores" / "metrics.json"
    merge_metrics(metrics_path, updates)
    print(f"[metrics] updated {metrics_path}")
    return updates


if __name__ == "__main__":
    main()
