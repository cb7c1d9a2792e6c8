#!/usr/bin/env python3
"""Prefix-generation benchmark of a trained codon LM on the MI355X (mirrors
scripts/eval_generation_prefix.py).

    python -m codonlm_amd.eval_generation_prefix --run_dir runs/<RUN_ID> \\
        --k_list 1,3,5,10 --samples 5 --max_genes 50 --max_new 300 --temperature 0.8 --topk 5

The reference's flags and defaults; ``--run_dir`` stands in for ``--run_id`` and ``--batch_size`` sets
how many (gene, k, sample) rows one generation batch holds.  Writes, under
``<run>/scores/<out_label>/``: samples.csv, protocol_samples.csv, generated_protocols.fasta,
protocol_summary.csv, protocol_manifest.json and summary.csv, with the reference's columns (the critic
columns hold 0).  The library is ``codonlm_amd.gen_prefix``.

The CDS source is, in order: ``--cds_file`` (one CDS per line), the frozen split of ``--dataset_manifest``
(or the checkpoint config's ``dataset_manifest``; seeded shuffle, then round-robin by genome),
``<run>/combined_manifest.json``'s first ``dna`` entry, the config keys ``dna_path`` / ``cds_dna`` /
``primary_dna``.  The training tokens of the memorization audit are the config's ``train_npz`` (or
``--train_npz``); ``--max_train_audit_tokens 0`` indexes all of them.

Not part of this tool: the protein critic and EBM (--critic_* / --ebm_*), --target_protein, the plots.
"""
from __future__ import annotations

import argparse
import csv
import hashlib
import json
import random
from pathlib import Path
from typing import Dict, List, Optional, Tuple

from . import gen_prefix as GP


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Prefix-generation benchmark with a training-set memorization audit.")
    ap.add_argument("--run_dir", required=True, help="run directory (checkpoints/, itos.txt)")
    ap.add_argument("--dataset_manifest", type=Path, default=None,
                    help="Frozen dataset manifest. Defaults to the checkpoint configuration.")
    ap.add_argument("--source_split", choices=("train", "val", "test"), default="test",
                    help="Frozen source-record split from which generation prefixes are sampled.")
    ap.add_argument("--cds_file", type=Path, default=None, help="CDS DNA, one sequence per line (overrides discovery)")
    ap.add_argument("--train_npz", action="append", default=None,
                    help="training tokens of the memorization audit (default: the config's train_npz)")
    ap.add_argument("--preset", choices=sorted(GP.PRESETS), default=None,
                    help="Evaluation size preset. Explicit --max_genes/--samples/--max_new override it.")
    ap.add_argument("--k_list", default="1,3,5,10")
    ap.add_argument("--samples", type=int, default=None)
    ap.add_argument("--max_genes", type=int, default=None)
    ap.add_argument("--max_new", type=int, default=None)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--topk", type=int, default=5)
    ap.add_argument("--device", choices=["auto", "cuda"], default="auto")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--seed", type=int, default=1337)
    ap.add_argument("--ci_resamples", type=int, default=1000,
                    help="Bootstrap resamples for per-protocol 95%% confidence intervals.")
    ap.add_argument("--out_label", default="gen_prefix", help="Subdirectory under <run>/scores for outputs.")
    ap.add_argument("--progress_every", type=int, default=20, help="accepted for compatibility; batches print nothing")
    ap.add_argument("--batch_size", type=int, default=256, help="(gene, k, sample) rows per generation batch")
    ap.add_argument("--min_aa_len", type=int, default=100)
    ap.add_argument("--target_aa_len", type=int, default=256)
    ap.add_argument("--max_aa_len", type=int, default=400)
    ap.add_argument("--require_terminal_stop", action="store_true", default=False)
    ap.add_argument("--special_margin", type=int, default=6)
    ap.add_argument("--termination_bias", action="store_true", default=False)
    ap.add_argument("--termination_stop_bias", type=float, default=0.0)
    ap.add_argument("--termination_trigger_class_max", type=int, default=0)
    ap.add_argument("--termination_bias_window", type=int, default=0,
                    help="Only apply termination stop bias within this many codons of target length.")
    ap.add_argument("--allow_non_cds_tokens", action="store_true", default=False,
                    help="Permit non-codon tokens during CDS continuation generation for diagnostics.")
    ap.add_argument("--multi_offset_prior", action="store_true", default=False,
                    help="Enable multi-offset prior-guided decoding.")
    ap.add_argument("--multi_offset_prior_weights", type=str, default=None,
                    help="JSON dict mapping offsets to prior weights (e.g. '{\"4\":0.1,\"8\":0.05}').")
    ap.add_argument("--gqs_normalize", choices=["none", "len"], default="none")
    ap.add_argument("--no_memorization_audit", action="store_false", dest="memorization_audit",
                    help="Disable training-set memorization and similarity audit.")
    ap.add_argument("--memorization_n_list", type=str, default="10,20",
                    help="Comma-separated list of N-gram window sizes for memorization checks.")
    ap.add_argument("--max_train_audit_tokens", type=int, default=10000000,
                    help="Maximum training tokens to index (the reference's cap); 0 indexes everything.")
    ap.add_argument("--ckpt", default="best.pt", help="Which checkpoint to use (e.g., best.pt or last.pt)")
    ap.add_argument("--critic_stability", action="store_true", default=False)
    ap.add_argument("--critic_ckpt", default="runs/protein_critic/checkpoints/best_critic.pt")
    ap.add_argument("--critic_cfg", default="configs/protein_critic.yaml")
    ap.add_argument("--critic_guidance", action="store_true", default=False)
    ap.add_argument("--ebm_guidance", action="store_true", default=False)
    ap.add_argument("--ebm_ckpt", default="runs/protein_ebm_1024/checkpoints/best_ebm.pt")
    ap.add_argument("--ebm_hidden_dim", type=int, default=1024)
    ap.add_argument("--guide_alpha", type=float, default=0.5)
    ap.add_argument("--guide_top_k", type=int, default=5)
    ap.add_argument("--target_protein", type=str, default=None)
    return ap


def settings_from(args, run_id: str, cfg: Dict) -> GP.Settings:
    """The argument checks that need no device, and the Settings of the run."""
    for flag in ("critic_stability", "critic_guidance", "ebm_guidance"):
        if getattr(args, flag):
            raise SystemExit(f"[gen-prefix] --{flag}: the protein critic / EBM are not part of codonlm_amd; "
                             "run the benchmark without them")
    if args.target_protein:
        raise SystemExit("[gen-prefix] --target_protein is not part of this tool; "
                         "generate.generate_cds_synonymous writes a CDS for a given protein")
    if not (0 < args.min_aa_len <= args.target_aa_len <= args.max_aa_len):
        raise SystemExit("require 0 < min_aa_len ≤ target_aa_len ≤ max_aa_len")
    from .sample import resolve_offset_prior_weights
    preset = GP.PRESETS.get(args.preset or "full", {})
    pick = lambda v, key: int(v if v is not None else preset[key])  # noqa: E731
    return GP.Settings(
        run_id=run_id, k_list=tuple(int(x) for x in args.k_list.split(",") if x),
        samples=pick(args.samples, "samples"), max_new=pick(args.max_new, "max_new"),
        temperature=float(args.temperature), topk=int(args.topk), seed=int(args.seed),
        ci_resamples=int(args.ci_resamples), min_aa_len=args.min_aa_len, target_aa_len=args.target_aa_len,
        max_aa_len=args.max_aa_len, require_terminal_stop=bool(args.require_terminal_stop),
        special_margin=int(args.special_margin), termination_bias=bool(args.termination_bias),
        termination_stop_bias=float(args.termination_stop_bias),
        termination_trigger_class_max=int(args.termination_trigger_class_max),
        termination_bias_window=int(args.termination_bias_window), allow_non_cds_tokens=bool(args.allow_non_cds_tokens),
        multi_offset_prior=bool(args.multi_offset_prior),
        multi_offset_prior_weights=resolve_offset_prior_weights(args.multi_offset_prior, args.multi_offset_prior_weights,
                                                                cfg),
        gqs_normalize=args.gqs_normalize, memorization_audit=bool(args.memorization_audit),
        batch_size=int(args.batch_size), guide_top_k=int(args.guide_top_k))


def frozen_split_cds(run_dir: Path, manifest_path: Path, split: str, max_genes: int, seed: int) -> Tuple[Path, dict]:
    """The CDS of one frozen split (:209-274): records grouped by genome, each group shuffled with
    random.Random(seed), then taken round-robin over the sorted groups up to ``max_genes``."""
    from .provenance import manifest_artifact_path
    manifest = json.loads(manifest_path.read_text())
    resolved = manifest_path.expanduser().resolve()
    metadata_path = manifest_artifact_path(manifest, resolved, "source_metadata")
    dna_path = manifest_artifact_path(manifest, resolved, "source_dna")
    grouped: Dict[str, List[Tuple[str, str]]] = {}
    with metadata_path.open(newline="") as meta, dna_path.open() as dna:
        for index, (row, sequence) in enumerate(zip(csv.DictReader(meta, delimiter="\t"), dna)):
            if int(row["line_idx"]) != index:
                raise ValueError(f"source metadata line_idx mismatch at row {index}: {row['line_idx']}")
            if row["split"] != split:
                continue
            group = row.get("genome") or row.get("source_id") or "unknown"
            grouped.setdefault(group, []).append((row.get("source_id") or f"record-{index}", sequence.strip()))
    if not grouped:
        raise ValueError(f"frozen manifest contains no records for split {split!r}")
    rng = random.Random(seed)
    for records in grouped.values():
        rng.shuffle(records)
    names = sorted(grouped)
    selected: List[Tuple[str, str, str]] = []
    cursor = 0
    while len(selected) < max_genes:
        progress = False
        for group in names:
            if cursor < len(grouped[group]):
                source_id, sequence = grouped[group][cursor]
                selected.append((source_id, group, sequence))
                progress = True
                if len(selected) >= max_genes:
                    break
        if not progress:
            break
        cursor += 1
    out_path = run_dir / "scores" / f"_eval_{split}_cds_dna.txt"
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("".join(f"{sequence}\n" for _, _, sequence in selected))
    return out_path, {
        "manifest": str(resolved), "manifest_sha256": hashlib.sha256(resolved.read_bytes()).hexdigest(),
        "split": split, "selection": "seeded_shuffle_then_round_robin_by_genome", "seed": seed,
        "available_groups": names,
        "selected_group_counts": {g: sum(1 for _, sg, _ in selected if sg == g) for g in names},
        "selected_source_ids": [source_id for source_id, _, _ in selected]}


def resolve_cds_path(args, run_dir: Path, cfg: Dict, max_genes: int) -> Tuple[Optional[Path], dict]:
    if args.cds_file is not None:
        return Path(args.cds_file), {"status": "explicit_cds_file"}
    configured = args.dataset_manifest or (Path(str(cfg["dataset_manifest"])) if cfg.get("dataset_manifest") else None)
    if configured is not None and Path(configured).exists():
        return frozen_split_cds(run_dir, Path(configured), args.source_split, max_genes, int(args.seed))
    combined = run_dir / "combined_manifest.json"
    if combined.exists():
        datasets = json.loads(combined.read_text()).get("datasets") or []
        if datasets and datasets[0].get("dna") and Path(datasets[0]["dna"]).exists():
            return Path(datasets[0]["dna"]), {"status": "legacy_unverified"}
    for key in ("dna_path", "cds_dna", "primary_dna"):
        if cfg.get(key) and Path(str(cfg[key])).exists():
            return Path(str(cfg[key])), {"status": "legacy_unverified"}
    return None, {"status": "unresolved"}


def load_cds(path: Path, max_genes: int) -> List[str]:
    cds = []
    with open(path) as f:
        for line in f:
            s = line.strip().upper().replace("U", "T")
            if len(s) >= 9:
                cds.append(s)
            if len(cds) >= max_genes:
                break
    return cds


def main(argv=None) -> Dict[str, Path]:
    args = build_parser().parse_args(argv)
    run_dir = Path(args.run_dir)
    from . import memorization as M, query_model as Q
    from .checkpoints import load_codon_checkpoint

    state_dict, cfg, weights_path = load_codon_checkpoint(run_dir, args.ckpt)
    s = settings_from(args, run_dir.name, cfg)
    preset = GP.PRESETS.get(args.preset or "full", {})
    max_genes = int(args.max_genes if args.max_genes is not None else preset["max_genes"])
    itos, stoi = Q._load_vocab(run_dir)
    model = Q.build_model_from_state(state_dict, cfg, compute_dtype=args.dtype, device=Q.dev())
    print(f"[gen-prefix] run_dir={run_dir} ckpt={weights_path.name} preset={args.preset or 'full'} max_genes={max_genes} "
          f"samples={s.samples} max_new={s.max_new} seed={s.seed} batch_size={s.batch_size}", flush=True)

    dna_path, provenance = resolve_cds_path(args, run_dir, cfg, max_genes)
    if dna_path is None or not dna_path.exists():
        raise SystemExit("[gen-prefix] could not locate a CDS dna file: pass --cds_file or --dataset_manifest")
    train_indices = {}
    if s.memorization_audit:
        train = args.train_npz or cfg.get("train_npz")
        paths = [Path(p) for p in (train if isinstance(train, list) else [train] if train else []) if Path(p).exists()]
        cap = int(args.max_train_audit_tokens) or None
        for n in (int(x) for x in args.memorization_n_list.split(",") if x.strip()):
            if paths:
                train_indices[n] = M.TrainIndex.from_npz(paths, n, max_tokens=cap)
                print(f"[gen-prefix] training index: {train_indices[n].n_unique} unique {n}-grams of "
                      f"{train_indices[n].tokens_indexed} tokens", flush=True)
    with open(dna_path) as f:
        usage = GP.UsageReference.from_lines(f, itos, stoi)
    cds = load_cds(dna_path, max_genes)
    samples, protocol_rows, sequences, guidance = GP.run_benchmark(model, cds, stoi, itos, s, usage, train_indices)
    record = GP.manifest(s, str(weights_path), provenance, guidance, any(r.protocol == "guided" for r in protocol_rows))
    paths = GP.write_outputs(run_dir / "scores" / args.out_label, samples, protocol_rows, sequences, s, record)
    for p in paths.values():
        print(f"[gen-prefix] wrote {p}")
    return paths


if __name__ == "__main__":
    main()
