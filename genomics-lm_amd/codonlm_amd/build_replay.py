#!/usr/bin/env python3
"""Build generated-prefix replay data on the MI355X (replaces scripts/build_generated_prefix_replay.py).

    python -m codonlm_amd.build_replay --run_dir runs/<RUN_ID> --dna cds.txt [--out replay.jsonl]

From every CDS of --dna (one sequence per line) and every prefix length of --k_list, --samples
continuations are generated; a continuation that reaches the hard cap without a terminal stop is kept
and its last --replay_window generated states are labelled with the distance bucket to the stop that
should have come next (replay.replay_labels).  The output is the reference's JSONL (one record per
kept continuation, the same keys) with its .summary.json beside it; both the reference's loader and
replay.GeneratedTerminationReplayDataset read it.

All (gene, k, sample) jobs run as on-device batches (generate.generate_batch /
generate._constrained_batch), --batch jobs at a time.  Job j draws from stream j of --seed, and a
sequence's draws depend on (seed, stream, step) only, so the output does not depend on --batch.
The reference resolves the CDS file from dataset manifests and presets; here --dna is required.
"""
from __future__ import annotations

import argparse
import json
from collections import Counter
from pathlib import Path
from typing import Callable, Dict, List, Sequence, Tuple

from .replay import replay_labels


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Collect hard-cap generation failures as termination-head replay data.")
    ap.add_argument("--run_dir", required=True)
    ap.add_argument("--dna", required=True, help="file of CDS DNA sequences, one per line")
    ap.add_argument("--ckpt", default="best.pt")
    ap.add_argument("--k_list", default="1,3,5,10")
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--max_genes", type=int, default=10)
    ap.add_argument("--max_new", type=int, default=100)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--topk", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1337)
    ap.add_argument("--min_aa_len", type=int, default=100)
    ap.add_argument("--target_aa_len", type=int, default=256)
    ap.add_argument("--max_aa_len", type=int, default=400)
    ap.add_argument("--special_margin", type=int, default=6)
    ap.add_argument("--replay_window", type=int, default=30)
    ap.add_argument("--bucket_edges", default="0,3,10,30")
    ap.add_argument("--decoder", choices=("raw", "cds_constrained"), default="cds_constrained",
                    help="generation distribution used to collect hard-cap failures")
    ap.add_argument("--out", default=None)
    ap.add_argument("--allow_non_cds_tokens", action="store_true",
                    help="permit non-codon tokens during CDS continuation generation")
    ap.add_argument("--allow_empty", action="store_true",
                    help="write an empty replay file instead of failing when no hard-cap failure is found")
    ap.add_argument("--batch", type=int, default=64, help="jobs per on-device batch")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    return ap


def read_cds(path: Path, max_genes: int) -> List[str]:
    cds = []
    with Path(path).open() as fh:
        for line in fh:
            seq = line.strip().upper().replace("U", "T")
            if len(seq) >= 9:
                cds.append(seq)
            if len(cds) >= max_genes:
                break
    return cds


def plan_jobs(cds: Sequence[str], k_list: Sequence[int], samples: int, block_size: int, args,
              to_ids: Callable[[str], List[int]]) -> List[Dict]:
    """One job per (gene, k, sample) in the reference's loop order, with its caps
    (build_generated_prefix_replay.py:179-190) and its stream id = its place in that order."""
    jobs = []
    for gene_idx, dna in enumerate(cds):
        n_codons = len(dna) // 3
        for k in k_list:
            prefix_k = min(int(k), n_codons)
            ctx = to_ids(dna[: 3 * prefix_k])
            room = int(block_size) - prefix_k - int(args.special_margin)
            if room < args.min_aa_len:
                raise ValueError("block_size too small for requested replay generation lengths")
            hard_cap = int(min(room, args.max_aa_len, args.max_new))
            target = int(max(args.min_aa_len, min(args.target_aa_len, hard_cap)))
            for sample_id in range(int(samples)):
                jobs.append({"gene_idx": gene_idx, "k": prefix_k, "sample_id": sample_id, "ctx": ctx,
                             "hard_cap": hard_cap, "target_codons": target, "stream": len(jobs)})
    return jobs


def collect(jobs: Sequence[Dict], generate: Callable[[List[Dict]], List[Tuple[List[int], Dict]]], args,
            bucket_edges: Sequence[int], out_fh, source_run_id: str) -> Dict:
    """Run the jobs ``--batch`` at a time through ``generate`` (a list of jobs with equal caps ->
    [(ids, info)]), keep hard_cap-without-stop continuations and write their records
    (build_generated_prefix_replay.py:216-245).  Returns the counters of the summary."""
    done = written = hard_caps = terminal_stops = 0
    class_counts: Counter = Counter()
    # jobs of one batch share their caps (they are launch parameters); the order of the records
    # stays the job order
    results: Dict[int, Tuple[List[int], Dict]] = {}
    groups: Dict[Tuple[int, int], List[Dict]] = {}
    for job in jobs:
        groups.setdefault((job["hard_cap"], job["target_codons"]), []).append(job)
    for group in groups.values():
        for i in range(0, len(group), max(1, int(args.batch))):
            part = group[i: i + max(1, int(args.batch))]
            for job, res in zip(part, generate(part)):
                results[job["stream"]] = res
    for job in jobs:
        ids, info = results[job["stream"]]
        done += 1
        if info.get("had_terminal_stop"):
            terminal_stops += 1
        if not (info.get("hit_hard_cap") and not info.get("had_terminal_stop")):
            continue
        hard_caps += 1
        labels = replay_labels(len(ids), len(job["ctx"]), int(args.replay_window), bucket_edges)
        if not labels:
            continue
        class_counts.update(item["class"] for item in labels)
        record = {"source_run_id": source_run_id, "source_ckpt": args.ckpt, "gene_idx": job["gene_idx"],
                  "k": job["k"], "sample_id": job["sample_id"], "ids": [int(t) for t in ids], "labels": labels,
                  "target_codons": int(job["target_codons"]),
                  "generated_codons": int(info.get("generated_codons", 0)), "hard_cap": int(job["hard_cap"]),
                  "decoder": args.decoder, "synthetic_boundary": "next_token_after_failed_prefix",
                  "last_termination_class": info.get("last_termination_class")}
        out_fh.write(json.dumps(record, separators=(",", ":")) + "\n")
        written += 1
    return {"generated_samples": done, "hard_cap_without_stop": hard_caps, "terminal_stops": terminal_stops,
            "records_written": written,
            "label_class_counts": {str(c): int(class_counts[c]) for c in range(len(bucket_edges) + 1)}}


def build(args, cds: Sequence[str], block_size: int, to_ids, generate, out_path: Path, source_run_id: str) -> Dict:
    """jobs -> records at out_path and the summary beside it; returns the summary."""
    if not (0 < args.min_aa_len <= args.target_aa_len <= args.max_aa_len):
        raise SystemExit("require 0 < min_aa_len <= target_aa_len <= max_aa_len")
    k_list = [int(x) for x in str(args.k_list).split(",") if x]
    bucket_edges = tuple(int(x) for x in str(args.bucket_edges).split(",") if x)
    if bucket_edges != tuple(sorted(bucket_edges)):
        raise SystemExit("--bucket_edges must be sorted")
    jobs = plan_jobs(cds, k_list, int(args.samples), block_size, args, to_ids)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    with out_path.open("w") as fh:
        counts = collect(jobs, generate, args, bucket_edges, fh, source_run_id)
    summary = {"run_id": source_run_id, "ckpt": args.ckpt, "device": "cuda", "samples": int(args.samples),
               "max_genes": int(args.max_genes), "k_list": k_list, **counts, "decoder": args.decoder,
               "replay_window": int(args.replay_window), "bucket_edges": list(bucket_edges),
               "cds_only": args.decoder == "cds_constrained" and not bool(args.allow_non_cds_tokens),
               "out": str(out_path)}
    summary_path = out_path.with_suffix(".summary.json")
    summary_path.write_text(json.dumps(summary, indent=2, sort_keys=True) + "\n")
    if counts["records_written"] == 0 and not args.allow_empty:
        raise SystemExit("[replay] no hard-cap replay records were written; use --allow_empty only when this is "
                         "expected")
    print(f"[replay] wrote {out_path}")
    print(f"[replay] wrote {summary_path}")
    return summary


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    from . import query_model as Q
    from .checkpoints import load_codon_checkpoint
    from .generate import _constrained_batch, generate_batch, raw_info

    run_dir = Path(args.run_dir)
    itos, stoi = Q._load_vocab(run_dir)
    state_dict, cfg, _ = load_codon_checkpoint(run_dir, args.ckpt)
    model = Q.build_model_from_state(state_dict, cfg, compute_dtype=args.dtype, device=Q.dev())
    model.eval()
    seed, topk = int(args.seed), int(args.topk) if args.topk > 0 else 0

    def generate(part):
        contexts = [job["ctx"] for job in part]
        streams = [job["stream"] for job in part]
        hard_cap, target = part[0]["hard_cap"], part[0]["target_codons"]
        if args.decoder == "raw":
            res = generate_batch(model, contexts, stoi, itos, seed=seed, streams=streams, max_tokens=hard_cap,
                                 temperature=float(args.temperature), topk=topk)
            return [(ids, raw_info(rec, hard_cap)) for ids, rec in res]
        return _constrained_batch(model, contexts, stoi, itos, target, hard_cap, require_terminal_stop=True,
                                  temperature=float(args.temperature), topk=topk, termination_bias_enabled=False,
                                  termination_stop_bias=0.0, termination_trigger_class_max=0,
                                  termination_bias_window=0, cds_only=not bool(args.allow_non_cds_tokens), seed=seed,
                                  streams=streams)

    cds = read_cds(Path(args.dna), int(args.max_genes))
    out_path = Path(args.out) if args.out else run_dir / "scores" / "generated_prefix_replay.jsonl"
    build(args, cds, int(cfg.get("block_size", model.block_size)), lambda dna: Q.dna_prefix_to_ids(dna, stoi),
          generate, out_path, run_dir.name)


if __name__ == "__main__":
    main()
