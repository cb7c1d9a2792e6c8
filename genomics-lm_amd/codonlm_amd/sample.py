#!/usr/bin/env python3
"""Sample sequences from a trained codon LM on the MI355X (mirrors src/codonlm/sample.py).

    python -m codonlm_amd.sample --run_dir outputs/checkpoints/<RUN_ID> \\
        --max_codons 300 --stop_on_eos --stop_on_bio_stop --prompt "ATG GCT" --n 64 --seed 1

The reference's flags (--run_dir --prompt --max_codons --stop_on_eos --stop_on_bio_stop) keep
their meaning: up to --max_codons new tokens from the whole vocabulary, ended early by <EOS_CDS>
or a stop codon when the flag is given.  --n sequences are drawn as one on-device batch
(generate.generate_batch; sequence i uses stream i of --seed), with --temperature / --topk and,
with --cds_only, the codon mask.  One line of space-separated tokens per sequence.

--multi_offset_prior adds the model's multi-offset heads to every step's logits
(eval_generation_prefix.py's flag): the weights are --multi_offset_prior_weights, a JSON object
{offset: weight}, or else the run config's ``multi_offset_weights`` (a dict, or a list zipped
with ``multi_offset_targets``).
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path
from typing import Dict, List, Optional


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Sample sequences from a trained codon LM.")
    ap.add_argument("--run_dir", required=True)
    ap.add_argument("--prompt", default="", help="space-separated codons or empty for <BOS_CDS>")
    ap.add_argument("--max_codons", type=int, default=300)
    ap.add_argument("--stop_on_eos", action="store_true")
    ap.add_argument("--stop_on_bio_stop", action="store_true")
    ap.add_argument("--n", type=int, default=1, help="number of sequences (one batch)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--topk", type=int, default=0)
    ap.add_argument("--cds_only", action="store_true", help="sample codon tokens only")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--multi_offset_prior", action="store_true",
                    help="add the multi-offset heads' logits to every step (needs a model trained with them)")
    ap.add_argument("--multi_offset_prior_weights", default=None,
                    help='JSON {offset: weight}; default: the run config\'s multi_offset_weights')
    return ap


def resolve_offset_prior_weights(enabled: bool, weights_json: Optional[str], cfg: Dict) -> Optional[Dict[int, float]]:
    """The {offset: weight} of --multi_offset_prior (eval_generation_prefix.py:802-819): None when
    the flag is off; the parsed JSON when given; else the run config's ``multi_offset_weights``, a
    dict or a list zipped with ``multi_offset_targets``; anything else (or a missing value) {}."""
    if not enabled:
        return None
    if weights_json:
        try:
            return {int(k): float(v) for k, v in json.loads(weights_json).items()}
        except Exception as exc:
            raise ValueError(f"Failed to parse --multi_offset_prior_weights: {exc}")
    raw = (cfg or {}).get("multi_offset_weights", {})
    if isinstance(raw, dict):
        return {int(k): float(v) for k, v in raw.items()}
    if isinstance(raw, (list, tuple)):
        return {int(t): float(w) for t, w in zip((cfg or {}).get("multi_offset_targets", []), raw)}
    return {}


def prompt_ids(prompt: str, stoi: Dict[str, int]) -> List[int]:
    """<BOS_CDS> + the prompt's known codons (sample.py:58-62)."""
    ids = [stoi.get("<BOS_CDS>", 1)]
    if prompt.strip():
        ids += [stoi[c] for c in (c.strip().upper() for c in prompt.split()) if c in stoi]
    return ids


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    from . import query_model as Q
    from .generate import generate_batch

    run_dir = Path(args.run_dir)
    itos, stoi = Q._load_vocab(run_dir)
    state_dict, cfg = Q._load_checkpoint(run_dir)
    model = Q.build_model_from_state(state_dict, cfg, compute_dtype=args.dtype, device=Q.dev())
    model.eval()
    ids = prompt_ids(args.prompt, stoi)
    res = generate_batch(model, [ids] * max(1, args.n), stoi, itos, seed=args.seed, max_tokens=args.max_codons,
                         temperature=args.temperature, topk=args.topk, stop_on_eos=args.stop_on_eos,
                         stop_on_bio_stop=args.stop_on_bio_stop, cds_only=args.cds_only,
                         multi_offset_prior_enabled=args.multi_offset_prior,
                         multi_offset_prior_weights=resolve_offset_prior_weights(
                             args.multi_offset_prior, args.multi_offset_prior_weights, cfg))
    for gen, _ in res:
        print(" ".join(itos[i] if 0 <= i < len(itos) else f"<{i}>" for i in gen))


if __name__ == "__main__":
    main()
