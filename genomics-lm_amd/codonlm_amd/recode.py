#!/usr/bin/env python3
"""Synonymous recoding (codon optimisation) of a protein or a CDS on the MI355X.

    python -m codonlm_amd.recode --run_dir runs/<ID> --protein MKAQLLV --n 64 --top 5
    python -m codonlm_amd.recode --ckpt runs/<ID>/checkpoints/best.pt --dna cds.fasta --keep 10-20,35-40 \\
        --out recoded.tsv

``--n`` candidate CDSs that translate exactly to the protein are drawn as on-device batches
(generate.generate_batch through cg_sample_step_plan: every step of every candidate has its own
synonymous codon set and the sampler returns the log-probability of what it drew), then ranked by
the model's log-probability ``logp_model``.  ``--dna`` recodes the translation of a CDS; ``--keep``
lists half-open codon-index ranges (0-based, ``a-b`` = codons a .. b-1) that stay as given.
``--topk 1`` is the deterministic greedy recoding.  TSV columns: ``rank logp_model logp_draw dna``.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path
from typing import Dict, List, Sequence, Tuple

from . import generate as G


def _run(model, targets, stoi, itos, sets, *, n, seed, temperature, topk, prefix, max_batch):
    """targets: [(protein, plan)].  Per target the n candidates, best logp_model first."""
    n, max_batch = int(n), int(max_batch)
    if n < 1 or max_batch < 1:
        raise ValueError("n and max_batch must be at least 1")
    prefix = [int(stoi.get("<BOS_CDS>", 1))] if prefix is None else [int(t) for t in prefix]
    jobs = [(i, i * n + c) for i in range(len(targets)) for c in range(n)]
    table = sets.array()
    out: List[List[dict]] = [[] for _ in targets]
    for at in range(0, len(jobs), max_batch):
        part = jobs[at:at + max_batch]
        res = G.generate_batch(model, [prefix] * len(part), stoi, itos, seed=seed, streams=[s for _, s in part],
                               max_tokens=G.INT_MAX, temperature=temperature, topk=topk, stop_on_eos=False,
                               stop_on_bio_stop=False, token_sets=table, plans=[targets[i][1] for i, _ in part],
                               end_with_plan=True, with_logp=True)
        for (i, stream), (ids, rec) in zip(part, res):
            protein = targets[i][0]
            codons = [itos[t] if 0 <= t < len(itos) else f"<{t}>" for t in ids[len(prefix):]]
            if G.translate(codons) != protein + "_":
                raise RuntimeError(f"candidate {stream} translates to {G.translate(codons)!r}, not {protein + '_'!r}")
            out[i].append({"ids": ids, "codons": codons, "dna": "".join(codons), "logp_model": rec["logp_model"],
                           "logp_draw": rec["logp_draw"], "stream": stream})
    for cands in out:
        cands.sort(key=lambda c: (-c["logp_model"], c["stream"]))
    return out


def recode_proteins(model, proteins: Sequence[str], stoi: Dict[str, int], itos: List[str], *, n: int = 1,
                    seed: int = 0, temperature: float = 1.0, topk: int = 0, prefix: Sequence[int] | None = None,
                    max_batch: int = 256) -> List[List[dict]]:
    """``n`` recodings of every protein, in batches of at most ``max_batch`` sequences; candidate c
    of protein i draws with stream i*n + c of ``seed``.  Per protein, the candidates sorted by
    ``logp_model`` descending (ties by stream): dicts of ``ids`` (prefix + generated tokens),
    ``codons``, ``dna``, ``logp_model``, ``logp_draw`` and ``stream``.  ``prefix`` defaults to
    <BOS_CDS>.  Every candidate is checked to translate to its protein plus a stop.  A residue
    that no codon of the vocabulary encodes is a ValueError."""
    sets = G.TokenSets(stoi, itos, int(model.vocab_size))
    proteins = [str(p).strip().upper() for p in proteins]
    targets = [(p, G.synonymous_plan(sets, p, strict=True)) for p in proteins]
    return _run(model, targets, stoi, itos, sets, n=n, seed=seed, temperature=temperature, topk=topk, prefix=prefix,
                max_batch=max_batch)


def dna_codons(dna: str) -> List[str]:
    """The codons of a CDS (upper-cased, U read as T) without its trailing stop codon, if any."""
    dna = "".join(dna.split()).upper().replace("U", "T")
    if len(dna) % 3:
        raise ValueError(f"DNA of {len(dna)} bases is not a whole number of codons")
    codons = [dna[i:i + 3] for i in range(0, len(dna), 3)]
    if codons and codons[-1] in G.STOP_CODONS:
        codons.pop()
    for k, c in enumerate(codons):
        if G.CODON_TABLE.get(c, "_") == "_":
            raise ValueError(f"codon {k} ({c!r}) is {'a stop' if c in G.STOP_CODONS else 'no codon'}")
    return codons


def dna_plan(sets: G.TokenSets, codons: Sequence[str], keep=None) -> Tuple[str, List[int]]:
    """(protein, plan) of a CDS: the synonymous set per codon, a one-token set inside ``keep``."""
    kept = set()
    for a, b in keep or []:
        a, b = int(a), int(b)
        if not 0 <= a < b <= len(codons):
            raise ValueError(f"keep range {a}-{b} outside the {len(codons)} codons")
        kept.update(range(a, b))
    plan = []
    for k, c in enumerate(codons):
        if k in kept:
            if c not in sets.stoi:
                raise ValueError(f"kept codon {k} ({c}) is not in the vocabulary")
            plan.append(sets.token(sets.stoi[c]))
        else:
            plan.append(sets.residue(G.CODON_TABLE[c], strict=True))
    return G.translate(codons), plan + [sets.stop()]


def recode_dna(model, dna: str, stoi: Dict[str, int], itos: List[str], *, n: int = 1, seed: int = 0,
               temperature: float = 1.0, topk: int = 0, prefix: Sequence[int] | None = None, max_batch: int = 256,
               keep=None) -> List[dict]:
    """The candidates of recode_proteins for the translation of ``dna`` (a whole number of codons,
    with or without its stop).  ``keep``: half-open codon-index ranges whose codons stay as given
    (one-token sets on the same kernel path)."""
    sets = G.TokenSets(stoi, itos, int(model.vocab_size))
    target = dna_plan(sets, dna_codons(dna), keep)
    return _run(model, [target], stoi, itos, sets, n=n, seed=seed, temperature=temperature, topk=topk,
                prefix=prefix, max_batch=max_batch)[0]


def parse_keep(text: str | None) -> List[Tuple[int, int]]:
    """"10-20,35-40" -> [(10, 20), (35, 40)]"""
    out = []
    for part in (text or "").split(","):
        if part.strip():
            a, b = part.split("-")
            out.append((int(a), int(b)))
    return out


def read_protein(arg: str) -> str:
    """``arg`` itself when it is a short string of letters, else the file it names: raw, or FASTA
    whose header lines are skipped."""
    if len(arg) <= 80 and arg.isalpha() and not Path(arg).exists():
        return arg
    lines = Path(arg).read_text().splitlines()
    return "".join(ln.strip() for ln in lines if not ln.startswith(">")).strip().rstrip("*")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Synonymous recodings of a protein or CDS, ranked by the model.")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt", help="checkpoint file (best.pt)")
    src.add_argument("--run_dir", help="run directory holding checkpoints/best.pt and itos.txt")
    what = ap.add_mutually_exclusive_group(required=True)
    what.add_argument("--protein", help="amino-acid string or path to file (raw or FASTA)")
    what.add_argument("--dna", help="DNA string (ACGT...) or path to file (raw or FASTA)")
    ap.add_argument("--n", type=int, default=64, help="number of candidates")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--topk", type=int, default=0)
    ap.add_argument("--keep", default=None, help="codon ranges of --dna to keep, e.g. 10-20,35-40 (half-open)")
    ap.add_argument("--top", type=int, default=5, help="number of ranked candidates to write")
    ap.add_argument("--out", default=None, help="write the TSV here (default: standard output)")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    return ap


def tsv_rows(cands: Sequence[dict], top: int) -> List[list]:
    rows = [["rank", "logp_model", "logp_draw", "dna"]]
    for r, c in enumerate(cands[:max(0, int(top))], 1):
        rows.append([r, f"{c['logp_model']:.4f}", f"{c['logp_draw']:.4f}", c["dna"]])
    return rows


def main(argv=None) -> List[dict]:
    args = build_parser().parse_args(argv)
    if args.keep and not args.dna:
        raise SystemExit("--keep needs --dna")
    from . import score_mutations as M
    ckpt = Path(args.ckpt) if args.ckpt else None
    run_dir = Path(args.run_dir) if args.run_dir else None
    model, _ = M.load_model(ckpt, run_dir, args.dtype)
    model.eval()
    itos = M.load_vocab(ckpt, run_dir)
    stoi = {t: i for i, t in enumerate(itos)}
    kw = dict(n=args.n, seed=args.seed, temperature=args.temperature, topk=args.topk)
    if args.dna:
        cands = recode_dna(model, M.read_dna(args.dna), stoi, itos, keep=parse_keep(args.keep), **kw)
    else:
        cands = recode_proteins(model, [read_protein(args.protein)], stoi, itos, **kw)[0]
    rows = tsv_rows(cands, args.top)
    if args.out:
        M.write_tsv(Path(args.out), rows)
        print(f"[save] {args.out}")
    else:
        for row in rows:
            sys.stdout.write("\t".join(str(v) for v in row) + "\n")
    return cands


if __name__ == "__main__":
    main()
