#!/usr/bin/env python3
"""Record what the REAL reference returns for the metric functions of the prefix-generation benchmark and
for the window functions of its leakage audit, on the cases of tests/memorization_restatement.py.

Run once where the reference checkout is available (GENOMICS_LM_REFERENCE, default /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gen_prefix.py

It calls scripts/eval_generation_prefix.py's _sample_seed, _bootstrap_interval, _score_stop_behavior,
_ngram_repeat_ratio, _training_match_coverage and _codon_to_aa, and src/codonlm/leakage_audit.py's
matching_substring_coverage, _coverage_from_index and _matched_query_windows, and writes
gen_prefix.npz next to this script: one JSON document of inputs and returns, no reference code.

leakage_audit imports Biopython, which is not installed here; an empty stand-in for Bio.Seq goes into
sys.modules before the import, so translate_cds (the only user of Bio) is NOT recorded.
"""
from __future__ import annotations

import json
import os
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
REF = os.environ.get("GENOMICS_LM_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

if "Bio" not in sys.modules:
    bio, bio_seq = types.ModuleType("Bio"), types.ModuleType("Bio.Seq")
    bio_seq.Seq = None
    bio.Seq = bio_seq
    sys.modules["Bio"], sys.modules["Bio.Seq"] = bio, bio_seq

import memorization_restatement as MR  # noqa: E402
from scripts import eval_generation_prefix as E  # noqa: E402  (reference)
from src.codonlm import leakage_audit as A  # noqa: E402  (reference)

CODONS = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]


def main() -> None:
    rng = np.random.default_rng(20)
    doc = {}
    seeds = [(1337, 0, 1, 0), (1337, 49, 10, 4), (0, 0, 0, 0), (7, 3, 5, 2), (2 ** 31, 12, 3, 1), (1337, 1, 1, 300)]
    doc["sample_seed"] = [{"args": list(a), "out": E._sample_seed(*a)} for a in seeds]

    boots = []
    for values, statistic, seed, n in (
            ([], "mean", 1, 100), ([3.5], "median", 2, 100), ([1.0, 2.0, 4.0], "mean", 3, 0),
            (rng.uniform(0, 100, size=30).tolist(), "median", E._sample_seed(1337, 1, 3, 30), 1000),
            (rng.uniform(0, 100, size=30).tolist(), "mean", 12345, 1000),
            ([float(v) for v in rng.integers(0, 2, size=17)], "mean", 99, 250),
            ([float(v) for v in rng.integers(50, 300, size=8)], "mean", 4, 1000)):
        low, high = E._bootstrap_interval(values, statistic=statistic, seed=seed, n_resamples=n)
        boots.append({"values": values, "statistic": statistic, "seed": seed, "n_resamples": n, "out": [low, high]})
    doc["bootstrap_interval"] = boots

    def codons(k):
        return [CODONS[int(i)] for i in rng.integers(0, 64, size=k)]

    sense = [c for c in CODONS if c not in ("TAA", "TAG", "TGA")]

    def sense_codons(k):
        return [sense[int(i)] for i in rng.integers(0, len(sense), size=k)]

    stop_cases = [([], 10), (["TAA"], 1), (sense_codons(20) + ["TGA"], 21), (sense_codons(5) + ["TAG"] + sense_codons(20) + ["TAA"], 40),
                  (sense_codons(30), 30), (sense_codons(30), 33), (sense_codons(30), 100), (sense_codons(12), 10),
                  (sense_codons(38) + ["TAA"] + sense_codons(3) + ["TGA"], 40), (sense_codons(2) + ["TAA", "ATG"], 0),
                  (codons(60), 50)]
    doc["score_stop_behavior"] = [{"codons": c, "truth_len": t, "out": list(E._score_stop_behavior(c, t))}
                                  for c, t in stop_cases]

    rep_cases = [([], 3), (["ATG", "AAA"], 3), (["ATG", "AAA", "CCC"], 3), (["AAA"] * 9, 3), (["AAA"] * 10, 3),
                 (["ATG", "AAA", "CCC"] * 4 + ["GGG"], 3), (codons(31), 3), (codons(12), 2), (["AAA", "CCC"] * 5, 2)]
    doc["ngram_repeat_ratio"] = [{"tokens": t, "n": n, "out": E._ngram_repeat_ratio(t, n=n)} for t, n in rep_cases]

    doc["codon_to_aa"] = [{"codon": c, "out": E._codon_to_aa(c)} for c in CODONS + ["NNN", "AT", "<EOS_CDS>", "atg"]]

    tok = []
    for n, train, queries in MR.token_cases():
        table = {tuple(seq[s:s + n]) for seq in train for s in range(len(seq) - n + 1)}
        tok.append({"n": n, "training": train, "queries": queries,
                    "out": [E._training_match_coverage(q, n, table) for q in queries],
                    "out_empty_index": [E._training_match_coverage(q, n, set()) for q in queries[:2]]})
    doc["training_match_coverage"] = tok

    strings = []
    for name, window, train, queries in MR.string_cases():
        matched = A._matched_query_windows(queries, train, window)
        strings.append({"name": name, "window": window, "training": train, "queries": queries,
                        "matching_substring_coverage": [A.matching_substring_coverage(q, train, window) for q in queries],
                        "matched_query_windows": sorted(matched),
                        "coverage_from_index": [A._coverage_from_index(q, matched, window) for q in queries]})
    doc["leakage_audit"] = strings

    np.savez_compressed(HERE / "gen_prefix.npz", cases=np.array(json.dumps(doc)))
    print("wrote", HERE / "gen_prefix.npz", (HERE / "gen_prefix.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
