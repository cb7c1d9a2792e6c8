#!/usr/bin/env python3
"""Synonymous recoding throughput, measured on the GPU (not part of bench.py).

C4 geometry (12 layers, 8 heads, d = 512, block 1024, random weights, bf16), 256 candidates of one
300-residue protein = 301 generated tokens each, one batch:

  recode   codonlm_amd.recode.recode_proteins (cg_sample_step_plan: a synonymous set per step,
           log-probabilities, the plan ends the sequence), host translation check included
  plain    the same batch through generate_batch's constrained path (cg_sample_step, the codon
           mask, 301 tokens per sequence, stop rules off)

run alternately, host clock around calls that end in their read-back; candidates/s and tokens/s
are medians with the range.

    python tools/bench_recode.py            # one JSON line
    rocprofv3 --kernel-trace --stats -d DIR -o recode -- python tools/bench_recode.py --trace
                                            # one run of each path; per-launch kernel times of
                                            # sample_step_plan_kernel / sample_step_kernel are in
                                            # DIR/**/recode_kernel_stats.csv
"""
from __future__ import annotations

import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "genomics-lm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

V, T, N, RESIDUES, REPS = 68, 1024, 256, 300, 5


def setup():
    from codonlm_amd import TinyGPT
    from codonlm_amd import score as S
    torch.manual_seed(0)
    m = TinyGPT(V, T, n_layer=12, n_head=8, n_embd=512, dropout=0.0, compute_dtype="bf16", device="cuda").eval()
    itos = list(S.DEFAULT_VOCAB)
    stoi = {t: i for i, t in enumerate(itos)}
    rng = np.random.default_rng(0)
    protein = "M" + "".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), size=RESIDUES - 1))
    return m, stoi, itos, protein


def paths(m, stoi, itos, protein):
    from codonlm_amd import generate as G
    from codonlm_amd import recode as RC
    tokens = len(protein) + 1

    def recode():
        RC.recode_proteins(m, [protein], stoi, itos, n=N, seed=1, max_batch=N)

    def plain():
        G.generate_batch(m, [[stoi["<BOS_CDS>"]]] * N, stoi, itos, seed=1, max_tokens=tokens, cds_only=True,
                         stop_on_eos=False, stop_on_bio_stop=False)

    return recode, plain, tokens


def main(argv):
    if not torch.cuda.is_available():
        sys.exit("bench_recode.py measures on the GPU; none is visible")
    m, stoi, itos, protein = setup()
    recode, plain, tokens = paths(m, stoi, itos, protein)
    if "--trace" in argv:
        recode()
        plain()
        torch.cuda.synchronize()
        return
    for fn in (recode, plain):  # every shape of the timed window once
        fn()
    times = {"recode": [], "plain": []}
    for _ in range(REPS):
        for name, fn in (("recode", recode), ("plain", plain)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    res = {"what": "synonymous recoding vs plain constrained generation", "config": "c4 bf16", "candidates": N,
           "tokens_per_candidate": tokens, "reps": REPS}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = {"s_per_batch": round(med, 4), "candidates_per_s": round(N / med, 1),
                     "tok_per_s": round(N * tokens / med), "best_tok_per_s": round(N * tokens / min(ts)),
                     "worst_tok_per_s": round(N * tokens / max(ts))}
    res["recode_over_plain_time"] = round(statistics.median(times["recode"]) / statistics.median(times["plain"]), 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
