#!/usr/bin/env python3
"""Timings of the memorization audit's window index against the Python-set build it replaces.

    python tools/bench_memorization.py [--tokens 100000 1000000 10000000] [--n 10 20] [--out result.json]

Per training-token count and window length: cg_ngram_index_build (device time of the build launch alone,
the table filled outside the timed region, and ns per window), cg_ngram_coverage of 3000 queries of 300
tokens (half of them slices of the training rows, so that hits exist), and the wall time of the library
calls a user makes (TrainIndex.from_rows, training_match_coverage: uploads and read-backs included).
Beside them, on the host and for the same inputs, the set of tuples of the reference's
_build_train_ngram_set and the walk of _training_match_coverage, with the rows turned into Python ints
first (the reference keeps numpy scalars, which is slower); ``--host-max-tokens`` bounds the sizes the
host build is run at.  Both sides must agree on the number of distinct windows and on every coverage.
Warm-up launches first, then the median of ``--repeats`` event-timed runs.  Not wired into bench.py.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "genomics-lm_amd"))

from codonlm_amd import memorization as M  # noqa: E402
from codonlm_amd import ops  # noqa: E402

DEV = "cuda"
N_QUERIES, QUERY_LEN = 3000, 300


def median_ms(fn, warmup, repeats, before=None):
    ms = []
    for i in range(warmup + repeats):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def make_inputs(tokens, T, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(4, 68, size=(max(1, tokens // T), T)).astype(np.int64)
    queries = rng.integers(4, 68, size=(N_QUERIES, QUERY_LEN)).astype(np.int64)
    if T >= QUERY_LEN:
        for q in range(0, N_QUERIES, 2):  # every other query is copied from a training row
            r, c = int(rng.integers(0, X.shape[0])), int(rng.integers(0, T - QUERY_LEN + 1))
            queries[q] = X[r, c:c + QUERY_LEN]
            queries[q, int(rng.integers(0, QUERY_LEN))] = 3  # one edited token
    return X, queries


def host_baseline(X, queries, n):
    """The reference's set of tuples and its coverage walk (rows as Python ints)."""
    t0 = time.perf_counter()
    table = set()
    for row in X.tolist():
        for start in range(len(row) - n + 1):
            table.add(tuple(row[start:start + n]))
    t1 = time.perf_counter()
    cov = np.zeros(len(queries), dtype=np.float64)
    for q, tokens in enumerate(queries.tolist()):
        covered = bytearray(len(tokens))
        for start in range(len(tokens) - n + 1):
            if tuple(tokens[start:start + n]) in table:
                covered[start:start + n] = b"\x01" * n
        cov[q] = sum(covered) / len(tokens)
    t2 = time.perf_counter()
    return {"build_s": t1 - t0, "coverage_s": t2 - t1, "n_unique": len(table)}, cov


def bench_one(X, queries, n, warmup, repeats, host):
    rows, T = X.shape
    out = {"tokens": int(X.size), "T": T, "n": n, "windows": rows * max(0, T - n + 1)}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx = M.TrainIndex.from_rows(X, n)
    unique = idx.n_unique  # a read-back: the build has finished
    t1 = time.perf_counter()
    cov = M.training_match_coverage(idx, queries)
    t2 = time.perf_counter()
    out.update(n_unique=unique, capacity=idx.index.capacity, table_MiB=idx.index.capacity * 4 / 2 ** 20,
               library_build_wall_s=t1 - t0, library_coverage_wall_s=t2 - t1)
    index = idx.index

    def refill():
        index.table.fill_(-1)
        index.n_unique.zero_()
    ms = median_ms(lambda: ops.ngram_index_build(index), warmup, repeats, before=refill)
    out["build_ms"] = ms
    out["build_ns_per_window"] = ms * 1e6 / max(1, out["windows"])
    assert int(index.n_unique.item()) == unique and int(index.n_dropped.item()) == 0
    qsym = torch.from_numpy(queries.astype(np.uint8).reshape(-1)).to(DEV)
    qoff = np.arange(N_QUERIES + 1, dtype=np.int64) * QUERY_LEN
    ms = median_ms(lambda: ops.ngram_coverage(index, qsym, qoff, want=("covered",)), warmup, repeats)
    out["coverage_ms"] = ms
    out["coverage_ns_per_window"] = ms * 1e6 / (N_QUERIES * (QUERY_LEN - n + 1))
    out["mean_coverage"] = float(cov.mean())
    if host:
        base, host_cov = host_baseline(X, queries, n)
        assert base["n_unique"] == unique, (base["n_unique"], unique)
        assert np.array_equal(host_cov, cov)
        out["host"] = base
        out["build_speedup_vs_host"] = base["build_s"] / (out["build_ms"] * 1e-3)
        out["coverage_speedup_vs_host"] = base["coverage_s"] / (out["coverage_ms"] * 1e-3)
        out["library_wall_speedup_vs_host"] = (base["build_s"] + base["coverage_s"]) / (t2 - t0)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[100_000, 1_000_000, 10_000_000])
    ap.add_argument("--n", type=int, nargs="+", default=[10, 20])
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-max-tokens", type=int, default=10_000_000,
                    help="run the host set build only up to this many training tokens")
    ap.add_argument("--out", type=Path)
    args = ap.parse_args(argv)
    result = {"device": torch.cuda.get_device_name(0), "queries": N_QUERIES, "query_len": QUERY_LEN, "runs": []}
    for tokens in args.tokens:
        X, queries = make_inputs(tokens, args.T, seed=tokens % 1000)
        for n in args.n:
            result["runs"].append(bench_one(X, queries, n, args.warmup, args.repeats, tokens <= args.host_max_tokens))
            print(json.dumps(result["runs"][-1]), flush=True)
            if args.out:
                args.out.parent.mkdir(parents=True, exist_ok=True)
                args.out.write_text(json.dumps(result, indent=2) + "\n")
    return result


if __name__ == "__main__":
    main()
