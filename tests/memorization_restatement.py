"""Python-set restatement of the window index (cg_ngram_index_build / cg_ngram_coverage) and the case
generator the CPU fixture and the GPU tests share.

build() is the reference's set of windows (eval_generation_prefix.py _build_train_ngram_set,
leakage_audit.matching_substring_coverage), coverage() its walk over a generated sequence
(_training_match_coverage, _coverage_from_index) with the integers the kernels return instead of the
final division.  Sequences are uint8 numpy arrays; a window is the bytes of n consecutive symbols.
"""
from __future__ import annotations

import numpy as np

BUILD_N = (1, 3, 10, 20, 32)
ALPHABETS = (1, 2, 64)
OUTSIDE = 255  # a symbol no generated alphabet holds


def windows_of(seq, n):
    b = np.asarray(seq, dtype=np.uint8).tobytes()
    return [b[s:s + n] for s in range(len(b) - n + 1)]


def build(seqs, n, lo=0, hi=None):
    """The set of windows of seqs[lo:hi]; len() of it is n_unique."""
    out = set()
    for s in seqs[lo:hi]:
        out.update(windows_of(s, n))
    return out


def window_total(seqs, n):
    return sum(max(0, len(s) - n + 1) for s in seqs)


def coverage(seq, table, n):
    """(hit uint8 [len], n_hit, covered) of one query."""
    L = len(seq)
    hit = np.zeros(L, dtype=np.uint8)
    cov = np.zeros(L, dtype=np.uint8)
    for s, w in enumerate(windows_of(seq, n)):
        if w in table:
            hit[s] = 1
            cov[s:s + n] = 1
    return hit, int(hit.sum()), int(cov.sum())


def fraction(seq, table, n):
    """The reference's coverage: covered / len, 0.0 for a query shorter than the window."""
    return coverage(seq, table, n)[2] / len(seq) if len(seq) >= n and table else 0.0


def training_set(n, alphabet, seed=0):
    """Sequences of lengths {0, n-1, n, n+1, 2n, 257, 1000} (windows at a 256-position tile edge and
    at both ends of a sequence), two of them twice, in a fixed shuffled order."""
    rng = np.random.default_rng([seed, n, alphabet])
    lens = [0, n - 1, n, n + 1, 2 * n, 257, 1000, 0, n]
    order = rng.permutation(len(lens))
    return [rng.integers(0, alphabet, size=lens[i]).astype(np.uint8) for i in order]


def distinct_training_set(n, seed=0):
    """A set whose windows are all distinct (asserted), for the tight-capacity build."""
    rng = np.random.default_rng([seed, n, 7])
    if n == 1:
        seqs = [rng.permutation(200).astype(np.uint8)[:150], np.arange(200, 250, dtype=np.uint8)]
    else:
        seqs = [rng.integers(0, 251, size=k).astype(np.uint8) for k in (n, 257, 0, 700, n + 1)]
    assert len(build(seqs, n)) == window_total(seqs, n), "the windows of this set must all be distinct"
    return seqs


def tight_capacity(windows):
    """The smallest power of two strictly above ``windows``."""
    c = 2
    while c <= windows:
        c *= 2
    return c


def longest(seqs):
    return max(seqs, key=len)


def queries(n, alphabet, train, seed=0):
    """{name: query}: lengths {0, n-1, n, 3n+1, 1000} drawn from the alphabet, a verbatim copy of the
    longest training sequence, that copy with its middle symbol replaced by one outside the alphabet, and
    the concatenation of two training sequences (its boundary-spanning windows are no training windows
    unless they occur elsewhere)."""
    rng = np.random.default_rng([seed, n, alphabet, 1])
    out = {f"len{k}": rng.integers(0, alphabet, size=k).astype(np.uint8) for k in (0, n - 1, n, 3 * n + 1, 1000)}
    copy = longest(train).copy()
    out["copy"] = copy
    mutated = copy.copy()
    mutated[len(mutated) // 2] = OUTSIDE
    out["mutated"] = mutated
    by_len = sorted(train, key=len)
    out["concat"] = np.concatenate([by_len[-2], by_len[-3]])
    return out


def partial_hit_case(n, seed=0):
    """(training set, queries) over 4 symbols sized so that some, not all, query windows are training
    windows; the caller asserts 0 < hits < windows on the restatement's own result."""
    rng = np.random.default_rng([seed, n, 4])
    size = {5: 300, 10: 6000}[n]
    train = [rng.integers(0, 4, size=size).astype(np.uint8), rng.integers(0, 4, size=n + 3).astype(np.uint8)]
    qs = [rng.integers(0, 4, size=k).astype(np.uint8) for k in (1000, 700, 3 * n + 1)]
    return train, qs


# ------------------------------------------------------------------ the fixture's cases
NUCLEOTIDES = "ACGT"
AMINO = "ACDEFGHIKLMNPQRSTVWY"


def _text(symbols, letters):
    return "".join(letters[int(s)] for s in symbols)


def string_cases(seed=3):
    """Cases of leakage_audit's string functions: (name, window, training strings, query strings)."""
    out = []
    for name, letters, window, alphabet in (("nucleotide", NUCLEOTIDES, 30, 4), ("protein", AMINO, 10, 20),
                                            ("low_complexity", NUCLEOTIDES, 10, 2)):
        train = training_set(window, alphabet, seed)
        q = queries(window, alphabet, train, seed)
        q["mutated"][len(q["mutated"]) // 2] = (int(q["copy"][len(q["copy"]) // 2]) + 1) % len(letters)
        out.append((name, window, [_text(s, letters) for s in train], [_text(s, letters) for s in q.values()]))
    return out


def token_cases(seed=5):
    """Cases of _training_match_coverage: (n, training id lists, query id lists) over codon ids 4..67."""
    out = []
    for n in (3, 10, 20):
        train = training_set(n, 64, seed)
        q = queries(n, 64, train, seed)
        q["mutated"][len(q["mutated"]) // 2] = 200  # id 204: no codon id
        out.append((n, [(s.astype(np.int64) + 4).tolist() for s in train],
                    [(s.astype(np.int64) + 4).tolist() for s in q.values()]))
    return out
