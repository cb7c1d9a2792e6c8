"""Memorization audit on the MI355X: how much of a generated sequence is copied from the training data.

The reference answers this twice with Python sets of windows: scripts/eval_generation_prefix.py puts
every 10- and 20-gram of at most 10M training tokens into a ``set`` of tuples
(_build_train_ngram_set :164-206, _training_match_coverage :472-482), and src/codonlm/leakage_audit.py
does the same over nucleotide windows of 30 and protein windows of 10 (matching_substring_coverage,
_coverage_from_index, _matched_query_windows).  Both are one operator: exact window membership over
byte symbols.  Here the training symbols stay in device memory and cg_ngram_index_build /
cg_ngram_coverage (ops.NgramIndex) answer it for any number of tokens and queries; the token cap is
kept as an option only because the reference has one.

Token ids must be below 256 (one byte per symbol); strings are their ASCII bytes.  The MMseqs2 and
minimap2 parts of the reference's audit (nearest-neighbour identities) are not part of this module.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Mapping, Optional, Sequence, Set

import numpy as np
import torch

from . import ops
from .generate import CODON_TABLE


def _device(device=None) -> torch.device:
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("the memorization audit runs on the MI355X; codonlm_amd has no CPU path")
    return dev


def pack_sequences(seqs: Sequence[np.ndarray]):
    """(flat uint8 symbols, int64 offsets [n + 1]) of host uint8 arrays."""
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = np.concatenate([np.asarray(s, dtype=np.uint8).reshape(-1) for s in seqs]) if len(seqs) \
        else np.zeros(0, dtype=np.uint8)
    return flat, offsets


def ids_to_symbols(ids) -> np.ndarray:
    """A token-id sequence as uint8 symbols; an id outside 0..255 raises ValueError."""
    a = np.asarray(ids, dtype=np.int64).reshape(-1)
    if a.size and (a.min() < 0 or a.max() > 255):
        raise ValueError("the window index holds one byte per symbol: token ids must lie in 0..255")
    return a.astype(np.uint8)


def text_to_symbols(text: str) -> np.ndarray:
    """The ASCII bytes of a nucleotide or protein string."""
    try:
        return np.frombuffer(text.encode("ascii"), dtype=np.uint8)
    except UnicodeEncodeError as exc:
        raise ValueError(f"the window index takes ASCII strings: {exc}")


def _upload(seqs: Sequence[np.ndarray], dev):
    flat, offsets = pack_sequences(seqs)
    return torch.from_numpy(flat).to(dev), offsets


class TrainIndex:
    """The windows of ``n`` symbols of a training set, on the device (ops.NgramIndex, built)."""

    def __init__(self, index: ops.NgramIndex, rows_indexed: int, tokens_indexed: int):
        self.index, self.rows_indexed, self.tokens_indexed = index, int(rows_indexed), int(tokens_indexed)

    @property
    def n(self) -> int:
        return self.index.n

    @property
    def n_unique(self) -> int:
        """The number of distinct windows (the size of the reference's set); one read-back."""
        return int(self.index.n_unique.item())

    @classmethod
    def from_sequences(cls, seqs: Sequence[np.ndarray], n: int, *, device=None, capacity=None) -> "TrainIndex":
        """Index every window of the host uint8 sequences."""
        sym, offsets = _upload(seqs, _device(device))
        index = ops.ngram_index_build(ops.NgramIndex(sym, offsets, n, capacity=capacity))
        return cls(index, len(seqs), int(offsets[-1]))

    @classmethod
    def from_rows(cls, X, n: int, max_tokens: Optional[int] = None, *, device=None) -> "TrainIndex":
        """Index the rows of the token matrix ``X`` [R][T] (a host array or a tensor) in order, each row
        one sequence.  With ``max_tokens`` the rows before the first one at which the running token
        count has reached ``max_tokens`` are indexed (eval_generation_prefix.py:186-197: the check
        precedes the row, so the row that crosses the cap is still indexed); ``None`` indexes every
        row.  An id above 255 raises ValueError."""
        dev = _device(device if device is not None else (X.device if isinstance(X, torch.Tensor) and X.is_cuda else None))
        X = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(X))
        if X.dim() != 2:
            raise ValueError("from_rows: X is a [rows][tokens] matrix")
        R, T = X.shape
        rows = R if max_tokens is None or T == 0 else min(R, -(-max(int(max_tokens), 0) // T))
        X = X[:rows].to(dev)
        if X.numel() and (int(X.min()) < 0 or int(X.max()) > 255):
            raise ValueError("the window index holds one byte per symbol: token ids must lie in 0..255")
        sym = X.to(torch.uint8).contiguous().view(-1)
        offsets = np.arange(rows + 1, dtype=np.int64) * T
        return cls(ops.ngram_index_build(ops.NgramIndex(sym, offsets, n)), rows, rows * T)

    @classmethod
    def from_npz(cls, paths, n: int, max_tokens: Optional[int] = None, *, device=None) -> "TrainIndex":
        """Index the training tokens of packed ``.npz`` files, as the reference walks its dataset: ``X``
        [R][T] rows, or with a ``lengths`` array the sequences of the flat ``X``; the rows of all files in
        order, under the stop rule of ``from_rows``."""
        ids, lens = [], []
        for p in ([paths] if isinstance(paths, (str, Path)) else list(paths)):
            with np.load(p, allow_pickle=False) as data:
                X = np.asarray(data["X"])
                ln = np.asarray(data["lengths"]).astype(np.int64) if "lengths" in data \
                    else np.full(X.shape[0], X.shape[1] if X.ndim == 2 else 0, dtype=np.int64)
                ids.append(X.reshape(-1)[:int(ln.sum())])
                lens.append(ln)
        lens = np.concatenate(lens) if lens else np.zeros(0, dtype=np.int64)
        flat = np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        rows = len(lens) if max_tokens is None else int(np.searchsorted(offsets[:-1], int(max_tokens), side="left"))
        offsets = offsets[:rows + 1]
        sym = torch.from_numpy(ids_to_symbols(flat[:offsets[-1]])).to(_device(device))
        return cls(ops.ngram_index_build(ops.NgramIndex(sym, offsets, n)), rows, int(offsets[-1]))

    def coverage(self, seqs: Sequence[np.ndarray], want=("n_hit", "covered")):
        """(host offsets, ops.NgramCoverage) of the host uint8 query sequences."""
        qsym, qoff = _upload(seqs, self.index.sym.device)
        return qoff, ops.ngram_coverage(self.index, qsym, qoff, want=want)


def _fractions(index: TrainIndex, seqs: Sequence[np.ndarray]) -> np.ndarray:
    if not len(seqs):
        return np.zeros(0, dtype=np.float64)
    qoff, res = index.coverage(seqs, want=("covered",))
    covered = res.covered.cpu().numpy().astype(np.float64)
    lens = np.diff(qoff).astype(np.float64)
    return np.divide(covered, lens, out=np.zeros_like(covered), where=lens > 0)


def training_match_coverage(index: TrainIndex, id_lists: Sequence[Sequence[int]]) -> np.ndarray:
    """Per token list, the fraction of its positions covered by a window of the index
    (_training_match_coverage): float64, 0 for a list shorter than the window."""
    return _fractions(index, [ids_to_symbols(ids) for ids in id_lists])


def _string_index(training_sequences: Sequence[str], window: int) -> TrainIndex:
    if int(window) < 1:
        raise ValueError("window_size must be at least 1")
    return TrainIndex.from_sequences([text_to_symbols(s) for s in training_sequences], int(window))


def matching_substring_coverage(sequences: Sequence[str], training_sequences: Sequence[str], window: int,
                                *, index: Optional[TrainIndex] = None) -> np.ndarray:
    """leakage_audit.matching_substring_coverage for a list of query strings at once: per query the
    fraction of positions covered by an exact training window of ``window`` symbols.  ``index``
    reuses an index built earlier over the same training strings."""
    index = index if index is not None else _string_index(training_sequences, window)
    return _fractions(index, [text_to_symbols(s) for s in sequences])


def matched_windows(sequences: Sequence[str], training_sequences: Sequence[str], window: int,
                    *, index: Optional[TrainIndex] = None) -> Set[str]:
    """leakage_audit._matched_query_windows: the windows of the queries that occur in the training
    strings, as a set of strings."""
    if not len(sequences):
        return set()
    index = index if index is not None else _string_index(training_sequences, window)
    qoff, res = index.coverage([text_to_symbols(s) for s in sequences], want=("hit",))
    hit = res.hit.cpu().numpy()
    out: Set[str] = set()
    for q, s in enumerate(sequences):
        for start in np.nonzero(hit[qoff[q]:qoff[q + 1]])[0]:
            out.add(s[int(start):int(start) + index.n])
    return out


def normalize_cds(sequence: str) -> str:
    """leakage_audit.normalize_cds: whitespace removed, upper case, U read as T."""
    return "".join(str(sequence).split()).upper().replace("U", "T")


def translate_cds(sequence: str) -> str:
    """The protein of a CDS under the audit's rules: the incomplete tail is ignored, a trailing stop
    is dropped, an internal stop or a codon outside the table becomes X."""
    dna = normalize_cds(sequence)
    aas = [CODON_TABLE.get(dna[i:i + 3], "X") for i in range(0, len(dna) // 3 * 3, 3)]
    if aas and aas[-1] == "_":
        aas.pop()
    return "".join("X" if a == "_" else a for a in aas)


def generated_coverage(training_records: Sequence[Mapping], generated_records: Sequence[Mapping],
                       nucleotide_window: int = 30, protein_window: int = 10) -> List[Dict[str, object]]:
    """The two coverage columns of leakage_audit.audit_generated_sequences: per generated record
    {source_id, nucleotide_training_match_coverage, protein_training_match_coverage} against the
    ``sequence`` fields of the training records."""
    out = [{"source_id": str(r["source_id"])} for r in generated_records]
    for key, convert, window in (("nucleotide_training_match_coverage", normalize_cds, nucleotide_window),
                                 ("protein_training_match_coverage", translate_cds, protein_window)):
        cov = matching_substring_coverage([convert(r["sequence"]) for r in generated_records],
                                          [convert(r["sequence"]) for r in training_records], window)
        for row, c in zip(out, cov):
            row[key] = float(c)
    return out


__all__ = ["TrainIndex", "training_match_coverage", "matching_substring_coverage", "matched_windows",
           "generated_coverage", "normalize_cds", "translate_cds", "pack_sequences", "ids_to_symbols",
           "text_to_symbols"]
