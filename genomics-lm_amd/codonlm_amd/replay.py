"""Generated-state replay records for the termination head (replaces src/codonlm/replay.py and the
labelling of scripts/build_generated_prefix_replay.py of genomics-lm).

A replay record is one JSONL line: ``ids`` (a generated continuation of a true prefix that ran into
the hard cap without a stop) and sparse termination labels on its last generated states, either as
``labels: [{"pos": p, "class": c}, ...]`` or as the single pair ``label_position`` / ``target_class``.
Positions index ``ids`` before the sequence is clipped to the model's block from the left.
"""
from __future__ import annotations

import json
from pathlib import Path

import torch
from torch.utils.data import Dataset

IGNORE_INDEX = -100


def replay_labels(n_ids: int, prefix_tokens: int, window: int, bucket_edges) -> list[dict]:
    """Labels of a continuation that should have stopped right after its last token
    (build_generated_prefix_replay.py:43-63): the states ``max(prefix, last - window) .. last`` get
    the bucket of their distance to that stop, bucket = the number of edges below the distance."""
    edges = tuple(int(e) for e in bucket_edges)
    if edges != tuple(sorted(edges)):
        raise ValueError("bucket_edges must be sorted")
    n_ids, prefix_tokens = int(n_ids), int(prefix_tokens)
    if n_ids <= prefix_tokens:
        return []
    last = n_ids - 1
    first = max(prefix_tokens, last - max(0, int(window)))
    return [{"pos": pos, "class": sum(1 for e in edges if last - pos > e)} for pos in range(first, last + 1)]


def _label_pairs(record: dict) -> list[tuple[int, int]]:
    items = record.get("labels")
    if items is None and "label_position" in record and "target_class" in record:
        items = [{"pos": record["label_position"], "class": record["target_class"]}]
    if not isinstance(items, list):
        return []
    pairs = []
    for item in items:
        try:
            pairs.append((int(item["pos"]), int(item["class"])))
        except (KeyError, TypeError, ValueError, IndexError):
            continue  # a malformed entry is dropped, the rest of the record is kept
    return pairs


class GeneratedTerminationReplayDataset(Dataset):
    """(x, y) pairs of ``block_size`` tokens: x = the last block_size ids, right-padded with
    ``pad_id``; y = ``ignore_index`` except at the labelled states (replay.py:46-112).  A record
    without usable ids, without labels, or whose labels all fall off the left edge is skipped.
    ``n_classes`` (not in the reference): a label class outside [0, n_classes) raises ValueError
    at load -- the fused loss kernel would silently ignore it."""

    def __init__(self, path, block_size: int, *, pad_id: int = 0, ignore_index: int = IGNORE_INDEX,
                 n_classes: int | None = None) -> None:
        self.path = Path(path)
        self.block_size = int(block_size)
        self.pad_id = int(pad_id)
        self.ignore_index = int(ignore_index)
        if self.block_size <= 0:
            raise ValueError("block_size must be positive")
        if not self.path.exists():
            raise FileNotFoundError(f"replay dataset not found: {self.path}")
        self.records: list[tuple[list[int], list[tuple[int, int]]]] = []
        with self.path.open() as fh:
            for line_no, line in enumerate(fh, start=1):
                line = line.strip()
                if not line:
                    continue
                try:
                    record = json.loads(line)
                except json.JSONDecodeError as exc:
                    raise ValueError(f"invalid JSONL record at {self.path}:{line_no}: {exc}") from exc
                ids = record.get("ids") if isinstance(record, dict) else None
                if not isinstance(ids, list) or not ids:
                    continue
                try:
                    ids = [int(t) for t in ids]
                except (TypeError, ValueError):
                    continue
                cut = max(0, len(ids) - self.block_size)  # tokens clipped off the left
                kept = [(pos - cut, cls) for pos, cls in _label_pairs(record) if cut <= pos < len(ids)]
                if not kept:
                    continue
                if n_classes is not None:
                    for _, cls in kept:
                        if not 0 <= cls < int(n_classes):
                            raise ValueError(f"replay label class {cls} at {self.path}:{line_no} is outside "
                                             f"[0, {int(n_classes)})")
                self.records.append((ids, kept))
        if not self.records:
            raise ValueError(f"replay dataset has no usable records: {self.path}")

    def __len__(self) -> int:
        return len(self.records)

    def __getitem__(self, idx: int):
        ids, labels = self.records[idx]
        ids = ids[-self.block_size:]
        x = torch.full((self.block_size,), self.pad_id, dtype=torch.long)
        y = torch.full((self.block_size,), self.ignore_index, dtype=torch.long)
        x[: len(ids)] = torch.tensor(ids, dtype=torch.long)
        for pos, cls in labels:
            y[pos] = cls
        return x, y


__all__ = ["IGNORE_INDEX", "replay_labels", "GeneratedTerminationReplayDataset"]
