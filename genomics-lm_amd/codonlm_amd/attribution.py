"""Input attribution with a trained codon LM: gradient x input saliency, per-target attribution and
the codon-by-codon dependency map of a CDS.

Every function runs the eval forward on the native engine and then cg_model_input_grad: the
backward's dX chain alone, from a seed on the logits (cg_attr_seed), ending in the fused per-token
reductions of the gradient at the embedding output (cg_attr_reduce).  No parameter gradient is
formed or written.  Three values come back per input position:

  ``gxt``   sum_k g_k tok_emb[token]_k  -- gradient x input as the reference computes it, its hook
            sitting on tok_emb (position embeddings excluded),
  ``gxi``   sum_k g_k x0_k              -- against the embedding output the blocks consume (tok + pos),
  ``gnorm`` |g|.

The batches are the length buckets of codonlm_amd.score (batch_order), right-padded with PAD (0)
inputs and -1 targets: a -1 target seeds nothing, and the causal mask keeps the real rows
independent of the padding.  Inputs are uploaded batch by batch, the results of all batches stay
on the device, and one read-back ends each call.

Replaces, on the reference side: scripts/analyze_saliency.py (:48-81).
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch

from . import score as S
from .data_loading import PAD_ID

VALUES = ("gxt", "gxi", "gnorm")
OBJECTIVES = ("logprob", "loss")
MODES = ("logprob", "logit")


def _check_sequence(ids, limit: int) -> None:
    if len(ids) < 2:
        raise ValueError("attribution needs a sequence of at least two tokens")
    if len(ids) > limit:
        raise ValueError(f"a sequence of {len(ids)} tokens exceeds block_size + 1 = {limit}")


def plan_batches(seqs: Sequence[Sequence[int]], batch_size: int, max_tokens: int):
    """Host side of the batching: [(indices, x, y)] with x = seq[:-1] and y = seq[1:] of the
    sequences ``indices`` (score.batch_order's length buckets; every index exactly once), int64
    [B][longest - 1], right-padded with PAD inputs and -1 targets."""
    for s in seqs:
        _check_sequence(s, max_tokens)
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    out = []
    for b in S.batch_order(lens, batch_size):
        T = int(lens[b].max()) - 1
        x = np.full((len(b), T), PAD_ID, dtype=np.int64)
        y = np.full((len(b), T), -1, dtype=np.int64)
        for j, i in enumerate(b):
            ids = np.asarray(seqs[i], dtype=np.int64).reshape(-1)
            x[j, :len(ids) - 1], y[j, :len(ids) - 1] = ids[:-1], ids[1:]
        out.append((list(b), x, y))
    return out


def _to_dev(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@torch.no_grad()
def loss_saliency(model, x: np.ndarray, y: np.ndarray) -> dict:
    """{gxt, gxi, gnorm} fp32 [T] of the model's own loss on one sequence: inputs ``x`` [T] and
    targets ``y`` [T] as the training step sees them (PAD targets ignored, the model's label
    smoothing and class weights) -- the loss scripts/analyze_saliency.py differentiates."""
    x = np.asarray(x, dtype=np.int64).reshape(1, -1)
    y = np.asarray(y, dtype=np.int64).reshape(1, -1)
    if x.shape != y.shape or x.shape[1] < 1:
        raise ValueError("loss_saliency needs one target per input position")
    if x.shape[1] > int(model.block_size):
        raise ValueError(f"a sequence of {x.shape[1] + 1} tokens exceeds block_size + 1 = {int(model.block_size) + 1}")
    dev = S._device(model)
    eng = model.engine
    eng.forward(_to_dev(x, dev), _to_dev(y, dev), training=False)
    r = eng.input_grad(want=VALUES)
    return {k: getattr(r, k)[0].cpu().numpy() for k in VALUES}


@torch.no_grad()
def saliency(model, seqs: Sequence[Sequence[int]], *, objective: str = "logprob", batch_size: int = 32) -> List[dict]:
    """Per sequence (each at most block_size + 1 tokens), in input order, a dict of the three fp32
    arrays ``gxt``, ``gxi``, ``gnorm`` of length len - 1: the attribution of the objective to
    every input position, inputs ids[:-1] and targets ids[1:].
      "logprob": the sequence's own sum of log p(ids[t + 1] | ids[:t + 1]), every target weighted 1.
                 A sum per sequence, so a sequence's values do not depend on its batch.
      "loss":    the model's mean cross-entropy (label smoothing, class weights, PAD ignored), the
                 reference's objective.  The mean couples the rows of a batch, so every sequence
                 runs as a batch of its own."""
    if objective not in OBJECTIVES:
        raise ValueError(f"objective is one of {OBJECTIVES}")
    if not len(seqs):
        return []
    limit = int(model.block_size) + 1
    if objective == "loss":
        for s in seqs:
            _check_sequence(s, limit)
        return [loss_saliency(model, np.asarray(s)[:-1], np.asarray(s)[1:]) for s in seqs]
    dev = S._device(model)
    eng = model.engine
    parts = []
    for b, x, y in plan_batches(seqs, batch_size, limit):
        eng.forward(_to_dev(x, dev), None, training=False)
        parts.append((b, eng.input_grad(y=_to_dev(y, dev), mode="logprob", want=VALUES)))
    out: List[dict] = [None] * len(seqs)
    for b, r in parts:  # read back after every launch is queued
        vals = {k: getattr(r, k).cpu().numpy() for k in VALUES}
        for j, i in enumerate(b):
            n = len(seqs[i]) - 1
            out[i] = {k: vals[k][j, :n].copy() for k in VALUES}
    return out


@torch.no_grad()
def _attribute(model, ids, positions, classes, mode: str, value: str, batch_size: int) -> np.ndarray:
    """[len(positions)][n] of ``value``: row j from the seed (positions[j], classes[j]) alone.  The
    sequence is replicated as batch rows with one seeded position each; a chunk runs the forward
    only as far as its last seeded position (later positions cannot receive gradient)."""
    if mode not in MODES:
        raise ValueError(f"mode is one of {MODES}")
    if value not in VALUES:
        raise ValueError(f"value is one of {VALUES}")
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    _check_sequence(ids, int(model.block_size) + 1)
    n = len(ids) - 1
    positions = np.asarray(positions, dtype=np.int64).reshape(-1)
    if positions.size and (positions.min() < 0 or positions.max() >= n):
        raise ValueError(f"target positions lie in [0, {n}): position t is the prediction of ids[t + 1]")
    if classes is None:
        classes = ids[positions + 1]
    classes = np.asarray(classes, dtype=np.int64).reshape(-1)
    if classes.shape != positions.shape:
        raise ValueError("one class per target position")
    out = np.zeros((len(positions), n), dtype=np.float32)
    if not positions.size:
        return out
    bs = max(1, int(batch_size))
    dev = S._device(model)
    eng = model.engine
    parts = []
    for s in range(0, len(positions), bs):
        pos, cls = positions[s:s + bs], classes[s:s + bs]
        T = int(pos.max()) + 1
        x = np.repeat(ids[None, :T], len(pos), axis=0)
        y = np.full((len(pos), T), -1, dtype=np.int64)
        y[np.arange(len(pos)), pos] = cls
        eng.forward(_to_dev(x, dev), None, training=False)
        parts.append((s, T, getattr(eng.input_grad(y=_to_dev(y, dev), mode=mode, want=(value,)), value)))
    for s, T, r in parts:
        out[s:s + r.shape[0], :T] = r.cpu().numpy()
    return out


def target_attribution(model, ids: Sequence[int], positions: Sequence[int], classes=None, *, mode: str = "logprob",
                       batch_size: int = 32) -> np.ndarray:
    """fp32 [len(positions)][n], n = len(ids) - 1 input positions: row j is the ``gxt`` attribution
    of log p(classes[j]) (``mode`` "logit": of that logit) at target position positions[j] -- the
    prediction made from ids[:positions[j] + 1] -- to every input position.  classes[j] defaults to
    the actual next token ids[positions[j] + 1].  Columns past positions[j] are exactly 0."""
    return _attribute(model, ids, positions, classes, mode, "gxt", batch_size)


def dependency_map(model, ids: Sequence[int], *, value: str = "gxt", batch_size: int = 32) -> np.ndarray:
    """fp32 [n][n], n = len(ids) - 1: row t is the attribution of log p(ids[t + 1] | ids[:t + 1]) to
    every input position, lower-triangular (the strict upper triangle is exactly 0)."""
    n = len(ids) - 1
    return _attribute(model, ids, np.arange(max(n, 0)), None, "logprob", value, batch_size)


__all__ = ["VALUES", "plan_batches", "loss_saliency", "saliency", "target_attribution", "dependency_map"]
