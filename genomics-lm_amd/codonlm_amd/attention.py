"""Attention head analysis with a trained codon LM: per-head entropy, key-class and distance masses,
sink and received attention over any number of sequences, and the attention maps of a few.

The statistics come from cg_attn_stats (Engine.attn_stats): after one eval forward per batch, one
fused pass per layer recomputes QK^T from the layer's saved qkv rows, normalises each row itself in
fp32 and adds the probabilities into the row statistics and the fp64 per-head accumulator.  No
T x T tensor reaches memory, so a whole validation set costs what its forwards cost; the reference
reads a captured (L, B, H, T, T) tensor and therefore only ever looks at four rows.  Only
``attention_maps`` materialises probabilities (cg_attn_probs), for plotting.  There is no CPU path.

Replaces, on the reference side: the statistics of scripts/conference_attention.py (_head_stats and
its "most focused head" / "start specialist" rankings) and the tensors scripts/analyze_attention.py
and scripts/report_top_saliency.py load.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .context import token_classes
from .data_loading import PAD_ID

STATS = L.AS_STATS


@dataclass
class HeadStats:
    """``sums`` fp64 (L, H, 14): the sums over the kept rows of every statistic, in the order of
    ``STATS``; ``n_rows``: the kept (sequence, position) count, the same for every layer and head."""
    sums: np.ndarray
    n_rows: int

    @property
    def means(self) -> np.ndarray:
        return self.sums / max(self.n_rows, 1)

    def mean(self, name: str) -> np.ndarray:
        """(L, H) mean of the statistic ``name``."""
        return self.means[:, :, STATS.index(name)]


def _device(model) -> torch.device:
    return model.flat_parameters().device


def _n_layer(model) -> int:
    return int(model.engine.cfg.n_layer)


def _class_table(itos: Sequence[str], dev) -> torch.Tensor:
    return torch.from_numpy(token_classes(itos)).to(dev)


def _batches(source, batch: int, dev, row_keep):
    """(x, keep) device batches of an int array [N][T] (``row_keep``: None or an array of its shape)
    or of an iterable of x / (x, y) device batches (``row_keep``: None or a callable x -> mask)."""
    if isinstance(source, np.ndarray) or torch.is_tensor(source):
        ids = torch.as_tensor(np.asarray(source.cpu() if torch.is_tensor(source) else source), dtype=torch.int64)
        if ids.dim() != 2:
            raise ValueError("head_stats: an array of token ids is (N, T)")
        keep = None if row_keep is None else torch.as_tensor(np.asarray(row_keep) != 0).to(torch.uint8)
        if keep is not None and keep.shape != ids.shape:
            raise ValueError("head_stats: row_keep has the shape of the token array")
        for s in range(0, ids.shape[0], max(1, int(batch))):
            yield ids[s:s + batch].to(dev), None if keep is None else keep[s:s + batch].to(dev)
        return
    for item in source:
        x = item[0] if isinstance(item, (tuple, list)) else item
        if x.numel():
            yield x, None if row_keep is None else row_keep(x).to(torch.uint8)


@torch.no_grad()
def head_stats(model, loader_or_array, itos: Sequence[str], *, window: Optional[int] = None,
               row_keep=None, batch: int = 32) -> HeadStats:
    """Per-head statistics over every non-PAD position of the sequences: one eval forward per batch
    (the trunk alone), then cg_attn_stats for every layer into one (L, H, 14) fp64 device
    accumulator, read once at the end.  Key classes are context.token_classes(itos); ``row_keep``
    restricts the query rows (the keys stay)."""
    dev = _device(model)
    eng = model.engine
    Ln, H = _n_layer(model), int(eng.cfg.n_head)
    acc = torch.zeros(Ln, H, L.AS_NSTAT, dtype=torch.float64, device=dev)
    n_rows = torch.zeros(1, dtype=torch.float64, device=dev)
    cls = _class_table(itos, dev)
    was_training = model.training
    model.eval()
    try:
        for x, keep in _batches(loader_or_array, batch, dev, row_keep):
            eng.forward(x, None, training=False, window=window, head=False)
            for layer in range(Ln):
                eng.attn_stats(layer, pad_id=PAD_ID, tok_class=cls, row_keep=keep, want=(), head_acc=acc[layer],
                               n_rows=n_rows if layer == 0 else None)
    finally:
        model.train(was_training)
    return HeadStats(acc.cpu().numpy(), int(round(float(n_rows.item()))))


@torch.no_grad()
def received(model, ids) -> np.ndarray:
    """fp32 (L, B, H, T): how much attention key position k of sequence b receives in head h of every
    layer, summed over the non-PAD queries that see it."""
    dev = _device(model)
    x = torch.as_tensor(np.asarray(ids), dtype=torch.int64).reshape(-1, np.asarray(ids).shape[-1]).to(dev)
    eng = model.engine
    eng.forward(x, None, training=False, head=False)
    out = [eng.attn_stats(layer, pad_id=PAD_ID, want=("received",)).received for layer in range(_n_layer(model))]
    return torch.stack(out).cpu().numpy()


@torch.no_grad()
def attention_maps(model, ids, *, layers: Optional[Sequence[int]] = None, max_tokens: Optional[int] = None) -> np.ndarray:
    """fp32 (L, B, H, T, T): the attention probabilities of ``layers`` (default: all) on ids (B, T),
    cropped to the first ``max_tokens`` positions -- the tensor the reference's plotting scripts read.
    The mask is causal, so the crop is a forward over the cropped rows."""
    dev = _device(model)
    a = np.asarray(ids)
    x = torch.as_tensor(a, dtype=torch.int64).reshape(-1, a.shape[-1])
    if max_tokens is not None:
        if int(max_tokens) < 1:
            raise ValueError("max_tokens must be at least 1")
        x = x[:, :int(max_tokens)]
    layers = list(range(_n_layer(model))) if layers is None else [int(l) for l in layers]
    eng = model.engine
    eng.forward(x.to(dev).contiguous(), None, training=False, head=False)
    return np.stack([eng.attn_probs(l).cpu().numpy() for l in layers])


def triple_from_sums(sums: np.ndarray, tokens: Sequence[int], tok_class: np.ndarray) -> np.ndarray:
    """(..., H, 3) of conference_attention._head_stats from the sums (..., H, 14) over ALL T rows of
    one sequence: mean entropy; mean of P over every row and the start (stop) columns = the summed
    start (stop) mass / (T * number of such columns), 0 where the sequence has none."""
    tokens = np.asarray(tokens).reshape(-1)
    T = len(tokens)
    cls = np.asarray(tok_class)[tokens]
    out = np.zeros(sums.shape[:-1] + (3,))
    out[..., 0] = sums[..., L.AS_ENTROPY] / T
    for j, c, s in ((1, L.DIAG_CLS_START, L.AS_MASS_START), (2, L.DIAG_CLS_STOP, L.AS_MASS_STOP)):
        n = int((cls == c).sum())
        if n:
            out[..., j] = sums[..., s] / (T * n)
    return out


@torch.no_grad()
def reference_head_stats(model, ids_row, itos: Sequence[str]) -> np.ndarray:
    """(L, H, 3): the three numbers scripts/conference_attention._head_stats takes from the captured
    attention of one sequence -- mean row entropy, mean attention on the ATG columns, mean attention
    on the stop-codon columns, over every row, PAD rows included as there -- from the fused sums."""
    dev = _device(model)
    row = np.asarray(ids_row, dtype=np.int64).reshape(-1)
    eng = model.engine
    Ln, H = _n_layer(model), int(eng.cfg.n_head)
    acc = torch.zeros(Ln, H, L.AS_NSTAT, dtype=torch.float64, device=dev)
    cls = token_classes(itos)
    cls_d = torch.from_numpy(cls).to(dev)
    eng.forward(torch.from_numpy(row[None]).to(dev), None, training=False, head=False)
    for layer in range(Ln):
        eng.attn_stats(layer, pad_id=-1, tok_class=cls_d, want=(), head_acc=acc[layer])
    return triple_from_sums(acc.cpu().numpy(), row, cls)


SPECIALIST_KINDS = (("most_focused", "entropy", False), ("start_specialist", "mass_start", True),
                    ("stop_specialist", "mass_stop", True), ("self_attention", "dist_0", True),
                    ("sink", "first", True))


def specialists(stats: HeadStats, k: int = 8) -> dict:
    """For lowest mean entropy, highest start mass, highest stop mass, highest self mass (distance
    0) and highest sink mass (the first visible key): the top-k [(layer, head, value)].  Equal values
    keep (layer, head) order."""
    out = {}
    for name, stat, highest in SPECIALIST_KINDS:
        v = stats.mean(stat)
        flat = v.reshape(-1)
        order = np.argsort(-flat if highest else flat, kind="stable")[:max(0, int(k))]
        out[name] = [(int(i // v.shape[1]), int(i % v.shape[1]), float(flat[i])) for i in order]
    return out


__all__ = ["STATS", "HeadStats", "head_stats", "received", "attention_maps", "triple_from_sums",
           "reference_head_stats", "specialists", "SPECIALIST_KINDS"]
