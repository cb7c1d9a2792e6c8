"""Batched on-device scoring with a trained codon LM: per-token log-probabilities, sequence and
variant scores, mutation maps and the test / validation evaluation.

Every function runs the eval forward on the native engine and one fused cg_score_rows pass over
its logits (lse, target log-prob, rank, selected-class deltas, per-sequence fp64 sums, fp64
accumulators) instead of log_softmax / gather / F.cross_entropy passes over the whole logits
tensor.  No function synchronises with the device inside its batch loop: inputs are uploaded
once, the results of all batches stay on the device, and one read-back ends the call.

Replaces, on the reference side: the per-position scoring of src/codonlm/score_mutations.py
(:83-157), evaluate() of scripts/evaluate_test.py (:86-171) and score_sequence of
scripts/benchmark_zero_shot_mutations.py (:25-41).
"""
from __future__ import annotations

import math
from typing import Iterable, List, Sequence

import numpy as np
import torch

from . import ops
from .data_loading import PAD_ID, bucket_batches

CODONS = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
SPECIALS = ["<PAD>", "<BOS_CDS>", "<EOS_CDS>", "<SEP>"]
DEFAULT_VOCAB = SPECIALS + CODONS


def dna_to_ids(dna: str, stoi) -> List[int]:
    """BOS + the codons of ``dna`` + EOS: upper-cased, U read as T, a trailing partial codon and
    codons outside the vocabulary dropped (score_mutations.py :16-27)."""
    dna = dna.strip().upper().replace("U", "T")
    ids = [stoi["<BOS_CDS>"]]
    for i in range(0, len(dna) // 3 * 3, 3):
        tok = stoi.get(dna[i:i + 3])
        if tok is not None:
            ids.append(tok)
    ids.append(stoi["<EOS_CDS>"])
    return ids


def codon_ids(stoi) -> List[int]:
    """Token ids of the 64 codons in CODONS order; -1 for a codon the vocabulary lacks."""
    return [int(stoi.get(c, -1)) for c in CODONS]


def _device(model) -> torch.device:
    return model.flat_parameters().device


def sliding_windows(x: torch.Tensor, block: int):
    """The contexts of the streaming rule (score_mutations.py :99-108) for a 1-D token tensor ``x``
    of T tokens, where position t is predicted from x[max(0, t - block):t]:
    (head, windows).  ``head`` = x[:min(T - 1, block)]: row t - 1 of its forward predicts
    position t for every t <= block (causality makes the shorter prefixes rows of one forward).
    ``windows`` [T - 1 - block][block] (empty when T - 1 <= block): row j is the full-length
    context x[j + 1 : j + 1 + block], whose last row predicts position block + 1 + j.  Views only."""
    T = x.numel()
    head = x[:min(T - 1, block)]
    if T - 1 <= block:
        return head, x.new_empty((0, block))
    return head, x.unfold(0, block, 1)[1:T - block]


@torch.no_grad()
def _stream(model, x: torch.Tensor, sel, batch_size: int):
    """Device (logp [T-1], delta [T-1][n_sel] or None) of every predicted position 1..T-1 of the
    device token tensor ``x``, any length.  All targets count (ignore_index = -1); a target
    outside the vocabulary scores 0 with delta base 0."""
    eng = model.engine
    block = int(model.block_size)
    head, wins = sliding_windows(x, block)
    n = head.numel()
    want = ("logp",) + (("delta",) if sel is not None else ())
    r = eng.score(head[None], x[1:n + 1][None], ignore_index=-1, sel=sel, want=want)
    logp, delta = [r.logp], [r.delta]
    V = eng.cfg.vocab_size
    for s in range(0, wins.shape[0], batch_size):
        w = wins[s:s + batch_size].contiguous()
        b = w.shape[0]
        logits, _ = eng.forward(w, None, training=False)
        last = ops.gather_rows(logits.view(b * block, V), torch.full((b,), block, dtype=torch.int32, device=x.device),
                               block)
        r = ops.score_rows(last, x[block + 1 + s: block + 1 + s + b], ignore_index=-1, sel=sel, want=want)
        logp.append(r.logp)
        delta.append(r.delta)
    return torch.cat(logp), (torch.cat(delta) if sel is not None else None)


def _as_tokens(model, ids) -> torch.Tensor:
    x = torch.as_tensor(np.asarray(ids, dtype=np.int64)).to(_device(model))
    if x.dim() != 1 or x.numel() < 2:
        raise ValueError("scoring needs a 1-D sequence of at least two tokens")
    return x


def token_logprobs(model, ids, *, batch_size: int = 32) -> np.ndarray:
    """log p(ids[t] | ids[max(0, t - block_size):t]) for t = 1..len(ids)-1 (fp32).  Up to
    block_size + 1 tokens take one forward; longer inputs add one full-length window per further
    position, ``batch_size`` windows per forward."""
    logp, _ = _stream(model, _as_tokens(model, ids), None, batch_size)
    return logp.cpu().numpy()


@torch.no_grad()
def token_logprobs_batch(model, seqs: Sequence[Sequence[int]], *, batch_size: int = 32) -> List[np.ndarray]:
    """``token_logprobs`` of many sequences (each at most block_size + 1 tokens) in length-bucketed
    batches, in input order: per sequence the fp32 log p(ids[t] | ids[:t]) for t = 1..len-1, with 0
    where the target is PAD (0), as F.cross_entropy(ignore_index=0) leaves it.  One read-back."""
    if not len(seqs):
        return []
    eng = model.engine
    parts = []
    for b, x, y in _batches(model, seqs, batch_size, int(model.block_size) + 1):
        parts.append((b, x.shape[1], eng.score(x, y, ignore_index=PAD_ID, want=("logp",)).logp))
    logps = torch.cat([lp.reshape(-1) for _, _, lp in parts]).cpu().numpy()
    out: List[np.ndarray] = [None] * len(seqs)
    row = 0
    for b, T, _ in parts:
        for j, i in enumerate(b):
            out[i] = logps[row + j * T: row + j * T + len(seqs[i]) - 1].copy()
        row += len(b) * T
    return out


def _upload(seqs, dev):
    """One upload of all sequences: (flat int32 tokens, starts int64, lens int64) on the device."""
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    flat = np.concatenate([np.asarray(s, dtype=np.int32).reshape(-1) for s in seqs])
    starts = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    return (torch.from_numpy(flat).to(dev), torch.from_numpy(starts).to(dev), torch.from_numpy(lens).to(dev), lens)


def batch_order(lengths, batch_size: int):
    """Length-bucketed batches of sequence indices (data_loading.bucket_batches, no shuffle); every
    index appears exactly once, so results scatter back to input order."""
    return bucket_batches(np.asarray(lengths), int(batch_size), shuffle=False)


def _batches(model, seqs, batch_size, max_tokens):
    """Yields (indices, x, y) device batches of the right-padded sequences: x = seq[:-1],
    y = seq[1:], PAD (0) beyond each length (cg_gather_sequences)."""
    from . import _lib as L
    dev = _device(model)
    for s in seqs:
        if len(s) < 2:
            raise ValueError("every sequence needs at least two tokens")
        if len(s) > max_tokens:
            raise ValueError(f"a sequence of {len(s)} tokens exceeds block_size + 1 = {max_tokens}; "
                             "token_logprobs scores longer inputs")
    flat, starts, lens_dev, lens = _upload(seqs, dev)
    batches = batch_order(lens, batch_size)
    order = torch.from_numpy(np.array([i for b in batches for i in b], dtype=np.int64)).to(dev)
    at = 0
    for b in batches:
        B, Tout = len(b), int(lens[b].max()) - 1
        x = torch.empty(B, Tout, dtype=torch.int64, device=dev)
        y = torch.empty_like(x)
        L.check(L.lib.cg_gather_sequences(4, flat.data_ptr(), starts.data_ptr(), lens_dev.data_ptr(), len(seqs),
                                          order[at:at + B].data_ptr(), B, Tout, x.data_ptr(), y.data_ptr(),
                                          L.stream_ptr(dev)), "cg_gather_sequences")
        at += B
        yield b, x, y


@torch.no_grad()
def score_batch(model, seqs: Sequence[Sequence[int]], batch_size: int = 32) -> List[dict]:
    """Scores of token sequences (each BOS ... EOS, at most block_size + 1 tokens), in input order:
    ``logp_sum`` (fp64 sum of the target log-probs), ``n_tokens``, ``nll`` (mean), ``ppl`` =
    exp(min(20, nll)), ``top1_acc`` and the per-token ``logp`` array (len - 1 entries).  PAD (0)
    targets are not scored.  A sequence's ``logp_sum`` does not depend on its batch."""
    if not len(seqs):
        return []
    eng = model.engine
    parts = []
    for b, x, y in _batches(model, seqs, batch_size, int(model.block_size) + 1):
        r = eng.score(x, y, ignore_index=PAD_ID, want=("logp", "rank", "seq_logp", "seq_count"))
        parts.append((b, x.shape[1], r))
    # one read-back of everything
    sums = torch.cat([r.seq_logp for _, _, r in parts]).cpu().numpy()
    counts = torch.cat([r.seq_count for _, _, r in parts]).cpu().numpy()
    logps = torch.cat([r.logp for _, _, r in parts]).cpu().numpy()
    ranks = torch.cat([r.rank for _, _, r in parts]).cpu().numpy()
    out: List[dict] = [None] * len(seqs)
    k = row = 0
    for b, T, _ in parts:
        for j, i in enumerate(b):
            n = len(seqs[i]) - 1
            lp = logps[row + j * T: row + j * T + n].copy()
            hits = int((ranks[row + j * T: row + j * T + n] == 0).sum())
            cnt = int(counts[k + j])
            nll = -float(sums[k + j]) / max(1, cnt)
            out[i] = {"logp_sum": float(sums[k + j]), "n_tokens": cnt, "nll": nll, "ppl": math.exp(min(20.0, nll)),
                      "top1_acc": hits / max(1, cnt), "logp": lp}
        k += len(b)
        row += len(b) * T
    return out


def score_variants(model, wt_ids: Sequence[int], variants: Sequence[Sequence[int]], batch_size: int = 32) -> np.ndarray:
    """logp_sum(variant) - logp_sum(wild type) per variant (fp64), the wild type scored once."""
    res = score_batch(model, [list(wt_ids)] + [list(v) for v in variants], batch_size=batch_size)
    return np.array([r["logp_sum"] - res[0]["logp_sum"] for r in res[1:]], dtype=np.float64)


@torch.no_grad()
def mutation_maps(model, seqs: Sequence[Sequence[int]], codon_ids: Sequence[int], batch_size: int = 32) -> List[np.ndarray]:
    """Per CDS (BOS, codons, EOS) an array [len - 2][len(codon_ids)]: row pos - 1 holds
    logp(codon at pos) - logp(wild-type token at pos) for pos = 1..len-2, predicted from the
    tokens before pos (score_mutations.py :146-157).  -inf for a codon id outside the vocabulary
    (or negative); baseline 0 where the wild-type id is outside the vocabulary.  Sequences that fit
    block_size + 1 tokens run length-bucketed, longer ones through the sliding windows."""
    dev = _device(model)
    sel = torch.as_tensor(np.asarray(codon_ids, dtype=np.int32)).to(dev)
    limit = int(model.block_size) + 1
    out: List = [None] * len(seqs)
    short = [i for i, s in enumerate(seqs) if len(s) <= limit]
    pend = []
    if short:
        eng = model.engine
        for b, x, y in _batches(model, [seqs[i] for i in short], batch_size, limit):
            r = eng.score(x, y, ignore_index=-1, sel=sel, want=("delta",))
            pend.append(([short[j] for j in b], x.shape[1], r.delta))
    for i, s in enumerate(seqs):
        if len(s) > limit:
            pend.append(([i], len(s) - 1, _stream(model, _as_tokens(model, s), sel, batch_size)[1]))
    for idxs, T, delta in pend:  # read back after every launch is queued
        d = delta.cpu().numpy().reshape(len(idxs), T, len(codon_ids))
        for j, i in enumerate(idxs):
            out[i] = d[j, :len(seqs[i]) - 2].copy()
    return out


def mutation_map(model, ids: Sequence[int], codon_ids: Sequence[int], batch_size: int = 32) -> np.ndarray:
    """mutation_maps of one CDS."""
    return mutation_maps(model, [ids], codon_ids, batch_size=batch_size)[0]


OFFSET_KEYS = ("nll", "ppl", "unprojected_nll", "unprojected_ppl", "nll_improvement", "relative_nll_improvement",
               "evaluated_tokens")


@torch.no_grad()
def evaluate(model, batches: Iterable, *, label_smoothing: float = 0.0, offset_targets: Sequence[int] = ()):
    """(mean_nll, ppl, mean_objective, total_tokens, offset_metrics) over device (x, y) batches with
    PAD (0) targets ignored (evaluate_test.py :86-171): the unsmoothed NLL, exp(min(20, nll)), the
    label-smoothed objective, and per offset head k the NLL of its logits ("trained") and of the
    main logits ("unprojected") against y[t + k - 1] where that target is valid (cg_offset_targets).
    All sums are fp64 accumulators on the device, read once at the end; a batch without a valid
    target adds exactly 0."""
    dev = _device(model)
    offsets = [int(k) for k in offset_targets]
    acc = torch.zeros(1 + 2 * len(offsets), 4, dtype=torch.float64, device=dev)
    was_training = model.training
    model.eval()
    try:
        for x, y in batches:
            if x.numel() == 0:
                continue
            if not offsets:
                model.engine.score(x, y, ignore_index=PAD_ID, smoothing=label_smoothing, acc=acc[0], want=())
                continue
            logits, _, aux = model(x, return_aux=True)
            main = logits.view(-1, logits.shape[-1])
            ops.score_rows(main, y, ignore_index=PAD_ID, smoothing=label_smoothing, acc=acc[0], want=())
            heads = aux.get("offset_logits", {})
            for j, k in enumerate(offsets):
                if k not in heads:
                    continue
                tk, _ = ops.offset_targets(y, k, count=False)
                h = heads[k]
                ops.score_rows(h.view(-1, h.shape[-1]), tk, ignore_index=PAD_ID, acc=acc[1 + 2 * j], want=())
                ops.score_rows(main, tk, ignore_index=PAD_ID, acc=acc[2 + 2 * j], want=())
    finally:
        model.train(was_training)
    a = acc.cpu().numpy()
    total = int(a[0, 2])
    mean_nll = float(a[0, 0]) / max(1, total)
    mean_obj = float(a[0, 1]) / max(1, total)
    metrics = {}
    for j, k in enumerate(offsets):
        n = int(a[1 + 2 * j, 2])
        if n == 0:
            continue
        tr, un = float(a[1 + 2 * j, 0]) / n, float(a[2 + 2 * j, 0]) / n
        metrics[k] = {"nll": tr, "ppl": math.exp(min(20.0, tr)), "unprojected_nll": un,
                      "unprojected_ppl": math.exp(min(20.0, un)), "nll_improvement": un - tr,
                      "relative_nll_improvement": (un - tr) / un, "evaluated_tokens": n}
    return mean_nll, math.exp(min(20.0, mean_nll)), mean_obj, total, metrics


__all__ = ["CODONS", "DEFAULT_VOCAB", "dna_to_ids", "codon_ids", "sliding_windows", "token_logprobs", "token_logprobs_batch",
           "score_batch",
           "score_variants", "mutation_map", "mutation_maps", "evaluate", "batch_order"]
