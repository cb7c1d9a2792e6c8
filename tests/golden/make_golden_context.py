#!/usr/bin/env python3
"""Golden vectors of the context diagnostic, made by running the REAL reference (build container
only, like make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_context.py

context_diag.npz  for every window length of tests/context_restatement.py (its synthetic splits and
                  logits are the inputs) what the reference's own functions return:
                  fit_baselines / evaluate_baselines (scripts/eval_ppl_baselines.py, with _examples
                  replaced by an array source), _trigram_nll, _position_bin, _token_class, _add_slice
                  and _bootstrap_paired_rows (scripts/diagnose_context_learning.py), ece_from_logits
                  and brier_from_logits (scripts/calibration_metrics.py).
The slice loop of diagnose() (:322-357) is inline there and cannot be called: slice_table() below
builds a per-position membership table with the reference's _position_bin and _token_class (the
segment counter by a prefix scan), and slice_sums() adds every window through the reference's
_add_slice, as that loop does.  The losses it slices are F.cross_entropy of the
fp64 logits, and ECE / Brier run with torch's default dtype set to float64, so every stored value
is an fp64 one.  Inputs and outputs only, never reference code.
"""
from __future__ import annotations

import sys
from collections import defaultdict

import numpy as np
import torch
import torch.nn.functional as F

import make_golden as MG  # noqa: E402  (sets up the reference import path)
from scripts import calibration_metrics as RC  # noqa: E402  (reference)
from scripts import diagnose_context_learning as RD  # noqa: E402  (reference)
from scripts import eval_ppl_baselines as RB  # noqa: E402  (reference)

sys.path.insert(0, str(MG.HERE.parent))
import context_restatement as CR  # noqa: E402  (the shared synthetic inputs)

ALPHA = 0.01
N_BINS = 15
BOOT_SEED, BOOT_SAMPLES = 1337, 200


def counter_by_scan(valid, resets):
    """The segment counter of one row without a running variable: the valid positions before t,
    minus those before the last reset at or before t (another route than the restatement's loop)."""
    before = np.cumsum(valid) - valid
    at_reset = np.maximum.accumulate(np.where(resets, before, 0))
    return before - at_reset


def slice_table(targets, inputs, flags):
    """Per position the names of the slices it belongs to, decided by the reference's _position_bin and
    _token_class: a bool table [slice][row][position]."""
    valid = targets != RD.PAD_ID
    flagged = np.broadcast_to(np.asarray(flags, bool)[:, None], valid.shape)
    member = {name: np.zeros(valid.shape, bool) for name in CR.SLICES}
    member["all"] = valid
    member["after_separator"] = valid & (inputs == CR.SEP)
    member["window_with_chunk_continuation"] = valid & flagged
    member["window_without_chunk_continuation"] = valid & ~flagged
    class_of = [f"target_class_{RD._token_class(token)}" for token in CR.ITOS]
    for row in range(len(targets)):
        counter = counter_by_scan(valid[row], valid[row] & (inputs[row] == CR.SEP))
        for position in np.flatnonzero(valid[row]):
            member[RD._position_bin(int(counter[position]))][row, position] = True
            member[class_of[int(targets[row, position])]][row, position] = True
    return member


def slice_sums(losses, targets, inputs, flags):
    """(sum, count) per slice in CR.SLICES order, every window added through the reference's _add_slice."""
    slices = defaultdict(lambda: [0.0, 0])
    for name, table in slice_table(targets, inputs, flags).items():
        for row in range(len(targets)):
            RD._add_slice(slices, name, losses[row], table[row])
    return np.array([slices[name] for name in CR.SLICES], np.float64)


def main():
    out = {"alpha": np.float64(ALPHA), "n_bins": np.int64(N_BINS),
           "boot": np.array([BOOT_SEED, BOOT_SAMPLES], np.int64)}
    reset = frozenset([CR.SEP])
    for T in CR.TS:
        xtr, ytr, xte, yte, flags = CR.make_split(T)
        source = {"train": (xtr, ytr), "test": (xte, yte)}
        RB._examples = lambda path: iter(zip(*source[str(path)]))
        uni, bi, tri = RB.fit_baselines("train", CR.V, ALPHA, reset_token_ids=reset)
        results, tokens, best = RB.evaluate_baselines("test", (uni, bi, tri), CR.V, ALPHA, reset_token_ids=reset)
        bi_d = np.zeros((CR.V, CR.V), np.int64)
        tri_d = np.zeros((CR.V, CR.V, CR.V), np.int64)
        for p, row in bi.items():
            bi_d[p] = row
        for (p2, p), row in tri.items():
            tri_d[p2, p] = row
        bi_seen = np.zeros(CR.V, bool)
        bi_seen[list(bi)] = True
        tri_seen = np.zeros((CR.V, CR.V), bool)
        for p2, p in tri:
            tri_seen[p2, p] = True
        tri_tok = np.stack([RD._trigram_nll(xte[b], yte[b], tri, bi, alpha=ALPHA, active_size=CR.V - 1,
                                            reset_token_ids=reset) for b in range(len(xte))])
        z32 = CR.make_logits(np.random.default_rng(77 + T), xte, yte)
        zt, yt = torch.from_numpy(z32).double(), torch.from_numpy(yte.reshape(-1))
        losses = F.cross_entropy(zt, yt, ignore_index=RD.PAD_ID, reduction="none").reshape(yte.shape).numpy()
        torch.set_default_dtype(torch.float64)
        ece = RC.ece_from_logits(zt, yt, ignore_index=0, n_bins=N_BINS)
        brier = RC.brier_from_logits(zt, yt, ignore_index=0)
        torch.set_default_dtype(torch.float32)
        valid = yte != RD.PAD_ID
        row_model = (losses * valid).sum(1)
        row_tri = (tri_tok * valid).sum(1)
        row_tok = valid.sum(1).astype(np.int64)
        boot = RD._bootstrap_paired_rows(row_model, row_tri, row_tok, seed=BOOT_SEED, samples=BOOT_SAMPLES)
        k = f"T{T}_"
        out.update({
            k + "xtr": xtr.astype(np.int8), k + "ytr": ytr.astype(np.int8), k + "xte": xte.astype(np.int8),
            k + "yte": yte.astype(np.int8), k + "flags": flags, k + "logits": z32.astype(np.float16),  # exact: fp16-representable values
            k + "uni": uni.astype(np.int32), k + "bi": bi_d.astype(np.int32), k + "tri": tri_d.astype(np.int16),
            k + "bi_seen": bi_seen, k + "tri_seen": tri_seen,
            k + "baseline_nll": np.array([results[n]["cross_entropy_nats"] for n in RB.MODEL_NAMES], np.float64),
            k + "tokens": np.int64(tokens), k + "best": np.array(best),
            k + "tri_tok": tri_tok, k + "losses": losses, k + "slices": slice_sums(losses, yte, xte, flags),
            k + "ece": np.float64(ece), k + "brier": np.float64(brier),
            k + "boot": np.array([boot["codonlm_minus_trigram_nats_per_token"], *boot["ci95"]], np.float64),
        })
        print(f"[golden] context T={T}: tokens={tokens} best={best} ece={ece:.6f} brier={brier:.6f}")
    path = MG.HERE / "context_diag.npz"
    np.savez_compressed(path, **out)
    print("[golden] context_diag.npz", path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
