"""Context diagnostic on the native engine: attention-window sweeps, segment-aware n-gram baselines,
sliced loss and calibration (the reference's scripts/diagnose_context_learning.py,
scripts/eval_ppl_baselines.py and scripts/calibration_metrics.py).

Everything around the forward that is a Python loop per token in the reference is one device pass
here: cg_ngram_count / cg_ngram_totals fit the baselines, cg_ngram_nll evaluates them, cg_diag_rows
slices the loss and bins the confidences.  All sums are fp64 device accumulators read once at the
end.  The paired bootstrap stays on the host with the reference's ``default_rng`` draw order.
There is no CPU path.
"""
from __future__ import annotations

import hashlib
import math
from typing import Iterable, Mapping, Sequence

import numpy as np
import torch

from . import _lib as L
from . import ops

PAD_ID = 0
MODEL_NAMES = ("Uniform", "Unigram", "Bigram", "Trigram")
DEFAULT_WINDOWS = "1,2,4,8,32,128,full"


def _device(model) -> torch.device:
    return model.flat_parameters().device


def parse_windows(value: str) -> list:
    """"1, 2,FULL,2" -> [1, 2, None]: the --context-windows list in its first-seen order, None for
    the unlimited window (the flag syntax of diagnose_context_learning.py)."""
    names = [part.strip().lower() for part in value.split(",")]
    parsed = [None if name == "full" else int(name) for name in names if name]
    if any(w is not None and w < 1 for w in parsed):
        raise ValueError("context windows must be positive or 'full'")
    if not parsed:
        raise ValueError("at least one context window is required")
    return [w for i, w in enumerate(parsed) if w not in parsed[:i]]


def markdown_table(header: Sequence[str], rule: str, rows: Iterable[Sequence[str]]) -> list:
    """The lines of a pipe table: the header cells, the alignment rule as given, one line per row."""
    return ["| " + " | ".join(header) + " |", rule] + ["| " + " | ".join(cells) + " |" for cells in rows]


def token_classes(itos: Sequence[str]) -> np.ndarray:
    """uint8 [V] of L.DIAG_CLS_* (the reference's _token_class)."""
    out = np.empty(len(itos), np.uint8)
    for i, token in enumerate(itos):
        out[i] = (L.DIAG_CLS_SPECIAL if token.startswith("<") else L.DIAG_CLS_START if token == "ATG"
                  else L.DIAG_CLS_STOP if token in ("TAA", "TAG", "TGA") else L.DIAG_CLS_ORDINARY)
    return out


def vocabulary_block(itos: Sequence[str]) -> dict:
    """Size and sha256 of the vocabulary, as the trainer's cfg["vocabulary"] records them."""
    digest = hashlib.sha256("\n".join(itos).encode()).hexdigest()
    return {"size": len(itos), "sha256": digest}


def _rows(loader):
    """(dataset rows, x, y) of every non-empty batch this rank runs, in the loader's order."""
    return ((rows, x, y) for rows, x, y in loader.iter_rows() if x.numel())


# ------------------------------------------------------------------ n-gram baselines
def fit_ngrams(loader: Iterable, V: int, reset_ids: Sequence[int] = (), pad_id: int = PAD_ID) -> ops.NgramTables:
    """fit_baselines: the count tables of every (x, y) batch of ``loader`` and their row totals."""
    tables = None
    for x, y in loader:
        if x.numel() == 0:
            continue
        if tables is None:
            tables = ops.NgramTables(V, x.device, pad_id, reset_ids)
        ops.ngram_count(tables, x, y)
    if tables is None or int(tables.uni.sum()) == 0:
        raise ValueError("training dataset has no evaluable non-PAD targets")
    bad = int(tables.n_bad)
    if bad:
        raise ValueError(f"{bad} training positions hold a token outside [0, {V})")
    return ops.ngram_totals(tables)


def baseline_results(sums: Sequence[float], tokens: int):
    """The reference's results block, best simple baseline and improvements (evaluate_baselines)."""
    if tokens == 0:
        raise ValueError("test dataset has no evaluable non-PAD targets")
    mean = {name: float(total) / tokens for name, total in zip(MODEL_NAMES, sums)}
    fitted = [name for name in MODEL_NAMES if name != "Uniform"]
    best_name = fitted[int(np.argmin([mean[name] for name in fitted]))]  # the first of equal minima
    results = {name: {"cross_entropy_nats": nats, "perplexity": math.exp(nats), "bits_per_codon": nats / math.log(2),
                      "cross_entropy_improvement_over_best_simple": mean[best_name] - nats}
               for name, nats in mean.items()}
    return results, best_name


def evaluate_ngrams(loader: Iterable, tables: ops.NgramTables, alpha: float = 0.01):
    """evaluate_baselines: (results, evaluated tokens, best simple baseline)."""
    if alpha <= 0:
        raise ValueError("alpha must be positive")
    acc = None
    for x, y in loader:
        if x.numel() == 0:
            continue
        if acc is None:
            acc = torch.zeros(5, dtype=torch.float64, device=x.device)
        ops.ngram_nll(tables, x, y, alpha, acc=acc, want=())
    a = acc.cpu().numpy() if acc is not None else np.zeros(5)
    tokens = int(a[4])
    results, best = baseline_results(a[:4], tokens)
    return results, tokens, best


# ------------------------------------------------------------------ the model side
@torch.no_grad()
def context_ablation(model, loader: Iterable, windows: Sequence) -> dict:
    """NLL with attention limited to the last w input tokens, per window (None = full), from
    cg_score_rows' accumulator (diagnose_context_learning.py:259-317)."""
    dev = _device(model)
    was_training = model.training
    model.eval()
    out = {}
    try:
        for window in windows:
            acc = torch.zeros(4, dtype=torch.float64, device=dev)
            for x, y in loader:
                if x.numel():
                    model.engine.score(x, y, window=window, ignore_index=PAD_ID, acc=acc, want=())
            a = acc.cpu().numpy()
            out[window_label(window)] = ablation_entry(window, float(a[0]), int(a[2]))
    finally:
        model.train(was_training)
    return out


def window_label(window) -> str:
    return "full" if window is None else str(window)


def ablation_entry(window, nll_sum: float, tokens: int) -> dict:
    """One context_ablation record of the report, from a window's nll sum and token count."""
    if tokens == 0:
        raise ValueError("evaluation dataset has no evaluable non-PAD targets")
    mean_nll = nll_sum / tokens
    history = "full" if window is None else f"up_to_{window}_tokens_including_current_input"
    return {"attention_window_input_tokens": window, "target_history_interpretation": history,
            "nll": mean_nll, "perplexity": math.exp(mean_nll), "evaluated_tokens": tokens}


def _full_logits(model, x):
    logits, _ = model.engine.forward(x, None, training=False, window=None)
    return logits.view(-1, logits.shape[-1])


@torch.no_grad()
def loss_decomposition(model, loader, itos: Sequence[str], row_flags=None, *, tables: ops.NgramTables | None = None,
                       alpha: float = 0.01) -> dict:
    """The full-context loss by slice (diagnose_context_learning.py:322-367) and the per-window sums
    the paired gate needs.  ``row_flags``: bool per dataset row (the chunk-continuation windows).
    Returns {"decomposition", "nll_sum", "tokens", "row_model", "row_tokens", "row_trigram"} (the
    totals of the "all" slice; row arrays in dataset order; row_trigram only with ``tables``)."""
    dev = _device(model)
    sep = [i for i, t in enumerate(itos) if t == "<SEP>"]
    if len(sep) != 1:
        raise ValueError("diagnostic requires exactly one <SEP> token")
    n = len(loader.ds)
    flags = np.zeros(n, bool) if row_flags is None else np.asarray(row_flags, bool)
    if flags.shape != (n,):
        raise ValueError("row_flags holds one flag per dataset row")
    flags_dev = torch.from_numpy(flags.astype(np.uint8)).to(dev)
    cls = torch.from_numpy(token_classes(itos)).to(dev)
    slices = torch.zeros(len(L.DIAG_SLICES), 2, dtype=torch.float64, device=dev)
    row_model = torch.zeros(n, dtype=torch.float64, device=dev)
    row_tokens = torch.zeros(n, dtype=torch.int64, device=dev)
    row_tri = torch.zeros(n, dtype=torch.float64, device=dev) if tables is not None else None
    was_training = model.training
    model.eval()
    try:
        for rows, x, y in _rows(loader):
            rows_dev = torch.from_numpy(rows).to(dev)
            res = ops.diag_rows(_full_logits(model, x), x, y, V=len(itos), pad_id=PAD_ID, sep_id=sep[0],
                                row_flag=flags_dev[rows_dev].contiguous(), tok_class=cls, slices=slices,
                                want=("row_nll", "row_count"))
            row_model[rows_dev] = res.row_nll
            row_tokens[rows_dev] = res.row_count.to(torch.int64)
            if tables is not None:
                row_tri[rows_dev] = ops.ngram_nll(tables, x, y, alpha, want=("row_sums",)).row_sums[:, 3]
    finally:
        model.train(was_training)
    s = slices.cpu().numpy()
    named = {name: (float(s[i, 0]), int(s[i, 1])) for i, name in enumerate(L.DIAG_SLICES)}
    decomposition = {name: {"nll": total / count, "perplexity": math.exp(total / count), "tokens": count}
                     for name, (total, count) in sorted(named.items()) if count}
    return {"decomposition": decomposition, "nll_sum": named["all"][0], "tokens": named["all"][1],
            "row_model": row_model.cpu().numpy(),
            "row_tokens": row_tokens.cpu().numpy(),
            "row_trigram": row_tri.cpu().numpy() if row_tri is not None else None}


def _ece(calib: np.ndarray, tokens: float) -> float:
    n = calib[:, 0]
    keep = n > 0
    if tokens == 0:
        return float("nan")
    return float((n[keep] / tokens * np.abs(calib[keep, 1] / n[keep] - calib[keep, 2] / n[keep])).sum())


@torch.no_grad()
def calibration(model, loader, n_bins: int = 15) -> dict:
    """ECE and multiclass Brier score over the PAD-free targets (calibration_metrics.py:35-132).
    ``ece_val`` / ``brier_val`` follow the reference's rule: per batch, then weighted by the batch's
    token count, so ``ece_val`` depends on the loader's batch size (the reference's is 32);
    ``ece_global`` bins all tokens at once.  The bin edges are torch.linspace(0, 1, n_bins + 1)."""
    if not 1 <= n_bins <= L.DIAG_MAX_BINS:
        raise ValueError(f"n_bins must be in 1..{L.DIAG_MAX_BINS}")
    dev = _device(model)
    edges = torch.linspace(0, 1, steps=n_bins + 1).to(dev)
    nb = len(loader.shard())
    calib = torch.zeros(max(nb, 1), n_bins, 3, dtype=torch.float64, device=dev)
    brier = torch.zeros(max(nb, 1), 2, dtype=torch.float64, device=dev)
    was_training = model.training
    model.eval()
    try:
        for k, (_, x, y) in enumerate(_rows(loader)):
            ops.diag_rows(_full_logits(model, x), x, y, V=model.engine.cfg.vocab_size, pad_id=PAD_ID,
                          sep_id=-1, edges=edges, calib=calib[k], brier_acc=brier[k])
    finally:
        model.train(was_training)
    c, b = calib.cpu().numpy(), brier.cpu().numpy()
    tokens = float(b[:, 1].sum())
    out = {"evaluated_tokens": int(tokens), "n_bins": int(n_bins)}
    if tokens > 0:
        out["ece_val"] = float(sum(_ece(c[k], b[k, 1]) * b[k, 1] for k in range(len(c)) if b[k, 1] > 0) / tokens)
        out["brier_val"] = float(b[:, 0].sum() / tokens)
        out["ece_global"] = _ece(c.sum(0), tokens)
    return out


def paired_bootstrap(row_model, row_trigram, row_tokens, seed: int, samples: int) -> dict:
    """The paired gate of the reference's report (_bootstrap_paired_rows): the model-minus-trigram
    loss per token over the packed windows that hold tokens, and the 2.5 % / 97.5 % quantiles of that
    ratio over ``samples`` resamples of the windows with replacement.  The contract is the stream:
    ``default_rng(seed)`` yields n window indices per resample, resample after resample.  Blocks of
    resamples are drawn as one (k, n) matrix, which consumes the stream in the same order, and each
    row is gathered and summed on its own."""
    keep = np.asarray(row_tokens, np.int64) > 0
    gap = (np.asarray(row_model, np.float64) - np.asarray(row_trigram, np.float64))[keep]
    weight = np.asarray(row_tokens, np.int64)[keep]
    n = len(weight)
    rng = np.random.default_rng(seed)
    ratios = []
    block = max(1, (1 << 22) // max(n, 1))
    for first in range(0, samples, block):
        picks = rng.integers(0, n, size=(min(block, samples - first), n))
        ratios.extend(gap[row].sum() / weight[row].sum() for row in picks)
    ci = np.quantile(np.asarray(ratios, np.float64), [0.025, 0.975])
    return {"codonlm_minus_trigram_nats_per_token": float(gap.sum() / weight.sum()),
            "ci95": [float(ci[0]), float(ci[1])],
            "bootstrap_unit": "packed_window", "bootstrap_samples": samples, "seed": seed}


def mask_audit(model, ds, n: int) -> dict:
    """_mask_audit (diagnose_context_learning.py:166-194) on build_attention_mask: the mask of the
    first ``n`` packed windows is causal within SEP segments, a separator query does not see the token
    before it, and every other non-PAD query does."""
    count = min(int(n), len(ds))
    checked = resets = 0
    sep = int(model.sep_id)
    for index in range(count):
        rows = np.array([index], np.int64)
        x, _ = ds.gather(torch.from_numpy(rows).to(ds.device), rows)
        T = x.size(1)
        mask = model.build_attention_mask(x)[0, 0]
        pos = torch.arange(T, device=x.device)
        segment = torch.cumsum(x[0] == sep, dim=0)
        expected = (pos.unsqueeze(1) >= pos.unsqueeze(0)) & (segment.unsqueeze(1) == segment.unsqueeze(0))
        if not torch.equal(mask, expected):
            raise AssertionError(f"attention mask mismatch in packed window {index}")
        nonpad = x[0] != PAD_ID
        is_sep = nonpad & (x[0] == sep) & (pos > 0)
        prev = torch.zeros(T, dtype=torch.bool, device=x.device)
        prev[1:] = mask[pos[1:], pos[1:] - 1]
        if bool((is_sep & prev).any()):
            raise AssertionError("separator query can attend across reset boundary")
        if bool((nonpad & ~is_sep & (pos > 0) & ~prev).any()):
            raise AssertionError("within-segment query cannot attend previous token")
        checked += int(nonpad.sum())
        resets += int(is_sep.sum())
    return {"sampled_windows": count, "checked_nonpad_queries": checked, "separator_reset_queries": resets,
            "status": "passed"}


def diagnose(model, train_loader, test_loader, itos: Sequence[str], *, windows=DEFAULT_WINDOWS, alpha: float = 0.01,
             row_flags=None, bootstrap_samples: int = 2000, seed: int = 1337, mask_audit_windows: int = 32,
             provenance: Mapping | None = None, log=print) -> dict:
    """The reference's report dict (diagnose_context_learning.py:197-401).  ``provenance`` holds the
    blocks the caller binds (evaluation_split, checkpoint, checkpoint_dataset, dataset_manifest,
    packing metadata)."""
    if isinstance(windows, str):
        windows = parse_windows(windows)
    if None not in windows:
        raise ValueError("context windows must include 'full' for decomposition")
    if test_loader.ds.is_dynamic:
        raise ValueError("packing-aware context diagnostics currently require fixed windows")
    reset_ids = [i for i, t in enumerate(itos) if t == "<SEP>"]
    if len(reset_ids) != 1:
        raise ValueError("diagnostic requires exactly one <SEP> token")
    n = len(test_loader.ds)
    flags = np.zeros(n, bool) if row_flags is None else np.asarray(row_flags, bool)
    audit = mask_audit(model, test_loader.ds, mask_audit_windows)
    tables = fit_ngrams(train_loader, len(itos), reset_ids)
    baseline, baseline_tokens, best_simple = evaluate_ngrams(test_loader, tables, alpha)
    ablation, full = {}, None
    for window in windows:
        label = window_label(window)
        log(f"[context] evaluating attention window {label}")
        if window is None:
            # the full-context forward runs once: its sliced pass also gives the sweep's entry
            full = loss_decomposition(model, test_loader, itos, flags, tables=tables, alpha=alpha)
            ablation[label] = ablation_entry(None, full["nll_sum"], full["tokens"])
        else:
            ablation.update(context_ablation(model, test_loader, [window]))
        log(f"[context] window {label}: nll={ablation[label]['nll']:.6f} ppl={ablation[label]['perplexity']:.3f}")
    paired = paired_bootstrap(full["row_model"], full["row_trigram"], full["row_tokens"], seed, bootstrap_samples)
    prov = dict(provenance or {})
    return {
        "schema_version": 1,
        "status": "diagnostic_complete",
        "evaluation_split": prov.get("evaluation_split", "test"),
        "checkpoint": prov.get("checkpoint"),
        "checkpoint_dataset": prov.get("checkpoint_dataset"),
        "dataset_manifest": prov.get("dataset_manifest"),
        "vocabulary": vocabulary_block(itos),
        "packing": {"metadata": prov.get("packing_metadata"),
                    "windows_with_chunk_continuation": int(flags.sum()), "total_windows": n},
        "attention_mask_audit": audit,
        "markov": {"history_reset_token_ids": sorted(reset_ids),
                   "history_reset_tokens": [itos[i] for i in reset_ids],
                   "evaluated_tokens": baseline_tokens, "best_simple_baseline": best_simple,
                   "results": baseline},
        "context_ablation": ablation,
        "loss_decomposition": full["decomposition"],
        "paired_codonlm_vs_trigram": paired,
    }


__all__ = ["DEFAULT_WINDOWS", "MODEL_NAMES", "baseline_results", "calibration", "context_ablation", "diagnose",
           "evaluate_ngrams", "fit_ngrams", "loss_decomposition", "mask_audit", "paired_bootstrap", "parse_windows",
           "token_classes", "vocabulary_block"]
