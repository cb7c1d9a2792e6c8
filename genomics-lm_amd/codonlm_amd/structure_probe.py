"""Structural regression probes on the native engine (mirrors scripts/probe_structural_regression.py
and scripts/probe_structural_awareness.py of the reference).

Ridge probes from a block's hidden states to 14 per-codon DNAshape targets, scored by 5-fold
cross-validation, and the first-principal-component "awareness" score.  Everything both scripts
report is a function of the grouped augmented Gram matrix  G_f = sum over the rows of fold f of
z z^T, z = (hidden state, targets, 1): the train statistics of fold f are sum_g G_g - G_f, its
test metrics come from G_f alone.  So the job is one batched eval forward per batch plus one
cg_gram_accum per probed layer on the engine's hidden-state buffer in place; the N x d regression
matrix never exists, and each ridge fit is a (d x d) fp64 solve.  No sklearn.

Deliberate differences from the reference: targets are aligned to runs of codon tokens (special
tokens end a run and are no regression rows, where the reference joins the tokens' strings);
the closed form is solved in fp64 (sklearn solves the fp32 hidden states in fp32); any layer, all
layers at once and the whole split can be probed.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import ops

NAMES = ("MGW", "Roll", "EP", "ProT", "HelT", "Slide", "Rise", "Shift", "Tilt", "Buckle", "Opening", "Shear",
         "Stagger", "Stretch")
AWARENESS_DNA = "ATG" + "GGCC" * 5 + "AAAA" * 5 + "CGTA" * 5 + "TGA"
_EPS = 2.0 ** -53


def default_vocab():
    from .score import DEFAULT_VOCAB
    return list(DEFAULT_VOCAB)


def codon_table(itos: Optional[Sequence[str]] = None):
    """One int per id of the vocabulary (default: the trainer's SPECIALS + CODONS): three 2-bit
    nucleotides, the first in the high bits, A, C, G, T = 0..3; -1 for a token that is no codon."""
    itos = default_vocab() if itos is None else list(itos)
    if len(itos) > 256:
        raise ValueError("codon_table: at most 256 ids")
    nt = {"A": 0, "C": 1, "G": 2, "T": 3}
    return [nt[t[0]] << 4 | nt[t[1]] << 2 | nt[t[2]] if len(t) == 3 and all(c in nt for c in t) else -1
            for t in itos]


def kfold_assign(n: int, k: int = 5, seed: int = 42) -> np.ndarray:
    """int32 [n]: the test fold of every row under sklearn's KFold(k, shuffle=True,
    random_state=seed): RandomState(seed).shuffle(arange(n)), fold f takes the next n // k entries
    (one more for the first n % k folds)."""
    order = np.arange(n)
    np.random.RandomState(seed).shuffle(order)
    sizes = np.full(k, n // k, dtype=np.int64)
    sizes[: n % k] += 1
    fold = np.empty(n, dtype=np.int32)
    fold[order] = np.repeat(np.arange(k, dtype=np.int32), sizes)
    return fold


# ---------------------------------------------------------------------------- closed forms on the Gram
def _blocks(g: torch.Tensor, d: int, m: int):
    P = d + m + 1
    return (g[:d, :d], g[:d, d:d + m], torch.diagonal(g)[d:d + m], g[:d, P - 1], g[d:d + m, P - 1], g[P - 1, P - 1])


def ridge_fit_from_gram(g: torch.Tensor, d: int, m: int, alpha: float = 1.0):
    """(coef [m][d], intercept [m]) of Ridge(alpha, fit_intercept=True) for every target from the
    augmented Gram g [P][P] of the training rows: (Sxx + alpha I) w = Sxy, b = ybar - mu . w."""
    xx, xy, _, sx, sy, n = _blocks(g, d, m)
    n = n.clamp(min=1.0)
    mu, ybar = sx / n, sy / n
    sxx = xx - n * torch.outer(mu, mu)
    sxy = xy - n * torch.outer(mu, ybar)
    a = sxx + alpha * torch.eye(d, dtype=g.dtype, device=g.device)
    w = torch.linalg.solve(a, sxy) if d else sxy
    return w.T.contiguous(), ybar - mu @ w


def metrics_from_gram(g: torch.Tensor, d: int, m: int, coef: torch.Tensor, intercept: torch.Tensor):
    """(r2 [m], corr [m]) of the probes (coef, intercept) on the rows behind the augmented Gram g:
    ss_res = y'y - 2 v'Z'y + v'Z'Z v with v = (w, b), ss_tot = y'y - (sum y)^2 / n, Pearson r from
    the same moments.  ss_tot <= 4 n 2^-53 sum y^2 counts as a constant target: r2 = corr = 0; a
    prediction without variance gives corr = 0."""
    xx, xy, yy, sx, sy, n = _blocks(g, d, m)
    w, b = coef.T, intercept  # w [d][m]
    wsx = sx @ w
    sp = wsx + n * b
    spp = ((xx @ w) * w).sum(0) + 2.0 * b * wsx + n * b * b
    spy = (xy * w).sum(0) + b * sy
    nn = n.clamp(min=1.0)
    ss_res = yy - 2.0 * spy + spp
    ss_tot = yy - sy * sy / nn
    flat = ss_tot <= 4.0 * nn * _EPS * yy
    one = torch.ones_like(ss_tot)
    r2 = torch.where(flat, torch.zeros_like(one), 1.0 - ss_res / torch.where(flat, one, ss_tot))
    var_p = spp - sp * sp / nn
    flat_p = var_p <= 4.0 * nn * _EPS * spp
    cov = spy - sp * sy / nn
    den = torch.sqrt(torch.where(flat | flat_p, one, var_p * ss_tot))
    corr = torch.where(flat | flat_p, torch.zeros_like(one), cov / den)
    return r2, corr


def ridge_cv_from_gram(gram, d: int, m: int, alpha: float = 1.0) -> Dict[str, torch.Tensor]:
    """The cross-validated ridge probes of fold Grams gram fp64 [G][P][P] (any device): per fold f the
    fit on sum_g gram[g] - gram[f] and its r2 / corr on gram[f], and the final fit on all rows.
    Returns fp64 tensors fold_r2 / fold_corr [G][m], r2 / corr [m] (the fold means), coef [m][d],
    intercept [m], and n_rows."""
    gram = torch.as_tensor(gram)
    P = d + m + 1
    if gram.dim() != 3 or gram.dtype != torch.float64 or tuple(gram.shape[1:]) != (P, P):
        raise ValueError("ridge_cv_from_gram: gram is fp64 [G][d + m + 1][d + m + 1]")
    total = gram.sum(0)
    fold_r2, fold_corr = [], []
    for f in range(gram.shape[0]):
        coef, icpt = ridge_fit_from_gram(total - gram[f], d, m, alpha)
        r2, corr = metrics_from_gram(gram[f], d, m, coef, icpt)
        fold_r2.append(r2)
        fold_corr.append(corr)
    coef, icpt = ridge_fit_from_gram(total, d, m, alpha)
    fold_r2, fold_corr = torch.stack(fold_r2), torch.stack(fold_corr)
    return {"fold_r2": fold_r2, "fold_corr": fold_corr, "r2": fold_r2.mean(0), "corr": fold_corr.mean(0),
            "coef": coef, "intercept": icpt, "n_rows": total[P - 1, P - 1]}


def awareness_from_gram(g: torch.Tensor, d: int, m: int) -> torch.Tensor:
    """|corr| [m] between every target and the projection of the hidden states on their first
    principal component: the top eigenvector v of Sxx, |v'Sxy| / sqrt(v'Sxx v * Syy); 0 for a
    constant target or hidden states without variance."""
    xx, xy, yy, sx, sy, n = _blocks(g, d, m)
    n = n.clamp(min=1.0)
    sxx = xx - torch.outer(sx, sx) / n
    sxy = xy - torch.outer(sx, sy) / n
    syy = yy - sy * sy / n
    val, vec = torch.linalg.eigh(sxx)
    v, lam = vec[:, -1], val[-1]
    flat = (syy <= 4.0 * n * _EPS * yy) | (lam <= 0)
    one = torch.ones_like(syy)
    return torch.where(flat, torch.zeros_like(one), (v @ sxy).abs() / torch.sqrt(torch.where(flat, one, lam * syy)))


# ---------------------------------------------------------------------------- the forward loop
def layer_list(model, layers):
    n_layer = int(model.n_layer)
    if isinstance(layers, str):
        if layers != "all":
            raise ValueError("layers: a list of block indices or 'all'")
        return list(range(n_layer))
    if isinstance(layers, (int, np.integer)):
        layers = (layers,)
    out = []
    for l in layers:
        l = int(l)
        if not -n_layer <= l < n_layer:
            raise ValueError(f"layer {l} outside the model's {n_layer} blocks")
        out.append(l % n_layer)
    if not out:
        raise ValueError("layers: at least one block")
    return out


@torch.no_grad()
def collect_gram(model, ids, layers=(-1,), batch_size: int = 64, min_tokens: int = 10, k: int = 5, seed: int = 42,
                 itos: Optional[Sequence[str]] = None, pad_id: int = 0):
    """(gram fp64 [len(layers)][k][P][P] on the device, n_rows): the fold Grams of the outputs of the
    blocks ``layers`` (-1 = the last block's output before ln_f, 'all' = every block) and the 14
    targets, P = n_embd + 15, over every codon position of ids int [S][T] (PAD = ``pad_id``;
    trimmed to block_size).  Row numbers run in (sequence, position) order over the codon positions
    of the sequences with at least ``min_tokens`` non-PAD tokens; row i is in fold
    kfold_assign(n_rows, k, seed)[i].  One host read (the row count); then per batch one eval
    forward of the trunk and one gram_accum per layer on the engine's hidden-state buffer in place."""
    if batch_size < 1 or k < 1:
        raise ValueError("batch_size and k must be at least 1")
    which = [l + 1 for l in layer_list(model, layers)]
    host = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids)
    if host.ndim != 2:
        raise ValueError("ids must be [sequences][positions]")
    host = np.ascontiguousarray(host[:, :int(model.block_size)].astype(np.int64))
    S, T = host.shape
    dev = model.flat_parameters().device
    d, m = int(model.n_embd), ops.SHAPE_TARGETS
    P = d + m + 1
    gram = torch.zeros(len(which), k, P, P, dtype=torch.float64, device=dev)
    if S == 0 or T == 0:
        return gram, 0
    x = torch.from_numpy(host).to(dev)
    y, valid = ops.shape_targets(x, codon_table(itos))
    keep_seq = (x != pad_id).sum(1) >= min_tokens
    flat = (valid.view(S, T) * keep_seq[:, None].to(torch.int32)).reshape(-1)
    row = torch.cumsum(flat, 0, dtype=torch.int64) - 1
    n_rows = int(flat.sum().item())  # the one device read of the call
    if n_rows == 0:
        return gram, 0
    fold = torch.from_numpy(kfold_assign(n_rows, k, seed)).to(dev)
    grp = torch.where(flat > 0, fold[row.clamp(min=0)], torch.full_like(flat, -1)).contiguous()
    eng = model.engine
    ws = ops.gram_workspace(min(batch_size, S) * T, d, m, k, dev)
    for s in range(0, S, batch_size):
        eng.forward(x[s:s + batch_size], None, training=False, head=False)  # hidden states only
        for i, w in enumerate(which):
            ops.gram_accum(eng.hidden(w), y[s * T:(s + batch_size) * T], grp[s * T:(s + batch_size) * T], k, gram[i],
                           accumulate=True, workspace=ws)
    return gram, n_rows


def _metric_keys(prefix: str, r2, corr) -> Dict[str, float]:
    out = {}
    for j, name in enumerate(NAMES):
        out[f"{prefix}{name}.r2"] = float(r2[j])
        out[f"{prefix}{name}.corr"] = float(corr[j])
    out[f"{prefix}avg_r2"] = float(np.mean([out[f"{prefix}{n}.r2"] for n in NAMES]))
    out[f"{prefix}avg_corr"] = float(np.mean([out[f"{prefix}{n}.corr"] for n in NAMES]))
    return out


def probe(model, ids, layers=(-1,), batch_size: int = 64, min_tokens: int = 10, alpha: float = 1.0,
          cached: Optional[dict] = None, itos: Optional[Sequence[str]] = None, pad_id: int = 0):
    """(metrics, probes).  metrics: the reference's keys ``regression_probe.<name>.r2`` / ``.corr``
    and ``regression_probe.avg_r2`` / ``.avg_corr``, and with several layers the same keys under
    ``regression_probe.layer<l>.`` for each.  The plain keys are the reference's, the last block's:
    with one layer they hold that layer, with several the last block when it is among them and
    are absent otherwise.  probes: numpy
    ``coef`` [layers][14][d], ``intercept`` [layers][14], ``names``, ``layers``, ``alpha``,
    ``n_rows``.  Without ``cached`` the metrics are the 5-fold cross-validated means and the probes
    the final fits on all rows.  With ``cached`` (such a probes dict for the same layers) nothing
    is fitted: the cached probes are scored on all rows from the summed Gram."""
    lay = layer_list(model, layers)
    d, m = int(model.n_embd), ops.SHAPE_TARGETS
    if cached is not None:
        if [int(l) for l in cached["layers"]] != lay or tuple(np.asarray(cached["coef"]).shape) != (len(lay), m, d):
            raise ValueError("cached probes were fitted for other layers or another width")
        gram, n_rows = collect_gram(model, ids, lay, batch_size, min_tokens, k=1, itos=itos, pad_id=pad_id)
    else:
        gram, n_rows = collect_gram(model, ids, lay, batch_size, min_tokens, itos=itos, pad_id=pad_id)
    if n_rows == 0:
        raise ValueError("no codon position in a sequence of at least min_tokens tokens")
    metrics: Dict[str, float] = {}
    coefs, icpts = [], []
    for i, l in enumerate(lay):
        if cached is not None:
            coef = torch.as_tensor(np.asarray(cached["coef"])[i], dtype=torch.float64, device=gram.device)
            icpt = torch.as_tensor(np.asarray(cached["intercept"])[i], dtype=torch.float64, device=gram.device)
            r2, corr = metrics_from_gram(gram[i, 0], d, m, coef, icpt)
        else:
            res = ridge_cv_from_gram(gram[i], d, m, alpha)
            coef, icpt, r2, corr = res["coef"], res["intercept"], res["r2"], res["corr"]
        r2, corr = r2.cpu().numpy(), corr.cpu().numpy()
        if len(lay) == 1 or l == int(model.n_layer) - 1:
            metrics.update(_metric_keys("regression_probe.", r2, corr))
        if len(lay) > 1:
            metrics.update(_metric_keys(f"regression_probe.layer{l}.", r2, corr))
        coefs.append(coef.cpu().numpy())
        icpts.append(icpt.cpu().numpy())
    probes = {"coef": np.stack(coefs), "intercept": np.stack(icpts), "names": np.array(NAMES),
              "layers": np.array(lay, dtype=np.int64),
              "alpha": np.float64(alpha if cached is None else cached["alpha"]), "n_rows": np.int64(n_rows)}
    return metrics, probes


def dna_ids(dna: str, itos: Optional[Sequence[str]] = None):
    """The token ids of the whole codons of ``dna`` that the vocabulary holds."""
    itos = default_vocab() if itos is None else list(itos)
    stoi = {t: i for i, t in enumerate(itos)}
    codons = [dna[i:i + 3] for i in range(0, len(dna) - 2, 3)]
    return [stoi[c] for c in codons if c in stoi]


def awareness(model, ids=None, layer: int = -1, itos: Optional[Sequence[str]] = None, batch_size: int = 64,
              pad_id: int = 0) -> Dict[str, float]:
    """The structural awareness score (probe_structural_awareness.py): per target the |corr| between
    the target and the projection of block ``layer``'s output on its first principal component,
    plus ``avg``.  ids: int [S][T]; the default is the reference's one test sequence
    ATG (GGCC)x5 (AAAA)x5 (CGTA)x5 TGA."""
    if ids is None:
        ids = np.asarray([dna_ids(AWARENESS_DNA, itos)], dtype=np.int64)
    gram, n_rows = collect_gram(model, ids, (layer,), batch_size, min_tokens=0, k=1, itos=itos, pad_id=pad_id)
    if n_rows == 0:
        raise ValueError("no codon position")
    score = awareness_from_gram(gram[0, 0], int(model.n_embd), ops.SHAPE_TARGETS).cpu().numpy()
    out = {name: float(score[j]) for j, name in enumerate(NAMES)}
    out["avg"] = float(np.mean([out[n] for n in NAMES]))
    return out
