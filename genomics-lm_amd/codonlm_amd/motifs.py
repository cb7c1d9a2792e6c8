"""Motif mining on the native engine (mirrors src/eval/motif_extractor.py, motif_clusterer.py,
motif_analysis.py and scripts/mine_motifs.py of the reference).

Block hidden states are mean-pooled over sliding windows of codons, windows touching a special
token are dropped, the rest is optionally reduced with PCA, clustered with k-means and summarised
per cluster.  What runs differs from the reference: batched engine forwards, pooling that reads
the engine's hidden-state buffer in place (cg_window_keep / cg_window_pool) into one preallocated
matrix, and Lloyd's algorithm on the device (cg_kmeans_step), bitwise reproducible for a seed.
The clustering is plain k-means++ with one initialisation; sklearn's greedy seeding trials,
``n_init > 1`` and HDBSCAN are not part of this path.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import ops


# ---------------------------------------------------------------------------- windows
def window_meta(keep: np.ndarray, window: int, stride: int) -> np.ndarray:
    """int64 [N][3] (sequence, start, end) of the kept windows of keep [S][nwin], in (sequence,
    window start) order -- the reference's kept_metadata."""
    seq, j = np.nonzero(np.asarray(keep))
    return np.stack([seq, j * stride, j * stride + window], axis=1).astype(np.int64).reshape(-1, 3)


@torch.no_grad()
def window_embeddings(model, ids, window: int, stride: int, layer: int = -1, exclude_ids: Sequence[int] = (),
                      batch_size: int = 256):
    """(emb fp32 [N][d] on the device, meta int64 [N][3] rows (sequence, start, end)): the mean of
    block ``layer``'s output over every window of ``window`` positions, ``stride`` apart, that holds
    no id of ``exclude_ids`` (MotifExtractor.extract over all sequences, in its order).  ids: int
    [S][T], trimmed to the model's block_size; eval-mode forwards of ``batch_size`` sequences."""
    if isinstance(layer, bool) or not isinstance(layer, (int, np.integer)):
        raise ValueError("window_embeddings: one layer index (lists of layers are not supported)")
    if window < 1 or stride < 1 or batch_size < 1:
        raise ValueError("window, stride and batch_size must be at least 1")
    host = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids)
    if host.ndim != 2:
        raise ValueError("ids must be [sequences][positions]")
    host = np.ascontiguousarray(host[:, :int(model.block_size)].astype(np.int64))
    S, T = host.shape
    eng = model.engine
    dev = model.flat_parameters().device
    d = int(model.n_embd)
    which = int(layer) % int(model.n_layer) + 1
    nwin = ops.window_count(T, window, stride)
    if S == 0 or nwin == 0:
        return torch.empty(0, d, dtype=torch.float32, device=dev), torch.empty(0, 3, dtype=torch.int64)
    x = torch.from_numpy(host).to(dev)
    keep = ops.window_keep(x, window, stride, exclude_ids)  # [S][nwin]
    flat = keep.reshape(-1)
    dst = torch.where(flat > 0, torch.cumsum(flat, 0, dtype=torch.int32) - 1, torch.full_like(flat, -1))
    dst = dst.reshape(S, nwin).contiguous()
    keep_host = keep.cpu().numpy()  # the one device read of the call: row count and metadata
    meta = window_meta(keep_host, window, stride)
    emb = torch.empty(meta.shape[0], d, dtype=torch.float32, device=dev)
    if meta.shape[0]:
        for s in range(0, S, batch_size):
            eng.forward(x[s:s + batch_size], None, training=False)
            ops.window_pool(eng.hidden(which), window, stride, dst[s:s + batch_size], emb)
    return emb, torch.from_numpy(meta)


# ---------------------------------------------------------------------------- PCA
def pca_project(X: torch.Tensor, n_components: int, chunk: int = 65536):
    """(Y [N][m], components [m][d] fp64, mean [d] fp64), m = min(n_components, d, N): the
    projection of the centred rows on the covariance's leading eigenvectors (PCA.fit_transform of
    motif_clusterer.py:30-34).  Mean and covariance are accumulated in fp64 over row chunks;
    components are ordered by descending eigenvalue, each with its entry of largest magnitude
    positive.  Y has X's dtype.  Plain torch: runs on any device."""
    N, d = X.shape
    m = min(int(n_components), d, N)
    if m < 1:
        raise ValueError("pca_project needs at least one row, column and component")
    mean = torch.zeros(d, dtype=torch.float64, device=X.device)
    for s in range(0, N, chunk):
        mean += X[s:s + chunk].to(torch.float64).sum(0)
    mean /= N
    cov = torch.zeros(d, d, dtype=torch.float64, device=X.device)
    for s in range(0, N, chunk):
        c = X[s:s + chunk].to(torch.float64) - mean
        cov += c.T @ c
    cov /= max(N - 1, 1)
    _, vec = torch.linalg.eigh(cov)  # ascending eigenvalues
    comp = vec.flip(1)[:, :m].T.contiguous()
    big = comp.gather(1, comp.abs().argmax(1, keepdim=True))
    comp = comp * torch.where(big < 0, -1.0, 1.0)
    Y = torch.empty(N, m, dtype=X.dtype, device=X.device)
    for s in range(0, N, chunk):
        Y[s:s + chunk] = ((X[s:s + chunk].to(torch.float64) - mean) @ comp.T).to(X.dtype)
    return Y, comp, mean


# ---------------------------------------------------------------------------- k-means
def kmeans_pp_init(X: torch.Tensor, n_clusters: int, seed: int = 42) -> torch.Tensor:
    """Plain k-means++ centres fp32 [k][d].  u = numpy.random.default_rng(seed).random(k): the first
    centre is row floor(u0 N); centre c is drawn by inverse CDF of u_c over the current minimum
    squared distances (fp64 cumsum, the first row whose cumulative mass exceeds u_c * total), the
    distances from kmeans_step against the newest centre; a zero total takes the lowest row not yet
    chosen.  No host read."""
    N = X.shape[0]
    u = np.random.default_rng(seed).random(n_clusters)
    first = min(int(np.floor(u[0] * N)), N - 1)
    idx = torch.full((), first, dtype=torch.int64, device=X.device)
    chosen = torch.zeros(N, dtype=torch.bool, device=X.device)
    centers = torch.empty(n_clusters, X.shape[1], dtype=torch.float32, device=X.device)
    mind = None
    for c in range(n_clusters):
        if c > 0:
            cum = torch.cumsum(mind.to(torch.float64), 0)
            total = cum[-1]
            drawn = torch.searchsorted(cum, (total * float(u[c])).reshape(1), right=True)[0].clamp(max=N - 1)
            lowest = (~chosen).to(torch.int32).argmax()
            idx = torch.where(total > 0, drawn, lowest)
        chosen[idx] = True
        centers[c] = X[idx]
        if c + 1 < n_clusters:
            d2 = ops.kmeans_step(X, centers[c:c + 1], want_stats=False, want_inertia=False).dist2
            mind = d2 if mind is None else torch.minimum(mind, d2)
    return centers


def kmeans(X: torch.Tensor, n_clusters: int, seed: int = 42, max_iter: int = 300, tol: float = 1e-4,
           init: Optional[torch.Tensor] = None):
    """(labels int32 [N], centers fp32 [k][d], inertia float, n_iter): Lloyd's algorithm on fp32
    points, one kmeans_step and one 8-byte host read per iteration.  New centres are sums / counts
    rounded to fp32; an empty cluster takes the point with the largest dist2 (lowest index on
    ties, one point per empty cluster in cluster order), which leaves its old cluster -- sklearn's
    rule.  Stops when no label changed, or when the summed squared centre shift is at most ``tol``
    times the mean per-column variance of X; one assign-only step then makes labels and inertia
    those of the returned centres."""
    if X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError("kmeans: fp32 points [N][d]")
    N, d = X.shape
    k = int(n_clusters)
    if k < 1 or k > N:
        raise ValueError(f"kmeans: n_clusters={k} needs 1 <= n_clusters <= N={N}")
    if init is None:
        centers = kmeans_pp_init(X, k, seed)
    else:
        centers = torch.as_tensor(init).to(device=X.device, dtype=torch.float32).contiguous().clone()
        if tuple(centers.shape) != (k, d):
            raise ValueError("kmeans: init must be [n_clusters][d]")
    x64 = X.to(torch.float64)
    tol_abs = tol * x64.var(0, unbiased=False).mean()
    del x64
    prev = torch.full((N,), -1, dtype=torch.int32, device=X.device)
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        r = ops.kmeans_step(X, centers, want_inertia=False)
        filled = r.counts > 0
        new = torch.where(filled[:, None], r.sums / r.counts.clamp(min=1)[:, None], centers.to(torch.float64))
        new = new.to(torch.float32)
        shift = ((new - centers).to(torch.float64) ** 2).sum()
        n_empty = (~filled).sum()
        n_changed = (r.labels != prev).sum()
        word = int((n_changed * 1024 + n_empty * 2 + (shift <= tol_abs).to(torch.int64)).item())
        changed, empties, small_shift = word >> 10, (word >> 1) & 511, bool(word & 1)
        if empties:
            new = _relocate_empty(X, r, new, filled, empties)
            small_shift = False  # the shift read above belongs to the centres before the relocation
        centers, prev = new, r.labels
        if changed == 0 or small_shift:
            break
    r = ops.kmeans_step(X, centers, want_stats=False)
    return r.labels, centers, float(r.inertia), n_iter


def _relocate_empty(X, r, new, filled, n_empty):
    """The e-th empty cluster (in cluster order) becomes the point with the e-th largest dist2
    (stable descending sort: lowest index first among equals); that point leaves its cluster."""
    far = torch.sort(r.dist2, descending=True, stable=True).indices[:n_empty]
    empty = torch.nonzero(~filled).reshape(-1)
    sums, counts = r.sums.clone(), r.counts.clone()
    pts = X[far].to(torch.float64)
    donors = r.labels[far].to(torch.int64)
    sums.index_add_(0, donors, -pts)
    counts.index_add_(0, donors, -torch.ones_like(donors))
    sums[empty] = pts
    counts[empty] = 1
    ok = counts > 0
    out = torch.where(ok[:, None], sums / counts.clamp(min=1)[:, None], new.to(torch.float64))
    return out.to(torch.float32)


# ---------------------------------------------------------------------------- analysis and report
def calculate_pwm(sequences: Sequence[Sequence[str]], vocab: Sequence[str]) -> np.ndarray:
    """Position weight matrix [len(vocab)][L] of equally long token sequences: the share of each
    vocabulary token at each position (motif_analysis.py:4-33; tokens outside vocab are not
    counted).  No sequences: an empty [0][0] matrix."""
    if not sequences:
        return np.zeros((0, 0))
    index = {t: i for i, t in enumerate(vocab)}
    counts = np.zeros((len(vocab), len(sequences[0])))
    for seq in sequences:
        for pos, tok in enumerate(seq):
            i = index.get(tok)
            if i is not None:
                counts[i, pos] += 1
    return counts / len(sequences)


def get_consensus(pwm: np.ndarray, vocab: Sequence[str]) -> str:
    """The most frequent token of every position, first in vocabulary order on ties, joined
    (motif_analysis.py:35-41)."""
    if pwm.size == 0:
        return ""
    return "".join(vocab[i] for i in pwm.argmax(0))


def cluster_order(labels: np.ndarray) -> List[int]:
    """Cluster labels by size descending; equal sizes in order of first appearance (the reference
    sorts a dict filled in window order with a stable sort)."""
    labels = np.asarray(labels)
    uniq, first, counts = np.unique(labels, return_index=True, return_counts=True)
    by_first = np.argsort(first, kind="stable")
    order = by_first[np.argsort(-counts[by_first], kind="stable")]
    return [int(uniq[i]) for i in order]


def build_report(title: str, n_sequences: int, labels: np.ndarray, windows: Sequence[Sequence[str]],
                 vocab: Sequence[str], method: str, layer: int) -> str:
    """motif_report.md in the reference's layout (scripts/mine_motifs.py:133-164)."""
    labels = np.asarray(labels)
    report = [f"# Motif Mining Report: {title}", "", f"- **Sequences sampled:** {n_sequences}",
              f"- **Total windows:** {len(labels)}", f"- **Method:** {method}", f"- **Layer:** {layer}", ""]
    for lab in cluster_order(labels):
        seqs = [windows[i] for i in np.nonzero(labels == lab)[0]]
        cons = get_consensus(calculate_pwm(seqs, vocab), vocab)
        report += [f"## Cluster {lab} (size={len(seqs)})", f"**Consensus:** `{cons}`", "", "**Top 5 Examples:**"]
        report += [f"- `{' '.join(ex)}`" for ex in seqs[:5]]
        report.append("")
    return "\n".join(report)


def window_tokens(ids: np.ndarray, meta: np.ndarray, vocab: Sequence[str]) -> List[List[str]]:
    return [[vocab[t] if 0 <= t < len(vocab) else f"tok_{t}" for t in ids[s, a:b]] for s, a, b in np.asarray(meta)]


def check_method(method: str) -> None:
    if method == "hdbscan":
        raise ValueError("--method hdbscan is not on the MI355X path: only kmeans runs on the native engine")
    if method != "kmeans":
        raise ValueError(f"Unknown clustering method: {method}")


def mine(model, ids, *, window: int = 9, stride: int = 3, n_clusters: int = 10, pca: int = 50, layer: int = -1,
         exclude_ids: Sequence[int] = (), seed: int = 42, batch_size: int = 256, method: str = "kmeans",
         max_iter: int = 300, tol: float = 1e-4) -> Optional[dict]:
    """Window embeddings -> optional PCA (pca = 0: off) -> k-means.  None when no window is kept;
    else a dict of numpy arrays: labels int32 [N], centers fp32 [k][m] (in the clustered space, as
    the reference's cluster_centers_), meta int64 [N][3], and inertia, n_iter."""
    check_method(method)
    emb, meta = window_embeddings(model, ids, window, stride, layer=layer, exclude_ids=exclude_ids,
                                  batch_size=batch_size)
    if emb.shape[0] == 0:
        return None
    X = pca_project(emb, pca)[0].contiguous() if pca else emb
    labels, centers, inertia, n_iter = kmeans(X, n_clusters, seed=seed, max_iter=max_iter, tol=tol)
    return {"labels": labels.cpu().numpy(), "centers": centers.cpu().numpy(), "meta": meta.numpy(),
            "inertia": inertia, "n_iter": n_iter}
