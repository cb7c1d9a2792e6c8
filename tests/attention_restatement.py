"""fp64 numpy restatement of the cg_attn_stats contract of include/codonlm_hip.h, plus the seeded
inputs the tests of that kernel share.

tests/test_attention_cpu.py ties this restatement to the reference's own head statistics
(scripts/conference_attention._head_stats) through tests/golden/attention_heads.npz; the GPU op test
compares the kernels with it.
"""
from __future__ import annotations

import numpy as np

V, PAD, SEP = 20, 0, 3
# itos of the V = 20 inputs: ids 0..3 special, 4 = ATG, 5..7 the stop codons, the rest ordinary
ITOS = ["<PAD>", "<BOS>", "<EOS>", "<SEP>", "ATG", "TAA", "TAG", "TGA"] + [f"C{i:02d}" for i in range(8, V)]
STATS = ("entropy", "norm_entropy", "mass_special", "mass_start", "mass_stop", "mass_ordinary",
         "dist_0", "dist_1_3", "dist_4_15", "dist_16_63", "dist_64_plus", "mean_dist", "max_prob", "first")
NSTAT = len(STATS)
ENTROPY, NORM_ENTROPY, MASS0, DIST0, MEAN_DIST, MAX_PROB, FIRST = 0, 1, 2, 6, 11, 12, 13
DIST_BINS = ((0, 0), (1, 3), (4, 15), (16, 63), (64, None))
GOLDEN_SHAPES = (5, 64)          # T of the golden cases; L = 2 layers, B = 2, H = 3, KV = 3, hd = 8
GOLDEN_L, GOLDEN_B, GOLDEN_H, GOLDEN_HD = 2, 2, 3, 8


def token_classes(itos):
    """uint8 [V]: 0 special, 1 start, 2 stop, 3 ordinary (the reference's _token_class)."""
    out = np.empty(len(itos), np.uint8)
    for i, tok in enumerate(itos):
        out[i] = 0 if tok.startswith("<") else 1 if tok == "ATG" else 2 if tok in ("TAA", "TAG", "TGA") else 3
    return out


# ------------------------------------------------------------------ inputs
def make_tokens(B, T, seed=0):
    """int64 [B][T] of tokens 4..V-1 with about 6 % SEP and the planted corners: SEP at position 0, at
    63 / 64 and at 127 / 128 (where T reaches them), two adjacent SEPs, every token class, a PAD tail
    on every row but the first (row 0 keeps every position).  A SEP row sees only itself."""
    rng = np.random.default_rng(7919 * T + 31 * B + seed)
    x = rng.integers(4, V, size=(B, T))
    x[rng.random((B, T)) < 0.06] = SEP
    for b in range(B):
        r = x[b]
        if b % 2 == 0:
            r[0] = SEP
        for p in (63, 64, 127, 128):
            if p < T and (p + b) % 2 == 1:
                r[p] = SEP
        if T >= 5:
            r[2:4] = SEP                       # two adjacent SEPs
            r[4] = 4 + (b % 4)                 # ATG or a stop codon right after them
        if T >= 12:
            r[8:12] = (1, 4, 6, 9)             # special, start, stop, ordinary
        if b > 0 and T > 1:
            tail = 1 + int(rng.integers(0, max(1, T // 3)))
            r[T - tail:] = PAD
    return x.astype(np.int64)


def make_qkv(B, T, H, KV, hd, seed=0):
    """fp32 [B*T][(H + 2 KV) hd] of unit-variance rows (q | k | v), as cg_attn_fwd reads them."""
    rng = np.random.default_rng(104729 * T + 1009 * H + 13 * hd + seed)
    return rng.standard_normal((B * T, (H + 2 * KV) * hd)).astype(np.float32)


# ------------------------------------------------------------------ the contract
def attention_mask(idx, B, T, *, sep_id=None, window=0):
    """bool [B][T][T]: key k visible to query q iff k <= q, q - k < window (window > 0) and no
    separator in (k, q] (equal cumulative separator counts), the forward's mask."""
    pos = np.arange(T)
    dist = pos[:, None] - pos[None, :]
    m = dist >= 0
    if window and window > 0:
        m = m & (dist < int(window))
    m = np.broadcast_to(m[None], (B, T, T)).copy()
    if sep_id is not None and idx is not None:
        seg = np.cumsum(idx == int(sep_id), axis=1)
        m &= seg[:, :, None] == seg[:, None, :]
    return m


def probabilities(qkv, m, B, T, H, KV, hd):
    """fp64 [B][H][T][T]: softmax over the visible keys of q . k / sqrt(hd), 0 elsewhere; query head
    h reads KV head h // (H // KV)."""
    a = np.asarray(qkv, dtype=np.float64).reshape(B, T, (H + 2 * KV), hd)
    q, k = a[:, :, :H], a[:, :, H:H + KV]
    k = np.repeat(k, H // KV, axis=2)
    s = np.einsum("bqhd,bkhd->bhqk", q, k) / np.sqrt(float(hd))
    s = np.where(m[:, None], s, -np.inf)
    s -= s.max(-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(-1, keepdims=True)


def stats_from_probs(P, m, *, idx=None, pad_id=-1, tok_class=None, row_keep=None):
    """Every output of cg_attn_stats from the probabilities P [B][H][T][T] under the mask m:
    dict(rows [B][H][T][14], nvis [B][T], received [B][H][T], head_acc [H][14], n_rows, keep [B][T])."""
    B, H, T, _ = P.shape
    pos = np.arange(T)
    dist = pos[:, None] - pos[None, :]
    nvis = m.sum(-1).astype(np.int64)
    lo = m.argmax(-1)                                             # the first visible key
    rows = np.zeros((B, H, T, NSTAT))
    with np.errstate(divide="ignore", invalid="ignore"):
        plogp = np.where(P > 0, P * np.log(P), 0.0)
    ent = -plogp.sum(-1)
    rows[..., ENTROPY] = ent
    with np.errstate(divide="ignore", invalid="ignore"):
        rows[..., NORM_ENTROPY] = np.where(nvis[:, None] > 1, ent / np.log(np.maximum(nvis, 2))[:, None], 0.0)
    if tok_class is not None:
        if idx is None:
            raise ValueError("tok_class needs idx")
        ok = (idx >= 0) & (idx < len(tok_class))
        cls = np.where(ok, np.asarray(tok_class)[np.clip(idx, 0, len(tok_class) - 1)], 255)
        for c in range(4):
            rows[..., MASS0 + c] = (P * (cls == c)[:, None, None, :]).sum(-1)
    for i, (a, b) in enumerate(DIST_BINS):
        sel = (dist >= a) if b is None else (dist >= a) & (dist <= b)
        rows[..., DIST0 + i] = (P * sel).sum(-1)
    rows[..., MEAN_DIST] = (P * dist).sum(-1)
    rows[..., MAX_PROB] = P.max(-1)
    rows[..., FIRST] = np.take_along_axis(P, np.broadcast_to(lo[:, None, :, None], (B, H, T, 1)), -1)[..., 0]
    keep = np.ones((B, T), bool)
    if idx is not None:
        keep &= idx != pad_id
    if row_keep is not None:
        keep &= np.asarray(row_keep).reshape(B, T) != 0
    rows *= keep[:, None, :, None]
    received = (P * keep[:, None, :, None]).sum(2)
    return dict(rows=rows, nvis=nvis, received=received, head_acc=rows.sum((0, 2)), n_rows=int(keep.sum()), keep=keep)


def attn_stats(qkv, B, T, H, KV, hd, *, idx=None, sep_id=None, window=0, pad_id=-1, tok_class=None, row_keep=None):
    """The outputs of cg_attn_stats for the qkv rows (plus ``P``, the probabilities themselves)."""
    m = attention_mask(idx, B, T, sep_id=sep_id, window=window)
    P = probabilities(qkv, m, B, T, H, KV, hd)
    out = stats_from_probs(P, m, idx=idx, pad_id=pad_id, tok_class=tok_class, row_keep=row_keep)
    out["P"] = P
    return out


def reference_triple(rows, tokens, tok_class):
    """(H, 3) of conference_attention._head_stats for ONE sequence from its fused row sums
    ``rows`` [H][T][14] (every row kept): the mean entropy, and the mean of P over all rows and the
    start (stop) columns = sum of MASS_START (MASS_STOP) / (T * number of such columns), 0 where the
    sequence has no such column."""
    H, T, _ = rows.shape
    cls = np.asarray(tok_class)[np.asarray(tokens)]
    out = np.zeros((H, 3))
    out[:, 0] = rows[:, :, ENTROPY].mean(1)
    for j, c in ((1, 1), (2, 2)):
        n = int((cls == c).sum())
        if n:
            out[:, j] = rows[:, :, MASS0 + c].sum(1) / (T * n)
    return out


def golden_case(T):
    """(tokens [B][T], P fp64 [L][B][H][T][T]) of the golden case at length T: SEP-masked layers."""
    B, H, hd = GOLDEN_B, GOLDEN_H, GOLDEN_HD
    idx = make_tokens(B, T, seed=5)
    P = np.stack([attn_stats(make_qkv(B, T, H, H, hd, seed=layer), B, T, H, H, hd, idx=idx, sep_id=SEP)["P"]
                  for layer in range(GOLDEN_L)])
    return idx, P
