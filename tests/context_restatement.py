"""fp64 numpy restatement of the context-diagnostic contracts of include/codonlm_hip.h
(cg_ngram_count, cg_ngram_totals, cg_ngram_nll, cg_diag_rows) and of the paired bootstrap, plus the
synthetic inputs the tests of those kernels share.

tests/test_context_cpu.py ties this restatement to the reference's own functions through
tests/golden/context_diag.npz; the GPU op tests compare the kernels with it.
"""
from __future__ import annotations

import numpy as np

V, PAD, SEP = 20, 0, 3
HELD_OUT = 19          # the token id kept out of the training rows
TS = (1, 63, 64, 65, 130)
N_TRAIN, N_TEST = 40, 7
SLICES = ("all", "after_separator", "window_with_chunk_continuation", "window_without_chunk_continuation",
          "segment_position_0", "segment_position_1_3", "segment_position_4_15", "segment_position_16_63",
          "segment_position_64_plus", "target_class_special", "target_class_start_codon",
          "target_class_stop_codon", "target_class_ordinary_codon")
# itos of the V = 20 inputs: ids 0..3 special, 4 = ATG, 5..7 the stop codons, the rest ordinary
ITOS = ["<PAD>", "<BOS>", "<EOS>", "<SEP>", "ATG", "TAA", "TAG", "TGA"] + [f"C{i:02d}" for i in range(8, V)]


def token_classes(itos):
    """uint8 [V]: 0 special, 1 start, 2 stop, 3 ordinary (the reference's _token_class)."""
    out = np.empty(len(itos), np.uint8)
    for i, tok in enumerate(itos):
        out[i] = 0 if tok.startswith("<") else 1 if tok == "ATG" else 2 if tok in ("TAA", "TAG", "TGA") else 3
    return out


# ------------------------------------------------------------------ inputs
def make_rows(rng, n, T, *, top=V, p_sep=0.06):
    """n packed windows of T positions: tokens 4..top-1, SEP with probability p_sep, a PAD tail of up
    to T / 2 positions; x = tokens[:-1], y = tokens[1:]."""
    tok = rng.integers(4, top, size=(n, T + 1))
    tok[rng.random((n, T + 1)) < p_sep] = SEP
    x, y = tok[:, :-1].copy(), tok[:, 1:].copy()
    for b in range(n):
        tail = int(rng.integers(0, T // 2 + 1))
        if tail:
            y[b, T - tail:] = PAD
            x[b, T - tail + 1:] = PAD
    return x.astype(np.int64), y.astype(np.int64)


def make_split(T, seed=0):
    """(train x, y, test x, y, test row flags) at window length T with the forced corners: a PAD
    target in mid-row under a SEP input, SEP at positions 0 and T-1, two adjacent SEPs, the held-out
    token after a SEP and in mid-segment of three test rows, and at T = 130 a test row without SEP
    and PAD."""
    rng = np.random.default_rng(1000 * T + seed)
    xtr, ytr = make_rows(rng, N_TRAIN, T, top=HELD_OUT)
    xte, yte = make_rows(rng, N_TEST, T, top=HELD_OUT)
    for x, y in ((xtr, ytr), (xte, yte)):
        x[0][x[0] == PAD] = 9           # row 0 has no PAD tail: its SEP at T-1 is a valid position
        y[0][y[0] == PAD] = 9
        x[0, 0] = SEP
        x[0, T - 1] = SEP
        if T >= 8:
            x[1, T // 2] = SEP
            y[1, T // 2] = PAD          # PAD target in mid-row under a SEP input
            y[1, T // 2 + 1] = 9        # (valid targets follow it)
            x[2, 4] = x[2, 5] = SEP     # two adjacent SEPs
            y[2, 3] = y[2, 4] = SEP
            y[2, 5] = 9
    if T >= 8:
        for b in (3, 4, 5):
            xte[b, 2], yte[b, 1] = SEP, SEP
            xte[b, 3], yte[b, 2] = HELD_OUT, HELD_OUT     # the held-out token after a SEP ...
            yte[b, 3] = 8
            xte[b, 6], xte[b, 7] = 10, 11
            yte[b, 5], yte[b, 6] = 10, 11
            xte[b, 8], yte[b, 7] = HELD_OUT, HELD_OUT     # ... and in mid-segment
            yte[b, 8] = 12
    else:
        xte[3, 0] = HELD_OUT
    if T == 130:
        tok = rng.integers(4, HELD_OUT, size=T + 1)
        xte[6], yte[6] = tok[:-1], tok[1:]
    flags = (np.arange(N_TEST) % 3 == 1).astype(np.uint8)
    return xtr, ytr, xte, yte, flags


def make_logits(rng, x, y, Vz=V, *, scale=2.0, wide=False):
    """fp32 logits [B*T][ldl] (fp16-representable values) for targets y < Vz; with ``wide``, ldl > Vz
    and NaN in the pad columns."""
    n = x.size
    ldl = (Vz + 15) // 16 * 16 + 16 if wide else Vz
    z = np.full((n, ldl), np.nan, np.float32)
    z[:, :Vz] = (rng.standard_normal((n, Vz)) * scale).astype(np.float32)
    hit = rng.random(n) < 0.4   # some rows predict their target
    z[hit, y.reshape(-1)[hit]] += np.float32(4.0)
    z[:, :Vz] = z[:, :Vz].astype(np.float16).astype(np.float32)  # a fixture can hold them as fp16
    return z


# ------------------------------------------------------------------ cg_ngram_count / totals / nll
def _positions(x, y, Vn, pad, reset):
    """previous, previous2, counted and bad masks of every position."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    B, T = x.shape
    isreset = np.zeros(Vn, bool)
    isreset[list(reset)] = True
    ok = lambda a: (a >= 0) & (a < Vn)  # noqa: E731
    shifted = np.concatenate([np.full((B, 1), pad, np.int64), x[:, :-1]], axis=1)
    restart = (np.arange(T)[None, :] == 0) | (ok(x) & isreset[np.where(ok(x), x, 0)])
    p2 = np.where(restart, pad, shifted)
    live = y != pad
    good = ok(x) & ok(y) & ok(p2)
    return x, y, p2, live & good, live & ~good


def count_tables(x, y, Vn=V, pad=PAD, reset=(SEP,)):
    """(uni, bi, tri, n_bad) of cg_ngram_count."""
    p, t, p2, counted, bad = _positions(x, y, Vn, pad, reset)
    uni = np.bincount(t[counted], minlength=Vn).astype(np.int64)
    bi = np.bincount(p[counted] * Vn + t[counted], minlength=Vn * Vn).astype(np.int64).reshape(Vn, Vn)
    tri = np.bincount((p2[counted] * Vn + p[counted]) * Vn + t[counted],
                      minlength=Vn ** 3).astype(np.int64).reshape(Vn, Vn, Vn)
    return uni, bi, tri, int(bad.sum())


def totals(uni, bi, tri):
    """cg_ngram_totals: sums over the targets 1 .. V-1."""
    return uni[1:].sum(keepdims=True), bi[:, 1:].sum(-1), tri[:, :, 1:].sum(-1)


def ngram_nll(x, y, tables, alpha, Vn=V, pad=PAD, reset=(SEP,)):
    """Everything cg_ngram_nll returns plus the bookkeeping the tests assert on."""
    uni, bi, tri = tables[:3]
    tu, tb, tt = totals(uni, bi, tri)
    p, t, p2, counted, _ = _positions(x, y, Vn, pad, reset)
    ps, ts, p2s = (np.where(counted, a, 0) for a in (p, t, p2))
    active = Vn - 1
    den0 = alpha * active
    backoff = counted & (tt[p2s, ps] == 0)
    unseen = counted & (tb[ps] == 0)
    with np.errstate(divide="ignore"):
        l_uni = -np.log((uni[ts] + alpha) / (float(tu[0]) + den0))
        l_bi = -np.log((bi[ps, ts] + alpha) / (tb[ps] + den0))
        ct = np.where(backoff, bi[ps, ts], tri[p2s, ps, ts])
        ctot = np.where(backoff, tb[ps], tt[p2s, ps])
        l_tri = -np.log((ct + alpha) / (ctot + den0))
    tok = np.stack([np.full(x.shape, np.log(active)), l_uni, l_bi, l_tri]) * counted[None]
    row_sums = tok.sum(-1).T.copy()                       # [B][4]
    row_count = counted.sum(-1)
    acc = np.concatenate([row_sums.sum(0), [row_count.sum()]])
    return {"tok": tok, "counted": counted, "backoff": backoff, "unseen": unseen, "row_sums": row_sums,
            "row_count": row_count, "acc": acc, "abs_terms": np.abs(tok).sum((1, 2))}


# ------------------------------------------------------------------ cg_diag_rows
def segment_positions(x, y, Vn=V, pad=PAD, sep=SEP):
    """The reference's counter: over the valid positions of a row, 0 at a valid separator input,
    +1 after each valid position; -1 where invalid."""
    x, y = np.asarray(x), np.asarray(y)
    out = np.full(x.shape, -1, np.int32)
    for b in range(x.shape[0]):
        k = 0
        for t in range(x.shape[1]):
            if y[b, t] == pad or not 0 <= y[b, t] < Vn:
                continue
            if x[b, t] == sep:
                k = 0
            out[b, t] = k
            k += 1
    return out


def position_slice(sp):
    return np.where(sp == 0, 4, np.where(sp < 4, 5, np.where(sp < 16, 6, np.where(sp < 64, 7, 8))))


def diag_rows(z32, x, y, Vz, *, pad=PAD, sep=SEP, row_flag=None, tok_class=None, edges=None):
    """The outputs of cg_diag_rows for logits z32 [B*T][ldl]; ``calib64`` holds the fp64 confidence
    sums next to the contract's sums of the fp32-rounded confidence."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    B, T = x.shape
    z = z32[:, :Vz].astype(np.float64)
    n = z.shape[0]
    valid = ((y != pad) & (y >= 0) & (y < Vz)).reshape(-1)
    yy = np.where(valid, y.reshape(-1), 0)
    amax = z.argmax(1)
    m = z[np.arange(n), amax]
    e = np.exp(z - m[:, None])
    e[np.arange(n), amax] = 0.0
    s1, s2 = e.sum(1), (e * e).sum(1)
    lgs = np.log1p(s1)
    dzy = z[np.arange(n), yy] - m
    nll = np.where(valid, lgs - dzy, 0.0)
    conf = 1.0 / (1.0 + s1)
    py = np.where(yy == amax, conf, np.exp(dzy) * conf)
    brier = (1.0 + s2) * conf * conf - 2.0 * py + 1.0
    correct = (amax == yy) & valid
    conf32 = conf.astype(np.float32)
    sp = segment_positions(x, y, Vz, pad, sep).reshape(-1)
    flag = np.zeros(B, bool) if row_flag is None else np.asarray(row_flag).astype(bool)
    member = np.zeros((len(SLICES), n), bool)
    member[0] = valid
    member[1] = valid & (x.reshape(-1) == sep)
    member[2] = valid & np.repeat(flag, T)
    member[3] = valid & ~np.repeat(flag, T)
    ps = position_slice(sp)
    for s in range(4, 9):
        member[s] = valid & (ps == s)
    if tok_class is not None:
        k = np.asarray(tok_class)[yy]
        for c in range(4):
            member[9 + c] = valid & (k == c)
    slices = np.array([[nll[mk].sum(), mk.sum()] for mk in member])
    out = {"nll": nll.reshape(B, T), "segpos": sp.reshape(B, T), "conf": np.where(valid, conf, 0.0).reshape(B, T),
           "valid": valid.reshape(B, T), "correct": correct.reshape(B, T), "slices": slices,
           "brier_acc": np.array([brier[valid].sum(), valid.sum()], np.float64),
           "row_nll": nll.reshape(B, T).sum(1), "row_count": valid.reshape(B, T).sum(1).astype(np.int32),
           "conf64": conf, "margin_ok": None}
    if edges is not None:
        edges = np.asarray(edges, np.float32)
        nb = len(edges) - 1
        bin_ = np.full(n, -1)
        for i in range(nb - 1, -1, -1):
            bin_[(conf32 > edges[i]) & (conf32 <= edges[i + 1])] = i
        bin_[~valid] = -1
        calib = np.zeros((nb, 3))
        calib64 = np.zeros((nb, 3))
        for i in range(nb):
            sel = bin_ == i
            calib[i] = [sel.sum(), conf32[sel].astype(np.float64).sum(), correct[sel].sum()]
            calib64[i] = [sel.sum(), conf[sel].sum(), correct[sel].sum()]
        # distance of every valid confidence to the nearest interior edge, in fp32 ulps at the edge
        inner = edges[1:-1].astype(np.float64)
        dist = np.abs(conf32[valid].astype(np.float64)[:, None] - inner[None, :]) / np.spacing(edges[1:-1])[None, :]
        out.update(bin=bin_.reshape(B, T), calib=calib, calib64=calib64,
                   edge_ulps=float(dist.min()) if dist.size else np.inf)
    return out


def ece_from_calib(calib):
    """sum_i (n_i / N) |mean conf_i - accuracy_i| over the non-empty bins."""
    n = calib[:, 0]
    keep = n > 0
    if not keep.any():
        return float("nan")
    return float((n[keep] / n.sum() * np.abs(calib[keep, 1] / n[keep] - calib[keep, 2] / n[keep])).sum())


# ------------------------------------------------------------------ the paired bootstrap
def paired_bootstrap(row_model, row_baseline, row_tokens, seed, samples):
    """(observed, low, high) of the paired gate: the per-token loss gap over the windows that hold
    tokens and its 95 % interval over resampled windows.  The stream is the contract: default_rng(seed)
    gives one vector of n window indices per resample; a resample's ratio is the sum of its gathered
    gaps over the sum of its gathered token counts."""
    used = np.flatnonzero(np.asarray(row_tokens) > 0)
    gap = np.asarray(row_model, np.float64)[used] - np.asarray(row_baseline, np.float64)[used]
    tok = np.asarray(row_tokens, np.int64)[used]
    rng = np.random.default_rng(seed)
    draws = [rng.integers(0, len(used), size=len(used)) for _ in range(samples)]
    ratios = np.array([np.take(gap, d).sum() / np.take(tok, d).sum() for d in draws], np.float64)
    return float(gap.sum() / tok.sum()), float(np.quantile(ratios, 0.025)), float(np.quantile(ratios, 0.975))
