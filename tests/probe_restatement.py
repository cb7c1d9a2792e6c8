"""Plain numpy fp64 restatement of the three contracts of the structural regression probes
(include/codonlm_hip.h cg_shape_targets / cg_gram_accum, codonlm_amd.structure_probe
ridge_cv_from_gram): targets from token ids, the grouped augmented Gram, ridge cross-validation on
explicit matrices.  Written from the contracts; slow and obvious on purpose."""
import numpy as np

NAMES = ("MGW", "Roll", "EP", "ProT", "HelT", "Slide", "Rise", "Shift", "Tilt", "Buckle", "Opening", "Shear",
         "Stagger", "Stretch")
# per target: (words, value) rules in order, then the default
RULES = (
    ((("AAAA",), 3.5), (("GGGG", "CCCC"), 5.8), 4.5),
    ((("GC", "CG"), 5.0), (("AA", "TT"), 0.0), 2.5),
    ((("AAAA",), -10.0), (("GGCC",), -2.0), -5.0),
    ((("GC",), -11.0), (("AT",), -18.0), -14.0),
    ((("CG",), 36.0), (("TA",), 32.0), 34.0),
    ((("AAAA",), -0.8), (("GC", "CG"), 0.2), -0.3),
    ((("CG",), 3.2), (("AA",), 3.4), 3.3),
    ((("AA", "TT"), 0.0), (("GC",), 0.2), -0.1),
    ((("AA",), 0.0), (("CG",), 0.5), -0.2),
    ((("GC",), -12.0), (("AT",), 0.0), -6.0),
    ((("AT",), 2.0), (("GC",), 0.5), 1.0),
    ((("GC",), 0.0), 0.1),
    ((("AA",), 0.1), -0.1),
    ((("CG",), -0.1), 0.0),
)


def nucleotide_values(dna):
    """fp64 [len(dna)][14]: every nucleotide's values from its window dna[i-2 : i+3]."""
    out = np.zeros((len(dna), 14))
    for i in range(len(dna)):
        w = dna[max(0, i - 2):min(len(dna), i + 3)]
        for k, rule in enumerate(RULES):
            val = rule[-1]
            for words, v in rule[:-1]:
                if any(x in w for x in words):
                    val = v
                    break
            out[i, k] = val
    return out


def codon_targets(dna):
    """fp32 [len(dna) // 3][14]: ((a + b) + c) / 3 of each codon's nucleotides in fp64, rounded once."""
    v = nucleotide_values(dna)
    n = len(dna) // 3
    out = np.zeros((n, 14), dtype=np.float32)
    for c in range(n):
        out[c] = (((v[3 * c] + v[3 * c + 1]) + v[3 * c + 2]) / 3.0).astype(np.float32)
    return out


def shape_targets(idx, itos):
    """(y fp32 [B*T][14] with zeros in the rows no codon owns, valid int32 [B*T]) for ids [B][T]: a run
    is a maximal stretch of codon tokens in one row."""
    idx = np.asarray(idx)
    B, T = idx.shape
    is_codon = [len(t) == 3 and set(t) <= set("ACGT") for t in itos]
    y = np.zeros((B * T, 14), dtype=np.float32)
    valid = np.zeros(B * T, dtype=np.int32)
    for b in range(B):
        t = 0
        while t < T:
            ok = lambda u: 0 <= idx[b, u] < len(itos) and is_codon[idx[b, u]]
            if not ok(t):
                t += 1
                continue
            e = t
            while e < T and ok(e):
                e += 1
            y[b * T + t:b * T + e] = codon_targets("".join(itos[idx[b, u]] for u in range(t, e)))
            valid[b * T + t:b * T + e] = 1
            t = e
    return y, valid


def augmented(h, y, m):
    """z fp64 [rows][d + m + 1] = (h, y[:, :m], 1)."""
    h = np.asarray(h, dtype=np.float64)
    cols = [h]
    if m:
        cols.append(np.asarray(y, dtype=np.float64)[:, :m])
    cols.append(np.ones((h.shape[0], 1)))
    return np.concatenate(cols, axis=1)


def gram(h, y, m, grp, G):
    """(gram fp64 [G][P][P], bound [G][P][P] = sum |z_i||z_j|, counts [G]); rows whose group is
    outside [0, G) are dropped before anything of them is used."""
    grp = np.asarray(grp)
    P = np.asarray(h).shape[1] + m + 1
    out, mag, cnt = np.zeros((G, P, P)), np.zeros((G, P, P)), np.zeros(G, dtype=np.int64)
    for g in range(G):
        rows = np.nonzero(grp == g)[0]
        if rows.size == 0:
            continue
        z = augmented(np.asarray(h)[rows], None if y is None else np.asarray(y)[rows], m)
        out[g] = z.T @ z
        mag[g] = np.abs(z).T @ np.abs(z)
        cnt[g] = rows.size
    return out, mag, cnt


def ridge(X, y, alpha):
    """(w, b) of ridge with an unpenalised intercept, on explicit fp64 matrices."""
    mu, yb = X.mean(0), y.mean()
    Xc = X - mu
    w = np.linalg.solve(Xc.T @ Xc + alpha * np.eye(X.shape[1]), Xc.T @ (y - yb))
    return w, yb - mu @ w


def scores(X, y, w, b):
    """(r2, corr) of the probe on explicit rows; a constant target gives (0, 0), a constant
    prediction corr 0."""
    p = X @ w + b
    n = len(y)
    ss_tot = ((y - y.mean()) ** 2).sum()
    if ss_tot <= 4 * n * 2.0 ** -53 * (y * y).sum():
        return 0.0, 0.0
    r2 = 1.0 - ((y - p) ** 2).sum() / ss_tot
    vp = ((p - p.mean()) ** 2).sum()
    if vp <= 4 * n * 2.0 ** -53 * (p * p).sum():
        return r2, 0.0
    return r2, ((p - p.mean()) * (y - y.mean())).sum() / np.sqrt(vp * ss_tot)


def ridge_cv(X, Y, fold, k, alpha=1.0):
    """dict of fold_r2 / fold_corr [k][m], r2 / corr [m], coef [m][d], intercept [m] on explicit fp64
    matrices X [n][d], Y [n][m] with the test fold of every row in ``fold``."""
    X, Y, fold = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64), np.asarray(fold)
    m = Y.shape[1]
    fr, fc = np.zeros((k, m)), np.zeros((k, m))
    for f in range(k):
        tr, te = fold != f, fold == f
        for j in range(m):
            w, b = ridge(X[tr], Y[tr, j], alpha)
            fr[f, j], fc[f, j] = scores(X[te], Y[te, j], w, b)
    coef, icpt = np.zeros((m, X.shape[1])), np.zeros(m)
    for j in range(m):
        coef[j], icpt[j] = ridge(X, Y[:, j], alpha)
    return {"fold_r2": fr, "fold_corr": fc, "r2": fr.mean(0), "corr": fc.mean(0), "coef": coef, "intercept": icpt}


def condition(X, alpha=1.0):
    """kappa = (lambda_max(Sxx) + alpha) / (lambda_min(Sxx) + alpha) of the centred X."""
    Xc = np.asarray(X, dtype=np.float64)
    Xc = Xc - Xc.mean(0)
    ev = np.linalg.eigvalsh(Xc.T @ Xc)
    return (ev[-1] + alpha) / (max(ev[0], 0.0) + alpha)
