"""Host side of the structural regression probes (cg_shape_targets, cg_gram_accum and
codonlm_amd.structure_probe): the fp64 restatement against the reference's recorded targets, the
fold rule against sklearn's recorded folds, the closed-form ridge cross-validation on the Gram
against the recorded sklearn procedure, and the CLI's device-free parts.

Fixtures (tests/golden, data only): shape_targets.npz -- get_theoretical_shape with the reference's
per-codon pooling on codon-only DNA strings; ridge_kfold.npz -- X fp32 [203][12], Y [203][3] (a
well-predicted, a two-valued {0, 0.1} and a constant target), sklearn's KFold(5, shuffle,
random_state=42) fold ids for n = 10, 23, 203, 1000, and the reference procedure (Ridge(1.0) per
fold, clf.score, guarded np.corrcoef, final fit) run with X as fp64 and with X as fp32, kappa =
(lambda_max(Sxx) + 1) / (lambda_min(Sxx) + 1) = 312.

The constant target: the closed form gives r2 = corr = 0.0 by its degenerate-target rule, as the
recorded fp32 run does.  The recorded fp64 run holds r2 = 1.0 there (ss_res = ss_tot = 0 exactly,
which sklearn's r2_score reports as 1.0), so that one entry is compared with the rule, not with the
fp64 record.
"""
import ctypes
import random
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import probe_restatement as R

ROOT = Path(__file__).resolve().parent.parent
VOCAB = ["<PAD>", "<BOS_CDS>", "<EOS_CDS>", "<SEP>"] + [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]


# ------------------------------------------------------------------ ABI
def test_symbols_are_declared_exported_and_bound():
    from codonlm_amd import _lib as L
    header = (ROOT / "include" / "codonlm_hip.h").read_text()
    for name in ("cg_shape_targets", "cg_gram_accum", "cg_gram_workspace"):
        assert re.search(rf"\b{name}\s*\(", header) and hasattr(L.lib, name) and name in L.SIGNATURES, name
    from codonlm_amd import ops
    assert int(re.search(r"#define CG_SHAPE_TARGETS (\d+)", header).group(1)) == ops.SHAPE_TARGETS == len(R.NAMES)


def test_argument_checks_need_no_device():
    """Every CG_EINVAL / CG_EUNSUPPORTED of the two contracts is decided before anything is launched."""
    from codonlm_amd import _lib as L
    tab = (ctypes.c_int32 * 68)(*([-1] * 4 + list(range(64))))
    P = 0x1000  # a non-NULL, 256-byte aligned stand-in: no call below reaches a launch

    def st(idx=P, B=2, T=8, tab=tab, V=68, y=P, ldy=14, valid=P):
        return L.lib.cg_shape_targets(idx, B, T, tab, V, y, ldy, valid, None)
    assert st(B=0) == L.CG_OK and st(T=0) == L.CG_OK
    for bad in (dict(idx=None), dict(y=None), dict(valid=None), dict(B=-1), dict(T=-1), dict(V=257), dict(V=-1),
                dict(ldy=13), dict(tab=None)):
        assert st(**bad) == L.CG_EINVAL, bad
    assert st(tab=(ctypes.c_int32 * 68)(*([64] * 68))) == L.CG_EINVAL

    def ga(dtype=L.CG_F32, h=P, ldh=32, d=32, y=P, ldy=14, m=14, grp=P, rows=100, G=5, acc=0, gram=P, ldg=47, ws=P,
           wsb=1 << 40):
        return L.lib.cg_gram_accum(dtype, h, ldh, d, y, ldy, m, grp, rows, G, acc, gram, ldg, ws, wsb, None)
    assert ga(rows=0, acc=1, gram=None) == L.CG_OK
    need = L.lib.cg_gram_workspace(100, 32, 14, 5)
    assert need > 0 and L.lib.cg_gram_workspace(10000, 32, 14, 5) > need
    for bad in (dict(h=None), dict(y=None), dict(grp=None), dict(gram=None), dict(ws=None), dict(ws=P + 8),
                dict(rows=-1), dict(rows=2 ** 30 + 1, wsb=1 << 60), dict(G=0), dict(d=-1), dict(m=-1), dict(ldh=31), dict(ldy=13),
                dict(ldg=46), dict(acc=2), dict(wsb=need - 1)):
        assert ga(**bad) == L.CG_EINVAL, bad
    assert ga(dtype=99) == L.CG_EUNSUPPORTED
    assert ga(G=4097) == L.CG_EUNSUPPORTED and ga(d=8192, ldh=8192, ldg=9000) == L.CG_EUNSUPPORTED
    for bad in ((-1, 32, 14, 5), (100, -1, 14, 5), (100, 32, 14, 0), (100, 32, 14, 4097), (100, 8192, 0, 1)):
        assert L.lib.cg_gram_workspace(*bad) == 0, bad


# ------------------------------------------------------------------ targets
def test_restated_targets_equal_the_reference_bitwise(golden):
    _, g = golden("shape_targets")
    assert list(g["names"]) == list(R.NAMES)
    dna = [str(s) for s in g["dna"]]
    assert dna[0] == "ATG" + "GGCC" * 5 + "AAAA" * 5 + "CGTA" * 5 + "TGA"
    assert {len(s) // 3 for s in dna} >= {1, 2, 60}
    stoi = {t: i for i, t in enumerate(VOCAB)}
    for i, s in enumerate(dna):
        want = g[f"y_{i}"]
        assert want.dtype == np.float32 and want.shape == (len(s) // 3, 14)
        assert np.array_equal(R.codon_targets(s).view(np.uint32), want.view(np.uint32)), s
        ids = np.array([[stoi[s[j:j + 3]] for j in range(0, len(s), 3)]])
        y, valid = R.shape_targets(ids, VOCAB)
        assert valid.all() and np.array_equal(y.view(np.uint32), want.view(np.uint32)), s


def test_codon_table_and_library_constants():
    from codonlm_amd import structure_probe as SP
    tab = SP.codon_table()
    assert tab[:4] == [-1] * 4 and tab[4:] == list(range(64)) and len(tab) == 68
    assert SP.codon_table(["<PAD>", "TGA", "NNN", "acg", "AT", "GATC"]) == [-1, 3 << 4 | 2 << 2, -1, -1, -1, -1]
    assert SP.NAMES == R.NAMES
    from codonlm_amd.training.loop import VOCAB as TRAINER_VOCAB
    assert SP.default_vocab() == list(TRAINER_VOCAB) == VOCAB
    assert SP.dna_ids(SP.AWARENESS_DNA) == [VOCAB.index(SP.AWARENESS_DNA[i:i + 3]) for i in range(0, 66, 3)]
    with pytest.raises(ValueError):
        SP.codon_table(["AAA"] * 257)


# ------------------------------------------------------------------ folds
@pytest.mark.parametrize("n", [10, 23, 203, 1000])
def test_kfold_assign_is_sklearns(golden, n):
    from codonlm_amd.structure_probe import kfold_assign
    _, g = golden("ridge_kfold")
    got = kfold_assign(n)
    assert got.dtype == np.int32 and np.array_equal(got, g[f"fold_{n}"])


# ------------------------------------------------------------------ ridge
def _host_gram(g):
    X, Y = g["X"], g["Y"]
    assert X.dtype == np.float32 and X.shape == (203, 12) and Y.dtype == np.float32 and Y.shape == (203, 3)
    gram, _, cnt = R.gram(X, Y, 3, g["fold_203"], 5)
    assert cnt.sum() == 203
    return gram


def test_ridge_cv_from_gram_reproduces_sklearn(golden):
    from codonlm_amd.structure_probe import ridge_cv_from_gram
    _, g = golden("ridge_kfold")
    kappa = float(g["kappa"])
    assert kappa <= 1e4 and abs(R.condition(g["X"]) - kappa) <= 1e-9 * kappa
    assert len(np.unique(g["Y"][:, 1])) == 2 and len(np.unique(g["Y"][:, 2])) == 1
    res = {k: v.numpy() for k, v in ridge_cv_from_gram(torch.from_numpy(_host_gram(g)), 12, 3, alpha=1.0).items()}
    assert float(res["n_rows"]) == 203.0
    # the constant target by the degenerate rule, in every fold; the recorded fp32 run agrees
    assert np.all(res["fold_r2"][:, 2] == 0.0) and np.all(res["fold_corr"][:, 2] == 0.0)
    assert res["r2"][2] == 0.0 and res["corr"][2] == 0.0
    assert np.all(g["fold_r2_f32"][:, 2] == 0.0) and np.all(g["fold_r2_f64"][:, 2] == 1.0)  # see the module docstring
    live = np.ones((5, 3), bool)
    live[:, 2] = False
    worst = 0.0
    for key in ("fold_r2", "fold_corr", "r2", "corr", "coef", "intercept"):
        want64, want32 = g[f"{key}_f64"], g[f"{key}_f32"]
        mask = live if key == "fold_r2" else live[0] if key == "r2" else np.ones(want64.shape, bool)
        err = np.abs(res[key] - want64)
        worst = max(worst, float(err[mask].max()))
        print(f"{key}: max |closed form - sklearn fp64| = {err[mask].max():.3e}, "
              f"sklearn fp32 - fp64 = {np.abs(want32 - want64)[mask].max():.3e}")
        assert err[mask].max() <= 1e-9, key
        # no further from the fp64 run than the fp32 run is: per quantity over the live entries, and
        # entrywise wherever the fp32 run itself is off by more than fp64 rounding noise (1e-12)
        gap = np.abs(want32 - want64)
        assert err[mask].max() <= gap[mask].max(), key
        assert (err <= gap)[gap > 1e-12].all(), key
    assert worst <= 1e-9


def test_ridge_cv_from_gram_equals_the_restatement(golden):
    from codonlm_amd.structure_probe import ridge_cv_from_gram
    _, g = golden("ridge_kfold")
    res = ridge_cv_from_gram(torch.from_numpy(_host_gram(g)), 12, 3, alpha=1.0)
    want = R.ridge_cv(g["X"], g["Y"], g["fold_203"], 5, alpha=1.0)
    for key, w in want.items():
        assert np.abs(res[key].numpy() - w).max() <= 1e-9, key
    with pytest.raises(ValueError):
        ridge_cv_from_gram(torch.zeros(5, 15, 15, dtype=torch.float64), 12, 3)
    with pytest.raises(ValueError):
        ridge_cv_from_gram(torch.zeros(5, 16, 16, dtype=torch.float32), 12, 3)


def test_cached_probe_metrics_and_awareness_from_gram(golden):
    """metrics_from_gram with G = 1 scores a given probe on all rows; awareness_from_gram is the |corr|
    with the first principal component's projection."""
    from codonlm_amd import structure_probe as SP
    _, g = golden("ridge_kfold")
    X, Y = g["X"].astype(np.float64), g["Y"].astype(np.float64)
    gram, _, _ = R.gram(g["X"], g["Y"], 3, np.zeros(203, np.int32), 1)
    coef, icpt = g["coef_f64"], g["intercept_f64"]
    r2, corr = SP.metrics_from_gram(torch.from_numpy(gram[0]), 12, 3, torch.from_numpy(coef), torch.from_numpy(icpt))
    for j in range(3):
        wr, wc = R.scores(X, Y[:, j], coef[j], icpt[j])
        assert abs(float(r2[j]) - wr) <= 1e-9 and abs(float(corr[j]) - wc) <= 1e-9
    Xc = X - X.mean(0)
    proj = Xc @ np.linalg.eigh(Xc.T @ Xc)[1][:, -1]
    got = SP.awareness_from_gram(torch.from_numpy(gram[0]), 12, 3).numpy()
    for j in range(2):
        assert abs(got[j] - abs(np.corrcoef(proj, Y[:, j])[0, 1])) <= 1e-9
    assert got[2] == 0.0


# ------------------------------------------------------------------ CLI
def test_cli_arguments_and_sequence_selection(tmp_path):
    from codonlm_amd import probe_structural_regression as C
    args = C.build_parser().parse_args(["--run_id", "r1"])
    assert (args.ckpt, args.sample_size, args.no_cache, args.layers, args.dtype) == ("best.pt", 150, False, "-1",
                                                                                      "fp32")
    C.check_args(args)
    assert C.parse_layers("-1") == [-1] and C.parse_layers("0, 2,3") == [0, 2, 3] and C.parse_layers("all") == "all"
    for bad in (["--sample_size", "-1", "--run_id", "r"], ["--batch_size", "0", "--run_id", "r"],
                ["--layers", "x", "--run_id", "r"], []):
        with pytest.raises(ValueError):
            C.check_args(C.build_parser().parse_args(bad))
    idxs = list(range(40))
    random.Random(42).shuffle(idxs)
    assert C.select_indices(40, 7) == idxs[:7] and C.select_indices(40, 150) == idxs
    assert C.select_indices(6, 0) == list(range(6))
    # fixed-window file: the selected rows in selection order, trimmed
    X = np.arange(40 * 12).reshape(40, 12)
    np.savez(tmp_path / "fixed.npz", X=X)
    got = C.load_sequences(tmp_path / "fixed.npz", 7, 10)
    assert got.dtype == np.int64 and np.array_equal(got, X[idxs[:7], :10])
    assert np.array_equal(C.load_sequences(tmp_path / "fixed.npz", 0, 64), X)
    # dynamic file: sequences back to back, right-padded with PAD
    lengths = np.array([3, 12, 5, 1])
    flat = np.arange(1, 22)
    np.savez(tmp_path / "dyn.npz", X=flat, lengths=lengths)
    got = C.load_sequences(tmp_path / "dyn.npz", 0, 8)
    assert got.shape == (4, 8)
    assert got[0].tolist() == [1, 2, 3, 0, 0, 0, 0, 0] and got[1].tolist() == list(range(4, 12))
    assert got[2].tolist() == [16, 17, 18, 19, 20, 0, 0, 0] and got[3].tolist() == [21] + [0] * 7
    order = list(range(4))
    random.Random(42).shuffle(order)
    two = C.load_sequences(tmp_path / "dyn.npz", 2, 8)  # as wide as the longest selected sequence, at most 8
    assert np.array_equal(two, got[order[:2], :min(8, int(lengths[order[:2]].max()))])
    with pytest.raises(FileNotFoundError):
        C.load_sequences(tmp_path / "nope.npz", 1, 8)
