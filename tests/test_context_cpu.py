"""The fp64 restatement of the context-diagnostic kernels (tests/context_restatement.py) against
what the reference's own functions returned for the same inputs (tests/golden/context_diag.npz,
made by tests/golden/make_golden_context.py), and the host side of the three CLIs.

Integers agree exactly; the bootstrap quantiles agree exactly (same rng, same draw order, same
arithmetic); fp64 values agree to 1e-12 relative: a sum here has at most 4096 terms, each a few
fp64 ulps off, and an ordered sum adds at most n * 2^-53 relative.  ece_from_logits keeps its
per-bin accuracy in fp32; the test rounds the accuracy the same way and then holds the ECE to 1e-12 too.
"""
import ctypes
import json

import numpy as np
import pytest

import context_restatement as CR

RTOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    z = np.load(CR.__file__.replace("context_restatement.py", "golden/context_diag.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _split(gold, T):
    k = f"T{T}_"
    got = CR.make_split(T)
    for name, arr in zip(("xtr", "ytr", "xte", "yte", "flags"), got):
        assert np.array_equal(gold[k + name].astype(np.int64), arr.astype(np.int64)), (T, name)
    return got


@pytest.fixture(scope="module")
def restated(gold):
    """Per T: the split, the tables, the baseline and the diagnostic restatement (computed once)."""
    out = {}
    alpha, n_bins = float(gold["alpha"]), int(gold["n_bins"])
    import torch
    edges = torch.linspace(0, 1, steps=n_bins + 1).numpy()  # the caller's edges: the reference's own bits
    for T in CR.TS:
        xtr, ytr, xte, yte, flags = _split(gold, T)
        tables = CR.count_tables(xtr, ytr)
        z32 = gold[f"T{T}_logits"].astype(np.float32)
        out[T] = {"split": (xtr, ytr, xte, yte, flags), "tables": tables,
                  "nll": CR.ngram_nll(xte, yte, tables, alpha),
                  "diag": CR.diag_rows(z32, xte, yte, CR.V, row_flag=flags, tok_class=CR.token_classes(CR.ITOS),
                                       edges=edges)}
    return out


def test_fixture_is_small():
    from pathlib import Path
    assert Path(CR.__file__).with_name("golden").joinpath("context_diag.npz").stat().st_size < 200 * 1024


@pytest.mark.parametrize("T", CR.TS)
def test_counts_match_fit_baselines(gold, restated, T):
    uni, bi, tri, bad = restated[T]["tables"]
    k = f"T{T}_"
    assert bad == 0
    assert np.array_equal(uni, gold[k + "uni"])
    assert np.array_equal(bi, gold[k + "bi"])
    assert np.array_equal(tri, gold[k + "tri"])
    # the dense form's "context exists" is the reference's dict membership
    _, tb, tt = CR.totals(uni, bi, tri)
    assert np.array_equal(tb > 0, gold[k + "bi_seen"])
    assert np.array_equal(tt > 0, gold[k + "tri_seen"])


@pytest.mark.parametrize("T", CR.TS)
def test_baseline_nll_matches_evaluate_baselines(gold, restated, T):
    r = restated[T]["nll"]
    k = f"T{T}_"
    assert int(r["acc"][4]) == int(gold[k + "tokens"])
    np.testing.assert_allclose(r["acc"][:4] / r["acc"][4], gold[k + "baseline_nll"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(r["tok"][3], gold[k + "tri_tok"], rtol=RTOL, atol=0)
    names = ("Uniform", "Unigram", "Bigram", "Trigram")
    best = min(names[1:], key=lambda n: r["acc"][names.index(n)])
    assert best == str(gold[k + "best"])


@pytest.mark.parametrize("T", CR.TS)
def test_slices_and_calibration_match_the_reference(gold, restated, T):
    d = restated[T]["diag"]
    k = f"T{T}_"
    np.testing.assert_allclose(d["nll"], gold[k + "losses"], rtol=RTOL, atol=0)
    assert np.array_equal(d["slices"][:, 1], gold[k + "slices"][:, 1])
    np.testing.assert_allclose(d["slices"][:, 0], gold[k + "slices"][:, 0], rtol=RTOL, atol=0)
    # bin membership is no rounding question on these inputs ...
    assert d["edge_ulps"] > 4
    # ... so the fp64 confidence sums give the reference's ECE, once the per-bin accuracy is rounded
    # as ece_from_logits rounds it: it keeps `correct` in fp32 whatever the default dtype, so a bin's
    # accuracy is an exact integer sum and one fp32 division.  The contract's sums of the
    # fp32-rounded confidence differ from the fp64 ones by that rounding alone (2^-24 relative per term).
    c64 = d["calib64"][d["calib64"][:, 0] > 0]
    acc32 = (c64[:, 2].astype(np.float32) / c64[:, 0].astype(np.float32)).astype(np.float64)
    ece = float((c64[:, 0] / c64[:, 0].sum() * np.abs(c64[:, 1] / c64[:, 0] - acc32)).sum())
    np.testing.assert_allclose(ece, float(gold[k + "ece"]), rtol=RTOL, atol=0)
    assert abs(CR.ece_from_calib(d["calib64"]) - ece) <= 2.0 ** -24
    assert np.array_equal(d["calib"][:, [0, 2]], d["calib64"][:, [0, 2]])
    assert (np.abs(d["calib"][:, 1] - d["calib64"][:, 1]) <= d["calib"][:, 0] * 2.0 ** -24).all()
    np.testing.assert_allclose(d["brier_acc"][0] / d["brier_acc"][1], float(gold[k + "brier"]), rtol=RTOL, atol=0)


@pytest.mark.parametrize("T", CR.TS)
def test_bootstrap_matches_exactly(gold, restated, T):
    from codonlm_amd import context as X
    d, r = restated[T]["diag"], restated[T]["nll"]
    seed, samples = (int(v) for v in gold["boot"])
    # the reference summed rows of its own arrays; feed the restatement the same row values
    valid = d["valid"]
    row_model = (gold[f"T{T}_losses"] * valid).sum(1)
    row_tri = (gold[f"T{T}_tri_tok"] * valid).sum(1)
    obs, lo, hi = CR.paired_bootstrap(row_model, row_tri, d["row_count"], seed, samples)
    assert np.array_equal(np.array([obs, lo, hi]), gold[f"T{T}_boot"])
    lib = X.paired_bootstrap(row_model, row_tri, d["row_count"], seed, samples)
    assert [lib["codonlm_minus_trigram_nats_per_token"], *lib["ci95"]] == list(gold[f"T{T}_boot"])
    assert lib["bootstrap_unit"] == "packed_window" and lib["bootstrap_samples"] == samples and lib["seed"] == seed
    np.testing.assert_allclose(d["row_nll"], row_model, rtol=RTOL, atol=0)
    np.testing.assert_allclose(r["row_sums"][:, 3], row_tri, rtol=RTOL, atol=0)


def test_inputs_reach_every_branch(restated):
    """Assertions on the restatement's own bookkeeping: the inputs exercise what the kernels branch on."""
    slice_counts = np.zeros(len(CR.SLICES))
    flags_seen = set()
    for T in CR.TS:
        r, d = restated[T]["nll"], restated[T]["diag"]
        if T >= 63:
            assert r["unseen"].sum() >= 1 and r["backoff"].sum() >= 1, T
        slice_counts += d["slices"][:, 1]
        flags_seen |= set(int(f) for f in restated[T]["split"][4])
        x, y = restated[T]["split"][2:4]
        if T >= 8:
            assert ((x == CR.SEP) & (y == CR.PAD))[:, 1:-1].any()          # PAD target under a SEP input
            assert x[0, 0] == CR.SEP and x[0, -1] == CR.SEP and y[0, -1] != CR.PAD
            assert ((x[:, 1:] == CR.SEP) & (x[:, :-1] == CR.SEP)).any()    # adjacent SEPs
    assert restated[130]["diag"]["slices"][8, 1] >= 60
    assert (slice_counts > 0).all(), dict(zip(CR.SLICES, slice_counts))
    assert flags_seen == {0, 1}
    assert restated[1]["nll"]["unseen"].sum() >= 1


# ------------------------------------------------------------------ ABI and the CLIs' host side
def test_struct_mirrors_and_workspace_queries():
    from codonlm_amd import _lib as L
    assert L.lib.cg_struct_bytes(b"cg_ngram_nll_desc") == ctypes.sizeof(L.NgramNllDesc)
    assert L.lib.cg_struct_bytes(b"cg_diag_desc") == ctypes.sizeof(L.DiagDesc)
    assert L.lib.cg_diag_workspace(1) >= 8 * (2 * 13 + 3 * 32 + 2)
    assert L.lib.cg_diag_workspace(10 ** 6) == L.lib.cg_diag_workspace(10 ** 7)  # the grid is capped
    assert L.lib.cg_ngram_nll_workspace(1) >= 40
    assert len(L.DIAG_SLICES) == 13 and L.DIAG_SLICES == CR.SLICES
    # refused before any launch, without a device
    d = L.NgramNllDesc(B=1, T=1, V=129, alpha=0.01)
    assert L.lib.cg_ngram_nll(ctypes.byref(d), None) == L.CG_EUNSUPPORTED
    d = L.NgramNllDesc(B=1, T=1, V=20, alpha=0.0)
    assert L.lib.cg_ngram_nll(ctypes.byref(d), None) == L.CG_EINVAL
    assert L.lib.cg_diag_rows(ctypes.byref(L.DiagDesc(B=0, T=5, V=20)), None) == L.CG_OK
    assert L.lib.cg_diag_rows(ctypes.byref(L.DiagDesc(B=1, T=5, V=129)), None) == L.CG_EUNSUPPORTED


def test_token_classes_and_windows():
    from codonlm_amd import context as X
    assert np.array_equal(X.token_classes(CR.ITOS), CR.token_classes(CR.ITOS))
    assert X.parse_windows("1, 2,FULL,2") == [1, 2, None]
    with pytest.raises(ValueError):
        X.parse_windows("0,full")
    block = X.vocabulary_block(CR.ITOS)
    assert block["size"] == CR.V and len(block["sha256"]) == 64


def _report():
    from codonlm_amd import context as X
    results, best = X.baseline_results([3.0 * 10, 2.5 * 10, 2.0 * 10, 2.25 * 10], 10)
    assert best == "Bigram" and results["Trigram"]["cross_entropy_improvement_over_best_simple"] == -0.25
    return {
        "context_ablation": {"1": {"nll": 2.5, "perplexity": 12.182, "evaluated_tokens": 10},
                             "full": {"nll": 2.0, "perplexity": 7.389, "evaluated_tokens": 10}},
        "markov": {"results": results},
        "paired_codonlm_vs_trigram": {"codonlm_minus_trigram_nats_per_token": -0.25, "ci95": [-0.5, -0.125]},
        "loss_decomposition": {"all": {"nll": 2.0, "perplexity": 7.389, "tokens": 10}},
    }, results


def test_diagnose_cli_arguments_and_markdown(tmp_path):
    from codonlm_amd import diagnose_context_learning as D
    base = ["--run-dir", "r", "--train", "a.npz", "--test", "b.npz", "--manifest", "m.json", "--output-prefix",
            str(tmp_path / "o" / "ctx")]
    args = D.build_parser().parse_args(base)
    assert (args.context_windows, args.batch_size, args.alpha, args.bootstrap_samples, args.mask_audit_windows,
            args.seed, args.checkpoint_name, args.split) == ("1,2,4,8,32,128,full", 4, 0.01, 2000, 32, 1337,
                                                               "best.pt", "test")
    assert D.check_args(args) == [1, 2, 4, 8, 32, 128, None]
    with pytest.raises(ValueError, match="full"):
        D.check_args(D.build_parser().parse_args(base + ["--context-windows", "1,2"]))
    with pytest.raises(SystemExit):
        D.build_parser().parse_args(base + ["--device", "cpu"])      # no CPU path
    with pytest.raises(SystemExit):
        D.build_parser().parse_args(base[2:])                         # --run-dir is required
    report, _ = _report()
    text = D.write_report(report, args.output_prefix)
    lines = text.splitlines()
    assert lines[0] == "# Context Learning Diagnostic" and lines[4] == "| Input attention window | NLL | PPL |"
    assert "| 1 | 2.500000 | 12.182 |" in lines and "| full | 2.000000 | 7.389 |" in lines
    assert "| Bigram | 2.000000 | 7.389 |" in lines
    assert ("CodonLM minus trigram: `-0.250000` nats/token (95% packed-window bootstrap CI "
            "`[-0.500000, -0.125000]`).") in lines
    assert lines[-1] == "| all | 10 | 2.000000 | 7.389 |"
    assert json.loads(args.output_prefix.with_suffix(".json").read_text()) == report
    assert args.output_prefix.with_suffix(".md").read_text() == text
    tsv = tmp_path / "pack.tsv"
    tsv.write_text("window_index\tcontinues_from_previous\tcontinues_to_next\n0\t0\t0\n2\t1\t0\n3\t0\t1\n")
    assert D.packing_window_flags(tsv, 4).tolist() == [False, False, True, True]
    with pytest.raises(ValueError, match="out of range"):
        D.packing_window_flags(tsv, 3)


def test_baselines_cli_arguments_and_markdown(tmp_path):
    from codonlm_amd import eval_ppl_baselines as E
    args = E.build_parser().parse_args(["--train_npz", "a.npz", "--test", "b.npz", "--itos", "itos.txt"])
    assert (args.train, args.test, args.alpha, args.split) == ("a.npz", "b.npz", 0.01, "test")
    assert str(E.check_args(args)) == "itos.txt"
    with pytest.raises(ValueError, match="itos"):
        E.check_args(E.build_parser().parse_args(["--train", "a", "--test", "b"]))
    with pytest.raises(ValueError, match="alpha"):
        E.check_args(E.build_parser().parse_args(["--train", "a", "--test", "b", "--itos", "i", "--alpha", "0"]))
    _, results = _report()
    text = E.write_report({"results": results}, tmp_path / "base")
    lines = text.splitlines()
    assert lines[0].startswith("| Model | Cross-entropy (nats) | Perplexity | Bits/codon |") and lines[1] == "|---|---:|---:|---:|---:|"
    assert [ln.split(" | ")[0] for ln in lines[2:]] == ["| Uniform", "| Unigram", "| Bigram", "| Trigram"]
    assert lines[4] == f"| Bigram | 2.000000 | {np.exp(2.0):.6f} | {2.0 / np.log(2):.6f} | 0.000000 |"
    assert (tmp_path / "base.json").exists() and (tmp_path / "base.md").read_text() == text


def test_calibration_cli_arguments():
    from codonlm_amd import calibration_metrics as M
    args = M.build_parser().parse_args(["--ckpt", "c.pt", "--npz", "v.npz", "--out", "m.json"])
    assert (args.batch_size, args.n_bins) == (32, 15)
    M.check_args(args)
    with pytest.raises(ValueError):
        M.check_args(M.build_parser().parse_args(["--ckpt", "c", "--npz", "v", "--out", "m", "--n-bins", "33"]))
    with pytest.raises(SystemExit):
        M.build_parser().parse_args(["--ckpt", "c", "--npz", "v", "--out", "m", "--device", "cpu"])
