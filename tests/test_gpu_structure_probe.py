"""codonlm_amd.structure_probe and the probe_structural_regression CLI on the GPU against the numpy
restatement (tests/probe_restatement.py) run on the hidden states read back from the engine.

Model: n_layer 2, n_head 2, n_embd 32, block_size 32, V 68, fp32 and bf16 compute.  Data: 9
sequences of T = 32 with BOS / EOS / SEP and PAD tails mixed in, one of them below 10 tokens;
batch_size 4, so the last batch is ragged.

Tolerances.  Gram entries: (n_g + 2) 2^-53 sum |z_i||z_j| (test_gpu_gram_op.py).  Metrics and
coefficients: the closed form on the Gram and the restatement on explicit matrices solve the same
system, conditioned by kappa = (lambda_max(Sxx) + 1) / (lambda_min(Sxx) + 1) of the centred hidden
states, from sums of n terms taken in different orders, so they may differ by C kappa n 2^-53
(absolute, for the metrics and for the coefficients and intercepts alike).  The test computes
kappa and n itself.  C = 8 x the largest ratio seen on the first run on the MI355X: n = 209,
kappa = 18.6, largest |difference| / (kappa n 2^-53) = 0.6771 with fp32 and 1.1503 with bf16 hidden
states, so C = 9.2.  A C above 64 would have meant that something other than the summation order
differs.
"""
import json

import numpy as np
import pytest
import torch

import probe_restatement as R
from oracle import tinygpt_oracle as O
from test_gpu_score import _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -53
VOCAB = ["<PAD>", "<BOS_CDS>", "<EOS_CDS>", "<SEP>"] + [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
CFG = O.OracleConfig(vocab_size=68, block_size=32, n_layer=2, n_head=2, n_embd=32, sep_id=3)
D, M, P = 32, 14, 47
OBSERVED_RATIO = 1.1503  # largest |difference| / (kappa n 2^-53) of the first MI355X run
C_TOL = 8 * OBSERVED_RATIO
assert C_TOL <= 64.0


@pytest.fixture(scope="module")
def params():
    return O.synthetic_params(CFG, seed=31)


def _sequences():
    rng = np.random.default_rng(23)
    x = rng.integers(4, 68, size=(9, 32)).astype(np.int64)
    x[:, 0] = 1
    for b, n in enumerate((32, 30, 21, 32, 9, 27, 32, 16, 32)):  # sequence 4: 9 tokens, below min_tokens
        x[b, n:] = 0
    x[1, 29] = 2     # EOS before the PAD tail
    x[3, 15] = 3     # SEP in the middle
    x[6, 10:12] = (2, 1)  # EOS BOS inside
    x[8, 31] = 2
    return x


def _explicit(m, x, which, batch_size=4, min_tokens=10):
    """(X fp64 [N][d] read back from eng.hidden per batch, Y fp32 [N][14], fold [N]) in (sequence,
    position) order over the codon positions of the long-enough sequences."""
    from codonlm_amd.structure_probe import kfold_assign
    y, valid = R.shape_targets(x, VOCAB)
    keep = valid.reshape(x.shape).astype(bool) & ((x != 0).sum(1) >= min_tokens)[:, None]
    hs = []
    for s in range(0, len(x), batch_size):
        for w, t in m.iter_hidden_states(torch.from_numpy(x[s:s + batch_size]).to(DEV)):
            if w == which:
                hs.append(t.to(torch.float64).cpu().numpy())
    h = np.concatenate(hs).reshape(-1, D)
    rows = np.nonzero(keep.reshape(-1))[0]
    return h[rows], y[rows], kfold_assign(len(rows))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_collect_gram_and_probe_match_the_restatement(params, dtype):
    from codonlm_amd import structure_probe as SP
    m = _model(CFG, params, dtype)
    x = _sequences()
    X, Y, fold = _explicit(m, x, 2)
    n = len(X)
    assert n == int(((x >= 4) & ((x != 0).sum(1) >= 10)[:, None]).sum()) and 150 < n < 9 * 32
    gram, n_rows = SP.collect_gram(m, x, layers=(-1,), batch_size=4)
    assert n_rows == n and gram.dtype == torch.float64 and tuple(gram.shape) == (1, 5, P, P) and gram.is_cuda
    ref, mag, cnt = R.gram(X, Y, M, fold, 5)
    got = gram[0].cpu().numpy()
    assert np.array_equal(got[:, P - 1, P - 1], cnt.astype(np.float64))
    assert (np.abs(got - ref) <= (cnt[:, None, None] + 2) * EPS * mag).all()
    assert np.array_equal(got, got.transpose(0, 2, 1))
    # ---- metrics and coefficients
    metrics, probes = SP.probe(m, x, layers=(-1,), batch_size=4)
    want = R.ridge_cv(X, Y, fold, 5, alpha=1.0)
    kappa = R.condition(X)
    unit = kappa * n * EPS
    ratio = 0.0
    for j, name in enumerate(R.NAMES):
        ratio = max(ratio, abs(metrics[f"regression_probe.{name}.r2"] - want["r2"][j]) / unit,
                    abs(metrics[f"regression_probe.{name}.corr"] - want["corr"][j]) / unit)
        ratio = max(ratio, np.abs(probes["coef"][0, j] - want["coef"][j]).max() / unit,
                    abs(probes["intercept"][0, j] - want["intercept"][j]) / unit)
    print(f"[structure_probe {dtype}] n={n} kappa={kappa:.1f} unit={unit:.3e} "
          f"largest |difference| / (kappa n 2^-53) = {ratio:.4f}")
    assert ratio <= C_TOL
    assert abs(metrics["regression_probe.avg_r2"] - want["r2"].mean()) <= C_TOL * unit
    assert abs(metrics["regression_probe.avg_corr"] - want["corr"].mean()) <= C_TOL * unit
    assert set(metrics) == {f"regression_probe.{nm}.{k}" for nm in R.NAMES for k in ("r2", "corr")} | {
        "regression_probe.avg_r2", "regression_probe.avg_corr"}
    assert list(probes["names"]) == list(R.NAMES) and probes["layers"].tolist() == [1]
    assert int(probes["n_rows"]) == n and float(probes["alpha"]) == 1.0
    # ---- the cached probes are scored on all rows, not refitted
    cm, cp = SP.probe(m, x, layers=(-1,), batch_size=4, cached=probes)
    assert np.array_equal(cp["coef"], probes["coef"]) and np.array_equal(cp["intercept"], probes["intercept"])
    for j, name in enumerate(R.NAMES):
        wr, wc = R.scores(X, Y[:, j].astype(np.float64), probes["coef"][0, j], probes["intercept"][0, j])
        assert abs(cm[f"regression_probe.{name}.r2"] - wr) <= C_TOL * unit
        assert abs(cm[f"regression_probe.{name}.corr"] - wc) <= C_TOL * unit
    with pytest.raises(ValueError):
        SP.probe(m, x, layers=(0,), cached=probes)


def test_layers_all_is_bitwise_one_run_per_layer_and_rows_filter(params):
    from codonlm_amd import structure_probe as SP
    m = _model(CFG, params, "fp32")
    x = _sequences()
    both, n = SP.collect_gram(m, x, layers="all", batch_size=4)
    assert tuple(both.shape) == (2, 5, P, P)
    for l in (0, 1):
        one, n1 = SP.collect_gram(m, x, layers=(l,), batch_size=4)
        assert n1 == n and torch.equal(one[0], both[l])
    assert torch.equal(SP.collect_gram(m, x, layers=(-1,), batch_size=4)[0][0], both[1])
    assert not torch.equal(both[0], both[1])
    # the 9-token sequence contributes no row: without it the Gram is bitwise the same when the
    # batches keep their composition (a row of PAD in its place), and with min_tokens = 0 it counts
    blank = x.copy()
    blank[4] = 0
    g2, n2 = SP.collect_gram(m, blank, layers="all", batch_size=4)
    assert n2 == n
    g3, n3 = SP.collect_gram(m, x, layers="all", batch_size=4, min_tokens=0)
    assert n3 == n + int((x[4] >= 4).sum())
    X, Y, fold = _explicit(m, blank, 2)
    ref, mag, cnt = R.gram(X, Y, M, fold, 5)
    assert (np.abs(g2[1].cpu().numpy() - ref) <= (cnt[:, None, None] + 2) * EPS * mag).all()
    # the first block's Gram against the restatement on its own hidden states
    X0, Y0, fold0 = _explicit(m, x, 1)
    ref0, mag0, cnt0 = R.gram(X0, Y0, M, fold0, 5)
    assert not np.array_equal(X0, _explicit(m, x, 2)[0])
    assert (np.abs(both[0].cpu().numpy() - ref0) <= (cnt0[:, None, None] + 2) * EPS * mag0).all()
    # metrics of several layers: every layer's keys under layer<l>, the plain keys the last block's --
    # and absent when the last block is not among the layers
    metrics, probes = SP.probe(m, x, layers="all", batch_size=4)
    assert probes["coef"].shape == (2, M, D) and probes["layers"].tolist() == [0, 1]
    assert metrics["regression_probe.MGW.r2"] == metrics["regression_probe.layer1.MGW.r2"]
    assert metrics["regression_probe.avg_corr"] == metrics["regression_probe.layer1.avg_corr"]
    assert metrics["regression_probe.MGW.r2"] != metrics["regression_probe.layer0.MGW.r2"] and len(metrics) == 3 * 30
    last = SP.probe(m, x, layers=(-1,), batch_size=4)[0]
    assert all(metrics[k] == v for k, v in last.items())
    first = SP.probe(m, x, layers=(0,), batch_size=4)[0]   # one layer: the plain keys are that layer's
    assert first["regression_probe.MGW.r2"] == metrics["regression_probe.layer0.MGW.r2"] and len(first) == 30
    cfg3 = O.OracleConfig(vocab_size=68, block_size=32, n_layer=3, n_head=2, n_embd=32, sep_id=3)
    m3 = _model(cfg3, O.synthetic_params(cfg3, seed=5), "fp32")
    part = SP.probe(m3, x, layers=(0, 1), batch_size=4)[0]
    assert len(part) == 2 * 30 and all(k.startswith("regression_probe.layer") for k in part)
    with pytest.raises(ValueError):
        SP.collect_gram(m, x, layers=(2,))
    with pytest.raises(ValueError):
        SP.probe(m, np.zeros((2, 32), np.int64))


def test_awareness_is_the_first_component_correlation(params):
    from codonlm_amd import structure_probe as SP
    m = _model(CFG, params, "fp32")
    ids = np.asarray([SP.dna_ids(SP.AWARENESS_DNA, VOCAB)], dtype=np.int64)
    assert ids.shape == (1, 22)
    got = SP.awareness(m)
    h = None
    for w, t in m.iter_hidden_states(torch.from_numpy(ids).to(DEV)):
        if w == 2:
            h = t.to(torch.float64).cpu().numpy().reshape(-1, D)
    y = R.codon_targets(SP.AWARENESS_DNA).astype(np.float64)
    hc = h - h.mean(0)
    proj = hc @ np.linalg.eigh(hc.T @ hc)[1][:, -1]
    for j, name in enumerate(R.NAMES):
        t = y[:, j]
        flat = ((t - t.mean()) ** 2).sum() <= 4 * len(t) * EPS * (t * t).sum()
        want = 0.0 if flat else abs(np.corrcoef(proj, t)[0, 1])
        assert abs(got[name] - want) <= 1e-9, name
    assert abs(got["avg"] - np.mean([got[nm] for nm in R.NAMES])) <= 1e-15 and 0.0 < got["avg"] <= 1.0


def test_probe_structural_regression_cli(params, tmp_path, capsys):
    from codonlm_amd import probe_structural_regression as C
    from codonlm_amd import structure_probe as SP
    from codonlm_amd.score_mutations import load_model
    rd = tmp_path / "runs" / "r1"
    (rd / "checkpoints").mkdir(parents=True)
    (rd / "itos.txt").write_text("\n".join(VOCAB) + "\n")
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd["head.weight"] = sd["tok_emb.weight"]
    run_cfg = {"vocab_size": 68, "block_size": 32, "n_layer": 2, "n_head": 2, "n_embd": 32, "dropout": 0.1,
               "sep_mask_enabled": True, "tie_embeddings": True}
    torch.save({"model": sd, "cfg": run_cfg}, rd / "checkpoints" / "best.pt")
    (rd / "scores").mkdir()
    (rd / "scores" / "metrics.json").write_text(json.dumps({"test.ppl": 12.5}))
    x = _sequences()
    np.savez(tmp_path / "test.npz", X=x.astype(np.int32))
    argv = ["--run_dir", str(rd), "--test_npz", str(tmp_path / "test.npz"), "--sample_size", "0", "--batch_size", "4"]
    got = C.main(argv)
    model, _ = load_model(None, rd, "fp32")
    want, probes = SP.probe(model, x, layers=(-1,), batch_size=4)
    assert got == want
    saved = json.loads((rd / "scores" / "metrics.json").read_text())
    assert saved["test.ppl"] == 12.5 and all(saved[k] == v for k, v in want.items())
    with np.load(rd / "checkpoints" / C.PROBE_FILE, allow_pickle=False) as z:
        assert set(z.files) == {"coef", "intercept", "names", "layers", "alpha", "n_rows"}
        assert np.array_equal(z["coef"], probes["coef"]) and z["layers"].tolist() == [1]
    assert not (rd / "checkpoints" / "structural_regression_probes.pt").exists()
    assert "Training Probe" in capsys.readouterr().out
    # second run: the saved probes are loaded and scored on all rows
    cached = C.main(argv)
    assert "Cached Probe" in capsys.readouterr().out
    assert cached == SP.probe(model, x, layers=(-1,), batch_size=4, cached=probes)[0]
    assert cached != want
    # --no_cache fits again; a sample in the reference's order; several layers
    assert C.main(argv + ["--no_cache"]) == want
    sel = C.select_indices(9, 5)
    five = C.main(argv[:4] + ["--sample_size", "5", "--batch_size", "4", "--no_cache", "--layers", "all"])
    assert five == SP.probe(model, x[sel], layers="all", batch_size=4)[0]
    assert "regression_probe.layer1.Roll.corr" in five
    # a dynamic file (lengths) gives the sequences without their PAD tails
    lengths = (x != 0).sum(1)
    np.savez(tmp_path / "dyn.npz", X=np.concatenate([x[b, :lengths[b]] for b in range(9)]), lengths=lengths)
    dyn = C.main(["--run_dir", str(rd), "--test_npz", str(tmp_path / "dyn.npz"), "--sample_size", "0",
                  "--batch_size", "4", "--no_cache"])
    assert dyn == want
