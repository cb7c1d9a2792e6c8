"""codonlm_amd.context and its three CLIs against the CPU oracle.

Bounds, as in test_gpu_score: the fp32 logit bound is 1e-4 * max|logits|, a log-probability moves by
at most twice that, so TOL = 2e-4 * max|oracle logits| per token and count * TOL for a sum over
count tokens.  log conf = zmax - lse moves by at most TOL too, so conf (<= 1) moves by at most TOL
and a token can change its calibration bin only when the oracle's conf lies within TOL of an edge,
its correctness only when the oracle's top-2 margin is within TOL; the Brier term
sum_c p_c^2 - 2 p_y + 1 moves by at most (2 sum_c p_c^2 + 2 p_y) TOL <= 4 TOL.
The n-gram side has no model in it: it must equal the fp64 restatement to 1e-12.
"""
import json

import numpy as np
import pytest
import torch

import context_restatement as CR
from oracle import tinygpt_oracle as O
from test_gpu_inference import VOCAB
from test_gpu_score import CONFIGS, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
WINDOWS = (1, 2, 8, None)
N_BINS, BATCH = 15, 4
V, T = 68, 64


def _split(seed, n):
    rng = np.random.default_rng(seed)
    tok = rng.integers(4, V, size=(n, T + 1))
    tok[rng.random((n, T + 1)) < 0.06] = 3
    tok[:, 0] = 1
    x, y = tok[:, :-1].copy(), tok[:, 1:].copy()
    for b in range(1, n, 2):
        tail = int(rng.integers(1, T // 2))
        y[b, T - tail:] = 0
        x[b, T - tail + 1:] = 0
    return x.astype(np.int32), y.astype(np.int32)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    root = tmp_path_factory.mktemp("context")
    xtr, ytr = _split(1, 48)
    xte, yte = _split(2, 10)
    np.savez(root / "train_bs64.npz", X=xtr, Y=ytr)
    np.savez(root / "test_bs64.npz", X=xte, Y=yte)
    np.savez(root / "val_bs64.npz", X=xte[:3], Y=yte[:3])
    flags = np.zeros(10, bool)
    flags[[2, 7]] = True
    return {"root": root, "train": (xtr.astype(np.int64), ytr.astype(np.int64)),
            "test": (xte.astype(np.int64), yte.astype(np.int64)), "flags": flags}


@pytest.fixture(scope="module")
def nets(data):
    """Per config: the model and the oracle's logits of the test split at every window (once)."""
    out = {}
    x = data["test"][0]
    for name, cfg in CONFIGS.items():
        params = O.synthetic_params(cfg, seed=2024)
        with torch.no_grad():
            z = {w: O.forward(cfg, params, x, attention_window=w)["logits"].float().numpy().reshape(-1, V)
                 for w in WINDOWS}
        out[name] = (cfg, params, _model(cfg, params), z)
    return out


def _loaders(data, bs=BATCH):
    from codonlm_amd.data_loading import DeviceBatchLoader, DeviceCodonDataset
    mk = lambda p, b: DeviceBatchLoader(DeviceCodonDataset(p, device=DEV), b, shuffle=False, drop_remainder=False)  # noqa: E731
    return mk(data["root"] / "train_bs64.npz", 16), mk(data["root"] / "test_bs64.npz", bs)


def _tol(z):
    return 2e-4 * float(np.abs(z).max())


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_window_nll_matches_oracle(nets, data, name):
    from codonlm_amd import context as X
    _, _, m, z = nets[name]
    x, y = data["test"]
    got = X.context_ablation(m, _loaders(data)[1], WINDOWS)
    assert list(got) == ["1", "2", "8", "full"]
    for w in WINDOWS:
        ref = CR.diag_rows(z[w], x, y, V, sep=3)
        total, count = ref["slices"][0]
        r = got["full" if w is None else str(w)]
        print(f"[{name} window={w}] nll {r['nll']:.6f} oracle {total / count:.6f} (tol {_tol(z[w]):.2e})")
        assert r["evaluated_tokens"] == count and r["attention_window_input_tokens"] == w
        assert abs(r["nll"] - total / count) <= _tol(z[w])
        assert r["perplexity"] == np.exp(r["nll"])
    # the windows matter: the oracle's own window-1 loss differs from its full-context loss
    assert abs(got["1"]["nll"] - got["full"]["nll"]) > 4 * _tol(z[None])


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_loss_decomposition_matches_oracle(nets, data, name):
    from codonlm_amd import context as X
    _, _, m, z = nets[name]
    x, y = data["test"]
    itos = list(VOCAB)
    ref = CR.diag_rows(z[None], x, y, V, sep=3, row_flag=data["flags"], tok_class=CR.token_classes(itos))
    tol = _tol(z[None])
    train, test = _loaders(data)
    tables = X.fit_ngrams(train, V, [3])
    got = X.loss_decomposition(m, test, itos, data["flags"], tables=tables, alpha=0.01)
    for i, slice_name in enumerate(CR.SLICES):
        total, count = ref["slices"][i]
        if count == 0:
            assert slice_name not in got["decomposition"]
            continue
        r = got["decomposition"][slice_name]
        assert r["tokens"] == count, slice_name
        assert abs(r["nll"] * count - total) <= count * tol, slice_name
    assert {"all", "after_separator", "window_with_chunk_continuation", "segment_position_16_63",
            "target_class_special", "target_class_start_codon", "target_class_stop_codon"} <= set(got["decomposition"])
    assert np.array_equal(got["row_tokens"], ref["row_count"])
    assert (np.abs(got["row_model"] - ref["row_nll"]) <= ref["row_count"] * tol).all()
    base = CR.ngram_nll(x, y, CR.count_tables(*data["train"], V, 0, (3,)), 0.01, V, 0, (3,))
    np.testing.assert_allclose(got["row_trigram"], base["row_sums"][:, 3], rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_calibration_matches_oracle(nets, data, name):
    """The synthetic parameters give peaked rows (conf ~ 1, the last bin), so the oracle alone keeps
    the fragile tokens under 2 %; the spread of confidences over all bins is test_gpu_diag_rows_op's."""
    from codonlm_amd import context as X
    _, _, m, z = nets[name]
    x, y = data["test"]
    edges = torch.linspace(0, 1, steps=N_BINS + 1).numpy()
    tol = _tol(z[None])
    ref = CR.diag_rows(z[None], x, y, V, sep=3, edges=edges)
    valid = ref["valid"].reshape(-1)
    conf = ref["conf64"][valid]
    srt = np.sort(z[None][valid].astype(np.float64), -1)
    near_edge = np.abs(conf[:, None] - edges[None, 1:-1].astype(np.float64)).min(1) <= tol
    near_tie = (srt[:, -1] - srt[:, -2]) <= tol
    fragile = int((near_edge | near_tie).sum())
    print(f"[{name}] tokens {valid.sum()} fragile {fragile} (edge {near_edge.sum()}, tie {near_tie.sum()}) tol {tol:.2e}")
    assert fragile <= 0.02 * valid.sum()
    got = X.calibration(m, _loaders(data)[1], n_bins=N_BINS)
    assert got["evaluated_tokens"] == valid.sum() and got["n_bins"] == N_BINS
    # the reference's rule on the oracle: per batch of BATCH windows, weighted by its token count
    ece_b, tok_b = [], []
    for a in range(0, len(x), BATCH):
        rb = CR.diag_rows(z[None][a * T:(a + BATCH) * T], x[a:a + BATCH], y[a:a + BATCH], V, sep=3, edges=edges)
        ece_b.append(CR.ece_from_calib(rb["calib"]))
        tok_b.append(rb["brier_acc"][1])
    ece_ref = float(np.dot(ece_b, tok_b) / np.sum(tok_b))
    # a bin's |mean conf - accuracy| term moves by TOL through conf and by its share of the fragile tokens
    slack = tol + 2.0 * fragile / valid.sum()
    assert abs(got["ece_val"] - ece_ref) <= slack
    assert abs(got["ece_global"] - CR.ece_from_calib(ref["calib"])) <= slack
    assert abs(got["brier_val"] - ref["brier_acc"][0] / ref["brier_acc"][1]) <= 4 * tol
    # token by token, through the op on the engine's logits: a token may leave the oracle's bin only
    # when it is near an edge, its hit may change only when it is near a tie
    from codonlm_amd import ops
    calib = torch.zeros(N_BINS, 3, dtype=torch.float64, device=DEV)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    logits, _ = m.engine.forward(xd, None, training=False)
    res = ops.diag_rows(logits.view(-1, V), xd, yd, V=V, sep_id=3, edges=torch.from_numpy(edges).to(DEV), calib=calib,
                        want=("conf",))
    conf_e = res.conf.cpu().numpy().reshape(-1)[valid]
    assert float(np.abs(conf_e - conf).max()) <= tol
    bin_e = np.full(conf_e.shape, -1)
    for i in range(N_BINS - 1, -1, -1):
        bin_e[(conf_e > edges[i]) & (conf_e <= edges[i + 1])] = i
    bin_o = ref["bin"].reshape(-1)[valid]
    assert not ((bin_e != bin_o) & ~near_edge).any()
    yv = y.reshape(-1)[valid]
    hit_e = logits.view(-1, V).argmax(-1).cpu().numpy()[valid] == yv
    hit_o = ref["correct"].reshape(-1)[valid]
    assert not ((hit_e != hit_o) & ~near_tie).any()
    # the accumulated bins are those tokens': counts, confidence sums and hits
    c = calib.cpu().numpy()
    assert np.array_equal(c[:, 0], np.bincount(bin_e[bin_e >= 0], minlength=N_BINS))
    assert np.array_equal(c[:, 2], np.bincount(bin_e[bin_e >= 0], weights=hit_e[bin_e >= 0], minlength=N_BINS))
    np.testing.assert_allclose(c[:, 1], np.bincount(bin_e[bin_e >= 0], weights=conf_e[bin_e >= 0].astype(np.float64),
                                                    minlength=N_BINS), rtol=1e-12, atol=0)


def _run_dir(data, cfg, params):
    """A run directory, vocabulary, packing metadata and a frozen manifest around the splits."""
    from codonlm_amd import provenance as P
    root = data["root"]
    rd = root / "runs" / "r1"
    (rd / "checkpoints").mkdir(parents=True, exist_ok=True)
    (rd / "itos.txt").write_text("\n".join(VOCAB) + "\n")
    (root / "itos.txt").write_text("\n".join(VOCAB) + "\n")
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd["head.weight"] = sd["tok_emb.weight"]
    run_cfg = {"vocab_size": V, "block_size": T, "n_layer": cfg.n_layer, "n_head": cfg.n_head, "n_embd": cfg.n_embd,
               "dropout": 0.1, "sep_mask_enabled": True, "tie_embeddings": True}
    torch.save({"model": sd, "cfg": run_cfg}, rd / "checkpoints" / "best.pt")
    rows = ["window_index\tcontinues_from_previous\tcontinues_to_next"]
    rows += [f"{i}\t{int(i == 2)}\t{int(i == 7)}" for i in range(10)]
    (root / "test_packing.tsv").write_text("\n".join(rows) + "\n")
    files = {"vocabulary": root / "itos.txt"}
    for split in P.SPLITS:
        files[f"{split}_tokens"] = root / f"{split}_bs64.npz"
    for aux in ("source_metadata", "source_dna", "fragment_metadata", "leakage_audit", "train_packing_metadata",
                "val_packing_metadata", "test_packing_metadata"):
        (root / f"{aux}.json").write_text(json.dumps({"name": aux}))
        files[aux] = root / f"{aux}.json"
    arts = {n: {"path": p.name, "role": n, "bytes": p.stat().st_size, "sha256": P.file_sha256(p)}
            for n, p in files.items()}
    manifest = {
        "schema": {"name": P.SCHEMA_NAME, "version": P.SCHEMA_VERSION},
        "dataset": {"source_record_count": 10, "scientific_valid": True},
        "split_policy": {"record_counts": {"train": 6, "val": 2, "test": 2},
                         "requested_fractions": {"val": 0.2, "test": 0.2}, "scientific_valid": True,
                         "effective_group_by": "genome"},
        "leakage_audit": {"status": "passed"},
        "vocabulary": {"size": V, "sha256": P.file_sha256(files["vocabulary"]),
                       "special_tokens": {t: i for i, t in enumerate(VOCAB[:4])}},
        "sources": {}, "tokenization": {"ambiguous_codon_policy": "drop"},
        "packing": {"mode": "fixed", "transition_policy": "exactly_once"},
        "reproducibility": {"split_seed": 1, "packing_seed": 2},
        "artifacts": arts,
    }
    manifest["dataset"]["id"] = P.dataset_identity(manifest)
    (root / "manifest.json").write_text(json.dumps(manifest))
    return rd


def test_diagnose_and_the_three_clis(nets, data, tmp_path):
    from codonlm_amd import calibration_metrics as M
    from codonlm_amd import diagnose_context_learning as D
    from codonlm_amd import eval_ppl_baselines as E
    cfg, params, _, z = nets["mha_gelu"]
    rd = _run_dir(data, cfg, params)
    root = data["root"]
    x, y = data["test"]
    prefix = tmp_path / "out" / "context"
    report = D.main(["--run-dir", str(rd), "--train", str(root / "train_bs64.npz"), "--test", str(root / "test_bs64.npz"),
                     "--manifest", str(root / "manifest.json"), "--packing-tsv", str(root / "test_packing.tsv"),
                     "--context-windows", "1,8,full", "--bootstrap-samples", "50", "--mask-audit-windows", "4",
                     "--output-prefix", str(prefix)])
    assert json.loads(prefix.with_suffix(".json").read_text()) == json.loads(json.dumps(report))
    assert sorted(report) == sorted(["schema_version", "status", "evaluation_split", "checkpoint", "checkpoint_dataset",
                                     "dataset_manifest", "vocabulary", "packing", "attention_mask_audit", "markov",
                                     "context_ablation", "loss_decomposition", "paired_codonlm_vs_trigram"])
    assert report["status"] == "diagnostic_complete" and report["vocabulary"]["size"] == V
    assert report["dataset_manifest"]["status"] == "frozen_manifest_verified"
    assert report["packing"] == {"metadata": report["packing"]["metadata"], "windows_with_chunk_continuation": 2,
                                 "total_windows": 10}
    audit = report["attention_mask_audit"]
    assert audit["status"] == "passed" and audit["sampled_windows"] == 4
    assert audit["checked_nonpad_queries"] == int((x[:4] != 0).sum())
    assert audit["separator_reset_queries"] == int((x[:4, 1:] == 3).sum())
    tol = _tol(z[None])
    ref = CR.diag_rows(z[None], x, y, V, sep=3)
    assert list(report["context_ablation"]) == ["1", "8", "full"]
    assert abs(report["context_ablation"]["full"]["nll"] - ref["slices"][0, 0] / ref["slices"][0, 1]) <= tol
    tables = CR.count_tables(*data["train"], V, 0, (3,))
    base = CR.ngram_nll(x, y, tables, 0.01, V, 0, (3,))
    assert report["markov"]["evaluated_tokens"] == base["acc"][4]
    for i, model_name in enumerate(("Uniform", "Unigram", "Bigram", "Trigram")):
        np.testing.assert_allclose(report["markov"]["results"][model_name]["cross_entropy_nats"],
                                   base["acc"][i] / base["acc"][4], rtol=1e-12)
    paired = report["paired_codonlm_vs_trigram"]
    want = (ref["row_nll"].sum() - base["row_sums"][:, 3].sum()) / ref["row_count"].sum()
    assert abs(paired["codonlm_minus_trigram_nats_per_token"] - want) <= tol
    assert paired["ci95"][0] <= paired["codonlm_minus_trigram_nats_per_token"] <= paired["ci95"][1]
    md = prefix.with_suffix(".md").read_text()
    assert md.startswith("# Context Learning Diagnostic\n") and "## Paired Gate" in md and "| all | " in md
    with pytest.raises(ValueError, match="full"):
        D.main(["--run-dir", str(rd), "--train", "a", "--test", "b", "--manifest", "m", "--context-windows", "1",
                "--output-prefix", str(prefix)])

    rep = E.main(["--train", str(root / "train_bs64.npz"), "--test", str(root / "test_bs64.npz"), "--run-dir", str(rd),
                  "--manifest", str(root / "manifest.json"), "--output-prefix", str(tmp_path / "base")])
    assert rep["results"] == report["markov"]["results"] and rep["evaluated_tokens"] == base["acc"][4]
    assert rep["context_boundary"] == {"method": "reset_history_after_tokens", "token_ids": [3], "tokens": ["<SEP>"]}
    assert json.loads((tmp_path / "base.json").read_text())["best_simple_baseline"] == rep["best_simple_baseline"]
    assert (tmp_path / "base.md").read_text().startswith("| Model | Cross-entropy (nats) |")

    out = tmp_path / "scores" / "metrics.json"
    out.parent.mkdir()
    out.write_text(json.dumps({"train_loss": 1.25}))
    got = M.main(["--ckpt", str(rd / "checkpoints" / "best.pt"), "--npz", str(root / "test_bs64.npz"), "--out", str(out),
                  "--batch-size", str(BATCH)])
    merged = json.loads(out.read_text())
    assert merged["train_loss"] == 1.25 and merged["ece_val"] == got["ece_val"] and "brier_val" in merged
    edges = torch.linspace(0, 1, steps=N_BINS + 1).numpy()
    full = CR.diag_rows(z[None], x, y, V, sep=3, edges=edges)
    assert abs(got["brier_val"] - full["brier_acc"][0] / full["brier_acc"][1]) <= 4 * tol
