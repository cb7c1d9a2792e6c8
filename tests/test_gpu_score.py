"""codonlm_amd.score and its two CLIs against the CPU oracle.

Bounds.  The project's fp32 logit bound is 1e-4 * max|logits| (test_gpu_model, smoke); a
log-probability z_y - lse moves by at most twice the logit error, so every per-token quantity is
held to TOL = 2 * 1e-4 * max|oracle logits|, a sum over n tokens to n * TOL, a difference of two
such sums to their two bounds added.  bf16 adds no tolerance of its own: the library's values are
compared with the fp64 restatement of test_gpu_score_op applied to the engine's own logits, at
that test's 1-ulp bound.
"""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tinygpt_oracle as O
from test_gpu_inference import VOCAB
from test_gpu_score_op import restate, within_ulp

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model(cfg, params, dtype="fp32"):
    from codonlm_amd import TinyGPT
    m = TinyGPT(cfg.vocab_size, cfg.block_size, n_layer=cfg.n_layer, n_head=cfg.n_head, n_embd=cfg.n_embd,
                dropout=0.0, label_smoothing=cfg.label_smoothing, sep_id=cfg.sep_id, n_kv_head=cfg.n_kv_head,
                termination_aux=cfg.termination_aux, multi_offset_targets=cfg.multi_offset_targets or None,
                use_swiglu=cfg.use_swiglu, use_rope=cfg.use_rope, compute_dtype=dtype, device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    return m.eval()


CONFIGS = {
    # the run of test_gpu_inference: V 68, block 64, 2 layers, d 128, SEP mask
    "mha_gelu": O.OracleConfig(vocab_size=68, block_size=64, n_layer=2, n_head=2, n_embd=128, sep_id=3),
    # the smoke() geometry: GQA + RoPE + SwiGLU
    "gqa_rope_swiglu": O.OracleConfig(vocab_size=68, block_size=64, n_layer=2, n_head=4, n_embd=64, n_kv_head=2,
                                      use_rope=True, use_swiglu=True),
}


@pytest.fixture(scope="module")
def nets():
    out = {}
    for name, cfg in CONFIGS.items():
        params = O.synthetic_params(cfg, seed=2024)
        out[name] = (cfg, params, _model(cfg, params))
    return out


def _oracle_logp(cfg, params, ids):
    """(log_softmax rows fp64 [len - 1][V], max|logits|) of one forward of ids[:-1]."""
    with torch.no_grad():
        z = O.forward(cfg, params, np.array([ids[:-1]]))["logits"][0].double()
    return torch.log_softmax(z, -1).numpy(), float(z.abs().max())


def _sequences():
    rng = np.random.default_rng(11)
    seqs = []
    for n in (2, 3, 9, 20, 33, 50, 64):
        seqs.append([1] + rng.integers(4, 68, size=n - 2).tolist() + [2])
    seqs[4][15] = 3  # one sequence holds a SEP: the segment mask is in play
    return seqs


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_score_batch_matches_oracle(nets, name):
    from codonlm_amd import score as S
    cfg, params, m = nets[name]
    seqs = _sequences()
    by_bs = {bs: S.score_batch(m, seqs, batch_size=bs) for bs in (3, 1)}
    for i, ids in enumerate(seqs):
        lp, scale = _oracle_logp(cfg, params, ids)
        tol = 2 * 1e-4 * scale
        n = len(ids) - 1
        ref = lp[np.arange(n), ids[1:]]
        for bs in (3, 1):
            r = by_bs[bs][i]
            assert r["logp"].shape == (n,) and r["n_tokens"] == n
            err = float(np.abs(r["logp"] - ref).max())
            print(f"[{name} bs={bs} len={len(ids)}] max|dlogp| {err:.2e} (tol {tol:.2e})")
            assert err <= tol
            assert abs(r["logp_sum"] - ref.sum()) <= tol * n
            assert abs(r["nll"] + r["logp_sum"] / n) < 1e-12 and r["ppl"] == math.exp(min(20.0, r["nll"]))
            # top-1 hits may differ from the oracle's only where its top-2 margin is within the bound
            srt = np.sort(lp, -1)
            close = int(((srt[:, -1] - srt[:, -2]) <= 2 * tol).sum())
            hits = int((lp.argmax(-1) == np.array(ids[1:])).sum())
            assert abs(r["top1_acc"] * n - hits) <= close
        assert abs(by_bs[3][i]["logp_sum"] - by_bs[1][i]["logp_sum"]) <= tol * n
        assert float(np.abs(by_bs[3][i]["logp"] - by_bs[1][i]["logp"]).max()) <= tol
    # a full block fits; one token more does not
    rng = np.random.default_rng(5)
    full = [1] + rng.integers(4, 68, size=63).tolist() + [2]
    lp, scale = _oracle_logp(cfg, params, full)
    r = S.score_batch(m, [full])[0]
    assert float(np.abs(r["logp"] - lp[np.arange(64), full[1:]]).max()) <= 2e-4 * scale
    with pytest.raises(ValueError, match="block_size"):
        S.score_batch(m, [full + [2]])
    assert S.score_batch(m, []) == []


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_bf16_scores_are_the_restatement_of_the_engine_logits(nets, name):
    from codonlm_amd import score as S
    cfg, params, _ = nets[name]
    m = _model(cfg, params, "bf16")
    rng = np.random.default_rng(3)
    seqs = [[1] + rng.integers(4, 68, size=38).tolist() + [2] for _ in range(3)]  # equal lengths: one batch
    res = S.score_batch(m, seqs, batch_size=8)
    z = m.engine.score_logits.cpu().numpy()
    assert z.shape == (3, 39, 68)
    for i, ids in enumerate(seqs):
        ref = restate(z[i], np.array(ids[1:]), 68)
        within_ulp(res[i]["logp"], ref["logp"])
        assert abs(res[i]["logp_sum"] - ref["logp"].sum()) <= 1e-12 * abs(ref["logp"].sum())
    ids = seqs[0][:21]
    lp = S.token_logprobs(m, ids)
    z = m.engine.score_logits.cpu().numpy()
    assert z.shape == (1, 20, 68)
    within_ulp(lp, restate(z[0], np.array(ids[1:]), 68)["logp"])


@pytest.fixture(scope="module")
def long_case(nets):
    """A 73-token CDS and the oracle's log_softmax rows for positions 1..72, window by window as
    the streaming rule runs them: position t from ids[max(0, t - 64):t], last row."""
    cfg, params, _ = nets["mha_gelu"]
    rng = np.random.default_rng(73)
    ids = [1] + rng.integers(4, 68, size=71).tolist() + [2]
    rows, scale = [], 0.0
    for t in range(1, len(ids)):
        ctx = ids[max(0, t - 64):t]
        with torch.no_grad():
            z = O.forward(cfg, params, np.array([ctx]))["logits"][0, -1].double()
        scale = max(scale, float(z.abs().max()))
        rows.append(torch.log_softmax(z, -1).numpy())
    return ids, np.stack(rows), scale


def test_token_logprobs_sliding_windows(nets, long_case):
    from codonlm_amd import score as S
    _, _, m = nets["mha_gelu"]
    ids, lp, scale = long_case
    ref = lp[np.arange(72), ids[1:]]
    for bs in (3, 32):  # 8 windows past the head: three forwards, or one
        got = S.token_logprobs(m, ids, batch_size=bs)
        assert got.shape == (72,)
        err = float(np.abs(got - ref).max())
        print(f"[token_logprobs bs={bs}] max|dlogp| {err:.2e} (tol {2e-4 * scale:.2e})")
        assert err <= 2e-4 * scale
    short = S.token_logprobs(m, ids[:40])
    assert float(np.abs(short - ref[:39]).max()) <= 2e-4 * scale


def test_mutation_map_matches_oracle(nets, long_case):
    from codonlm_amd import score as S
    stoi = {t: i for i, t in enumerate(VOCAB)}
    cids = S.codon_ids(stoi)
    for name in sorted(CONFIGS):
        cfg, params, m = nets[name]
        seqs = [s for s in _sequences() if len(s) >= 3]
        maps = S.mutation_maps(m, seqs, cids, batch_size=4)
        for ids, got in zip(seqs, maps):
            lp, scale = _oracle_logp(cfg, params, ids)
            n = len(ids) - 2
            ref = lp[:n][:, cids] - lp[np.arange(n), ids[1:-1]][:, None]
            assert got.shape == (n, 64)
            assert float(np.abs(got - ref).max()) <= 2e-4 * scale, (name, len(ids))
    # longer than the block: the sliding windows; codon classes outside the vocabulary give -inf
    _, _, m = nets["mha_gelu"]
    ids, lp, scale = long_case
    sel = cids[:10] + [-1, 68, 1000]
    got = S.mutation_map(m, ids, sel)
    ref = lp[:71][:, cids[:10]] - lp[np.arange(71), ids[1:-1]][:, None]
    assert got.shape == (71, 13) and np.all(np.isneginf(got[:, 10:]))
    assert float(np.abs(got[:, :10] - ref).max()) <= 2e-4 * scale


def test_score_mutations_cli_with_a_67_token_vocabulary(tmp_path):
    from codonlm_amd import score as S
    from codonlm_amd import score_mutations as M
    vocab = [t for t in VOCAB if t != "CCC"]
    cfg = O.OracleConfig(vocab_size=67, block_size=64, n_layer=2, n_head=2, n_embd=128, sep_id=3)
    params = O.synthetic_params(cfg, seed=7)
    rd = tmp_path / "run67"
    (rd / "checkpoints").mkdir(parents=True)
    (rd / "itos.txt").write_text("\n".join(vocab) + "\n")
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd["head.weight"] = sd["tok_emb.weight"]
    run_cfg = {"vocab_size": 67, "block_size": 64, "n_layer": 2, "n_head": 2, "n_embd": 128, "dropout": 0.1,
               "sep_mask_enabled": True, "tie_embeddings": True}
    torch.save({"model": sd, "cfg": run_cfg}, rd / "checkpoints" / "best.pt")
    dna = tmp_path / "cds.txt"
    dna.write_text("augAAACCCGGGTTTGCAGCCnnnGCGTGGCATTAA\n")  # CCC and NNN are outside the vocabulary: dropped
    stoi = {t: i for i, t in enumerate(vocab)}
    ids = S.dna_to_ids("ATGAAAGGGTTTGCAGCCGCGTGGCATTAA", stoi)
    assert len(ids) == 12
    lp, scale = _oracle_logp(cfg, params, ids)
    out = M.main(["--run_dir", str(rd), "--dna", str(dna), "--out", str(tmp_path / "o" / "map.tsv")])
    lines = out.read_bytes().decode().split("\r\n")  # csv rows end in CR LF, as the reference writes them
    assert lines[0].split("\t") == ["pos", "wt"] + S.CODONS and lines[-1] == "" and len(lines) == 1 + 10 + 1
    ccc = 2 + S.CODONS.index("CCC")
    for pos, line in enumerate(lines[1:-1], start=1):
        f = line.split("\t")
        assert f[0] == str(pos) and f[1] == vocab[ids[pos]] and f[ccc] == "-inf" and len(f) == 66
        for c, cod in enumerate(S.CODONS):
            if cod == "CCC":
                continue
            ref = lp[pos - 1, stoi[cod]] - lp[pos - 1, ids[pos]]
            assert abs(float(f[2 + c]) - ref) <= 2e-4 * scale + 1e-4, (pos, cod)
            assert len(f[2 + c].split(".")[1]) == 4
    # --ckpt with the itos.txt one level above the checkpoint gives the same file
    out2 = M.main(["--ckpt", str(rd / "checkpoints" / "best.pt"), "--dna", str(dna), "--out", str(tmp_path / "b.tsv")])
    assert out2.read_text() == out.read_text()
    # shape-guided checkpoints are refused as query_model refuses them
    torch.save({"model": sd, "cfg": dict(run_cfg, use_shape_guidance=True)}, rd / "checkpoints" / "best.pt")
    with pytest.raises(ValueError, match="shape-guided"):
        M.main(["--run_dir", str(rd), "--dna", str(dna), "--out", str(tmp_path / "c.tsv")])


def test_score_variants_match_oracle(nets):
    from codonlm_amd import score as S
    cfg, params, m = nets["gqa_rope_swiglu"]
    rng = np.random.default_rng(17)
    wt = [1] + rng.integers(4, 68, size=28).tolist() + [2]
    variants = []
    for pos in (1, 5, 9, 14, 20, 28):  # six single-codon substitutions
        v = list(wt)
        v[pos] = 4 + (v[pos] - 4 + 1 + pos) % 64
        variants.append(v)

    def total(ids):
        lp, scale = _oracle_logp(cfg, params, ids)
        return lp[np.arange(len(ids) - 1), ids[1:]].sum(), scale
    wt_sum, scale = total(wt)
    got = S.score_variants(m, wt, variants, batch_size=4)
    assert got.shape == (6,) and got.dtype == np.float64
    for v, g in zip(variants, got):
        s, sc = total(v)
        # two sums of 29 tokens, each within 29 * TOL of the oracle's
        assert abs(g - (s - wt_sum)) <= 29 * 2e-4 * (scale + sc)


# ------------------------------------------------------------------ evaluation
AUX_CFG = O.OracleConfig(vocab_size=68, block_size=64, n_layer=2, n_head=2, n_embd=128, sep_id=3,
                         termination_aux=True, multi_offset_targets=[2, 4])


def _eval_batches():
    """Three (x, y) batches with PAD tails and SEP / EOS boundaries, as the dynamic collate pads them."""
    rng = np.random.default_rng(29)
    out = []
    for B, T in ((4, 40), (3, 64), (2, 17)):
        x = np.zeros((B, T), np.int64)
        y = np.zeros((B, T), np.int64)
        for b in range(B):
            n = T if b == 0 else int(rng.integers(3, T))
            seq = [1] + rng.integers(4, 68, size=n).tolist()
            if n > 12:
                seq[n // 2], seq[n // 2 + 1] = 2, 3  # EOS SEP inside the packed window
            x[b, :n], y[b, :n] = seq[:-1], seq[1:]
        out.append((x, y))
    return out


def _restated_eval(cfg, params, batches, eps):
    """evaluate_test.py :102-150 on the oracle's logits, fp64 F.cross_entropy(reduction="sum")."""
    nll = obj = 0.0
    tokens = 0
    off = {k: [0.0, 0.0, 0] for k in cfg.multi_offset_targets}
    scale = 0.0
    for x, y in batches:
        with torch.no_grad():
            o = O.forward(cfg, params, x)
        z = o["logits"].double()
        scale = max(scale, float(z.abs().max()))
        yt = torch.from_numpy(y)
        if int((yt != 0).sum()) == 0:
            continue
        nll += float(F.cross_entropy(z.reshape(-1, 68), yt.reshape(-1), ignore_index=0, reduction="sum"))
        obj += float(F.cross_entropy(z.reshape(-1, 68), yt.reshape(-1), ignore_index=0, reduction="sum",
                                     label_smoothing=eps))
        tokens += int((yt != 0).sum())
        for k in cfg.multi_offset_targets:
            tgt = yt[:, k - 1:]
            mask = O.offset_target_mask(yt, k)
            if int(mask.sum()) == 0:
                continue
            zk = o["aux"]["offset_logits"][k].double()
            scale = max(scale, float(zk.abs().max()))
            off[k][0] += float(F.cross_entropy(zk[:, :tgt.shape[1]][mask], tgt[mask], reduction="sum"))
            off[k][1] += float(F.cross_entropy(z[:, :tgt.shape[1]][mask], tgt[mask], reduction="sum"))
            off[k][2] += int(mask.sum())
    return nll, obj, tokens, off, scale


@pytest.fixture(scope="module")
def aux_net():
    params = O.synthetic_params(AUX_CFG, seed=31)
    return AUX_CFG, params, _model(AUX_CFG, params)


def test_evaluate_matches_restated_cross_entropy(aux_net):
    from codonlm_amd import score as S
    cfg, params, m = aux_net
    batches = _eval_batches()
    batches.insert(1, (np.zeros((2, 9), np.int64), np.zeros((2, 9), np.int64)))  # an all-PAD batch
    eps = 0.05
    dev_batches = [(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)) for x, y in batches]
    nll, ppl, obj, tokens, off = S.evaluate(m, dev_batches, label_smoothing=eps, offset_targets=(2, 4))
    r_nll, r_obj, r_tok, r_off, scale = _restated_eval(cfg, params, batches, eps)
    tol = 2e-4 * scale
    print(f"[evaluate] nll {nll:.6f} ref {r_nll / r_tok:.6f}; objective {obj:.6f} ref {r_obj / r_tok:.6f}; tol {tol:.2e}")
    assert tokens == r_tok and np.isfinite([nll, ppl, obj]).all()
    assert abs(nll - r_nll / r_tok) <= tol and abs(obj - r_obj / r_tok) <= tol
    assert ppl == math.exp(min(20.0, nll))
    assert sorted(off) == [2, 4]
    for k in (2, 4):
        v = off[k]
        assert sorted(v) == sorted(S.OFFSET_KEYS)
        assert v["evaluated_tokens"] == r_off[k][2] > 0
        assert abs(v["nll"] - r_off[k][0] / r_off[k][2]) <= tol
        assert abs(v["unprojected_nll"] - r_off[k][1] / r_off[k][2]) <= tol
        assert v["ppl"] == math.exp(min(20.0, v["nll"])) and v["unprojected_ppl"] == math.exp(min(20.0, v["unprojected_nll"]))
        assert v["nll_improvement"] == v["unprojected_nll"] - v["nll"]
        assert v["relative_nll_improvement"] == v["nll_improvement"] / v["unprojected_nll"]
    # without offset heads the engine scores its own logits buffer: both runs are within tol of the oracle
    nll2, _, obj2, tok2, off2 = S.evaluate(m, dev_batches, label_smoothing=eps)
    assert tok2 == tokens and off2 == {} and abs(nll2 - nll) <= 2 * tol and abs(obj2 - obj) <= 2 * tol
    # only PAD: zeros, no NaN
    assert S.evaluate(m, dev_batches[1:2], label_smoothing=eps, offset_targets=(2, 4)) == (0.0, 1.0, 0.0, 0, {})


def test_evaluate_test_cli(tmp_path, aux_net, monkeypatch):
    from codonlm_amd import evaluate_test as E
    cfg, params, _ = aux_net
    rng = np.random.default_rng(41)
    X = rng.integers(4, 68, size=(10, 64)).astype(np.int32)
    X[:, 0] = 1
    X[3, 20:22] = (2, 3)
    Y = np.concatenate([X[:, 1:], np.full((10, 1), 2, np.int32)], 1)
    Y[7, 30:] = 0  # a PAD tail
    np.savez(tmp_path / "test_bs64.npz", X=X, Y=Y)
    np.savez(tmp_path / "val.npz", X=X[:4], Y=Y[:4])
    rd = tmp_path / "runs" / "r1"
    (rd / "checkpoints").mkdir(parents=True)
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd["head.weight"] = sd["tok_emb.weight"]
    run_cfg = {"vocab_size": 68, "block_size": 64, "n_layer": 2, "n_head": 2, "n_embd": 128, "dropout": 0.1,
               "sep_mask_enabled": True, "tie_embeddings": True, "label_smoothing": 0.05,
               "termination_loss_enabled": True, "multi_offset_targets": [2, 4],
               "val_npz": [str(tmp_path / "val.npz")]}
    torch.save({"model": sd, "cfg": run_cfg}, rd / "checkpoints" / "best.pt")
    (rd / "scores").mkdir()
    (rd / "scores" / "metrics.json").write_text(json.dumps({"train_loss": 1.25, "test_nll": 99.0}))
    E.main(["--run_dir", str(rd), "--data_dir", str(tmp_path), "--batch_size", "4"])
    mt = json.loads((rd / "scores" / "metrics.json").read_text())
    names = ["loss", "nll", "ppl", "objective_loss", "label_smoothing", "evaluated_tokens", "evaluation_provenance"]
    names += [f"offset_{k}_{n}" for k in (2, 4) for n in
              ("nll", "ppl", "unprojected_nll", "unprojected_ppl", "nll_improvement", "relative_nll_improvement",
               "evaluated_tokens")]
    assert sorted(mt) == sorted(["train_loss", "timestamp"] + [f"test_{n}" for n in names])
    assert mt["train_loss"] == 1.25  # a foreign key survives the merge
    r_nll, r_obj, r_tok, r_off, scale = _restated_eval(cfg, params, [(X.astype(np.int64), Y.astype(np.int64))], 0.05)
    tol = 2e-4 * scale
    assert mt["test_evaluated_tokens"] == r_tok and mt["test_label_smoothing"] == 0.05
    assert abs(mt["test_nll"] - r_nll / r_tok) <= tol and mt["test_loss"] == mt["test_nll"]
    assert abs(mt["test_objective_loss"] - r_obj / r_tok) <= tol and mt["test_ppl"] == math.exp(min(20.0, mt["test_nll"]))
    for k in (2, 4):
        assert mt[f"test_offset_{k}_evaluated_tokens"] == r_off[k][2]
        assert abs(mt[f"test_offset_{k}_nll"] - r_off[k][0] / r_off[k][2]) <= tol
        assert abs(mt[f"test_offset_{k}_unprojected_nll"] - r_off[k][1] / r_off[k][2]) <= tol
    prov = mt["test_evaluation_provenance"]
    assert sorted(prov) == sorted(["schema_version", "loss_definition", "dataset_manifest", "checkpoint_dataset",
                                   "checkpoint", "test_tokens", "derived_dataset"])
    assert prov["dataset_manifest"] == {"status": "legacy_unverified"} and prov["derived_dataset"] is None
    assert prov["test_tokens"]["path"] == str((tmp_path / "test_bs64.npz").resolve())
    assert len(prov["checkpoint"]["sha256"]) == 64
    # the validation split under its own prefix, merged into the same file; --run_id resolves under runs/
    monkeypatch.chdir(tmp_path)
    E.main(["--run_id", "r1", "--split", "validation", "--metric-prefix", "val2", "--dtype", "bf16"])
    mt2 = json.loads((rd / "scores" / "metrics.json").read_text())
    assert mt2["test_nll"] == mt["test_nll"] and mt2["val2_evaluated_tokens"] == 4 * 64
    assert "val_tokens" in mt2["val2_evaluation_provenance"] and math.isfinite(mt2["val2_nll"])
    with pytest.raises(ValueError, match="--test_npz cannot be used with --split validation"):
        E.main(["--run_dir", str(rd), "--split", "validation", "--test_npz", str(tmp_path / "val.npz")])
    with pytest.raises(ValueError, match="derived_provenance"):
        E.main(["--run_dir", str(rd), "--derived_provenance", str(tmp_path / "p.json")])
