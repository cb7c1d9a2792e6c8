"""codonlm_amd.attention and the analyze_attention CLI on a tiny model, against fp64 reductions of
the engine's own captured attention maps (model.capture_attn: cg_attn_probs, an independent kernel
that normalises with the forward's LSE).

Bounds: that path's stated row-sum bound in fp32, 1e-4, and its tolerance in bf16, 2e-2, per
probability-weighted row statistic (MEAN_DIST scales with T, the entropies with 1 + ln T).
"""
import math

import numpy as np
import pytest
import torch

import attention_restatement as AR
from oracle import tinygpt_oracle as O
from test_gpu_inference import VOCAB
from test_gpu_score import _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 130
CFG = O.OracleConfig(vocab_size=68, block_size=192, n_layer=2, n_head=4, n_embd=64, n_kv_head=2, use_rope=True,
                     use_swiglu=True, sep_id=3)


def _tokens():
    """int64 [3][130]: BOS, codons, SEPs in rows 0 and 1 (63 / 64 among them), a PAD tail on row 2."""
    rng = np.random.default_rng(5)
    x = rng.integers(4, 68, size=(3, T)).astype(np.int64)
    x[:, 0] = 1
    x[0, [20, 64, 100]] = 3
    x[1, [63, 64]] = 3
    x[2, 90:] = 0
    return x


@pytest.fixture(scope="module")
def nets():
    params = O.synthetic_params(CFG, seed=11)
    return {dt: _model(CFG, params, dt) for dt in ("fp32", "bf16")}


def _captured(m, x):
    """fp64 (L, B, H, T, T) of the model's capture_attn maps."""
    m.capture_attn = True
    try:
        with torch.no_grad():
            m(torch.from_numpy(x).to(DEV))
        return np.stack([b.attn.last_attn.double().cpu().numpy() for b in m.blocks])
    finally:
        m.capture_attn = False


def _scaled_tol(base):
    t = np.full(AR.NSTAT, base)
    t[AR.MEAN_DIST] *= T
    t[AR.ENTROPY] *= 1 + math.log(T)
    t[AR.NORM_ENTROPY] *= (1 + math.log(T)) / math.log(2)
    return t


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_library_matches_reductions_of_the_captured_maps(nets, dtype):
    from codonlm_amd import attention as A
    from codonlm_amd.context import token_classes
    m = nets[dtype]
    x = _tokens()
    cls = token_classes(VOCAB)
    base = 1e-4 if dtype == "fp32" else 2e-2
    tol = _scaled_tol(base)
    P = _captured(m, x)
    mask = AR.attention_mask(x, 3, T, sep_id=3)
    ref = [AR.stats_from_probs(P[l], mask, idx=x, pad_id=0, tok_class=cls) for l in range(CFG.n_layer)]
    n = int((x != 0).sum())
    hs = A.head_stats(m, x, VOCAB, batch=2)                   # two batches: 2 rows + 1 row
    assert hs.sums.shape == (2, 4, AR.NSTAT) and hs.n_rows == n == ref[0]["n_rows"]
    want = np.stack([r["head_acc"] for r in ref]) / n
    err = np.abs(hs.means - want).max((0, 1))
    print(f"head_stats {dtype}: err/tol " + " ".join(f"{s}={e / t:.3f}" for s, e, t in zip(AR.STATS, err, tol)))
    assert (err <= tol).all()
    assert np.abs(hs.mean("entropy") - want[:, :, AR.ENTROPY]).max() <= tol[AR.ENTROPY]
    # an iterable of (x, y) device batches and a row filter give the same numbers as the array
    xd = torch.from_numpy(x).to(DEV)
    hs2 = A.head_stats(m, [(xd[:2], None), (xd[2:], None)], VOCAB)
    assert np.array_equal(hs2.sums, hs.sums) and hs2.n_rows == n
    stops = np.isin(x, [VOCAB.index(c) for c in ("TAA", "TAG", "TGA")])
    hs3 = A.head_stats(m, x, VOCAB, row_keep=stops)
    assert hs3.n_rows == int(stops.sum()) > 0
    want3 = np.stack([(r["rows"] * stops[:, None, :, None]).sum((0, 2)) for r in ref]) / hs3.n_rows
    assert (np.abs(hs3.means - want3).max((0, 1)) <= tol).all()
    # received
    rec = A.received(m, x)
    assert rec.shape == (2, 3, 4, T) and rec.dtype == np.float32
    wr = np.stack([r["received"] for r in ref])
    rerr = float((np.abs(rec - wr) / (base * (1 + wr))).max())
    print(f"received {dtype}: err/tol {rerr:.3f}")
    assert rerr <= 1.0
    # the reference's triple of one sequence, PAD rows included as there
    for b in (0, 2):
        got = A.reference_head_stats(m, x[b], VOCAB)
        rows_b = [AR.stats_from_probs(P[l][b:b + 1], mask[b:b + 1], idx=x[b:b + 1], pad_id=-1, tok_class=cls)["rows"][0]
                  for l in range(CFG.n_layer)]
        want_t = np.stack([AR.reference_triple(r, x[b], cls) for r in rows_b])
        assert got.shape == (2, 4, 3)
        assert np.abs(got[..., 0] - want_t[..., 0]).max() <= tol[AR.ENTROPY]
        assert np.abs(got[..., 1:] - want_t[..., 1:]).max() <= base
    sp = A.specialists(hs, k=3)
    assert all(len(v) == 3 for v in sp.values()) and sp["most_focused"][0][2] == hs.mean("entropy").min()


def test_attention_maps_shape_and_crop(nets):
    from codonlm_amd import attention as A
    m = nets["fp32"]
    x = _tokens()
    full = A.attention_maps(m, x[:2])
    assert full.shape == (2, 2, 4, T, T) and full.dtype == np.float32
    assert np.abs(full.sum(-1) - 1).max() <= 1e-4 and (np.triu(full, 1) == 0).all()
    assert np.abs(full - _captured(m, x[:2])).max() <= 1e-6
    crop = A.attention_maps(m, x[:2], layers=[1], max_tokens=60)
    assert crop.shape == (1, 2, 4, 60, 60)
    assert np.abs(crop[0] - full[1][:, :, :60, :60]).max() <= 1e-5
    with pytest.raises(ValueError):
        A.attention_maps(m, x[:1], max_tokens=0)


def test_analyze_attention_cli(tmp_path):
    import csv
    from codonlm_amd import analyze_attention as C
    from codonlm_amd import attention as A
    from codonlm_amd.score_mutations import load_model
    cfg = O.OracleConfig(vocab_size=68, block_size=64, n_layer=2, n_head=2, n_embd=128, sep_id=3)
    params = O.synthetic_params(cfg, seed=7)
    rd = tmp_path / "runs" / "r1"
    (rd / "checkpoints").mkdir(parents=True)
    (rd / "itos.txt").write_text("\n".join(VOCAB) + "\n")
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd["head.weight"] = sd["tok_emb.weight"]
    run_cfg = {"vocab_size": 68, "block_size": 64, "n_layer": 2, "n_head": 2, "n_embd": 128, "dropout": 0.1,
               "sep_mask_enabled": True, "tie_embeddings": True}
    torch.save({"model": sd, "cfg": run_cfg}, rd / "checkpoints" / "best.pt")
    rng = np.random.default_rng(2)
    X = rng.integers(4, 68, size=(5, 24)).astype(np.int32)
    X[:, 0] = 1
    X[1, 10] = 3
    X[4, 18:] = 0
    np.savez(rd / "artifacts.npz", val_inputs=X)
    out = C.main(["--run_dir", str(rd), "--n_seqs", "4", "--batch", "3", "--maps", "2", "--max_tokens", "16"])
    assert out["csv"] == rd / "tables" / "attention_heads.csv" and out["maps"] == rd / "attention" / "attn_maps.npz"
    model, _ = load_model(None, rd, "fp32")
    want = A.head_stats(model, X[:4].astype(np.int64), VOCAB, batch=3)
    with out["csv"].open(newline="") as f:
        rows = list(csv.reader(f))
    assert rows == [[str(c) for c in r] for r in C.csv_rows(want)] and len(rows) == 1 + 2 * 2
    with np.load(out["npz"]) as z:
        assert np.array_equal(z["sums"], want.sums) and int(z["n_rows"]) == 4 * 24
        assert np.array_equal(z["reference_row0"], A.reference_head_stats(model, X[0], VOCAB))
    assert out["report"].read_text() == C.report_markdown(want)
    with np.load(out["maps"]) as z:
        assert z["attn"].shape == (2, 2, 2, 16, 16) and z["attn"].dtype == np.float32
        assert np.array_equal(z["val_inputs"], X[:2, :16])
    # --npz X, every row, PAD rows dropped
    np.savez(tmp_path / "val.npz", X=X)
    out2 = C.main(["--run_dir", str(rd), "--npz", str(tmp_path / "val.npz")])
    assert "maps" not in out2
    with np.load(out2["npz"]) as z:
        assert int(z["n_rows"]) == int((X != 0).sum())
