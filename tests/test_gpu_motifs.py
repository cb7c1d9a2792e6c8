"""codonlm_amd.motifs and the mine_motifs CLI on the GPU: window embeddings against the torch
restatement of the reference's extractor, the k-means driver on the native step against the numpy
Lloyd restatement of test_motifs_cpu, and the CLI's files."""
import re

import numpy as np
import pytest
import torch

from oracle import tinygpt_oracle as O
from test_gpu_inference import VOCAB
from test_gpu_score import _model
from test_motifs_cpu import ref_kmeans

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
CFG = O.OracleConfig(vocab_size=68, block_size=64, n_layer=2, n_head=4, n_embd=64, sep_id=3)
SPECIAL = (0, 1, 2, 3)
WINDOW, STRIDE = 9, 3


@pytest.fixture(scope="module")
def params():
    return O.synthetic_params(CFG, seed=2024)


def _sequences():
    """6 sequences of T = 40: BOS first, PAD tails of several lengths, one SEP and one EOS inside."""
    rng = np.random.default_rng(17)
    x = rng.integers(4, 68, size=(6, 40)).astype(np.int64)
    x[:, 0] = 1
    for b, n in enumerate((40, 33, 25, 40, 12, 38)):
        x[b, n:] = 0
    x[3, 20] = 3   # a SEP in the middle of a full row
    x[1, 32] = 2   # an EOS before the PAD tail
    return x


def _restatement(m, x, layer):
    """MotifExtractor.extract over the whole batch: unfold + mean of the block's output (fp64 from
    the stored values), windows holding a special token dropped, in (sequence, start) order."""
    want = int(layer) % CFG.n_layer + 1
    h = None
    for which, t in m.iter_hidden_states(torch.from_numpy(x).to(DEV)):
        if which == want:
            h = t.to(torch.float64)
    win = h.unfold(1, WINDOW, STRIDE)  # (B, nwin, d, window)
    mean, absum = win.mean(-1).cpu().numpy(), win.abs().sum(-1).cpu().numpy()
    rows, meta, bound = [], [], []
    for b in range(x.shape[0]):
        for j in range(win.shape[1]):
            s = j * STRIDE
            if set(x[b, s:s + WINDOW].tolist()) & set(SPECIAL):
                continue
            rows.append(mean[b, j])
            bound.append((WINDOW + 2) * U * absum[b, j] / WINDOW)
            meta.append((b, s, s + WINDOW))
    return np.array(rows), np.array(meta, np.int64).reshape(-1, 3), np.array(bound)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_window_embeddings_match_the_extractor(params, dtype):
    from codonlm_amd import motifs as M
    m = _model(CFG, params, dtype)
    x = _sequences()
    for layer in (-1, 0):
        want, meta, bound = _restatement(m, x, layer)
        emb, got_meta = M.window_embeddings(m, x, WINDOW, STRIDE, layer=layer, exclude_ids=SPECIAL)
        assert emb.dtype == torch.float32 and emb.is_cuda and got_meta.dtype == torch.int64
        assert 10 < len(want) < 6 * 11 and tuple(emb.shape) == want.shape
        assert np.array_equal(got_meta.numpy(), meta)
        err = np.abs(emb.cpu().numpy().astype(np.float64) - want)
        print(f"[window_embeddings {dtype} layer={layer}] N={len(want)} max err/bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        e4 = M.window_embeddings(m, x, WINDOW, STRIDE, layer=layer, exclude_ids=SPECIAL, batch_size=4)
        e6 = M.window_embeddings(m, x, WINDOW, STRIDE, layer=layer, exclude_ids=SPECIAL, batch_size=6)
        assert torch.equal(e4[0], e6[0]) and torch.equal(e6[0], emb) and torch.equal(e4[1], e6[1])
    a, b = (M.window_embeddings(m, x, WINDOW, STRIDE, layer=ly, exclude_ids=SPECIAL)[0] for ly in (-1, 0))
    assert not torch.equal(a, b)  # two different blocks
    # longer than block_size: trimmed; shorter than the window, or all special: nothing kept
    long = np.concatenate([x, x], axis=1)
    assert M.window_embeddings(m, long, WINDOW, STRIDE, exclude_ids=SPECIAL)[1][:, 2].max() <= CFG.block_size
    e, mt = M.window_embeddings(m, x[:, :5], WINDOW, STRIDE)
    assert tuple(e.shape) == (0, 64) and tuple(mt.shape) == (0, 3)
    e, mt = M.window_embeddings(m, np.zeros((2, 40), np.int64), WINDOW, STRIDE, exclude_ids=SPECIAL)
    assert tuple(e.shape) == (0, 64) and tuple(mt.shape) == (0, 3)
    with pytest.raises(ValueError, match="lists of layers"):
        M.window_embeddings(m, x, WINDOW, STRIDE, layer=[0, 1])


def _blobs():
    rng = np.random.default_rng(23)
    planted = rng.integers(0, 3, size=600)
    means = 25.0 * rng.standard_normal((3, 16))
    X = (means[planted] + rng.standard_normal((600, 16))).astype(np.float32)
    init = (means + 2.0 * rng.standard_normal((3, 16))).astype(np.float32)
    return X, planted, init


def test_kmeans_recovers_planted_blobs_and_matches_the_restatement():
    from codonlm_amd import motifs as M
    X, planted, init = _blobs()
    lab, cen, inertia, n_iter = M.kmeans(torch.from_numpy(X).to(DEV), 3, init=torch.from_numpy(init))
    rl, rc, ri, rn = ref_kmeans(X, 3, init=init)
    assert lab.dtype == torch.int32 and cen.dtype == torch.float32 and lab.is_cuda
    assert np.array_equal(lab.cpu().numpy(), planted)  # init row c lies next to blob c
    assert np.array_equal(lab.cpu().numpy(), rl) and n_iter == rn
    assert np.abs(cen.cpu().numpy() - rc).max() <= 1e-5 * np.abs(rc).max()
    assert abs(inertia - ri) <= 1e-5 * ri


def test_kmeans_is_reproducible_and_inertia_never_grows():
    from codonlm_amd import motifs as M
    rng = np.random.default_rng(3)
    X = torch.from_numpy((rng.standard_normal((3000, 24)) * rng.uniform(0.5, 3, 24)).astype(np.float32)).to(DEV)
    a = M.kmeans(X, 12, seed=42)
    b = M.kmeans(X, 12, seed=42)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]
    c = M.kmeans(X, 12, seed=43)
    assert not torch.equal(a[1], c[1])
    assert int(torch.bincount(a[0].long(), minlength=12).min()) >= 1
    init = M.kmeans_pp_init(X, 12, 42)
    inert = [M.kmeans(X, 12, init=init, tol=0.0, max_iter=i)[2] for i in range(0, 7)]
    print("[kmeans] inertia over iterations:", [f"{v:.6e}" for v in inert])
    assert all(later <= earlier for earlier, later in zip(inert, inert[1:])) and inert[-1] < inert[0]
    with pytest.raises(ValueError, match="n_clusters"):
        M.kmeans(X[:5], 6)


def _write_run(tmp_path, params):
    rd = tmp_path / "runs" / "r1"
    (rd / "checkpoints").mkdir(parents=True)
    (rd / "itos.txt").write_text("\n".join(VOCAB) + "\n")
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd["head.weight"] = sd["tok_emb.weight"]
    run_cfg = {"vocab_size": 68, "block_size": 64, "n_layer": 2, "n_head": 4, "n_embd": 64, "dropout": 0.1,
               "sep_mask_enabled": True, "tie_embeddings": True}
    torch.save({"model": sd, "cfg": run_cfg}, rd / "checkpoints" / "best.pt")
    return rd


def test_mine_motifs_cli(tmp_path, params, capsys):
    from codonlm_amd import mine_motifs as C
    rd = _write_run(tmp_path, params)
    x = np.concatenate([_sequences(), _sequences()[::-1]], axis=0).astype(np.int32)
    x = np.concatenate([x, np.zeros((12, 30), np.int32)], axis=1)  # 70 columns: trimmed to block_size 64
    np.savez(tmp_path / "data.npz", X=x)
    out = C.main(["--run_dir", str(rd), "--data_npz", str(tmp_path / "data.npz"), "--pca", "8", "--n_clusters", "4",
                  "--n_samples", "10", "--batch_size", "4"])
    assert out == rd / "motif_mining" / "clusters.npz" and out.exists()
    report = (rd / "motif_mining" / "motif_report.md").read_text()
    z = np.load(out)
    assert sorted(z.files) == sorted(["labels", "centers", "window_size", "stride", "layer", "method", "inertia",
                                      "n_iter", "seed"])
    N = len(z["labels"])
    assert z["labels"].dtype == np.int32 and z["labels"].shape == (N,) and N > 20
    assert z["centers"].dtype == np.float32 and z["centers"].shape == (4, 8)
    assert (int(z["window_size"]), int(z["stride"]), int(z["layer"]), str(z["method"]), int(z["seed"])) == \
        (9, 3, -1, "kmeans", 42)
    assert z["inertia"].dtype == np.float64 and float(z["inertia"]) > 0 and int(z["n_iter"]) >= 1
    assert set(z["labels"].tolist()) <= {0, 1, 2, 3}
    lines = report.split("\n")
    assert lines[0] == "# Motif Mining Report: r1" and "- **Sequences sampled:** 10" in lines
    assert f"- **Total windows:** {N}" in lines and "- **Method:** kmeans" in lines and "- **Layer:** -1" in lines
    sizes = [int(s) for s in re.findall(r"^## Cluster \d+ \(size=(\d+)\)$", report, flags=re.M)]
    assert sum(sizes) == N and sizes == sorted(sizes, reverse=True)
    assert sorted(sizes) == sorted(np.bincount(z["labels"], minlength=4)[np.bincount(z["labels"], minlength=4) > 0])
    examples = [ln for ln in lines if ln.startswith("- `")]
    assert examples and all(len(ln[3:-1].split(" ")) == 9 and "<" not in ln for ln in examples)
    assert "[success]" in capsys.readouterr().out
    # no window survives: the reference's message, and nothing written
    rd2 = _write_run(tmp_path / "second", params)
    np.savez(tmp_path / "pad.npz", X=np.zeros((3, 40), np.int32))
    assert C.main(["--run_dir", str(rd2), "--data_npz", str(tmp_path / "pad.npz")]) is None
    assert "No windows kept after filtering special tokens" in capsys.readouterr().out
    assert not (rd2 / "motif_mining").exists()
