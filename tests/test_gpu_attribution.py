"""cg_model_input_grad, codonlm_amd.attribution and the analyze_saliency CLI against the CPU oracle.

Bounds.  The project's fp32 gradient bound (test_gpu_model.test_fp32_grads_match_reference) is
GB = 2e-4 * max(1e-3, max|reference gradient|), taken here over the whole (B, T, d) input gradient.
A dot product of that gradient with an activation row a moves by at most GB * |a|_1, its norm by at
most GB * sqrt(d): the bounds of gxt / gxi and gnorm.  bf16 has no measured bound of its own yet, so
it is calibrated inside the test against the unchanged full backward (see that test).
"""
import numpy as np
import pytest
import torch

from oracle import tinygpt_oracle as O
from test_gpu_inference import VOCAB
from test_gpu_score import CONFIGS, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"

ALL = dict(CONFIGS)
# the smoke() geometry with a block long enough for T = 130: one key tile (64) and one query tile
# (128) of the attention backward are crossed
ALL["long"] = O.OracleConfig(vocab_size=68, block_size=192, n_layer=1, n_head=4, n_embd=64, n_kv_head=2,
                             use_rope=True, use_swiglu=True)
CASES = [(n, T) for n in ("mha_gelu", "gqa_rope_swiglu") for T in (1, 2, 33, 64)] + [("long", 64), ("long", 130)]


@pytest.fixture(scope="module")
def nets():
    out = {}
    for name, cfg in ALL.items():
        params = O.synthetic_params(cfg, seed=2024)
        out[name] = (cfg, params, _model(cfg, params))
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _batch(T, seed):
    """x, y int64 [2][T]: row 0 a full sequence (a SEP at position 15 when it is long enough), row 1
    one that ends after two thirds and is padded with PAD inputs and -1 targets."""
    rng = np.random.default_rng(seed)
    x = rng.integers(4, 68, size=(2, T))
    x[:, 0] = 1
    y = rng.integers(4, 68, size=(2, T))
    y[:, :-1] = x[:, 1:]
    if T > 20:
        x[0, 15] = 3
        y[0, 14] = 3
    n1 = max(1, (2 * T) // 3)
    if T > 1:
        x[1, n1:], y[1, n1:] = 0, -1
    return x.astype(np.int64), y.astype(np.int64)


def _oracle(cfg, params, x, targets=None):
    """The oracle's forward with every tensor in the graph: (out, embedding output)."""
    P = O._to_t(params, True)
    out = O.forward(cfg, P, x, targets)
    return out, out["hidden"][0]


def _objective(out, y, w, mode):
    z = out["logits"]
    rows = z.log_softmax(-1) if mode == "logprob" else z
    yt = torch.from_numpy(y)
    live = (yt >= 0) & (yt < z.shape[-1])
    picked = rows.gather(-1, yt.clamp(0, z.shape[-1] - 1)[..., None])[..., 0]
    wt = torch.ones_like(picked) if w is None else torch.from_numpy(w)
    return (picked * wt * live).sum()


def _check_against(ref_g, x0, tok_rows, r, d, tag):
    """dx0 and the three reductions of an AttrResult against the oracle gradient ref_g (B, T, d)."""
    ref = ref_g.numpy().astype(np.float64)
    gb = 2e-4 * max(1e-3, float(np.abs(ref).max()))
    got = r.dx0.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref).max())
    print(f"[{tag}] max|dx0 - ref| {err:.3e} (bound {gb:.3e}, max|ref| {float(np.abs(ref).max()):.3e})")
    assert err <= gb
    a_tok, a_x0 = tok_rows.astype(np.float64), x0.astype(np.float64)
    for name, want, bound in (("gxt", (ref * a_tok).sum(-1), gb * np.abs(a_tok).sum(-1)),
                              ("gxi", (ref * a_x0).sum(-1), gb * np.abs(a_x0).sum(-1)),
                              ("gnorm", np.sqrt((ref * ref).sum(-1)), gb * np.sqrt(d) * np.ones(ref.shape[:2]))):
        e = np.abs(getattr(r, name).cpu().numpy().astype(np.float64) - want)
        print(f"[{tag}] {name}: max err/bound {float((e / bound).max()):.3f}")
        assert (e <= bound).all(), name


@pytest.mark.parametrize("name,T", CASES)
def test_fp32_input_gradient_matches_the_oracle(nets, name, T):
    """Both seed modes, weighted and unweighted seeds, a padded batch, a SEP inside one sequence."""
    cfg, params, m = nets[name]
    x, y = _batch(T, seed=100 + T)
    w = np.random.default_rng(T).standard_normal((2, T)).astype(np.float32)
    out, h0 = _oracle(cfg, params, x)
    tok_rows = params["tok_emb.weight"][np.clip(x, 0, None)]
    eng = m.engine
    eng.forward(_dev(x), None, training=False)
    for mode, wt in (("logprob", None), ("logprob", w), ("logit", w)):
        (ref,) = torch.autograd.grad(_objective(out, y, wt, mode), h0, retain_graph=True)
        r = eng.input_grad(y=_dev(y), w=None if wt is None else _dev(wt), mode=mode, dx0=True)
        _check_against(ref, h0.detach().numpy(), tok_rows, r, cfg.n_embd, f"{name} T={T} {mode} w={wt is not None}")
        pad = y < 0
        assert (r.gnorm.cpu().numpy()[pad] == 0).all()  # nothing reaches a position after the last seed


def test_loss_seed_matches_the_oracle_loss(nets):
    """y = None: the gradient of the forward's own mean cross-entropy, label smoothing and the
    ignored PAD targets included."""
    base, params, _ = nets["mha_gelu"]
    cfg = O.OracleConfig(**dict(base.to_dict(), label_smoothing=0.1))
    m = _model(cfg, params)
    x, y = _batch(40, seed=7)
    y[y < 0] = 0  # PAD: the ignored class of the loss
    out, h0 = _oracle(cfg, params, x, y)
    (ref,) = torch.autograd.grad(out["loss"], h0)
    eng = m.engine
    _, loss = eng.forward(_dev(x), _dev(y), training=False)
    lref = float(out["loss"].detach())
    assert abs(float(loss) - lref) <= 1e-4 * max(1.0, abs(lref))
    r = eng.input_grad(dx0=True)
    _check_against(ref, h0.detach().numpy(), params["tok_emb.weight"][x], r, cfg.n_embd, "loss seed")
    # a seeded call replaces the loss gradient: the loss seed then needs a new forward
    eng.input_grad(y=_dev(y), want=("gxt",))
    with pytest.raises(ValueError, match="forward again"):
        eng.input_grad()
    eng.forward(_dev(x), None, training=False)
    with pytest.raises(ValueError):
        eng.input_grad()  # that forward had no targets
    eng.forward(_dev(x), _dev(y), training=False)
    r2 = eng.input_grad(dx0=True)
    assert torch.equal(r2.dx0, r.dx0)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name,T,t_seed", [("mha_gelu", 40, 20), ("gqa_rope_swiglu", 40, 20), ("long", 130, 70)])
def test_exact_zeros_outside_the_seeded_context(nets, name, T, t_seed, dtype):
    """One seeded position per row: nothing after it, nothing before its SEP segment and nothing
    in a row without a seed receives gradient -- exactly 0, in fp32 and bf16."""
    cfg, params, m32 = nets[name]
    m = m32 if dtype == "fp32" else _model(cfg, params, "bf16")
    rng = np.random.default_rng(3)
    x = rng.integers(4, 68, size=(3, T)).astype(np.int64)
    x[:, 0] = 1
    x[1, 15] = 3  # row 1: the seeded token's segment starts at the SEP
    y = np.full((3, T), -1, np.int64)
    y[0, t_seed], y[1, t_seed + 10] = 9, 11
    eng = m.engine
    eng.forward(_dev(x), None, training=False)
    for mode in ("logprob", "logit"):
        r = eng.input_grad(y=_dev(y), mode=mode, dx0=True)
        outs = {k: getattr(r, k).cpu().numpy() for k in ("gxt", "gxi", "gnorm")}
        outs["dx0"] = np.abs(r.dx0.cpu().numpy()).max(-1)
        for k, v in outs.items():
            assert np.isfinite(v).all()
            assert (v[0, t_seed + 1:] == 0).all(), (k, "after the seed")
            assert (v[1, t_seed + 11:] == 0).all() and (v[1, :15] == 0).all(), (k, "outside the segment")
            assert (v[2] == 0).all(), (k, "a row without a seed")
        assert (outs["gnorm"][0, :t_seed + 1] > 0).all() and (outs["gnorm"][1, 15:t_seed + 11] > 0).all()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_no_side_effects_on_gradients_or_a_later_training_step(nets, dtype):
    cfg, params, _ = nets["mha_gelu"]
    x, y = _batch(48, seed=5)
    y[y < 0] = 0
    xd, yd = _dev(x), _dev(y)

    def step(m):
        m.train()
        m.zero_grad()
        _, loss = m(xd, yd)
        loss.backward()
        torch.cuda.synchronize()
        return {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    m = _model(cfg, params, dtype)
    grads = m.flat_grads()
    sentinel = torch.arange(grads.numel(), dtype=torch.int32, device=DEV) * 2654435 + 0x7FC00000
    grads.view(torch.int32).copy_(sentinel)
    eng = m.engine
    eng.forward(xd, yd, training=False)
    eng.input_grad()
    eng.input_grad(y=yd, w=None, mode="logit", dx0=True)
    torch.cuda.synchronize()
    assert torch.equal(grads.view(torch.int32), sentinel)  # not one byte of the gradient buffer
    assert (eng.model.head_dw_pending, eng.model.reduce_pending.n) == (0, 0)
    grads.zero_()  # (a step leaves the pos_emb rows past T as they are: both models start from zeros)
    got = step(m)
    want = step(_model(cfg, params, dtype))  # a model that never ran attribution
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_bf16_input_gradient_is_calibrated_against_the_full_backward(nets):
    """B = 1 without RoPE: the full backward's pos_emb.grad[:T] is the input gradient (embed_bwd_pos
    sums over one row).  E_parent = max|pos_emb.grad - oracle| of the unchanged bf16 backward; the
    input-only path must come within 2 E_parent + the fp32 bound of the oracle (its dX products may
    take a kernel instance without the column-sum epilogue; the arithmetic chain is the same).
    Measured: see the printed pair and DESIGN.md."""
    cfg, params, m32 = nets["mha_gelu"]
    T = 64
    x, y = _batch(T, seed=21)
    x, y = x[:1], y[:1]
    out, h0 = _oracle(cfg, params, x, y)
    (ref,) = torch.autograd.grad(out["loss"], h0)
    ref = ref.numpy()[0].astype(np.float64)
    gb = 2e-4 * max(1e-3, float(np.abs(ref).max()))
    xd, yd = _dev(x), _dev(y)
    res = {}
    for dtype, m in (("fp32", m32), ("bf16", _model(cfg, params, "bf16"))):
        m.train()
        m.zero_grad()
        _, loss = m(xd, yd)
        loss.backward()
        parent = dict(m.named_parameters())["pos_emb.weight"].grad[:T].detach().cpu().numpy().astype(np.float64)
        m.eval()
        m.engine.forward(xd, yd, training=False)
        new = m.engine.input_grad(dx0=True).dx0[0].cpu().numpy().astype(np.float64)
        res[dtype] = (float(np.abs(parent - ref).max()), float(np.abs(new - ref).max()), float(np.abs(new - parent).max()))
        print(f"[{dtype}] E_parent {res[dtype][0]:.3e}  E_new {res[dtype][1]:.3e}  max|new - parent| {res[dtype][2]:.3e}  "
              f"(fp32 bound {gb:.3e}, max|ref| {float(np.abs(ref).max()):.3e})")
    assert res["fp32"][2] <= gb and res["fp32"][1] <= gb
    assert res["bf16"][1] <= 2 * res["bf16"][0] + gb


# ------------------------------------------------------------------ library and CLI
def test_dependency_map_equals_row_by_row_target_attribution(nets):
    from codonlm_amd import attribution as A
    cfg, params, m = nets["mha_gelu"]
    rng = np.random.default_rng(12)
    ids = [1] + rng.integers(4, 68, size=18).tolist() + [2]
    n = len(ids) - 1
    out, h0 = _oracle(cfg, params, np.array([ids[:-1]]))
    logp = out["logits"][0].log_softmax(-1)
    tok = params["tok_emb.weight"][ids[:-1]].astype(np.float64)
    ref = np.zeros((n, n))
    tol = np.zeros((n, n))
    ref_gn, tol_gn = np.zeros((n, n)), np.zeros((n, n))
    for t in range(n):
        (g,) = torch.autograd.grad(logp[t, ids[t + 1]], h0, retain_graph=True)
        g = g[0].numpy().astype(np.float64)
        ref[t] = (g * tok).sum(-1)
        tol[t] = 2e-4 * max(1e-3, float(np.abs(g).max())) * np.abs(tok).sum(-1)
        ref_gn[t] = np.sqrt((g * g).sum(-1))
        tol_gn[t] = 2e-4 * max(1e-3, float(np.abs(g).max())) * np.sqrt(cfg.n_embd)
    maps = {bs: A.dependency_map(m, ids, batch_size=bs) for bs in (3, 1, 32)}
    rows = np.stack([A.target_attribution(m, ids, [t])[0] for t in range(n)])
    for tag, got in list(maps.items()) + [("rows", rows)]:
        assert got.shape == (n, n) and got.dtype == np.float32
        assert (np.triu(got, 1) == 0).all(), tag  # strictly upper triangle: exactly 0
        e = np.abs(got - ref)
        print(f"[dependency_map {tag}] max err/bound {float((e / tol).max()):.3f}")
        assert (e <= tol).all(), tag
        assert (np.abs(got - maps[32]) <= 2 * tol).all(), tag
    # explicit classes and the logit mode: row j = the chosen class at the chosen position
    alt = A.target_attribution(m, ids, [5, 5, 12], [9, 40, ids[13]], mode="logit", batch_size=2)
    z = out["logits"][0]
    for j, (t, c) in enumerate(((5, 9), (5, 40), (12, ids[13]))):
        (g,) = torch.autograd.grad(z[t, c], h0, retain_graph=True)
        g = g[0].numpy().astype(np.float64)
        bound = 2e-4 * max(1e-3, float(np.abs(g).max())) * np.abs(tok).sum(-1)
        assert (np.abs(alt[j] - (g * tok).sum(-1)) <= bound).all(), j
    # the other two values of the map, and saliency = the column sums of the map (one seed per target)
    sal = A.saliency(m, [ids], batch_size=4)[0]
    assert (np.abs(sal["gxt"] - ref.sum(0)) <= tol.sum(0)).all()
    gn = A.dependency_map(m, ids, value="gnorm")
    assert (np.triu(gn, 1) == 0).all() and (np.abs(gn - ref_gn) <= tol_gn).all() and float(gn.max()) > 1.0
    with pytest.raises(ValueError, match="block_size"):
        A.dependency_map(m, [1] + [5] * 64 + [2])
    assert A.saliency(m, []) == []


def test_saliency_batches_match_single_sequences(nets):
    from codonlm_amd import attribution as A
    cfg, params, m = nets["gqa_rope_swiglu"]
    rng = np.random.default_rng(31)
    seqs = [[1] + rng.integers(4, 68, size=n - 2).tolist() + [2] for n in (2, 9, 33, 20, 65)]
    seqs[2][12] = 3
    batched = A.saliency(m, seqs, batch_size=3)
    for ids, r in zip(seqs, batched):
        n = len(ids) - 1
        out, h0 = _oracle(cfg, params, np.array([ids[:-1]]))
        lp = out["logits"][0].log_softmax(-1)
        (g,) = torch.autograd.grad(lp[torch.arange(n), torch.tensor(ids[1:])].sum(), h0)
        g = g[0].numpy().astype(np.float64)
        gb = 2e-4 * max(1e-3, float(np.abs(g).max()))
        tok = params["tok_emb.weight"][ids[:-1]].astype(np.float64)
        assert r["gxt"].shape == (n,)
        assert (np.abs(r["gxt"] - (g * tok).sum(-1)) <= gb * np.abs(tok).sum(-1)).all(), len(ids)
        assert (np.abs(r["gnorm"] - np.sqrt((g * g).sum(-1))) <= gb * np.sqrt(cfg.n_embd)).all(), len(ids)


def test_analyze_saliency_cli(tmp_path):
    import csv
    from codonlm_amd import analyze_saliency as C
    from codonlm_amd import attribution as A
    from codonlm_amd import score as S
    from codonlm_amd.score_mutations import load_model
    cfg = O.OracleConfig(vocab_size=68, block_size=64, n_layer=2, n_head=2, n_embd=128, sep_id=3, label_smoothing=0.05)
    params = O.synthetic_params(cfg, seed=7)
    rd = tmp_path / "runs" / "r1"
    (rd / "checkpoints").mkdir(parents=True)
    (rd / "itos.txt").write_text("\n".join(VOCAB) + "\n")
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd["head.weight"] = sd["tok_emb.weight"]
    run_cfg = {"vocab_size": 68, "block_size": 64, "n_layer": 2, "n_head": 2, "n_embd": 128, "dropout": 0.1,
               "sep_mask_enabled": True, "tie_embeddings": True, "label_smoothing": 0.05}
    torch.save({"model": sd, "cfg": run_cfg}, rd / "checkpoints" / "best.pt")
    rng = np.random.default_rng(2)
    X = rng.integers(4, 68, size=(3, 24)).astype(np.int32)
    X[:, 0] = 1
    Y = np.concatenate([X[:, 1:], np.full((3, 1), 2, np.int32)], 1)
    np.savez(rd / "artifacts.npz", val_inputs=X, val_targets=Y)
    ids = X[0].tolist() + [2]
    out = C.main(["--run_dir", str(rd), "--map", str(tmp_path / "maps" / "dep.npy")])
    assert out == rd / "tables" / "saliency.csv"
    with out.open(newline="") as f:
        rows = list(csv.reader(f))
    model, _ = load_model(None, rd, "fp32")
    want = A.saliency(model, [ids], objective="loss")[0]["gxt"]
    assert rows[0] == ["position", "token", "saliency"] and len(rows) == 1 + 24
    for i, row in enumerate(rows[1:]):
        assert row == [str(i), VOCAB[ids[i]], f"{float(want[i]):.6f}"]
    # the oracle's loss gives the same table up to the fp32 bound
    o, h0 = _oracle(cfg, params, X[:1].astype(np.int64), Y[:1].astype(np.int64))
    (g,) = torch.autograd.grad(o["loss"], h0)
    g = g[0].numpy().astype(np.float64)
    tok = params["tok_emb.weight"][X[0]].astype(np.float64)
    bound = 2e-4 * max(1e-3, float(np.abs(g).max())) * np.abs(tok).sum(-1) + 5e-7  # + the %.6f rounding
    assert (np.abs(np.array([float(r[2]) for r in rows[1:]]) - (g * tok).sum(-1)) <= bound).all()
    dep = np.load(tmp_path / "maps" / "dep.npy")
    assert dep.shape == (24, 24) and (np.triu(dep, 1) == 0).all()
    assert np.array_equal(dep, A.dependency_map(model, ids))
    # --dna: BOS + codons + EOS, inputs ids[:-1]
    out2 = C.main(["--run_dir", str(rd), "--dna", "ATGAAACCCGGGTTTTAA"])
    dna_ids = S.dna_to_ids("ATGAAACCCGGGTTTTAA", {t: i for i, t in enumerate(VOCAB)})
    want = A.saliency(model, [dna_ids], objective="loss")[0]["gxt"]
    with out2.open(newline="") as f:
        rows = list(csv.reader(f))
    assert [r[1] for r in rows[1:]] == ["<BOS_CDS>", "ATG", "AAA", "CCC", "GGG", "TTT", "TAA"]
    assert [r[2] for r in rows[1:]] == [f"{float(v):.6f}" for v in want]
