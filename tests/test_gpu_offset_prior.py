"""Multi-offset priors in batched generation: cg_offset_prior_add against fp64, the ln_f history
the ragged cache keeps (cg_model_prefill_hist / cg_model_decode_ragged_hist), and
generate_cds_constrained with priors replayed under teacher forcing.

Tolerances.  The op: what tests/test_gpu_aux.py asks of ``offset_logits`` -- 1e-4 of
max(1, |offset logit|max) in fp32 -- times sum |w_i|; in bf16 that file bounds the heads only through
the objective (2e-2 relative), and 2e-2 of the same scale is used here: three chained products with
bf16 operands (2^-9 relative rounding each, twice more for the stored u1 and u2) stay well
below it at d <= 98 (measured: 0.4 % of the scale).  The fp64 expectation is computed from the
model's fp32 parameters and the history rows read back from the device, never from the code under
test.

End to end (the method of tests/test_gpu_generate.py): one full forward with return_aux of every
finished sequence, row r's logits + sum_k w_k offset_logits[k][r + 1 - k] over the heads with
r + 1 - k >= 0 in dict order, replayed by the fp64 sampler restatement.  A draw is exempt by the
existing rule with delta' = delta (1 + sum |w_k|), delta = max(1e-4, 5e-6 |.|max) over base and
offset logits.  Weights {2: 0.5, 4: 0.25} and seed 77: the restated sampler run autoregressively
on the CPU oracle's forward gives 113 draws / 3 exempt without and 68 / 1 with the termination
bias, and a prior above 8 delta' on every step with ctx_len >= 2."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sampler_restatement as R
from conftest import load_golden
from oracle import tinygpt_oracle as O
from test_gpu_generate import BIAS, CONTEXTS, HARD_CAP, SEED, TARGET, _expected_info, _model, _params
from test_gpu_model import DEV, make_model

pytestmark = pytest.mark.gpu
LDL = 80
WEIGHTS = {2: 0.5, 4: 0.25}
WIDE_OFFSETS = [1, 2, 3, 5, 8, 13, 21, 31]
# (head index into cfg.offsets, weight) in call order: unsorted, with a zero weight
PRIORS = {"aux": [(1, 0.75), (0, -0.5)], "untied": [(6, -1.0), (1, 0.5)], "odd": [(4, 1.0), (1, -0.5), (0, 0.25)],
          "wide": [(3, 0.5), (0, -0.25), (7, 1.0), (2, 0.0), (5, 0.75), (1, 0.3), (6, -0.6), (4, 0.2)]}


def _lib():
    from codonlm_amd import _lib as L
    return L


@functools.lru_cache(maxsize=None)
def _op_model(kind, dtype):
    if kind == "aux":
        cfgd, g = load_golden("aux_heads")
    else:  # d = 96 = 2 heads x 48: 24 elements per wave, less than the 32 a lane holds at a time;
        # "odd": d = 98, rows off the 16-byte boundaries, so every load is element-wise
        cfgd = dict(vocab_size=68, block_size=32, n_layer=1, n_head=2, n_embd=98 if kind == "odd" else 96,
                    n_kv_head=None, dropout=0.0, label_smoothing=0.0, sep_id=3, tie_embeddings=kind != "untied",
                    use_swiglu=False, use_rope=False,
                    loss_weights=None, termination_aux=False, termination_n_classes=5,
                    multi_offset_targets=WIDE_OFFSETS)
        g = {"param_seed": np.array(5)}
    m, cfg, params = make_model(cfgd, g, dtype=dtype)
    rng = np.random.default_rng(11)
    for k in cfg.multi_offset_targets:  # random offset MLPs (the constructor's are the identity)
        for name in (f"offset_projs.{k}.0.weight", f"offset_projs.{k}.2.weight"):
            params[name] = (rng.standard_normal(params[name].shape) / np.sqrt(cfg.n_embd)).astype(np.float32)
        for name in (f"offset_projs.{k}.0.bias", f"offset_projs.{k}.2.bias"):
            params[name] = (0.3 * rng.standard_normal(params[name].shape)).astype(np.float32)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items() if k.startswith("offset_projs.")},
                      strict=False)
    m.eval()
    return m, cfg, params


def _prior(pairs):
    p = _lib().OffsetPrior()
    p.n = len(pairs)
    for i, (h, w) in enumerate(pairs):
        p.head[i], p.weight[i] = h, w
    return p


def _add(m, cache, pos, prior, logits):
    L = _lib()
    m.engine.sync_shadow()
    L.check(L.lib.cg_offset_prior_add(C.byref(m.engine.model), C.byref(prior), cache.hist.data_ptr(), cache.Tmax,
                                      pos.data_ptr(), cache.B, logits.data_ptr(), logits.stride(0),
                                      cache.prior_ws.data_ptr(), cache.prior_ws.numel(), L.stream_ptr(logits.device)),
            "cg_offset_prior_add")
    torch.cuda.synchronize()


def _head_logits64(params, k, x):
    """head(W2 gelu(W1 x + b1) + b2) of offset k in fp64 (erf GELU, tied head)."""
    p = {n: torch.from_numpy(np.asarray(params[f"offset_projs.{k}.{n}"], dtype=np.float64))
         for n in ("0.weight", "0.bias", "2.weight", "2.bias")}
    u = p["0.weight"] @ x + p["0.bias"]
    u = 0.5 * u * (1.0 + torch.erf(u / np.sqrt(2.0)))
    u = p["2.weight"] @ u + p["2.bias"]
    head = params["head.weight"] if "head.weight" in params else params["tok_emb.weight"]  # untied / tied
    return torch.from_numpy(np.asarray(head, dtype=np.float64)) @ u


@functools.lru_cache(maxsize=None)
def _op_case(kind, dtype, big=False):
    """One B = 7 call (``big``: B = 70, two 64-row tiles) and one B = 1 call per row (``big``: of
    the rows around the tile edge), shared by the op tests: (pos, logits before, logits after,
    per-row single-call results, expected fp64, applicable mask, head scale)."""
    m, cfg, params = _op_model(kind, dtype)
    Tmax = cfg.block_size
    pos_l = [(7 * b) % (Tmax + 2) - 1 for b in range(70)] if big else [-1, 0, 1, 3, 12, Tmax - 1, Tmax]
    B = len(pos_l)
    offs = list(cfg.multi_offset_targets)
    pairs = PRIORS[kind]
    gen = torch.Generator().manual_seed(3)
    cache = m.engine.new_ragged_kv_cache(B, Tmax, xf_history=True)
    cache.hist.copy_(torch.randn(B, Tmax, cfg.n_embd, generator=gen).to(cache.hist.dtype))
    before = torch.randn(B, LDL, generator=gen).to(DEV)
    logits = before.clone()
    pos = torch.tensor(pos_l, dtype=torch.int32, device=DEV)
    _add(m, cache, pos, _prior(pairs), logits)
    hist = cache.hist.cpu().double()
    want = before.cpu().double()[:, :cfg.vocab_size].clone()
    applies = np.zeros(B, dtype=bool)
    scale = 1.0
    for b, p in enumerate(pos_l):
        if not 0 <= p < Tmax:
            continue
        for h, w in pairs:
            src = p + 1 - offs[h]
            if w == 0.0 or src < 0:
                continue
            hl = _head_logits64(params, offs[h], hist[b, src])
            scale = max(scale, float(hl.abs().max()))
            want[b] += w * hl
            applies[b] = True
    single = {}
    for b in np.nonzero(applies)[0]:
        if big and b not in (0, 1, 62, 63, 64, 65, 69):
            continue
        c1 = m.engine.new_ragged_kv_cache(1, Tmax, xf_history=True)
        c1.hist.copy_(cache.hist[b:b + 1])
        l1 = before[b:b + 1].clone()
        _add(m, c1, pos[b:b + 1].clone(), _prior(pairs), l1)
        single[int(b)] = l1.cpu()
    return pos_l, before.cpu(), logits.cpu(), single, want, applies, scale


@pytest.mark.parametrize("kind,dtype", [("aux", "fp32"), ("aux", "bf16"), ("wide", "fp32"), ("wide", "bf16"),
                                        ("untied", "fp32"), ("odd", "fp32"), ("odd", "bf16")])
def test_offset_prior_add_against_fp64(kind, dtype):
    pos_l, before, after, single, want, applies, scale = _op_case(kind, dtype)
    V = want.shape[1]
    sum_w = sum(abs(w) for _, w in PRIORS[kind])
    tol = (1e-4 if dtype == "fp32" else 2e-2) * scale * sum_w
    assert applies.sum() >= 4 and not applies[0] and not applies[-1]
    if kind == "aux":
        assert not applies[1]  # pos 0: no head reaches back that far
    err = float((after[applies, :V].double() - want[applies]).abs().max())
    print(f"[offset_prior {kind} {dtype}] err {err:.3e} tol {tol:.3e} (|head logit|max {scale:.2f})")
    assert err <= tol, (err, tol)
    # B = 1: every applicable row alone, against the same expectation
    for b, l1 in single.items():
        assert float((l1[0, :V].double() - want[b]).abs().max()) <= tol, b
        assert torch.equal(l1[0, V:], before[b, V:])
    # untouched: inactive rows, rows no head applies to, and the columns V .. ldl of every row
    assert torch.equal(after[~applies], before[~applies])
    assert torch.equal(after[:, V:], before[:, V:])
    assert not torch.equal(after[applies, :V], before[applies, :V])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["aux", "wide"])
def test_a_row_is_bitwise_the_same_alone_and_in_the_batch(kind, dtype):
    _, _, after, single, _, applies, _ = _op_case(kind, dtype)
    assert len(single) == applies.sum()
    for b, l1 in single.items():
        assert torch.equal(l1[0], after[b]), b


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_row_tiles(dtype):
    """B = 70: the second 64-row tile holds 6 rows; every row against fp64, and the rows on both
    sides of the tile edge bitwise equal to themselves alone."""
    pos_l, before, after, single, want, applies, scale = _op_case("wide", dtype, True)
    V = want.shape[1]
    tol = (1e-4 if dtype == "fp32" else 2e-2) * scale * sum(abs(w) for _, w in PRIORS["wide"])
    assert applies[64:].sum() >= 4 and (~applies).sum() >= 2 and len(single) >= 5
    assert float((after[applies, :V].double() - want[applies]).abs().max()) <= tol
    assert torch.equal(after[~applies], before[~applies]) and torch.equal(after[:, V:], before[:, V:])
    for b, l1 in single.items():
        assert torch.equal(l1[0], after[b]), b


def test_no_heads_is_no_launch_and_bad_workspace_is_refused():
    m, cfg, _ = _op_model("aux", "fp32")
    L = _lib()
    cache = m.engine.new_ragged_kv_cache(2, 64, xf_history=True)
    logits = torch.randn(2, LDL).to(DEV)
    keep = logits.clone()
    pos = torch.tensor([5, 9], dtype=torch.int32, device=DEV)
    _add(m, cache, pos, _prior([]), logits)
    assert torch.equal(logits, keep)
    p = _prior([(0, 1.0)])
    assert L.lib.cg_offset_prior_add(C.byref(m.engine.model), C.byref(p), cache.hist.data_ptr(), 64, pos.data_ptr(),
                                     2, logits.data_ptr(), LDL, cache.prior_ws.data_ptr(),
                                     cache.prior_ws.numel() - 1, L.stream_ptr(logits.device)) == L.CG_EINVAL
    plain = m.engine.new_ragged_kv_cache(2, 64)
    assert plain.hist is None
    with pytest.raises(ValueError, match="xf_history"):
        plain.add_offset_priors(pos, {2: 1.0})
    # the dict form: order kept, zero weights and offsets without a head dropped
    q = cache.offset_prior({4: 0.5, 3: 1.0, 2: 0.0})
    assert (q.n, q.head[0], q.weight[0]) == (1, 1, 0.5)
    assert cache.offset_prior(None).n == 0 and cache.offset_prior({}).n == 0


def test_history_after_prefill_and_decode():
    """Ragged prefill (lengths 1, 4, 9), five decode steps with sequence 1 inactive: hist holds the
    ln_f rows of a full forward of each finished sequence, a sentinel everywhere else, and the
    logits of every step are bitwise those of a cache without the history."""
    m, cfg, _ = _op_model("aux", "fp32")
    eng = m.engine
    lens = [1, 4, 9]
    B, Tmax, T, steps = 3, cfg.block_size, 9, 5
    rng = np.random.default_rng(21)
    seqs = [list(rng.integers(4, 68, size=n + steps)) for n in lens]
    idx = np.full((B, T), 5, dtype=np.int64)
    for b, n in enumerate(lens):
        idx[b, :n] = seqs[b][:n]
    cache = eng.new_ragged_kv_cache(B, Tmax, xf_history=True)
    plain = eng.new_ragged_kv_cache(B, Tmax)
    cache.hist.fill_(7.0)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    x = torch.from_numpy(idx).to(DEV)
    a = cache.prefill(x, lens_t).clone()
    b_ = plain.prefill(x, lens_t).clone()
    assert torch.equal(a, b_)
    for s in range(steps):
        pos = torch.tensor([lens[0] + s, -1, lens[2] + s], dtype=torch.int32, device=DEV)
        tok = torch.tensor([seqs[0][lens[0] + s], 9, seqs[2][lens[2] + s]], dtype=torch.int64, device=DEV)
        a = cache.decode(tok, pos).clone()
        b_ = plain.decode(tok, pos).clone()
        assert torch.equal(a, b_), s
    hist = cache.hist.cpu().numpy()
    filled = [lens[0] + steps, lens[1], lens[2] + steps]
    for b in range(B):
        ids = seqs[b][:filled[b]]
        with torch.no_grad():
            m(torch.tensor([ids], dtype=torch.long, device=DEV))
        ref = eng.hidden(cfg.n_layer + 1)[0].float().cpu().numpy()
        assert ref.shape == (filled[b], cfg.n_embd)
        bound = max(1e-4, 5e-6 * float(np.abs(ref).max()))
        err = float(np.abs(hist[b, :filled[b]] - ref).max())
        print(f"[hist] sequence {b}: {filled[b]} rows, err {err:.2e} (bound {bound:.2e})")
        assert err <= bound, (b, err)
        assert np.all(hist[b, filled[b]:] == 7.0), b


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _gen():
    from codonlm_amd import generate
    return generate


def _kw(bias):
    kw = dict(termination_bias_enabled=False, termination_stop_bias=0.0, termination_trigger_class_max=0,
              termination_bias_window=0)
    kw.update(bias or {})
    return kw


def _run(m, weights, bias=None, contexts=CONTEXTS, streams=None, enabled=True, mode="constrained_req"):
    return _gen()._constrained_batch(m, contexts, R.STOI, R.ITOS, TARGET, HARD_CAP,
                                     require_terminal_stop=mode == "constrained_req", temperature=1.0, topk=0,
                                     cds_only=True, seed=SEED, streams=streams or list(range(len(contexts))),
                                     multi_offset_prior_enabled=enabled, multi_offset_prior_weights=weights,
                                     **_kw(bias))


def _with_component(info):
    comps = list(info["guidance_components"])
    comps.insert(1 if comps[:1] == ["termination_bias"] else 0, "multi_offset_prior")
    return dict(info, guidance_components=comps, protocol="guided")


def _replay(m, P, ctx, ids, stream, weights, want_term):
    x = torch.tensor([ids], dtype=torch.long, device=DEV)
    with torch.no_grad():
        logits, _, aux = m(x, return_aux=True)
    logits = logits[0].cpu().numpy().astype(np.float64)
    term = aux["termination_logits"][0].float().cpu().numpy() if want_term else None
    off = {k: aux["offset_logits"][k][0].float().cpu().numpy().astype(np.float64) for k in weights}
    delta = max(1e-4, 5e-6 * max(float(np.abs(logits).max()), max(float(np.abs(v).max()) for v in off.values())))
    delta *= 1.0 + sum(abs(w) for w in weights.values())
    temp = max(1e-6, float(np.float32(P["temperature"])))
    st = R.new_state(len(ctx), stream)
    exempt, big, steps2 = [], 0, 0
    n = len(ids) - len(ctx)
    for i in range(n):
        assert not st["flags"] & R.DONE, "tokens after the sequence was done"
        r = len(ctx) + i - 1
        prior = np.zeros(logits.shape[1])
        for k, w in weights.items():
            if r + 1 - k >= 0:
                prior = prior + w * off[k][r + 1 - k]
        if r + 1 >= 2:
            steps2 += 1
            big += float(np.abs(prior).max()) > 8 * delta
        tok, boundary, gap = R.sample_token(P, logits[r] + prior, None if term is None else term[r], st)
        if boundary <= 4 * delta / temp or gap < 4 * delta:
            exempt.append(i)
        else:
            assert ids[len(ctx) + i] == tok, (stream, i, ids[len(ctx) + i], tok, boundary)
        R.advance(P, ids[len(ctx) + i], st)
    assert st["flags"] & R.DONE, "the sequence ended before a stop rule fired"
    return st, exempt, n, big, steps2


@functools.lru_cache(maxsize=None)
def _verified(with_bias):
    m = _model("aux_heads")
    bias = BIAS if with_bias else None
    res = _run(m, WEIGHTS, bias)
    P = _params("constrained_req", 1.0, 0, SEED, bias)
    draws = n_exempt = big = steps2 = 0
    exempt_at = []
    for b, (ids, info) in enumerate(res):
        assert ids[:len(CONTEXTS[b])] == CONTEXTS[b]
        st, exempt, n, bg, s2 = _replay(m, P, CONTEXTS[b], ids, b, WEIGHTS, with_bias)
        assert info == _with_component(_expected_info("constrained_req", st, bias)), (b, info, st)
        draws, n_exempt, big, steps2 = draws + n, n_exempt + len(exempt), big + bg, steps2 + s2
        exempt_at.append(exempt[0] if exempt else None)
    print(f"[priors bias={with_bias}] {draws} draws, {n_exempt} exempt, prior > 8 delta' on {big}/{steps2} steps, "
          f"codons {[i['generated_codons'] for _, i in res]}")
    assert n_exempt <= 0.12 * draws, (n_exempt, draws)
    assert steps2 > 0 and 2 * big >= steps2, (big, steps2)
    return res, exempt_at


@pytest.mark.parametrize("with_bias", [False, True])
def test_generation_with_priors_replays_under_teacher_forcing(with_bias):
    res, _ = _verified(with_bias)
    for _, info in res:
        assert "multi_offset_prior" in info["guidance_components"] and info["protocol"] == "guided"
        assert ("termination_bias" in info["guidance_components"]) == with_bias


def test_degenerate_weights_leave_the_run_unguided():
    m = _model("aux_heads")
    base = _run(m, None, enabled=False)
    assert all("multi_offset_prior" not in i["guidance_components"] for _, i in base)
    want = [(ids, _with_component(info)) for ids, info in base]
    for weights in (None, {}, {2: 0.0}, {3: 1.0}):
        assert _run(m, weights) == want, weights
    changed = _run(m, {2: 1.0, 4: 1.0})
    assert [ids for ids, _ in changed] != [ids for ids, _ in base]


def test_a_sequence_alone_equals_its_stream_in_the_batch_with_priors():
    m = _model("aux_heads")
    res, exempt_at = _verified(False)
    G = _gen()
    for b in (0, 3, 5):
        (ids, info), = _run(m, WEIGHTS, contexts=[CONTEXTS[b]], streams=[b])
        n = len(CONTEXTS[b]) + (exempt_at[b] if exempt_at[b] is not None else 10 ** 6)
        assert ids[:n] == res[b][0][:n], b
        if exempt_at[b] is None:
            assert info == res[b][1]
        # the drop-in function is that batch of one
        ids2, info2 = G.generate_cds_constrained(m, torch.device(DEV), CONTEXTS[b], R.STOI, R.ITOS, TARGET, HARD_CAP,
                                                 require_terminal_stop=True, cds_only=True,
                                                 multi_offset_prior_enabled=True, multi_offset_prior_weights=WEIGHTS,
                                                 seed=SEED, stream=b)
        assert (ids2, info2) == (ids, info)


def test_model_without_offset_heads_is_refused():
    m = _model("mha_gelu_sep")
    with pytest.raises(NotImplementedError):
        _run(m, WEIGHTS)
