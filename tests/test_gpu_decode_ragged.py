"""Ragged KV-cached decoding: cg_attn_decode_ragged against fp64, and teacher-forced
cg_model_prefill_ragged / cg_model_decode_ragged against the reference's golden logits with every
sequence of the batch at its own position."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_model import DEV, make_model, _idx

pytestmark = pytest.mark.gpu
B_OP = 4


def _ops():
    from codonlm_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _inputs(H, KV, hd, Tmax, dtype):
    """q [B][H hd + 8] and cache [B][Tmax][2 KV hd + 8], rounded to `dtype`: fp64 copies (shared,
    read-only) and device copies."""
    g = torch.Generator().manual_seed(H * 1000 + KV * 100 + hd + Tmax)
    q = torch.randn(B_OP, H * hd + 8, generator=g).to(dtype)
    cache = torch.randn(B_OP, Tmax, 2 * KV * hd + 8, generator=g).to(dtype)
    return q.double(), cache.double(), q.to(DEV), cache.to(DEV)


def _ref(q, cache, pos, lo, window, H, KV, hd):
    out = torch.zeros(B_OP, H * hd, dtype=torch.float64)
    for b in range(B_OP):
        p = pos[b]
        if p < 0:
            continue
        l = lo[b]
        if window > 0:
            l = max(l, p - window + 1)
        for h in range(H):
            kvh = h // (H // KV)
            k = cache[b, l:p + 1, kvh * hd:(kvh + 1) * hd]
            v = cache[b, l:p + 1, (KV + kvh) * hd:(KV + kvh + 1) * hd]
            s = (k @ q[b, h * hd:(h + 1) * hd]) / math.sqrt(hd)
            out[b, h * hd:(h + 1) * hd] = torch.softmax(s, 0) @ v
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_seg,window", [(False, 0), (True, 0), (False, 17), (True, 100)])
@pytest.mark.parametrize("Tmax", [40, 300])
@pytest.mark.parametrize("group", [1, 2, 4])
@pytest.mark.parametrize("hd", [16, 48, 64])
def test_attn_decode_ragged(hd, group, Tmax, with_seg, window, dtype):
    """Positions 0, Tmax-1, an inactive -1 row and a middle position in one launch; hd 16 / 48 / 64
    (2, 6 of 8, 8 lanes per bf16 key row; 4, 12 of 16, 16 per fp32 row), 1 / 2 / 4 query heads per
    kv head, 40 keys (less than one pass of the four waves at hd 16) and 300, with and without
    segment starts and a window.  The inactive row keeps the sentinel it held."""
    KV = 2
    H = KV * group
    qr, cr, qd, cd = _inputs(H, KV, hd, Tmax, dtype)
    pos = [0, Tmax - 1, -1, (2 * Tmax) // 3]
    lo = [0, 7, 3, pos[3] - 1] if with_seg else [0, 0, 0, 0]
    seg = torch.tensor(lo, dtype=torch.int32, device=DEV) if with_seg else None
    y = torch.full((B_OP, H * hd), 7.0, dtype=dtype, device=DEV)
    _ops().attn_decode_ragged(qd, cd, torch.tensor(pos, dtype=torch.int32, device=DEV), H, KV, hd, segstate=seg,
                              window=window, out=y)
    torch.cuda.synchronize()
    ref = _ref(qr, cr, pos, lo, window, H, KV, hd)
    got = y.cpu().double()
    assert torch.all(got[2] == 7.0)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    act = [0, 1, 3]
    err = (got[act] - ref[act]).abs().max().item()
    print(f"attn_decode_ragged hd{hd} g{group} T{Tmax} seg{int(with_seg)} w{window} {dtype}: err/tol {err / tol:.4f}")
    assert err <= tol, err


def test_attn_decode_ragged_refuses_what_it_cannot_run():
    ops = _ops()
    pos = torch.zeros(2, dtype=torch.int32, device=DEV)
    for hd, dtype in ((72, torch.float32), (20, torch.bfloat16), (6, torch.float32)):
        q = torch.zeros(2, 2 * hd, dtype=dtype, device=DEV)
        cache = torch.zeros(2, 16, 4 * hd, dtype=dtype, device=DEV)
        with pytest.raises(ValueError):
            ops.attn_decode_ragged(q, cache, pos, 2, 2, hd)
    q = torch.zeros(2, 64, device=DEV)
    with pytest.raises(ValueError):
        ops.attn_decode_ragged(q, torch.zeros(2, 16, 128, device=DEV), pos, 4, 3, 16)  # H % KV
    out_of_range = torch.tensor([16, -5], dtype=torch.int32, device=DEV)  # both inactive: nothing runs
    y = ops.attn_decode_ragged(q, torch.zeros(2, 16, 128, device=DEV), out_of_range, 4, 4, 16)
    torch.cuda.synchronize()
    assert torch.all(y == 0)


def _teacher_forced(m, cfg, x, window, want_term=False):
    """Sequence b prefilled to 3 + 2b tokens in one ragged prefill, then all decoded together; row
    1 is switched inactive for steps 2 and 3 and then resumes where it stopped.  Yields (b, position, logits row
    [, term row]) for every row the engine produced."""
    B, T = x.shape
    cache = m.engine.new_ragged_kv_cache(B, cfg.block_size)
    lens = [3 + 2 * b for b in range(B)]
    Tp = max(lens)
    idx = x[:, :Tp].clone()
    for b in range(B):
        idx[b, lens[b]:] = 0  # padding, not the SEP id
    lg = cache.prefill(idx, torch.tensor(lens, dtype=torch.int32, device=DEV), window=window, want_term=want_term)
    out = [(b, lens[b] - 1, lg[b].cpu().numpy().copy(), cache.term[b].cpu().numpy().copy() if want_term else None)
           for b in range(B)]
    nxt = list(lens)  # the next row of each sequence
    step = 0
    while any(n < T for n in nxt):
        paused = 1 if step in (2, 3) and B > 1 else -1
        pos = [n if (n < T and b != paused) else -1 for b, n in enumerate(nxt)]
        tok = torch.stack([x[b, min(n, T - 1)] for b, n in enumerate(nxt)]).contiguous()
        before = cache.logits.clone()
        lg = cache.decode(tok, torch.tensor(pos, dtype=torch.int32, device=DEV), want_term=want_term)
        for b, p in enumerate(pos):
            if p >= 0:
                out.append((b, p, lg[b].cpu().numpy().copy(),
                            cache.term[b].cpu().numpy().copy() if want_term else None))
                nxt[b] += 1
            else:
                assert torch.equal(lg[b], before[b])  # an inactive row keeps its logits
        step += 1
    return out


@pytest.mark.parametrize("case", ["mha_gelu_sep", "gqa_rope_swiglu_w", "untied_causal", "hd48_gqa", "window8"])
def test_ragged_decode_matches_reference_logits(case):
    cfgd, g = load_golden(case)
    m, cfg, _ = make_model(cfgd, g)
    m.eval()
    x, _ = _idx(g)
    ref = g["logits"]
    scale = max(1.0, float(np.abs(ref).max()))
    rows = _teacher_forced(m, cfg, x, 8 if case == "window8" else None)
    B, T = x.shape
    assert len(rows) == sum(T - (3 + 2 * b) + 1 for b in range(B))
    worst = max(float(np.abs(lg - ref[b, p]).max()) for b, p, lg, _ in rows)
    print(f"[{case}] ragged decode: {len(rows)} rows, max |dlogit| {worst:.2e} (bound {1e-4 * scale:.2e})")
    assert worst <= 1e-4 * scale, (worst, scale)


def test_ragged_decode_bf16_close_to_full_forward():
    cfgd, g = load_golden("mha_gelu_sep")
    m, cfg, _ = make_model(cfgd, g, dtype="bf16")
    m.eval()
    x, _ = _idx(g)
    with torch.no_grad():
        full, _ = m(x)
    full = full.float().cpu().numpy()
    rows = _teacher_forced(m, cfg, x, None)
    worst = max(float(np.abs(lg - full[b, p]).max()) for b, p, lg, _ in rows)
    assert worst <= 3e-2 * max(1.0, float(np.abs(full).max())), worst


def test_ragged_decode_termination_logits():
    cfgd, g = load_golden("aux_heads")
    m, cfg, _ = make_model(cfgd, g)
    m.eval()
    x, _ = _idx(g)
    rows = _teacher_forced(m, cfg, x, None, want_term=True)
    ref, tref = g["logits"], g["termination_logits"]
    scale = max(1.0, float(np.abs(ref).max()))
    assert max(float(np.abs(lg - ref[b, p]).max()) for b, p, lg, _ in rows) <= 1e-4 * scale
    for b, p, _, tl in rows:  # the bound of tests/test_gpu_aux.py
        np.testing.assert_allclose(tl, tref[b, p], rtol=1e-4, atol=1e-4)
