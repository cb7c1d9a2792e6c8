"""The inference kernels -- one-token attention over a KV cache (cg_attn_decode), the materialised
attention probabilities (cg_attn_probs) and the decoding segment state (cg_segstate_step) --
against fp64 references, at positions and sequence lengths past the kernels' 256-thread strides.

Every test needs the MI355X (marker ``gpu``) and calls the C ABI through codonlm_amd.ops.
"""
import functools
import math

import pytest
import torch

from oracle import tinygpt_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
B_DEC, TMAX = 3, 1100


def _ops():
    from codonlm_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _decode_inputs(H, KV, hd, dtype):
    """(q [B][H hd + 8], cache [B][Tmax][2 KV hd + 8]) as fp64 values already rounded to `dtype`
    (shared, read-only), and their device copies."""
    g = torch.Generator().manual_seed(H * 100 + KV * 10 + hd)
    q = torch.randn(B_DEC, H * hd + 8, generator=g).to(dtype)
    cache = torch.randn(B_DEC, TMAX, 2 * KV * hd + 8, generator=g).to(dtype)
    return q.double(), cache.double(), q.to(DEV), cache.to(DEV)


def _decode_ref(q, cache, pos, lo, window, H, KV, hd):
    """fp64 softmax over keys lo[b]..pos: K head kvh at column kvh hd, V at KV hd + kvh hd"""
    out = torch.empty(B_DEC, H * hd, dtype=torch.float64)
    for b in range(B_DEC):
        l = lo[b]
        if window > 0:
            l = max(l, pos - window + 1)
        for h in range(H):
            kvh = h // (H // KV)
            k = cache[b, l:pos + 1, kvh * hd:(kvh + 1) * hd]
            v = cache[b, l:pos + 1, (KV + kvh) * hd:(KV + kvh + 1) * hd]
            s = (k @ q[b, h * hd:(h + 1) * hd]) / math.sqrt(hd)
            out[b, h * hd:(h + 1) * hd] = torch.softmax(s, 0) @ v
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_seg", [True, False])
@pytest.mark.parametrize("window", [0, 300])
@pytest.mark.parametrize("pos", [0, 255, 256, 700, 1099])
@pytest.mark.parametrize("H,KV,hd", [(8, 8, 64), (8, 4, 48), (4, 1, 20)])
def test_attn_decode(H, KV, hd, pos, window, with_seg, dtype):
    """cg_attn_decode on a random cache [3][1100][2 KV hd + 8]: positions below, at and past the
    256-thread stride of its score, softmax and value loops (one key, 256, 257, 701 and 1100
    keys), GQA groups of 1 / 2 / 4 query heads with hd 64 / 48 / 20 (4, 5 and 12 key groups in the
    value pass), a 300-key window, per-sequence segment starts (0, 10, pos: the whole prefix, most
    of it, the single key `pos`) or none.  Tolerances are the attention forward's at unit-variance
    inputs: 1e-5 absolute in fp32, 2e-2 in bf16."""
    qr, cr, qd, cd = _decode_inputs(H, KV, hd, dtype)
    lo = [0, min(10, pos), pos] if with_seg else [0, 0, 0]
    seg = torch.tensor(lo, dtype=torch.int32, device=DEV) if with_seg else None
    y = _ops().attn_decode(qd, cd, pos, H, KV, hd, segstate=seg, window=window)
    torch.cuda.synchronize()
    ref = _decode_ref(qr, cr, pos, lo, window, H, KV, hd)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    err = (y.cpu().double() - ref).abs().max().item()
    print(f"attn_decode H{H} KV{KV} hd{hd} pos{pos} w{window} seg{int(with_seg)} {dtype}: err/tol {err / tol:.4f}")
    assert tuple(y.shape) == (B_DEC, H * hd) and y.dtype == dtype
    assert err <= tol, err


def test_attn_decode_errors():
    """Arguments the kernel cannot run are refused before any launch."""
    ops = _ops()
    q = torch.zeros(2, 8 * 65, device=DEV)
    cache = torch.zeros(2, 16, 2 * 8 * 65, device=DEV)
    with pytest.raises(ValueError):
        ops.attn_decode(q, cache, 16, 8, 8, 64)          # pos >= Tmax
    with pytest.raises(ValueError):
        ops.attn_decode(q, cache, 3, 8, 8, 65)           # hd > 64
    with pytest.raises(ValueError):
        ops.attn_decode(q, cache, 3, 8, 3, 64)           # H % KV != 0
    ops.attn_decode(q, cache, 15, 8, 8, 64)               # the last legal position runs


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,KV,hd", [(4, 2, 64), (2, 1, 8)])
def test_attn_probs_long_rows(H, KV, hd, dtype):
    """cg_attn_probs at T = 300 (rows of more than 256 keys: the key loop's second pass), SEP
    segments and a 70-key window, with the LSE of cg_attn_fwd, against an fp64 masked softmax of
    the same (bf16-rounded) q and k: 1e-5 / 2e-2 absolute as test_last_attn_capture, entries
    outside the visible set exactly 0, and (fp32) every row summing to 1 within 1e-4."""
    ops = _ops()
    B, T, window, sep = 2, 300, 70, 3
    g = torch.Generator().manual_seed(T + H + hd)
    N = (H + 2 * KV) * hd
    qkv = torch.randn(B * T, N, generator=g).to(dtype)
    idx = torch.randint(4, 68, (B, T), generator=g)
    idx[0, 40], idx[0, 290], idx[1, 0], idx[1, 257] = sep, sep, sep, sep
    qd = qkv.to(DEV)
    seg = ops.segment_starts(idx.to(DEV), sep)
    _, lse = ops.attn_fwd(qd, seg, B, T, H, KV, hd, window=window)
    for use_seg, use_win in ((True, True), (False, False)):
        if not (use_seg and use_win):
            _, lse = ops.attn_fwd(qd, None, B, T, H, KV, hd)
        got = ops.attn_probs(qd, seg if use_seg else None, lse, B, T, H, KV, hd, window=window if use_win else 0)
        torch.cuda.synchronize()
        x = qkv.double()
        q = x[:, :H * hd].view(B, T, H, hd).transpose(1, 2)
        k = x[:, H * hd:(H + KV) * hd].view(B, T, KV, hd).transpose(1, 2).repeat_interleave(H // KV, 1)
        m = O.attention_mask(idx, sep if use_seg else None, window if use_win else None)[:, None]
        att = ((q @ k.transpose(-2, -1)) / math.sqrt(hd)).masked_fill(~m, float("-inf")).softmax(-1)
        gc = got.cpu().double()
        tol = 1e-5 if dtype == torch.float32 else 2e-2
        err = (gc - att).abs().max().item()
        rs = (gc.sum(-1) - 1).abs().max().item()
        print(f"attn_probs H{H} hd{hd} {dtype} seg{int(use_seg)}: err/tol {err / tol:.4f}, rowsum err/1e-4 {rs / 1e-4:.4f}")
        assert err <= tol, err
        assert torch.all(gc.masked_select(~m.expand_as(gc)) == 0)
        if dtype == torch.float32:
            assert rs <= 1e-4, rs


def test_segstate_step():
    """B = 130 (three 64-thread workgroups, the last ragged): the state takes `pos` exactly where
    the token is the SEP id; sep_id = -1 (no SEP masking) leaves it untouched."""
    ops = _ops()
    B, sep = 130, 3
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(4, 68, (B,), generator=g)
    for b in (0, 63, 64, 100, 127, 128, 129):
        tok[b] = sep
    st0 = torch.randint(0, 50, (B,), generator=g).to(torch.int32)
    st = st0.to(DEV)
    ops.segstate_step(tok.to(DEV), sep, 77, st)
    torch.cuda.synchronize()
    want = torch.where(tok == sep, torch.tensor(77, dtype=torch.int32), st0)
    assert torch.equal(st.cpu(), want)
    ops.segstate_step(tok.to(DEV), 5, 91, st)     # another id: only its own tokens move
    want = torch.where(tok == 5, torch.tensor(91, dtype=torch.int32), want)
    assert torch.equal(st.cpu(), want)
    for none in (-1, None):
        ops.segstate_step(tok.to(DEV), none, 99, st)
        torch.cuda.synchronize()
        assert torch.equal(st.cpu(), want)
