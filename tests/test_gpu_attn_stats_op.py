"""cg_attn_stats against the fp64 numpy restatement of its contract (tests/attention_restatement.py)
on the same dtype-rounded qkv rows.

Tolerances.  The project's fp32 attention bound is 1e-5 absolute on p at unit-variance inputs, so
sum_k |dp| <= 1e-5 per row.  The op keeps P in fp32 for bf16 inputs too (it normalises itself), so
both dtypes get the fp32 bounds: masses, distance bins, max and first 1e-5; MEAN_DIST 1e-5 T (every
|q - k| < T); entropy 1e-5 (1 + ln T) (d(-p ln p) = -(1 + ln p) dp, and the p that matter are above
1/T up to the log's own slack); normalised entropy the same over ln 2, the smallest divisor;
received 1e-5 (1 + reference value).  A ratio above 1 is a finding about the kernel.

Every test needs the MI355X (marker ``gpu``) and calls the C ABI through codonlm_amd.ops.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import attention_restatement as AR

pytestmark = pytest.mark.gpu
DEV = "cuda"
WINDOW = 70
HEADS = [(4, 2, 64), (8, 4, 48), (4, 1, 20), (2, 1, 8)]
TS = (1, 5, 64, 130, 300)
TOK_CLASS = AR.token_classes(AR.ITOS)


def _ops():
    from codonlm_amd import ops
    return ops


def _tol(T):
    t = np.full(AR.NSTAT, 1e-5)
    t[AR.MEAN_DIST] = 1e-5 * T
    t[AR.ENTROPY] = 1e-5 * (1 + math.log(T))
    t[AR.NORM_ENTROPY] = 1e-5 * (1 + math.log(T)) / math.log(2)
    return t


@functools.lru_cache(maxsize=None)
def _inputs(B, T, H, KV, hd, dtype):
    """(qkv rounded to dtype as fp64 numpy, its device copy, tokens, device tokens, segment starts)."""
    qkv = torch.from_numpy(AR.make_qkv(B, T, H, KV, hd)).to(dtype)
    idx = AR.make_tokens(B, T)
    idx_d = torch.from_numpy(idx).to(DEV)
    return qkv.double().numpy(), qkv.to(DEV), idx, idx_d, _ops().segment_starts(idx_d, AR.SEP)


@functools.lru_cache(maxsize=None)
def _reference(B, T, H, KV, hd, dtype, masked):
    """The restatement of one case, computed once and shared (read-only)."""
    q64, _, idx, _, _ = _inputs(B, T, H, KV, hd, dtype)
    return AR.attn_stats(q64, B, T, H, KV, hd, idx=idx, sep_id=AR.SEP if masked else None,
                         window=WINDOW if masked else 0, pad_id=AR.PAD, tok_class=TOK_CLASS)


def _run(B, T, H, KV, hd, dtype, masked, **kw):
    _, qd, _, idx_d, seg = _inputs(B, T, H, KV, hd, dtype)
    kw.setdefault("idx", idx_d)
    kw.setdefault("pad_id", AR.PAD)
    if kw["idx"] is not None:
        kw.setdefault("tok_class", torch.from_numpy(TOK_CLASS).to(DEV))
    r = _ops().attn_stats(qd, seg if masked else None, B, T, H, KV, hd, window=WINDOW if masked else 0, **kw)
    torch.cuda.synchronize()
    return r


def _accs(H):
    return torch.zeros(H, AR.NSTAT, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,KV,hd", HEADS)
@pytest.mark.parametrize("T", TS)
def test_attn_stats_matches_the_restatement(T, H, KV, hd, dtype):
    """Every output, B in {1, 3}, with SEP segments and a 70-key window and with neither.  T = 300
    reaches DIST_64_PLUS, a third q-tile and rows past 256 keys; hd 64 / 48 / 8 in bf16 run the MFMA
    kernel (4, 3 and 1 k-steps), hd 20 and fp32 the vector kernel."""
    tol = _tol(T)
    for B in (1, 3):
        for masked in (True, False):
            ref = _reference(B, T, H, KV, hd, dtype, masked)
            head_acc, n_rows = _accs(H)
            r = _run(B, T, H, KV, hd, dtype, masked, head_acc=head_acc, n_rows=n_rows)
            rows = r.rows.cpu().numpy().astype(np.float64)
            keep = ref["keep"]
            tag = f"attn_stats T{T} B{B} H{H} KV{KV} hd{hd} {dtype} masked{int(masked)}"
            assert np.array_equal(r.nvis.cpu().numpy(), ref["nvis"]), tag
            assert (rows[~np.broadcast_to(keep[:, None, :, None], rows.shape)] == 0).all(), tag
            assert float(n_rows.item()) == ref["n_rows"], tag
            err = np.abs(rows - ref["rows"]).max((0, 1, 2))
            print(tag + ": err/tol " + " ".join(f"{n}={e / t:.3f}" for n, e, t in zip(AR.STATS, err, tol)))
            rec = r.received.cpu().numpy().astype(np.float64)
            rerr = float((np.abs(rec - ref["received"]) / (1e-5 * (1 + ref["received"]))).max())
            print(f"{tag}: received err/tol {rerr:.3f}")
            assert (err <= tol).all(), (tag, dict(zip(AR.STATS, err / tol)))
            assert rerr <= 1.0, tag
            # head_acc: the fp64 sum of the returned fp32 rows
            terms = rows.sum((0, 2))
            scale = np.abs(rows).sum((0, 2))
            assert (np.abs(head_acc.cpu().numpy() - terms) <= 1e-12 * np.maximum(scale, 1e-300)).all(), tag
            # self-checks on the device output alone
            k = keep[:, None, :]
            cls_sum = rows[..., AR.MASS0:AR.MASS0 + 4].sum(-1)
            dist_sum = rows[..., AR.DIST0:AR.DIST0 + 5].sum(-1)
            assert (np.abs(cls_sum - 1)[np.broadcast_to(k, cls_sum.shape)] <= 1e-5).all(), tag
            assert (np.abs(dist_sum - 1)[np.broadcast_to(k, dist_sum.shape)] <= 1e-5).all(), tag
            assert (np.abs(rec.sum(-1) - keep.sum(1)[:, None]) <= 1e-5 * T).all(), tag


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,KV,hd", [(4, 2, 64), (4, 1, 20)])
def test_runs_are_bit_identical_and_launches_accumulate(H, KV, hd, dtype):
    """Two runs give the same bits on every output; the same rows split over two launches (even and
    odd queries by row_keep) accumulate to the one-launch head_acc within 1e-12 relative to the sum of
    |terms|, and to n_rows exactly."""
    B, T = 3, 300
    outs = []
    for _ in range(2):
        head_acc, n_rows = _accs(H)
        r = _run(B, T, H, KV, hd, dtype, True, head_acc=head_acc, n_rows=n_rows)
        outs.append((r.rows, r.nvis, r.received, head_acc, n_rows))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    rows, _, received, one_acc, one_n = outs[0]
    head_acc, n_rows = _accs(H)
    even = (torch.arange(T, device=DEV) % 2 == 0).to(torch.uint8).repeat(B, 1)
    parts = [_run(B, T, H, KV, hd, dtype, True, head_acc=head_acc, n_rows=n_rows, row_keep=k) for k in (even, 1 - even)]
    scale = rows.double().abs().sum((0, 2))
    assert ((head_acc - one_acc).abs() <= 1e-12 * scale.clamp_min(1e-300)).all()
    assert n_rows.item() == one_n.item()
    # the two halves partition the rows and the received mass
    assert torch.equal(parts[0].rows + parts[1].rows, rows)
    assert ((parts[0].received + parts[1].received - received).abs() <= 1e-5 * (1 + received)).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_row_keep_selects_the_stop_codon_queries(dtype):
    B, T, H, KV, hd = 3, 130, 4, 2, 64
    _, _, idx, _, _ = _inputs(B, T, H, KV, hd, dtype)
    stops = np.isin(idx, (5, 6, 7))
    assert stops.sum() > 3
    q64 = _inputs(B, T, H, KV, hd, dtype)[0]
    ref = AR.attn_stats(q64, B, T, H, KV, hd, idx=idx, sep_id=AR.SEP, window=WINDOW, pad_id=AR.PAD,
                        tok_class=TOK_CLASS, row_keep=stops)
    head_acc, n_rows = _accs(H)
    r = _run(B, T, H, KV, hd, dtype, True, head_acc=head_acc, n_rows=n_rows,
             row_keep=torch.from_numpy(stops.astype(np.uint8)).to(DEV))
    rows = r.rows.cpu().numpy().astype(np.float64)
    assert n_rows.item() == ref["n_rows"] == int(stops.sum())
    assert (rows[~np.broadcast_to(stops[:, None, :, None], rows.shape)] == 0).all()
    assert (np.abs(rows - ref["rows"]).max((0, 1, 2)) <= _tol(T)).all()
    rec = r.received.cpu().numpy()
    assert (np.abs(rec - ref["received"]) <= 1e-5 * (1 + ref["received"])).all()
    assert (np.abs(head_acc.cpu().numpy() - ref["head_acc"]) <= _tol(T) * stops.sum()).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_without_token_ids_every_row_is_kept_and_no_class_has_mass(dtype):
    B, T, H, KV, hd = 3, 130, 4, 2, 64
    q64 = _inputs(B, T, H, KV, hd, dtype)[0]
    ref = AR.attn_stats(q64, B, T, H, KV, hd, window=WINDOW)
    head_acc, n_rows = _accs(H)
    _, qd, _, _, _ = _inputs(B, T, H, KV, hd, dtype)
    r = _ops().attn_stats(qd, None, B, T, H, KV, hd, window=WINDOW, head_acc=head_acc, n_rows=n_rows)
    torch.cuda.synchronize()
    rows = r.rows.cpu().numpy().astype(np.float64)
    assert n_rows.item() == B * T
    assert (rows[..., AR.MASS0:AR.MASS0 + 4] == 0).all()
    assert np.array_equal(r.nvis.cpu().numpy(), ref["nvis"])
    assert (np.abs(rows - ref["rows"]).max((0, 1, 2)) <= _tol(T)).all()


def test_refusals_and_the_empty_batch():
    from codonlm_amd import _lib as L
    ops = _ops()
    B, T, H, KV, hd = 2, 5, 4, 2, 8
    qkv = torch.randn(B * T, (H + 2 * KV) * hd, device=DEV)
    idx = torch.randint(4, 20, (B, T), device=DEV)
    cls = torch.from_numpy(TOK_CLASS).to(DEV)
    with pytest.raises(ValueError, match="EINVAL"):
        ops.attn_stats(qkv, None, B, T, H, 3, hd)                       # H % KV != 0
    with pytest.raises(ValueError, match="EINVAL"):
        ops.attn_stats(qkv, None, B, T, H, KV, hd, tok_class=cls)       # tok_class without idx
    with pytest.raises(ValueError, match="EUNSUPPORTED"):
        ops.attn_stats(torch.randn(B * T, (H + 2 * KV) * 65, device=DEV), None, B, T, H, KV, 65)
    with pytest.raises(ValueError, match="EINVAL"):                     # a workspace one double short
        need = int(L.lib.cg_attn_stats_workspace(B, T, H))
        assert need > 0
        ops.attn_stats(qkv, None, B, T, H, KV, hd, workspace=torch.empty(need // 8 - 1, dtype=torch.float64, device=DEV))
    d = L.AttnStatsDesc(dtype=L.CG_F32, qkv=None, ldqkv=(H + 2 * KV) * hd, B=B, T=T, H=H, KV=KV, hd=hd)
    ws = ops.attn_stats_workspace(B, T, H, DEV)
    d.workspace, d.ws_bytes = ws.data_ptr(), ws.numel() * 8
    assert L.lib.cg_attn_stats(ctypes.byref(d), None) == L.CG_EINVAL    # NULL qkv
    # B = 0: CG_OK, nothing written
    head_acc, n_rows = _accs(H)
    r = ops.attn_stats(qkv[:0], None, 0, T, H, KV, hd, idx=idx[:0], head_acc=head_acc, n_rows=n_rows)
    torch.cuda.synchronize()
    assert tuple(r.rows.shape) == (0, H, T, AR.NSTAT) and n_rows.item() == 0 and not head_acc.any()
    assert L.lib.cg_attn_stats_workspace(0, T, H) == 0
    assert ops.attn_stats(qkv, None, B, T, H, KV, hd, idx=idx, tok_class=cls, pad_id=0).rows.isfinite().all()
