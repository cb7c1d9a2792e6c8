"""LayerNorm forward and backward at every width the dispatcher treats differently, against fp64
torch: the vector instances 128 / 256 / 768 / 1024, the widths 640 and 896 that pass the width
test and then leave the instance switch for the scalar kernel, the scalar kernel's extremes 1 and
2048, mean / rstd themselves, bf16 and fp32 dy, a g_out that is 8-B but not 16-B aligned (W = 4
drops to W = 2), strided views, and more rows than the backward's 1024 blocks x 32 rows.

Every test needs the MI355X (marker ``gpu``) and calls the C ABI through codonlm_amd.ops / _lib.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tinygpt_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
WIDTHS = [128, 256, 768, 1024, 640, 896, 1, 2048]


def _mods():
    from codonlm_amd import _lib, ops
    return ops, _lib


@functools.lru_cache(maxsize=None)
def _case(rows, cols):
    """Inputs and the fp64 forward / backward of one shape, computed once and shared (read-only).
    dy is held bf16-exact so the bf16 and fp32 dy runs share one reference."""
    g = torch.Generator().manual_seed(rows * 3 + cols)
    x = torch.randn(rows, cols, generator=g) * 3 + 1
    w = 1 + 0.1 * torch.randn(cols, generator=g)
    b = 0.1 * torch.randn(cols, generator=g)
    dy = torch.randn(rows, cols, generator=g).to(torch.bfloat16).float()
    gin = torch.randn(rows, cols, generator=g)
    xd = x.double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.layer_norm(xd, (cols,), wd, bd, EPS)
    y.backward(dy.double())
    mean = x.double().mean(1)
    var = x.double().var(1, unbiased=False)
    rstd = (var + EPS).rsqrt()
    xhat = (x.double() - mean[:, None]) * rstd[:, None]
    return dict(x=x, w=w, b=b, dy=dy, gin=gin, y=y.detach(), mean=mean, rstd=rstd,
                gx=xd.grad + gin.double(), dgamma=wd.grad, dbeta=bd.grad,
                dgamma_abs=(dy.double() * xhat).abs().sum(0), dbeta_abs=dy.double().abs().sum(0))


def _fwd_check(c, y, mean, rstd, tag):
    """mean: 1e-5 (1 + |mean|); rstd: 1e-5 relative (rsqrtf's 2 ulp and an fp32 sum of <= 2048
    terms, with a x10 margin); y: 4e-5 (+ 2^-8 |ref| in bf16)."""
    r_mean = ((mean.cpu().double() - c["mean"]).abs() / (1e-5 * (1 + c["mean"].abs()))).max().item()
    r_rstd = ((rstd.cpu().double() - c["rstd"]).abs() / (1e-5 * c["rstd"])).max().item()
    bound = 4e-5 + (2.0 ** -8 * c["y"].abs() if y.dtype == torch.bfloat16 else 0.0)
    r_y = ((y.cpu().double() - c["y"]).abs() / bound).max().item()
    print(f"ln fwd {tag}: err/bound mean {r_mean:.4f} rstd {r_rstd:.4f} y {r_y:.4f}")
    assert r_mean <= 1.0, r_mean
    assert r_rstd <= 1.0, r_rstd
    assert r_y <= 1.0, r_y


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows", [3, 37])
@pytest.mark.parametrize("cols", WIDTHS)
def test_layernorm_fwd_widths(cols, rows, out_dtype):
    """rows 3: fewer rows than one workgroup's; 37: a ragged last group of the 4-rows-per-wave
    prefetching kernel (W = 2 widths) and of the 4-row workgroups."""
    ops, _ = _mods()
    c = _case(rows, cols)
    y, mean, rstd = ops.layernorm_fwd(c["x"].to(DEV), c["w"].to(DEV), c["b"].to(DEV), out_dtype=out_dtype)
    torch.cuda.synchronize()
    _fwd_check(c, y, mean, rstd, f"cols={cols} rows={rows} {out_dtype}")


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cols", [256, 384, 100])
def test_layernorm_fwd_strided_views(cols, out_dtype):
    """x and y as column slices of wider buffers (ldx, ldy > cols; W = 4, W = 2 and the scalar
    kernel): the values, and the columns of the y buffer outside the slice untouched."""
    _, L = _mods()
    rows = 37
    c = _case(rows, cols)
    xb = torch.zeros(rows, cols + 8, device=DEV)
    xb[:, 4:4 + cols] = c["x"].to(DEV)
    x = xb[:, 4:4 + cols]
    yb = torch.full((rows, cols + 16), 7.0, dtype=out_dtype, device=DEV)
    y = yb[:, 8:8 + cols]
    mean = torch.empty(rows, device=DEV)
    rstd = torch.empty(rows, device=DEV)
    w, b = c["w"].to(DEV), c["b"].to(DEV)
    L.check(L.lib.cg_layernorm_fwd(L.CG_BF16 if out_dtype == torch.bfloat16 else L.CG_F32, x.data_ptr(), x.stride(0),
                                   w.data_ptr(), b.data_ptr(), y.data_ptr(), y.stride(0), mean.data_ptr(),
                                   rstd.data_ptr(), rows, cols, EPS, L.stream_ptr(DEV)), "cg_layernorm_fwd")
    torch.cuda.synchronize()
    _fwd_check(c, y, mean, rstd, f"views cols={cols} {out_dtype}")
    assert torch.all(yb[:, :8] == 7.0) and torch.all(yb[:, 8 + cols:] == 7.0)


def _bwd(L, c, rows, cols, dy_dtype, *, misalign=False, branch_dtype=None, seed=0, p=0.0):
    """cg_layernorm_bwd with mean / rstd from the fp64 reference rounded to fp32 -> (g_out, dgamma,
    dbeta, branch, colsum).  misalign: g_out starts 8 B past a 16-B boundary."""
    dev = lambda t: t.to(DEV)
    x, w, gin = dev(c["x"]), dev(c["w"]), dev(c["gin"])
    dy = dev(c["dy"]).to(dy_dtype)
    mean, rstd = dev(c["mean"].float()), dev(c["rstd"].float())
    gbuf = torch.empty(rows * cols + 4, device=DEV)
    off = 2 if misalign else 0
    g_out = gbuf[off:off + rows * cols].view(rows, cols)
    assert g_out.data_ptr() % 16 == (8 if misalign else 0)
    nbytes = int(L.lib.cg_layernorm_bwd_workspace(rows, cols, 1))
    part = torch.empty(nbytes // 4, device=DEV)
    dgamma = torch.empty(cols, device=DEV)
    dbeta = torch.empty(cols, device=DEV)
    branch = colsum = None
    if branch_dtype is not None:
        branch = torch.empty(rows, cols, dtype=branch_dtype, device=DEV)
        colsum = torch.empty(cols, device=DEV)
    cdt = lambda t: L.CG_BF16 if t == torch.bfloat16 else L.CG_F32
    L.check(L.lib.cg_layernorm_bwd(cdt(dy_dtype), dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0),
                                   mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), gin.data_ptr(), g_out.data_ptr(),
                                   cdt(branch_dtype), None if branch is None else branch.data_ptr(), seed, p,
                                   part.data_ptr(), nbytes, dgamma.data_ptr(), dbeta.data_ptr(),
                                   None if colsum is None else colsum.data_ptr(), 0, rows, cols, EPS,
                                   L.stream_ptr(DEV)), "cg_layernorm_bwd")
    torch.cuda.synchronize()
    return g_out, dgamma, dbeta, branch, colsum


def _bwd_check(c, g_out, dgamma, dbeta, tag):
    """g_out within 1e-4; dgamma / dbeta within 2e-5 sum_rows |term| per column, plus 1e-9 for the
    fp64 reference's own rounding (at cols = 1 every xhat is exactly 0, the kernel's dgamma is
    exactly 0, and autograd's fp64 xhat leaves 4e-13)."""
    r_g = ((g_out.cpu().double() - c["gx"]).abs() / 1e-4).max().item()
    r_dg = ((dgamma.cpu().double() - c["dgamma"]).abs() / (2e-5 * c["dgamma_abs"] + 1e-9)).max().item()
    r_db = ((dbeta.cpu().double() - c["dbeta"]).abs() / (2e-5 * c["dbeta_abs"] + 1e-9)).max().item()
    print(f"ln bwd {tag}: err/bound g_out {r_g:.4f} dgamma {r_dg:.4f} dbeta {r_db:.4f}")
    assert r_g <= 1.0, r_g
    assert r_dg <= 1.0, r_dg
    assert r_db <= 1.0, r_db


@pytest.mark.parametrize("dy_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("cols", WIDTHS)
def test_layernorm_bwd_widths(cols, dy_dtype):
    """cg_layernorm_bwd (row pass + in-call parameter reduction) with g_in, against fp64 autograd of
    the same (bf16-exact) dy, and the deferred route -- cg_layernorm_bwd_partials +
    cg_reduce_columns -- under the same bounds.  37 rows: two blocks, the second with 5 rows."""
    ops, L = _mods()
    rows = 37
    c = _case(rows, cols)
    g_out, dgamma, dbeta, _, _ = _bwd(L, c, rows, cols, dy_dtype)
    _bwd_check(c, g_out, dgamma, dbeta, f"cols={cols} {dy_dtype}")
    dev = lambda t: t.to(DEV)
    go_p, part, _ = ops.layernorm_bwd_partials(dev(c["dy"]).to(dy_dtype), dev(c["x"]), dev(c["mean"].float()),
                                               dev(c["rstd"].float()), dev(c["w"]), g_in=dev(c["gin"]))
    dg2, db2 = torch.empty(cols, device=DEV), torch.empty(cols, device=DEV)
    ops.reduce_columns([(part[:, :cols], dg2, 0), (part[:, cols:], db2, 0)])
    torch.cuda.synchronize()
    assert torch.equal(go_p, g_out)
    _bwd_check(c, go_p, dg2, db2, f"partials cols={cols} {dy_dtype}")


@pytest.mark.parametrize("branch_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("cols", [256, 1024, 640, 100])
def test_layernorm_bwd_branch_and_misaligned_g_out(cols, branch_dtype):
    """The dropout-masked consumer-branch copy and its column sum at W = 4 widths, a switch
    fall-out width and a scalar width, with g_out 16-B aligned and at an 8-B offset (W = 4 -> 2;
    the lanes then own other columns, so the row sums round differently: the same bounds, not
    the same bits).  Branch: kept elements g_out / (1 - p) within 1e-4 / (1 - p) (g_out's bound
    scaled) + 2^-8 |ref| in bf16 -- never looser than test_layernorm_fwd_bwd's 4 tol + 1e-4 --
    dropped ones exactly 0; its column sum (summed before the bf16 rounding) within
    2e-5 sum_rows |term|."""
    _, L = _mods()
    rows, p, seed = 37, 0.2, 777
    c = _case(rows, cols)
    keep = torch.from_numpy(O.dropout_keep(seed, np.arange(rows)[:, None], np.arange(cols)[None, :], p))
    ref_b = torch.where(keep, c["gx"] / (1 - p), torch.zeros((), dtype=torch.float64))
    for misalign in (False, True):
        g_out, dgamma, dbeta, br, cs = _bwd(L, c, rows, cols, torch.bfloat16, misalign=misalign,
                                            branch_dtype=branch_dtype, seed=seed, p=p)
        tag = f"branch cols={cols} {branch_dtype} misalign={int(misalign)}"
        _bwd_check(c, g_out, dgamma, dbeta, tag)
        bound = 1e-4 / (1 - p) + (2.0 ** -8 * ref_b.abs() if branch_dtype == torch.bfloat16 else 0.0)
        r_b = ((br.cpu().double() - ref_b).abs() / bound).max().item()
        r_c = ((cs.cpu().double() - ref_b.sum(0)).abs() / (2e-5 * ref_b.abs().sum(0) + 1e-30)).max().item()
        print(f"ln bwd {tag}: err/bound branch {r_b:.4f} colsum {r_c:.4f}")
        assert r_b <= 1.0, r_b
        assert r_c <= 1.0, r_c
        assert torch.all(br.cpu()[~keep] == 0)


@pytest.mark.parametrize("dy_dtype", [torch.bfloat16, torch.float32])
def test_layernorm_rows_past_block_cap(dy_dtype):
    """rows = 32768 + 33 at cols = 128: more than 1024 blocks x 32 rows, so every backward block
    walks 33 rows (the last one fewer) and the partial rows sum 32801 terms per column; the
    forward's grid is 2051 workgroups.  Same bounds."""
    ops, L = _mods()
    rows, cols = 32768 + 33, 128
    assert L.lib.cg_layernorm_bwd_blocks(rows) == 1024 and rows > 1024 * 32
    c = _case(rows, cols)
    if dy_dtype == torch.bfloat16:
        y, mean, rstd = ops.layernorm_fwd(c["x"].to(DEV), c["w"].to(DEV), c["b"].to(DEV), out_dtype=dy_dtype)
        torch.cuda.synchronize()
        _fwd_check(c, y, mean, rstd, f"rows={rows}")
    g_out, dgamma, dbeta, _, _ = _bwd(L, c, rows, cols, dy_dtype)
    _bwd_check(c, g_out, dgamma, dbeta, f"rows={rows} {dy_dtype}")
