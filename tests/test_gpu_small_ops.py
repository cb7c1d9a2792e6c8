"""The small memory-bound ops (embedding forward, casts, device-scalar scaling, padded casts, the
non-finite flag, column sums) against plain CPU references: bit for bit where the op is exact or
one IEEE rounding, fp64 with a forward-error bound where it sums.

Every test needs the MI355X (marker ``gpu``) and calls the C ABI through codonlm_amd.ops.
"""
import numpy as np
import pytest
import torch

from oracle import tinygpt_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
FMAX = float(np.finfo(np.float32).max)


def _ops():
    from codonlm_amd import ops
    return ops


def _bits(t):
    """bf16 tensor -> its 16-bit patterns (CPU int16)"""
    return t.detach().cpu().contiguous().view(torch.int16)


def _ulp32(ref):
    """spacing of fp32 at |ref| (fp64 tensor in, fp64 out)"""
    return torch.from_numpy(np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64))


def _split_pair(v):
    """fp32 -> (hi, lo) bf16 with hi = bf16(v), lo = bf16(v - hi)"""
    hi = v.to(torch.bfloat16)
    return hi, (v - hi.float()).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------
# cg_embed_fwd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("d,x_off", [(64, 0), (260, 0), (50, 0), (64, 1)])
def test_embed_fwd(d, x_off, with_pos, p):
    """Both kernels of cg_embed_fwd: the row kernel (d % 4 == 0, 16-B aligned buffers: d = 64 one
    partial wave pass, d = 260 two passes with a ragged second) and the scalar kernel (d = 50, and
    d = 64 with the output offset by one float).  p = 0: bitwise tok[idx] (+ pos[t]) in fp32.
    p > 0: dropped elements exactly 0 where the oracle's dropout_keep(seed, row, col, p) says so,
    kept ones within 1 fp32 ulp of (tok + pos) s with s = 1 / (1 - p) evaluated in fp32, as the
    C ABI (which takes p as a float) evaluates it: one rounding, of the product.  Against the
    exact quotient the roundings of 1 - p and of the reciprocal add up to 2 more ulp, and an exact
    fp32 emulation of the kernel's arithmetic measures 1.2 ulp there."""
    ops = _ops()
    B, T, V = 3, 77, 68
    M = B * T
    g = torch.Generator().manual_seed(d * 10 + x_off)
    idx = torch.randint(0, V, (B, T), generator=g)
    idx[0, 0], idx[2, T - 1] = 0, V - 1
    tok = torch.randn(V, d, generator=g)
    pos = torch.randn(T, d, generator=g) if with_pos else None
    buf = torch.full((M * d + 8,), float("nan"), device=DEV)
    out = buf[x_off:x_off + M * d].view(M, d)
    seed = 4321
    got = ops.embed_fwd(idx.to(DEV), tok.to(DEV), None if pos is None else pos.to(DEV), drop_seed=seed, drop_p=p,
                        out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    base = tok[idx.view(-1)]
    if pos is not None:
        base = base + pos.repeat(B, 1)          # fp32 add, as the kernel's
    got = got.cpu()
    if p == 0.0:
        assert torch.equal(got, base)
    else:
        keep = torch.from_numpy(O.dropout_keep(seed, np.arange(M)[:, None], np.arange(d)[None, :], p))
        assert 0.05 < 1.0 - keep.float().mean().item() < 0.15
        assert torch.all(got[~keep] == 0)
        ref = base.double() * float(np.float32(1) / (np.float32(1) - np.float32(p)))
        err = ((got.double() - ref).abs() / _ulp32(ref))[keep].max().item()
        print(f"embed_fwd d={d} off={x_off} pos={with_pos}: err/bound {err:.3f}")
        assert err <= 1.0, err
    # nothing outside the destination rows was written
    rest = torch.cat([buf[:x_off], buf[x_off + M * d:]]).cpu()
    assert torch.isnan(rest).all()


# ---------------------------------------------------------------------------------------------
# casts
# ---------------------------------------------------------------------------------------------
def test_cast_f32_to_bf16_bitwise():
    """cg_cast_f32_to_bf16 against torch's CPU fp32 -> bf16 cast (round to nearest even), bit for
    bit, n = 70001 (a ragged last workgroup): random values over 60 binades, +-0, +-inf, the
    largest finite fp32 (rounds to inf), exact ties (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6) and the
    fp32 neighbours either side of each tie.  A NaN is checked as NaN only (its payload is the
    hardware's).  fp32 denormals are left out of the bitwise set: whether the convert instruction
    flushes them follows the kernel's float mode, which the C ABI does not promise."""
    ops = _ops()
    n = 70001
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 30, (n,), generator=g).float())
    ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 256 * (1 + 3 * 2.0 ** -8)], dtype=np.float32)
    special = np.concatenate([
        np.array([0.0, -0.0, np.inf, -np.inf, FMAX, -FMAX], dtype=np.float32), ties,
        np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf))])
    x[:special.size] = torch.from_numpy(special)
    x[n - special.size:] = torch.from_numpy(special)          # the ragged tail too
    assert (x[x != 0].abs() >= float(np.finfo(np.float32).tiny)).all()   # no denormals
    nan_at = n // 2
    x[nan_at] = float("nan")
    got = ops.cast_to_bf16(x.to(DEV))
    torch.cuda.synchronize()
    ref = x.to(torch.bfloat16)
    assert torch.isinf(ref[4]) and ref[6].item() == 1.0 and ref[7].item() == 1 + 2.0 ** -6
    gb, rb = _bits(got), _bits(ref)
    assert torch.isnan(got[nan_at]).item()
    ok = torch.ones(n, dtype=torch.bool)
    ok[nan_at] = False
    assert torch.equal(gb[ok], rb[ok])


def test_cast_bf16_to_f32_bitwise():
    """cg_cast_bf16_to_f32 widens every one of the 65536 bit patterns (NaNs, denormals and
    infinities included) to pattern << 16, n = 70001."""
    ops = _ops()
    n = 70001
    pat = (torch.arange(n, dtype=torch.int32) * 40503) % 65536
    pat[:65536] = torch.arange(65536, dtype=torch.int32)
    src = (pat - ((pat >= 32768).int() << 16)).to(torch.int16).view(torch.bfloat16)
    got = ops.cast_from_bf16(src.to(DEV))
    torch.cuda.synchronize()
    want = (pat.to(torch.int64) << 16)
    want = (want - ((want >= 2 ** 31).long() << 32)).to(torch.int32)
    assert torch.equal(got.cpu().view(torch.int32), want)


# ---------------------------------------------------------------------------------------------
# cg_scale_dev
# ---------------------------------------------------------------------------------------------
ROWS, COLS = 37, 68


def _scale_case(kind, g):
    """(device buffer [ROWS][ld], CPU copy) with every column random, the gap columns included"""
    if kind == "f32":
        x = torch.randn(ROWS, 80, generator=g)
    elif kind == "bf16":
        x = torch.randn(ROWS, 80, generator=g).to(torch.bfloat16)
    else:
        v = torch.randn(ROWS, 80, generator=g)
        hi, lo = _split_pair(v)
        x = torch.cat([hi, lo], 1)                # hi in [0, 80), lo in [80, 160); cols 68 live
    return x.to(DEV), x


@pytest.mark.parametrize("kind", ["f32", "bf16", "bf16x2"])
def test_scale_dev(kind):
    """cg_scale_dev with the scale read from a device scalar, rows 37, cols 68 inside ld 80 (160
    for the split pairs).  F32: one IEEE product, within 1 ulp of x s in fp64.  BF16: bitwise
    bf16(float(x) s).  BF16X2: hi + lo within 2^-17 relative of (hi0 + lo0) s (two fp32 roundings
    at 2^-24, then a split whose residual is below 2^-9 2^-9).  The columns between cols and ld
    (for BF16X2 of both halves) are never written, and a scale of exactly 1 leaves every byte."""
    ops = _ops()
    g = torch.Generator().manual_seed(17)
    split = kind == "bf16x2"
    s32 = np.float32(0.37)
    sc = torch.tensor(float(s32), device=DEV)
    xd, x0 = _scale_case(kind, g)
    ops.scale_dev_(xd, sc, cols=COLS, split=split)
    torch.cuda.synchronize()
    got = xd.cpu()
    if kind == "f32":
        ref = x0[:, :COLS].double() * float(s32)
        err = ((got[:, :COLS].double() - ref).abs() / _ulp32(ref)).max().item()
        assert err <= 1.0, err
        assert torch.equal(got[:, COLS:], x0[:, COLS:])
    elif kind == "bf16":
        ref = (x0[:, :COLS].float() * torch.tensor(s32)).to(torch.bfloat16)
        assert torch.equal(_bits(got[:, :COLS]), _bits(ref))
        assert torch.equal(_bits(got[:, COLS:]), _bits(x0[:, COLS:]))
        err = 0.0
    else:
        ref = (x0[:, :COLS].double() + x0[:, 80:80 + COLS].double()) * float(s32)
        val = got[:, :COLS].double() + got[:, 80:80 + COLS].double()
        err = ((val - ref).abs() / (2.0 ** -17 * ref.abs() + 1e-30)).max().item()
        assert err <= 1.0, err
        # hi is a nearest bf16 of the pair's value: |lo| <= half a bf16 ulp of hi
        assert (got[:, 80:80 + COLS].double().abs() <= 2.0 ** -8 * got[:, :COLS].double().abs()).all()
        for sl in (slice(COLS, 80), slice(80 + COLS, 160)):
            assert torch.equal(_bits(got[:, sl]), _bits(x0[:, sl]))
    print(f"scale_dev {kind}: err/bound {err:.3f}")
    # scale exactly 1: nothing moves
    xd, x0 = _scale_case(kind, g)
    ops.scale_dev_(xd, torch.tensor(1.0, device=DEV), cols=COLS, split=split)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu().view(torch.uint8), x0.view(torch.uint8))


def test_scale_dev_ld_too_small():
    ops = _ops()
    sc = torch.tensor(0.5, device=DEV)
    with pytest.raises(ValueError):
        ops.scale_dev_(torch.zeros(4, 80, device=DEV), sc, cols=81)
    with pytest.raises(ValueError):
        ops.scale_dev_(torch.zeros(4, 160, device=DEV, dtype=torch.bfloat16), sc, cols=81, split=True)


# ---------------------------------------------------------------------------------------------
# cg_cast_pad_2d
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "bf16", "bf16x2"])
def test_cast_pad_2d(kind):
    """fp32 [37][69] (row stride 72) -> [37][80] inside a destination of row stride 88 (176 for
    the split pairs): values exact (F32), round to nearest even (BF16), hi = bf16(v) and hi + lo
    within 2^-17 relative of v (BF16X2, lo at column 80 + c); pad columns [69, 80) of every half
    exactly zero; the destination columns past 80 (past 160) untouched."""
    ops = _ops()
    rows, cols, dcols = 37, 69, 80
    g = torch.Generator().manual_seed(23)
    full = torch.randn(rows, 72, generator=g) * 3
    src = full.to(DEV)[:, :cols]
    v = full[:, :cols]
    split = kind == "bf16x2"
    dt = torch.float32 if kind == "f32" else torch.bfloat16
    width = 176 if split else 88
    dst0 = torch.randn(rows, width, generator=g).to(dt)
    dst = dst0.to(DEV)
    ops.cast_pad_2d(src, dcols, dtype=dt, out=dst, split=split)
    torch.cuda.synchronize()
    got = dst.cpu()
    if kind == "f32":
        assert torch.equal(got[:, :cols], v)
    else:
        assert torch.equal(_bits(got[:, :cols]), _bits(v.to(torch.bfloat16)))
    assert torch.all(got[:, cols:dcols] == 0)
    live = dcols
    if split:
        val = got[:, :cols].double() + got[:, dcols:dcols + cols].double()
        err = ((val - v.double()).abs() / (2.0 ** -17 * v.double().abs() + 1e-30)).max().item()
        print(f"cast_pad_2d bf16x2: err/bound {err:.3f}")
        assert err <= 1.0, err
        assert torch.all(got[:, dcols + cols:2 * dcols] == 0)
        live = 2 * dcols
    assert torch.equal(got[:, live:].contiguous().view(torch.uint8), dst0[:, live:].contiguous().view(torch.uint8))
    # the allocating form gives the same values
    got2 = ops.cast_pad_2d(src, dcols, dtype=dt, split=split).cpu()
    assert torch.equal(got2.view(torch.uint8), got[:, :live].contiguous().view(torch.uint8))


def test_cast_pad_2d_errors():
    ops = _ops()
    src = torch.zeros(5, 69, device=DEV)
    with pytest.raises(ValueError):
        ops.cast_pad_2d(src, 68)
    with pytest.raises(ValueError):   # destination rows narrower than the two halves
        ops.cast_pad_2d(src, 80, out=torch.zeros(5, 159, device=DEV, dtype=torch.bfloat16), split=True)


# ---------------------------------------------------------------------------------------------
# cg_nonfinite_flag
# ---------------------------------------------------------------------------------------------
SWEEP = 2048 * 256  # elements per sweep of the capped grid


@pytest.mark.parametrize("n", [1, 63, 257, SWEEP + 5])
def test_nonfinite_flag(n):
    """All-finite input (the largest finite value and a denormal included) leaves the flag 0 and
    leaves a flag preset to 1 at 1 (the kernel only ORs); a NaN, +inf or -inf at index 0, at n - 1
    or at 2048 256 + 1 (the grid's second sweep) sets it."""
    ops = _ops()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    x[0] = FMAX
    x[n - 1] = -FMAX if n > 1 else FMAX
    if n > 2:
        x[1] = 1e-42
        x[n // 2] = -1e-45
    xd = x.to(DEV)
    assert ops.nonfinite_flag(xd).item() == 0
    assert ops.nonfinite_flag(xd, torch.ones((), dtype=torch.int32, device=DEV)).item() == 1
    for at in sorted({0, n - 1, SWEEP + 1}):
        if at >= n:
            continue
        for bad in (float("nan"), float("inf"), float("-inf")):
            y = xd.clone()
            y[at] = bad
            assert ops.nonfinite_flag(y).item() == 1, (at, bad)


# ---------------------------------------------------------------------------------------------
# cg_colsum
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("rows", [1, 37, 1000])
@pytest.mark.parametrize("path,dtype,cols,ldx", [("scalar", torch.float32, 100, 100), ("scalar", torch.bfloat16, 100, 104),
                                                 ("scalar", torch.float32, 104, 105), ("vec", torch.float32, 104, 112)])
def test_colsum_paths(path, dtype, cols, ldx, rows, accumulate):
    """cg_colsum's scalar kernels (cols % 8 != 0, or an odd row stride) in fp32 and bf16, and the
    vectorised fp32 kernel, against the fp64 column sums of the same values: per column
    |err| <= 2e-5 (sum_rows |x| + |out0|), rows below / across / many times the row chunking."""
    ops = _ops()
    g = torch.Generator().manual_seed(rows + cols + ldx)
    full = (torch.randn(rows, ldx, generator=g) * 2 + 0.3).to(dtype)
    x = full.to(DEV)[:, :cols]
    out0 = torch.randn(cols, generator=g)
    out = out0.to(DEV)
    ops.colsum(x, out=out, accumulate=accumulate)
    torch.cuda.synchronize()
    xv = full[:, :cols].double()
    ref = xv.sum(0) + (out0.double() if accumulate else 0.0)
    bound = 2e-5 * (xv.abs().sum(0) + (out0.double().abs() if accumulate else 0.0)) + 1e-30
    err = ((out.cpu().double() - ref).abs() / bound).max().item()
    print(f"colsum {path} {dtype} rows={rows} acc={accumulate}: err/bound {err:.4f}")
    assert err <= 1.0, err


@pytest.mark.parametrize("cols,ldx", [(100, 100), (104, 112)])
def test_colsum_no_rows(cols, ldx):
    """rows = 0: zeros, or `out` unchanged with accumulate."""
    from codonlm_amd import _lib as L
    x = torch.ones(4, ldx, device=DEV)
    ws = torch.empty(64 * cols, device=DEV)
    out = torch.full((cols,), 7.0, device=DEV)
    for accumulate, want in ((1, 7.0), (0, 0.0)):
        L.check(L.lib.cg_colsum(L.CG_F32, x.data_ptr(), ldx, 0, cols, out.data_ptr(), accumulate, ws.data_ptr(),
                                ws.numel() * 4, L.stream_ptr(DEV)), "cg_colsum")
        torch.cuda.synchronize()
        assert torch.all(out == want)
